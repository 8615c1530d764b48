"""The KZG producers from a blob in evaluation form (zkw_kzg_commit_blobs, zkw_kzg_open_blobs, zkw_eip4844_prove_blobs) measured on one
MI355X beside the calls they are built from (zkw_kzg_commit, zkw_kzg_open on the coefficients) -> profiles/r23/kzg_blob_producers.json.

    python tools/probe_kzg_blob_producers.py [--out profiles/r23/kzg_blob_producers.json]

The method of tools/probe_kzg_verify_blobs.py: one process, one context, the ceremony's settings and [tau] G2 (tests/golden), 32 blobs of
full-range random elements (random.Random(23), every element below r: nobody's pubdata). Every step that uses the GPU runs under a time
limit of its own (SIGALRM with its default action: the process ends even inside a library call) and the first failure ends the probe:
nothing is started on the GPU after it. Host pointer mode, wall clock around the synchronised call, one untimed call, then five: median,
min, max, at 1 / 4 / 32 blobs per call.

  coefficients    zkw_kzg_blob_coefficients alone (twiddles, the inverse transform, the readback, 131 072 bytes a blob each way)
  commit, open    zkw_kzg_commit and zkw_kzg_open on the coefficients that call returned: the code the producers end in, on identical
                  scalars (the points of `open` are the points of `open_blobs`, little-endian)
  commit_blobs, open_blobs, prove_blobs   the three producers; every result is checked first: commit_blobs equals commit, open_blobs equals
                  open, and the device's verifier accepts (commitment, blob proof) from the blob itself
  split           ONE further call each under zkw_profile (HIP events around every launch): what each kernel costs alone; with it one
                  zkw_eip4844_prove of pubdata blobs for k_kzg_blob_ntt in the same run
  bounds          per producer: the composing call's median + the split's twiddles and inverse transform + the composing call's own
                  max - min; prove_blobs against open + the split's sponge where the sponge is the longer branch. met: median <= bound
"""
import argparse
import json
import os
import random
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BLOB_BYTES = 4096 * 31


def step(seconds, fn):
    """fn() under its own time limit"""
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(seconds)
    try:
        return fn()
    finally:
        signal.alarm(0)


def timed(fn, runs=5):
    fn()  # warm
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "runs": runs}


def split_of(ctx, fn):
    ctx.profile_enable(True)
    ctx.profile_reset()
    fn()
    ctx.synchronize()
    out = {k: round(v[0], 4) for k, v in sorted(ctx.profile().items()) if k.startswith("k_kzg")}
    ctx.profile_enable(False)
    return out


def bound(base, split, longer_branch=0.0):
    """(bound, its parts): the composing call's median + twiddles + inverse transform (+ what the sponge adds) + the call's own spread"""
    front = split["k_kzg_twiddles"] + split["k_kzg_blob_intt"]
    spread = base["max_ms"] - base["min_ms"]
    return round(base["median_ms"] + max(front, longer_branch) + spread, 4), {"front_ms": round(front, 4), "spread_ms": round(spread, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "kzg_blob_producers.json"))
    args = ap.parse_args()
    from era_zkevm_test_harness_amd import native

    golden = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(golden, "kzg_trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(golden, "kzg_trusted_setup_g2.bin"), "rb").read()
    ctx = native.Context(0)
    verifier = step(60, lambda: native.KzgVerifier(ctx, g2))
    settings = step(60, lambda: native.KzgSettings(ctx, g1))
    rng = random.Random(23)
    evals = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(32 * 4096)), np.uint8).reshape(32, 131072)
    points = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(32)), np.uint8).reshape(32, 32)
    pubdata = np.random.default_rng(4844).integers(0, 256, size=(32, BLOB_BYTES), dtype=np.uint8)
    out = {"blobs": {}}
    for n in (1, 4, 32):
        ev, z = np.ascontiguousarray(evals[:n]), np.ascontiguousarray(points[:n])
        z_le = np.ascontiguousarray(z[:, ::-1])
        coeffs = step(60, lambda: native.kzg_blob_coefficients(ctx, ev))
        com = step(60, lambda: settings.commit(coeffs, 4096))
        assert step(60, lambda: settings.commit_blobs(ev)).tobytes() == com.tobytes()
        proofs, values = step(60, lambda: settings.open(coeffs, 4096, z_le))
        got = step(60, lambda: settings.open_blobs(ev, z))
        assert got[0].tobytes() == proofs.tobytes() and got[1][:, ::-1].tobytes() == values.tobytes()
        assert step(60, lambda: verifier.verify(com, z_le, values, proofs)).tolist() == [1] * n
        blob_proofs = step(60, lambda: settings.eip4844_prove_blobs(ev, com))
        assert step(60, lambda: verifier.eip4844_verify_blobs(ev, com, blob_proofs)).tolist() == [1] * n
        pub = np.ascontiguousarray(pubdata[:n])
        rec = step(60, lambda: settings.eip4844_witness(pub))
        leg = {"coefficients": step(60, lambda: timed(lambda: native.kzg_blob_coefficients(ctx, ev))),
               "commit": step(60, lambda: timed(lambda: settings.commit(coeffs, 4096))),
               "open": step(60, lambda: timed(lambda: settings.open(coeffs, 4096, z_le))),
               "commit_blobs": step(60, lambda: timed(lambda: settings.commit_blobs(ev))),
               "open_blobs": step(60, lambda: timed(lambda: settings.open_blobs(ev, z))),
               "prove_blobs": step(120, lambda: timed(lambda: settings.eip4844_prove_blobs(ev, com))),
               "split_ms_serial": {"commit_blobs": step(60, lambda: split_of(ctx, lambda: settings.commit_blobs(ev))),
                                   "open_blobs": step(60, lambda: split_of(ctx, lambda: settings.open_blobs(ev, z))),
                                   "prove_blobs": step(60, lambda: split_of(ctx, lambda: settings.eip4844_prove_blobs(ev, com))),
                                   "eip4844_prove": step(60, lambda: split_of(ctx, lambda: settings.eip4844_prove(pub, rec)))}}
        split = leg["split_ms_serial"]
        leg["intt_over_ntt"] = round(split["prove_blobs"]["k_kzg_blob_intt"] / split["eip4844_prove"]["k_kzg_blob_ntt"], 3)
        sponge = split["prove_blobs"]["k_kzg_blob_challenge"]
        leg["bounds"] = {}
        for name, base, extra in (("commit_blobs", "commit", 0.0), ("open_blobs", "open", 0.0), ("prove_blobs", "open", sponge)):
            limit, parts = bound(leg[base], split[name], extra)
            leg["bounds"][name] = dict(parts, against=base, bound_ms=limit, median_ms=leg[name]["median_ms"], met=leg[name]["median_ms"] <= limit)
        out["blobs"][str(n)] = leg
        print(n, json.dumps(leg), flush=True)
    verifier.free()
    settings.free()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
