"""The verification of KZG proofs (zkw_kzg_verifier_create, zkw_kzg_verify, zkw_eip4844_verify) measured on one MI355X beside the cost of
proving the same blobs -> profiles/r18/kzg_verify.json.

    python tools/probe_kzg_verify.py [--out profiles/r18/kzg_verify.json]

One process, one context, the ceremony's settings and [tau] G2 (tests/golden), the 32 random blobs of tools/probe_eip4844_proofs.py
(numpy.random.default_rng(4844)). Every step that uses the GPU runs under a time limit of its own (SIGALRM with its default action: the
process ends even inside a library call) and the first failure ends the probe: nothing is started on the GPU after it.

  create          zkw_kzg_verifier_create: the first call of the process (cold: the code object's first kernels of this kind), then five more
  verify          zkw_kzg_verify at 1 / 8 / 64 / 1024 claims per call. The claims are true ones, made by the device's own prover:
                  polynomials of 16 coefficients through zkw_kzg_commit and zkw_kzg_open at random points; every verdict is checked to be 1.
                  Host pointer mode, wall clock around the synchronised call, one untimed call, then five: median, min, max
  eip4844_verify  zkw_eip4844_verify at 1 / 4 / 32 blobs (2 claims a blob) on the records of zkw_eip4844_witness and zkw_eip4844_prove,
                  the same way, beside zkw_eip4844_prove on the same blobs: verify_over_prove is the ratio of the medians
  split           ONE further call per count under zkw_profile (HIP events around every launch): what each kernel costs alone
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOB_BYTES = 4096 * 31
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N_COEFFS = 16


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "kzg_verify.json"))
    args = ap.parse_args()
    from era_zkevm_test_harness_amd import native

    golden = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(golden, "kzg_trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(golden, "kzg_trusted_setup_g2.bin"), "rb").read()
    ctx = native.Context(0)
    t = time.perf_counter()
    verifier = step(60, lambda: native.KzgVerifier(ctx, g2))
    cold = (time.perf_counter() - t) * 1e3

    def create():
        native.KzgVerifier(ctx, g2).free()

    out = {"verifier_bytes": verifier.nbytes, "create": {"cold_ms": round(cold, 4), "warm": step(60, lambda: timed(create)),
                                                         "split_ms": step(60, lambda: split_of(ctx, create))}, "verify": {}, "eip4844_verify": {}}
    print("create", json.dumps(out["create"]), flush=True)
    settings = step(60, lambda: native.KzgSettings(ctx, g1))
    rng = np.random.default_rng(4844)
    blobs = rng.integers(0, 256, size=(32, BLOB_BYTES), dtype=np.uint8)

    def scalars(n):
        return np.frombuffer(b"".join((int.from_bytes(rng.bytes(32), "little") % R).to_bytes(32, "little") for _ in range(n)), np.uint8).reshape(n, 32)

    coeffs, points = scalars(1024 * N_COEFFS), scalars(1024)
    commitments = step(60, lambda: settings.commit(coeffs, N_COEFFS))
    proofs, values = step(60, lambda: settings.open(coeffs, N_COEFFS, points))
    for n in (1, 8, 64, 1024):
        a = [np.ascontiguousarray(x[:n]) for x in (commitments, points, values, proofs)]
        assert step(60, lambda: verifier.verify(*a)).tolist() == [1] * n
        leg = {"verify": step(60, lambda: timed(lambda: verifier.verify(*a))), "split_ms_serial": step(60, lambda: split_of(ctx, lambda: verifier.verify(*a)))}
        leg["per_claim_ms"] = round(leg["verify"]["median_ms"] / n, 4)
        out["verify"][str(n)] = leg
        print(n, json.dumps(leg), flush=True)
    for n in (1, 4, 32):
        b = np.ascontiguousarray(blobs[:n])
        rec = step(60, lambda: settings.eip4844_witness(b))
        prf = step(60, lambda: settings.eip4844_prove(b, rec))
        assert step(60, lambda: verifier.eip4844_verify(rec, prf)).tolist() == [[1, 1]] * n
        leg = {"verify": step(60, lambda: timed(lambda: verifier.eip4844_verify(rec, prf))), "prove": step(60, lambda: timed(lambda: settings.eip4844_prove(b, rec))),
               "split_ms_serial": step(60, lambda: split_of(ctx, lambda: verifier.eip4844_verify(rec, prf)))}
        leg["verify_over_prove"] = round(leg["verify"]["median_ms"] / leg["prove"]["median_ms"], 4)
        out["eip4844_verify"][str(n)] = leg
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
