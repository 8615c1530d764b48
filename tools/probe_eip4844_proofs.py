"""The KZG proofs (zkw_kzg_open, zkw_eip4844_prove) measured on one MI355X beside the calls they build on
-> profiles/r16/eip4844_proofs.json.

    python tools/probe_eip4844_proofs.py [--out profiles/r16/eip4844_proofs.json]

One process, one context, the inputs of tools/probe_eip4844.py (the ceremony's settings, 32 random blobs of numpy.random.default_rng(4844),
the first 1, 4 and 32 per call). Every step that uses the GPU runs under a time limit of its own (SIGALRM with its default action: the
process ends even inside a library call) and the first failure ends the probe: nothing is started on the GPU after it.

  commit / open    zkw_kzg_commit and zkw_kzg_open on the SAME coefficient rows (open: one random point below r per polynomial): host pointer
                   mode, wall clock around the synchronised call, one untimed call, then five: median, min, max
  witness / prove  zkw_eip4844_witness, then zkw_eip4844_prove on its records (without the evaluation form), the same way
  split            ONE further commit, open and prove per count under zkw_profile (HIP events around every launch; the kernels then
                   run one after another on the context's stream: what each costs alone, not what the overlapped call costs)
  conditions       open's median against commit's median + the split's k_kzg_quotient and k_kzg_check_points + commit's max - min;
                   prove's median against twice the commit's; the side branch (twiddles, transform, sponge) against the main branch it
                   runs beside (the opening's quotient)
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
SIDE = ("k_kzg_twiddles", "k_kzg_blob_ntt", "k_kzg_blob_challenge")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "eip4844_proofs.json"))
    args = ap.parse_args()
    from era_zkevm_test_harness_amd import native

    raw = open(os.path.join(ROOT, "tests", "golden", "kzg_trusted_setup_g1.bin"), "rb").read()
    ctx = native.Context(0)
    settings = step(60, lambda: native.KzgSettings(ctx, raw))
    out = {"settings_bytes": settings.nbytes, "per_call": {}}
    rng = np.random.default_rng(4844)
    blobs = rng.integers(0, 256, size=(32, BLOB_BYTES), dtype=np.uint8)
    coeffs = np.zeros((32, 4096, 32), np.uint8)  # coefficient k of blob j = element 4095 - k, 31 bytes + a zero byte
    coeffs[:, :, :31] = blobs.reshape(32, 4096, 31)[:, ::-1, :]
    points = np.frombuffer(b"".join((int.from_bytes(rng.bytes(32), "little") % R).to_bytes(32, "little") for _ in range(32)), np.uint8).reshape(32, 32)
    for n in (1, 4, 32):
        b, c, z = np.ascontiguousarray(blobs[:n]), np.ascontiguousarray(coeffs[:n]), np.ascontiguousarray(points[:n])
        rec = step(60, lambda: settings.eip4844_witness(b))
        proofs, _ = step(60, lambda: settings.open(c, 4096, np.ascontiguousarray(np.pad(rec["evaluation_point"][:, ::-1], ((0, 0), (0, 16))))))
        prf = step(60, lambda: settings.eip4844_prove(b, rec))
        assert proofs.tobytes() == prf["opening_proof"].tobytes()  # the two entry points agree on the opening at z
        leg = {"commit": step(60, lambda: timed(lambda: settings.commit(c, 4096))),
               "open": step(60, lambda: timed(lambda: settings.open(c, 4096, z))),
               "witness": step(60, lambda: timed(lambda: settings.eip4844_witness(b))),
               "prove": step(60, lambda: timed(lambda: settings.eip4844_prove(b, rec))),
               "commit_split_ms_serial": step(60, lambda: split_of(ctx, lambda: settings.commit(c, 4096))),
               "open_split_ms_serial": step(60, lambda: split_of(ctx, lambda: settings.open(c, 4096, z))),
               "prove_split_ms_serial": step(60, lambda: split_of(ctx, lambda: settings.eip4844_prove(b, rec)))}
        extra = leg["open_split_ms_serial"].get("k_kzg_quotient", 0.0) + leg["open_split_ms_serial"].get("k_kzg_check_points", 0.0)
        bound = leg["commit"]["median_ms"] + extra + leg["commit"]["max_ms"] - leg["commit"]["min_ms"]
        side = sum(leg["prove_split_ms_serial"].get(k, 0.0) for k in SIDE)
        main_branch = leg["prove_split_ms_serial"].get("k_kzg_quotient", 0.0) / 2  # (two launches under one name: the opening's is one of them)
        leg["conditions"] = {"open_bound_ms": round(bound, 4), "open_within_bound": leg["open"]["median_ms"] <= bound,
                             "prove_over_two_commits": round(leg["prove"]["median_ms"] / (2 * leg["commit"]["median_ms"]), 4),
                             "side_branch_ms": round(side, 4), "main_branch_beside_it_ms": round(main_branch, 4)}
        out["per_call"][str(n)] = leg
        print(n, json.dumps(leg), flush=True)
    settings.free()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
