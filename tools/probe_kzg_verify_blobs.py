"""The blob check from the blob itself (zkw_eip4844_verify_blobs: challenge, barycentric evaluation, pairing) measured on one MI355X beside
the check of the records (zkw_eip4844_verify) on the same blobs -> profiles/r20/kzg_verify_blobs.json.

    python tools/probe_kzg_verify_blobs.py [--out profiles/r20/kzg_verify_blobs.json]

The method of tools/probe_kzg_verify.py: one process, one context, the ceremony's settings and [tau] G2 (tests/golden), the 32 random blobs
of tools/probe_eip4844_proofs.py (numpy.random.default_rng(4844)), claims made by the device's own prover. Every step that uses the GPU
runs under a time limit of its own (SIGALRM with its default action: the process ends even inside a library call) and the first failure
ends the probe: nothing is started on the GPU after it.

  verify_blobs    zkw_eip4844_verify_blobs at 1 / 4 / 32 blobs on the evaluation forms, commitments and blob proofs of zkw_eip4844_witness
                  and zkw_eip4844_prove; every verdict is checked to be 1 and the openings to equal the proof records. Host pointer mode,
                  wall clock around the synchronised call, one untimed call, then five: median, min, max. The call uploads 131 072 bytes a
                  blob, which the check of the records does not
  verify_records  zkw_eip4844_verify on the same blobs in the same process, the same way. It checks TWO claims a blob (the opening at the
                  record's point and the blob proof) from 352 bytes of records; verify_blobs checks ONE, from the blob
  verify_claims   zkw_kzg_verify on exactly the claims verify_blobs ends up checking (commitment, blob_challenge, blob_value, blob_proof as
                  four arrays): the same points kernel on the same data through the first claim form, so that a difference between
                  k_kzg_verify_points here and there is the form's and not the data's
  evaluate        zkw_kzg_evaluate_blobs alone on the same evaluation forms at the proof records' challenges (one readback)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "kzg_verify_blobs.json"))
    args = ap.parse_args()
    from era_zkevm_test_harness_amd import native

    golden = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(golden, "kzg_trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(golden, "kzg_trusted_setup_g2.bin"), "rb").read()
    ctx = native.Context(0)
    verifier = step(60, lambda: native.KzgVerifier(ctx, g2))
    settings = step(60, lambda: native.KzgSettings(ctx, g1))
    blobs = np.random.default_rng(4844).integers(0, 256, size=(32, BLOB_BYTES), dtype=np.uint8)
    out = {"claims_per_blob": {"verify_blobs": 1, "verify_records": 2}, "blobs": {}}
    for n in (1, 4, 32):
        b = np.ascontiguousarray(blobs[:n])
        rec = step(60, lambda: settings.eip4844_witness(b))
        prf, ev = step(60, lambda: settings.eip4844_prove(b, rec, evaluations=True))
        com, proof, z = (np.ascontiguousarray(x) for x in (rec["commitment"], prf["blob_proof"], prf["blob_challenge"]))
        verdicts, openings = step(60, lambda: verifier.eip4844_verify_blobs(ev, com, proof, openings=True))
        assert verdicts.tolist() == [1] * n
        assert openings[:, :32].tobytes() == prf["blob_challenge"].tobytes() and openings[:, 32:].tobytes() == prf["blob_value"].tobytes()
        assert step(60, lambda: verifier.eip4844_verify(rec, prf)).tolist() == [[1, 1]] * n
        assert step(60, lambda: native.kzg_evaluate_blobs(ctx, ev, z)).tobytes() == prf["blob_value"].tobytes()
        z_le, y_le = (np.ascontiguousarray(prf[f][:, ::-1]) for f in ("blob_challenge", "blob_value"))
        assert step(60, lambda: verifier.verify(com, z_le, y_le, proof)).tolist() == [1] * n
        leg = {"verify_blobs": step(60, lambda: timed(lambda: verifier.eip4844_verify_blobs(ev, com, proof))),
               "verify_records": step(60, lambda: timed(lambda: verifier.eip4844_verify(rec, prf))),
               "verify_claims": step(60, lambda: timed(lambda: verifier.verify(com, z_le, y_le, proof))),
               "evaluate": step(60, lambda: timed(lambda: native.kzg_evaluate_blobs(ctx, ev, z))),
               "split_ms_serial": {"verify_blobs": step(60, lambda: split_of(ctx, lambda: verifier.eip4844_verify_blobs(ev, com, proof))),
                                   "verify_records": step(60, lambda: split_of(ctx, lambda: verifier.eip4844_verify(rec, prf))),
                                   "verify_claims": step(60, lambda: split_of(ctx, lambda: verifier.verify(com, z_le, y_le, proof)))}}
        leg["blobs_minus_records_ms"] = round(leg["verify_blobs"]["median_ms"] - leg["verify_records"]["median_ms"], 4)
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
