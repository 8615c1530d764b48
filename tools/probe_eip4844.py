"""The EIP-4844 blob witness (zkw_kzg_settings_create, zkw_kzg_commit, zkw_eip4844_witness) measured on one MI355X
-> profiles/r14/eip4844.json.

    python tools/probe_eip4844.py [--out profiles/r14/eip4844.json]

One process, one context; the steps run one after another and the first failure ends the probe (nothing is started on the GPU after it).

  settings   zkw_kzg_settings_create over the ceremony's 4 096 points (tests/golden/kzg_trusted_setup_g1.bin): wall clock around the
             call, which ends synchronised — measured ONCE, cold (decompression + subgroup check, then the 32 x 4 096 table)
  commit     zkw_kzg_commit of 1, 4 and 32 polynomials of 4 096 coefficients (the blobs' elements) per call, and
  witness    zkw_eip4844_witness of the same 1, 4 and 32 blobs per call: host pointer mode, wall clock around the synchronised call, after
             one untimed call, five calls, their median with min - max
  split      ONE further witness call per blob count under zkw_profile (HIP events around every launch; the kernels then run one after
             another on the context's stream, so the split shows what each costs, not what the overlapped call costs)
  price      Fq multiplications per blob from the blob's nonzero digits -> multiply-adds (2 x 12^2 per Montgomery product) against the
             measured v_mad_u64_u32 issue ceiling of profiles/r05/valu_ceiling.json, for the accumulate kernel's time of the split
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MADS_PER_FQ_MUL = 2 * 12 * 12
BLOB_BYTES = 4096 * 31


def mad_ceiling_lane_ops_per_s():
    with open(os.path.join(ROOT, "profiles", "r05", "valu_ceiling.json")) as f:
        c = json.load(f)
    mad = next(x for x in c["classes"] if x["class"] == "v_mad_u64_u32")
    return mad["best_wave_insts_per_s"] * 64


def timed(fn, runs=5):
    fn()  # warm
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "runs": runs}


def fq_muls_per_blob(nonzero_digits):
    """useful multiplications: a mixed addition (11) per nonzero digit; the 255 folds of 64 partial sums and the eight folds of 128
    buckets (Jacobian additions, 16 each); seven doublings (7) and additions; one Fermat inversion (~570) and the conversions"""
    return 11 * nonzero_digits + 16 * (255 * 63 + 8 * 127 + 7) + 7 * 7 + 570 + 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "eip4844.json"))
    args = ap.parse_args()
    from era_zkevm_test_harness_amd import native

    raw = open(os.path.join(ROOT, "tests", "golden", "kzg_trusted_setup_g1.bin"), "rb").read()
    ctx = native.Context(0)
    t = time.perf_counter()
    settings = native.KzgSettings(ctx, raw)
    out = {"settings_create_ms_cold_once": round((time.perf_counter() - t) * 1e3, 3), "settings_bytes": settings.nbytes, "per_call": {}}
    rng = np.random.default_rng(4844)
    blobs = rng.integers(0, 256, size=(32, BLOB_BYTES), dtype=np.uint8)
    # the same polynomials as coefficient rows: coefficient k of blob j = element 4095 - k, 31 bytes + a zero byte
    coeffs = np.zeros((32, 4096, 32), np.uint8)
    coeffs[:, :, :31] = blobs.reshape(32, 4096, 31)[:, ::-1, :]
    digits = int(np.count_nonzero(blobs[0]))
    ceiling = mad_ceiling_lane_ops_per_s()
    for n in (1, 4, 32):
        b, c = np.ascontiguousarray(blobs[:n]), np.ascontiguousarray(coeffs[:n])
        rec = settings.eip4844_witness(b)
        assert rec["commitment"].tobytes() == settings.commit(c, 4096).tobytes()  # the two entry points agree
        leg = {"commit": timed(lambda: settings.commit(c, 4096)), "witness": timed(lambda: settings.eip4844_witness(b))}
        ctx.profile_enable(True)
        ctx.profile_reset()
        settings.eip4844_witness(b)
        ctx.synchronize()
        leg["split_ms_serial"] = {k: round(v[0], 4) for k, v in sorted(ctx.profile().items()) if k.startswith("k_kzg")}
        ctx.profile_enable(False)
        acc_s = leg["split_ms_serial"].get("k_kzg_accumulate", 0.0) * 1e-3
        muls = fq_muls_per_blob(digits) * n
        leg["price"] = {"nonzero_digits_per_blob": digits, "fq_multiplications": muls, "multiply_adds": muls * MADS_PER_FQ_MUL,
                        "mad_ceiling_lane_ops_per_s": ceiling,
                        "fraction_of_mad_ceiling_in_accumulate": round((11 * digits + 16 * 255 * 63) * n * MADS_PER_FQ_MUL / (acc_s * ceiling), 4) if acc_s else None,
                        "fraction_of_mad_ceiling_whole_commit": None}
        commit_s = sum(leg["split_ms_serial"].get(k, 0.0) for k in ("k_kzg_lists", "k_kzg_accumulate", "k_kzg_finish", "k_kzg_compress")) * 1e-3
        if commit_s:
            leg["price"]["fraction_of_mad_ceiling_whole_commit"] = round(muls * MADS_PER_FQ_MUL / (commit_s * ceiling), 4)
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
