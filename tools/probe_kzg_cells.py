"""The EIP-7594 cell proofs (zkw_kzg_cell_proofs_blobs) measured on one MI355X beside the only route the library had before them — the 128
quotient polynomials of a blob through zkw_kzg_commit -> profiles/r24/kzg_cells.json.

    python tools/probe_kzg_cells.py [--out profiles/r24/kzg_cells.json]

The method of tools/probe_kzg_blob_producers.py: one process, one context, the ceremony's settings (tests/golden), 32 blobs of full-range
random elements (random.Random(24), every element below r). Every step that uses the GPU runs under a time limit of its own (SIGALRM with
its default action: the process ends even inside a library call) and the first failure ends the probe: nothing is started on the GPU after
it. Host pointer mode, wall clock around the synchronised call, one untimed call, then five: median, min, max, at 1 / 4 / 32 blobs per call.

  settings        zkw_kzg_cell_settings_create, cold (the first call of the process) and once more, and the bytes it holds
  cell_proofs     zkw_kzg_cell_proofs_blobs without cells and with them; cells alone (zkw_kzg_cells_blobs)
  baseline        zkw_kzg_commit of n x 128 polynomials of 4 032 coefficients already on the host. Blob 0's rows are its 128 quotient
                  polynomials by the host model's division (not timed) and the call's first 128 results are checked against the new call's
                  proofs; the other blobs' rows are other full-range scalars (random bytes with the top byte masked below r): the division of 32 blobs
                  in Python integers would take longer than the probe, and the commitment's cost does not depend on whose scalars they are
  split           ONE further call under zkw_profile (HIP events around every launch): what each kernel costs alone
  g1_fft          zkw_kzg_g1_fft of 1 and of 64 transforms of 128 points (decompression and compression included), and its split
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "kzg_cells.json"))
    args = ap.parse_args()
    from era_zkevm_test_harness_amd import native
    from tests import kzg_cells_model as cm

    g1 = open(os.path.join(ROOT, "tests", "golden", "kzg_trusted_setup_g1.bin"), "rb").read()
    ctx = native.Context(0)
    settings = step(60, lambda: native.KzgSettings(ctx, g1))
    t = time.perf_counter()
    cs = step(60, lambda: native.KzgCellSettings(settings))
    cold = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    again = step(60, lambda: native.KzgCellSettings(settings))
    out = {"settings": {"create_cold_ms": round(cold, 3), "create_again_ms": round((time.perf_counter() - t) * 1e3, 3), "bytes": cs.nbytes,
                        "split_ms_serial": step(60, lambda: split_of(ctx, lambda: native.KzgCellSettings(settings).free()))}, "blobs": {}}
    again.free()
    rng = random.Random(24)
    evals = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(32 * 4096)), np.uint8).reshape(32, 131072)
    coeffs0 = step(60, lambda: native.kzg_blob_coefficients(ctx, np.ascontiguousarray(evals[:1])))[0]
    p0 = [int.from_bytes(row.tobytes(), "little") for row in coeffs0]
    rows0 = np.frombuffer(b"".join(c.to_bytes(32, "little") for q in cm.quotients(p0) for c in q), np.uint8).reshape(128, 4032, 32)
    filler = np.random.default_rng(7594).integers(0, 256, size=(31 * 128, 4032, 32), dtype=np.uint8)
    filler[:, :, 31] &= 0x3F  # below 2^254 < r
    rows = np.concatenate([rows0, filler])
    del filler
    for n in (1, 4, 32):
        ev = np.ascontiguousarray(evals[:n])
        quotient_rows = np.ascontiguousarray(rows[:128 * n])
        proofs = step(60, lambda: cs.cell_proofs_blobs(ev))
        base = step(120, lambda: settings.commit(quotient_rows, 4032))
        assert base[:128].tobytes() == proofs[0].tobytes()
        cells, again = step(60, lambda: cs.cell_proofs_blobs(ev, cells=True))
        assert again.tobytes() == proofs.tobytes() and cells[:, :64].tobytes() == ev.tobytes()
        leg = {"cell_proofs": step(120, lambda: timed(lambda: cs.cell_proofs_blobs(ev))),
               "cell_proofs_with_cells": step(120, lambda: timed(lambda: cs.cell_proofs_blobs(ev, cells=True))),
               "cells": step(60, lambda: timed(lambda: native.kzg_cells_blobs(ctx, ev))),
               "baseline_commit_of_quotients": step(240, lambda: timed(lambda: settings.commit(quotient_rows, 4032))),
               "split_ms_serial": {"cell_proofs_with_cells": step(60, lambda: split_of(ctx, lambda: cs.cell_proofs_blobs(ev, cells=True))),
                                   "baseline_commit_of_quotients": step(120, lambda: split_of(ctx, lambda: settings.commit(quotient_rows, 4032)))}}
        leg["baseline_over_cell_proofs"] = round(leg["baseline_commit_of_quotients"]["median_ms"] / leg["cell_proofs"]["median_ms"], 2)
        leg["faster_than_baseline"] = leg["cell_proofs"]["median_ms"] < leg["baseline_commit_of_quotients"]["median_ms"]
        out["blobs"][str(n)] = leg
        print(n, json.dumps(leg), flush=True)
    pts = np.ascontiguousarray(np.frombuffer(g1, np.uint8)[:64 * 128 * 48])
    out["g1_fft"] = {"1x128": step(60, lambda: timed(lambda: native.kzg_g1_fft(ctx, pts[:128 * 48], 128))),
                     "64x128": step(60, lambda: timed(lambda: native.kzg_g1_fft(ctx, pts, 128))),
                     "1x128_inverse": step(60, lambda: timed(lambda: native.kzg_g1_fft(ctx, pts[:128 * 48], 128, inverse=True))),
                     "split_ms_serial_1x128": step(60, lambda: split_of(ctx, lambda: native.kzg_g1_fft(ctx, pts[:128 * 48], 128))),
                     "split_ms_serial_64x128": step(60, lambda: split_of(ctx, lambda: native.kzg_g1_fft(ctx, pts, 128)))}
    print("g1_fft", json.dumps(out["g1_fft"]), flush=True)
    cs.free()
    settings.free()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
