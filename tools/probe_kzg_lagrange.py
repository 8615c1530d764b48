"""The wide G1 transform and the setup's change of basis (zkw_kzg_g1_fft_wide, zkw_kzg_settings_to_lagrange, _to_monomial) measured on one
MI355X beside two yardsticks taken in the same process -> profiles/r30/kzg_lagrange.json.

    python tools/probe_kzg_lagrange.py [--out profiles/r30/kzg_lagrange.json]

The method of tools/probe_kzg_cells.py: one process, one context, the ceremony's points (tests/golden; 16 copies of them where a call takes
65 536). Every step that uses the GPU runs under a time limit of its own (SIGALRM with its default action: the process ends even inside a
library call) and the first failure ends the probe: nothing is started on the GPU after it. Host pointer mode, wall clock around the
synchronised call, one untimed call, then five: median, min, max.

  g1_fft_wide     zkw_kzg_g1_fft_wide at 1 x 256, 1 x 1 024, 1 x 4 096 and 16 x 4 096 (decompression and compression included), forward and
                  inverse, and ONE further call each under zkw_profile (HIP events around every launch): what each kernel costs alone
  settings        zkw_kzg_settings_to_lagrange and _to_monomial at 4 096 points, their split, and the fixture's bytes checked
  yardsticks      zkw_kzg_g1_fft on 32 transforms of 128 points (as many points as one transform of 4 096) and zkw_kzg_settings_create on
                  4 096 points
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30", "kzg_lagrange.json"))
    args = ap.parse_args()
    from era_zkevm_test_harness_amd import native

    golden = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(golden, "kzg_trusted_setup_g1.bin"), "rb").read()
    fixture = open(os.path.join(golden, "kzg_trusted_setup_g1_lagrange.bin"), "rb").read()
    ctx = native.Context(0)
    pts = np.ascontiguousarray(np.tile(np.frombuffer(g1, np.uint8), 16))
    out = {"g1_fft_wide": {}, "settings": {}, "yardsticks": {}}
    for n_ffts, n in ((1, 256), (1, 1024), (1, 4096), (16, 4096)):
        src = pts[:n_ffts * n * 48]
        leg = {"forward": step(120, lambda: timed(lambda: native.kzg_g1_fft_wide(ctx, src, n))),
               "inverse": step(120, lambda: timed(lambda: native.kzg_g1_fft_wide(ctx, src, n, inverse=True))),
               "split_ms_serial_forward": step(60, lambda: split_of(ctx, lambda: native.kzg_g1_fft_wide(ctx, src, n))),
               "split_ms_serial_inverse": step(60, lambda: split_of(ctx, lambda: native.kzg_g1_fft_wide(ctx, src, n, inverse=True)))}
        out["g1_fft_wide"]["%dx%d" % (n_ffts, n)] = leg
        print(n_ffts, n, json.dumps(leg), flush=True)
    t = time.perf_counter()
    settings = step(60, lambda: native.KzgSettings(ctx, g1))
    out["yardsticks"]["settings_create_4096_first_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    out["yardsticks"]["settings_create_4096"] = step(120, lambda: timed(lambda: native.KzgSettings(ctx, g1).free()))
    out["yardsticks"]["g1_fft_32x128"] = step(60, lambda: timed(lambda: native.kzg_g1_fft(ctx, pts[:4096 * 48], 128)))
    out["yardsticks"]["g1_fft_32x128_inverse"] = step(60, lambda: timed(lambda: native.kzg_g1_fft(ctx, pts[:4096 * 48], 128, inverse=True)))
    lag = step(60, lambda: settings.to_lagrange())
    assert step(60, lambda: lag.points()).tobytes() == fixture
    back = step(60, lambda: lag.to_monomial())
    assert step(60, lambda: back.points()).tobytes() == g1
    back.free()
    out["settings"] = {"to_lagrange_4096": step(120, lambda: timed(lambda: settings.to_lagrange().free())),
                       "to_monomial_4096": step(120, lambda: timed(lambda: lag.to_monomial().free())),
                       "points_4096": step(60, lambda: timed(lambda: lag.points())),
                       "split_ms_serial_to_lagrange": step(60, lambda: split_of(ctx, lambda: settings.to_lagrange().free())),
                       "split_ms_serial_to_monomial": step(60, lambda: split_of(ctx, lambda: lag.to_monomial().free())),
                       "bytes": lag.nbytes, "equals_fixture": True}
    print("settings", json.dumps(out["settings"]), json.dumps(out["yardsticks"]), flush=True)
    lag.free()
    settings.free()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
