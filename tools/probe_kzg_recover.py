"""EIP-7594 recovery (zkw_kzg_recover_cells_blobs) measured on one MI355X beside the unchanged calls it ends in, zkw_kzg_cells_blobs and
zkw_kzg_cell_proofs_blobs, on the recovered blobs -> profiles/r25/kzg_recover.json.

    python tools/probe_kzg_recover.py [--out profiles/r25/kzg_recover.json]

The method of tools/probe_kzg_cells.py: one process, one context, the ceremony's settings (tests/golden), 32 blobs of full-range random
elements (random.Random(25), every element below r). Every step that uses the GPU runs under a time limit of its own (SIGALRM with its
default action: the process ends even inside a library call) and the first failure ends the probe: nothing is started on the GPU after it.
Host pointer mode, wall clock around the synchronised call, one untimed call, then five: median, min, max, at 1 / 4 / 32 blobs per call.

  recover         zkw_kzg_recover_cells_blobs from a seeded random 64 of the 128 cells and from 127 of them, without proofs and with them;
                  every result is checked against zkw_kzg_cells_blobs / zkw_kzg_cell_proofs_blobs of the blob before anything is timed
  yardsticks      zkw_kzg_cells_blobs and zkw_kzg_cell_proofs_blobs (with cells) on the same blobs, in the same process
  split           ONE further call of each form under zkw_profile (HIP events around every launch): what each kernel costs alone
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.probe_kzg_cells import R, split_of, step, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25", "kzg_recover.json"))
    args = ap.parse_args()
    from era_zkevm_test_harness_amd import native

    g1 = open(os.path.join(ROOT, "tests", "golden", "kzg_trusted_setup_g1.bin"), "rb").read()
    ctx = native.Context(0)
    settings = step(60, lambda: native.KzgSettings(ctx, g1))
    cs = step(60, lambda: native.KzgCellSettings(settings))
    rng = random.Random(25)
    evals = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(32 * 4096)), np.uint8).reshape(32, 131072)
    sets = {"random_64": sorted(rng.sample(range(128), 64)), "127_cells": [k for k in range(128) if k != 77]}
    out = {"cell_indices": sets, "blobs": {}}
    for n in (1, 4, 32):
        ev = np.ascontiguousarray(evals[:n])
        cells, proofs = step(120, lambda: cs.cell_proofs_blobs(ev, cells=True))
        assert cells[:, :64].tobytes() == ev.tobytes()
        leg = {"yardstick_cells": step(60, lambda: timed(lambda: native.kzg_cells_blobs(ctx, ev))),
               "yardstick_cell_proofs_with_cells": step(240, lambda: timed(lambda: cs.cell_proofs_blobs(ev, cells=True))), "split_ms_serial": {}}
        leg["split_ms_serial"]["yardstick_cells"] = step(60, lambda: split_of(ctx, lambda: native.kzg_cells_blobs(ctx, ev)))
        for name, idx in sets.items():
            supplied = np.ascontiguousarray(cells[:, idx])
            got = step(60, lambda: native.kzg_recover_cells(ctx, idx, supplied))
            assert got.tobytes() == cells.tobytes()
            got, got_proofs = step(120, lambda: cs.recover_cells_and_proofs(idx, supplied))
            assert got.tobytes() == cells.tobytes() and got_proofs.tobytes() == proofs.tobytes()
            leg["recover_" + name] = step(60, lambda: timed(lambda: native.kzg_recover_cells(ctx, idx, supplied)))
            leg["recover_with_proofs_" + name] = step(240, lambda: timed(lambda: cs.recover_cells_and_proofs(idx, supplied)))
            leg["split_ms_serial"]["recover_" + name] = step(60, lambda: split_of(ctx, lambda: native.kzg_recover_cells(ctx, idx, supplied)))
            leg["recover_%s_over_cells" % name] = round(leg["recover_" + name]["median_ms"] / leg["yardstick_cells"]["median_ms"], 2)
            leg["recover_with_proofs_%s_minus_cell_proofs_ms" % name] = round(
                leg["recover_with_proofs_" + name]["median_ms"] - leg["yardstick_cell_proofs_with_cells"]["median_ms"], 3)
        leg["split_ms_serial"]["recover_with_proofs_random_64"] = step(
            120, lambda: split_of(ctx, lambda: cs.recover_cells_and_proofs(sets["random_64"], np.ascontiguousarray(cells[:, sets["random_64"]]))))
        out["blobs"][str(n)] = leg
        print(n, json.dumps(leg), flush=True)
    cs.free()
    settings.free()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
