"""EIP-7594 cell-proof verification (zkw_kzg_verify_cells, zkw_kzg_commit_cells) measured on one MI355X beside the yardstick it is built
from, zkw_kzg_verify on the same number of claims in the same process -> profiles/r29/kzg_cell_verify.json.

    python tools/probe_kzg_cell_verify.py [--out profiles/r29/kzg_cell_verify.json]

The method of tools/probe_kzg_recover.py: one process, one context; every step that uses the GPU runs under a time limit of its own
(SIGALRM with its default action: the process ends even inside a library call) and the first failure ends the probe: nothing is started on
the GPU after it. The setup is one whose tau is known (tests/kzg_open_model.py: known_tau_setup), because a verifier needs [tau^64] G2 and
the fixtures hold the ceremony's [tau] G2 only; the kernels do the same work on any setup. 32 blobs of full-range random elements
(random.Random(29), every element below r), their commitments by zkw_kzg_commit_blobs, cells and proofs by zkw_kzg_cell_proofs_blobs; a
call takes all 128 cells of 1 / 4 / 32 blobs: 128 / 512 / 4 096 claims. Host pointer mode, wall clock around the synchronised call, one
untimed call, then five: median, min, max.

  verify_cells    zkw_kzg_verify_cells; before anything is timed every verdict is 1, and 0 for the claims whose proofs are exchanged
  commit_cells    zkw_kzg_commit_cells on the same cells (the interpolation and the sums alone, with their one readback)
  yardstick       zkw_kzg_verify on the same verifier and as many claims (the same commitments and proofs, z = c_k, y = 0: false claims,
                  which cost what true ones cost)
  split           ONE further call of each under zkw_profile (HIP events around every launch): what each kernel costs alone
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

TAU = 0x4844


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29", "kzg_cell_verify.json"))
    args = ap.parse_args()
    from era_zkevm_test_harness_amd import native
    from tests import kzg_cells_model as cm
    from tests import kzg_model as km
    from tests import kzg_open_model as om
    from tests import kzg_pairing_model as pm

    g1 = b"".join(km.compress(p) for p in om.known_tau_setup(TAU, 4096))
    ctx = native.Context(0)
    settings = step(60, lambda: native.KzgSettings(ctx, g1))
    short = step(60, lambda: native.KzgSettings(ctx, g1[:64 * 48]))
    cs = step(60, lambda: native.KzgCellSettings(settings))
    v64 = step(60, lambda: native.KzgVerifier(ctx, pm.g2_compress(pm.g2_mul(pow(TAU, 64, R), pm.G2_GEN))))
    rng = random.Random(29)
    evals = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(32 * 4096)), np.uint8).reshape(32, 131072)
    commitments = step(60, lambda: settings.commit_blobs(evals))
    cells, proofs = step(240, lambda: cs.cell_proofs_blobs(evals, cells=True))
    c_k = np.frombuffer(b"".join(cm.cell_constant(k).to_bytes(32, "little") for k in range(128)), np.uint8).reshape(128, 32)
    out = {"tau": TAU, "settings_bytes": settings.nbytes, "settings_of_64_points_bytes": short.nbytes, "claims": {}}
    for n in (1, 4, 32):
        claims = 128 * n
        cm_ = np.ascontiguousarray(np.repeat(commitments[:n], 128, axis=0))
        idx = np.tile(np.arange(128, dtype=np.uint64), n)
        ce = np.ascontiguousarray(cells[:n]).reshape(claims, 2048)
        pr = np.ascontiguousarray(proofs[:n]).reshape(claims, 48)
        got = step(60, lambda: v64.verify_cells(settings, cm_, idx, ce, pr))
        assert got.tolist() == [1] * claims, got.tolist()
        assert step(60, lambda: v64.verify_cells(short, cm_, idx, ce, pr)).tolist() == [1] * claims  # settings of exactly 64 points
        swapped = pr.copy()
        swapped[[0, claims - 1]] = swapped[[claims - 1, 0]]
        want = [0] + [1] * (claims - 2) + [0]
        assert step(60, lambda: v64.verify_cells(settings, cm_, idx, ce, swapped)).tolist() == want
        zs, ys = np.ascontiguousarray(np.tile(c_k, (n, 1))), np.zeros((claims, 32), np.uint8)
        leg = {"verify_cells": step(120, lambda: timed(lambda: v64.verify_cells(settings, cm_, idx, ce, pr))),
               "commit_cells": step(120, lambda: timed(lambda: settings.commit_cells(idx, ce))),
               "yardstick_verify": step(120, lambda: timed(lambda: v64.verify(cm_, zs, ys, pr))),
               "split_ms_serial": {"verify_cells": step(60, lambda: split_of(ctx, lambda: v64.verify_cells(settings, cm_, idx, ce, pr))),
                                   "commit_cells": step(60, lambda: split_of(ctx, lambda: settings.commit_cells(idx, ce))),
                                   "yardstick_verify": step(60, lambda: split_of(ctx, lambda: v64.verify(cm_, zs, ys, pr)))}}
        leg["verify_cells_minus_yardstick_ms"] = round(leg["verify_cells"]["median_ms"] - leg["yardstick_verify"]["median_ms"], 3)
        out["claims"][str(claims)] = leg
        print(claims, json.dumps(leg), flush=True)
    for h in (v64, cs, short, settings):
        h.free()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
