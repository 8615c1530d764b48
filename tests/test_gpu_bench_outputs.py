"""`bench.py --dump-outputs DIR`: a plain run (no --full) prints the contract's line and writes what its last timed step handed the caller —
the gathered closed-form records and a seeded sample of every ring slot that step wrote — and those arrays are the oracle's for the same
blocks. Two pipelines on a small batch with a ring of 3 slots per pipeline, so that the last pass wraps round its ring (slot -> instance map)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u64(pairs):
    return pairs[..., 0].astype(np.uint64) | (pairs[..., 1].astype(np.uint64) << np.uint64(32))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(tmp_path, oracle):
    out_dir = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ZKW_PIPELINES")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--blocks", "16",
                        "--pipelines", "2", "--ring", "6", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["validation"] is None and line["sensitivity"] is None and "full_block" not in line and "cpu_baseline" not in line

    files = sorted(os.listdir(out_dir))
    assert files == ["closed_form_records.npy", "trace_sample.npy", "trace_sample_cells.npy", "trace_sample_instances.npy"]
    arrays = {f[:-4]: np.load(out_dir / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 << 20
    rec = _u64(arrays["closed_form_records"])
    assert rec.shape == (16, 22)
    # 8 blocks per pipeline, 3 slots: the last pass's last launch wrote instances 6, 7 into slots 0, 1; slot 2 kept instance 5
    assert arrays["trace_sample_instances"].tolist() == [6, 7, 5, 14, 15, 13]
    sample, cells = _u64(arrays["trace_sample"]), arrays["trace_sample_cells"].astype(np.int64)
    assert sample.shape == (6, cells.size)

    sys.path.insert(0, ROOT)
    import bench
    from era_zkevm_test_harness_amd import native

    _base, q = bench.make_inputs(16, bench.CAPACITY, 0, "cpu")
    for blk in (0, 5, 6, 13, 15):  # one instance per block at this capacity: record row = block
        o = oracle.ram_build_instances(q[blk].numpy().reshape(-1).view(native.MEM_QUERY), bench.CAPACITY, 0)
        compact, pi = oracle.ram_public_inputs(o["instances"])
        assert np.array_equal(rec[blk], np.concatenate([compact[0], pi[0]])), blk
        if blk in (6, 13):  # a slot of each pipeline, one of them the wrapped one
            k = arrays["trace_sample_instances"].tolist().index(blk)
            exp = oracle.ram_synthesize(o, 0, bench.CAPACITY, 1 << 20)
            assert np.array_equal(sample[k], exp.reshape(-1)[cells]), blk
