"""Row A takes the grand-product accumulators from 64-cycle checkpoints that the builder pass leaves behind
(`ZKW_RAM_GP_CKPT`) and finishes the scan inside its wave; the synthesis call no longer recomputes the chains. The
smallest shapes at which the wave scan or the checkpoints can go wrong. Every case compares every cell of every trace
with `oracle.ram_synthesize` and requires 0 violations from the GPU checker; the accessor test compares the checkpoints
themselves with what the whole chains and the instances' FSM inputs give by definition."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from era_zkevm_test_harness_amd import synthetic
from era_zkevm_test_harness_amd.ram_circuit import min_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


def _queue(n, seed, heap_writes=2):
    """a consistent memory queue whose first items are nondeterministic heap writes (as tests/test_gpu_ram_fill_fused.py)"""
    q = synthetic.ram_trace(n, seed=seed, pages=3, indices=16)
    k = min(n, heap_writes)
    q["page"][:k] = 10
    q["index"][:k] = 1000 + np.arange(k)
    q["timestamp"][:k] = 0
    q["rw_flag"][:k] = 1
    q["value_is_pointer"][:k] = 0
    mem = {}
    for rec in q:
        key = (int(rec["page"]), int(rec["index"]))
        if rec["rw_flag"]:
            mem[key] = (rec["value"].copy(), rec["value_is_pointer"])
        elif key in mem:
            rec["value"], rec["value_is_pointer"] = mem[key]
        else:
            rec["value"], rec["value_is_pointer"] = 0, 0
    return q


def _rows(capacity):
    n = 256
    while n < min_rows(capacity):
        n *= 2
    return n


def _assert_equal(got, exp, what):
    if not np.array_equal(got, exp):
        cols, rows = np.nonzero(got != exp)
        raise AssertionError(f"{what}: {cols.size} cells differ, first at col {cols[0]} row {rows[0]}: "
                             f"{got[cols[0], rows[0]]} vs {exp[cols[0], rows[0]]}")


def _build(ctx, sizes, seed, capacity):
    qs = [_queue(n, seed=seed + b) for b, n in enumerate(sizes)]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    if len(sizes) == 1:
        w = ctx.compute_ram_circuit_snapshots(qs[0], capacity, 2)
    else:
        w = ctx.compute_ram_circuit_snapshots(np.concatenate(qs), capacity, 2, block_offsets=offs)
    return qs, offs, w


def _run_case(ctx, oracle, sizes, seed, capacity, calls, n_slots, what):
    """one builder pass over the blocks `sizes`; `calls` = (first instance, instances, first slot) of each synthesis call,
    which together cover every instance once; every trace against the oracle's, the GPU checker on every slot"""
    from era_zkevm_test_harness_amd import native

    n_rows = _rows(capacity)
    qs, _, w = _build(ctx, sizes, seed, capacity)
    exp = []
    for q in qs:
        o = oracle.ram_build_instances(q, capacity, 2)
        exp += [oracle.ram_synthesize(o, i, capacity, n_rows) for i in range(o["instances"].size)]
    assert w.num_instances == len(exp) == sum(-(-n // capacity) for n in sizes) <= n_slots
    t = native.Trace(ctx, n_rows, n_slots)
    slot_of = {}
    for first, n, first_slot in calls:
        ctx.synthesize_ram(w, t, first, n, first_slot)
        for k in range(n):
            slot_of[first + k] = (first_slot + k) % n_slots
    assert sorted(slot_of) == list(range(len(exp))) and len(set(slot_of.values())) == len(exp)
    for k, e in enumerate(exp):
        _assert_equal(t.get(slot_of[k]), e, f"{what}, instance {k}")
        bad, first = ctx.check_if_satisfied_ram(t, slot_of[k], capacity)
        assert bad == 0, (what, k, first)
    t.free()
    w.free()


THREE_BLOCKS = [130, 70, 210]  # 2 + 1 + 3 instances at capacity 100
# one call that starts at instance 1, inside block 0, and wraps the ring of 6 slots (4, 5, 0, 1, 2); instance 0 on its own into slot 3
THREE_BLOCKS_CALLS = [(1, 5, 4), (0, 1, 3)]

# (blocks, capacity, calls, slots)
CASES = {
    # one partial wave: lanes 37..63 are gap lanes that sit inside the scan; 3 instances, the last with 6 items
    "capacity_37": ([80], 37, [(0, 3, 0)], 3),
    # the last live lane of a wave is the instance's last item: nothing pads
    "capacity_64_full": ([64], 64, [(0, 1, 0)], 1),
    # ... then a second instance that pops one item: every lane after lane 0 takes the accumulator after that item
    "capacity_64_plus_1": ([65], 64, [(0, 2, 0)], 2),
    # two groups, the second one's checkpoint is the chain after item 63
    "capacity_128_full": ([128], 128, [(0, 1, 0)], 1),
    # ... and a second instance with one item followed by a whole padding group (its checkpoint: the chain at the last popped item)
    "capacity_128_plus_1": ([129], 128, [(0, 2, 0)], 2),
    # continuations whose first_item (100, 200) is no multiple of 64; the last instance is partly filled (50 of 100)
    "ragged": ([250], 100, [(0, 3, 0)], 3),
    # first_instance > 0, a call that starts mid-block, per-job checkpoint offsets, the ring wraps
    "three_blocks_from_instance_1": (THREE_BLOCKS, 100, THREE_BLOCKS_CALLS, 6),
}


@pytest.mark.parametrize("name", list(CASES))
def test_traces_equal_the_oracle(ctx, oracle, name):
    sizes, capacity, calls, n_slots = CASES[name]
    _run_case(ctx, oracle, sizes, 500, capacity, calls, n_slots, name)


CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import test_gpu_ram_gp_checkpoints as m
from era_zkevm_test_harness_amd import native
from oracle import pyoracle
pyoracle.build()
ctx = native.Context(0)
m._run_case(ctx, pyoracle, m.THREE_BLOCKS, 500, 100, m.THREE_BLOCKS_CALLS, 6, "small window")
m._check_checkpoints(ctx, m.THREE_BLOCKS, 500, 100)
ctx.close()
print("RESULT ok")
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_builder_window_smaller_than_the_batch():
    """ZKW_Z_WINDOW_ITEMS is read when a witness is allocated: in a fresh process with a window of one block's size the
    builder goes through blocks {0, 1} and {2} as two groups, so the checkpoints are written group by group, and the
    synthesis call that spans the three blocks is split at the sorted window"""
    env = dict(os.environ)
    env["ZKW_Z_WINDOW_ITEMS"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "RESULT ok" in r.stdout


def _check_checkpoints(ctx, sizes, seed, capacity):
    """ckpt[instance][g] = {lhs r0, lhs r1, rhs r0, rhs r1}: the accumulators entering cycle 64 g = the FSM input for
    g = 0, else the chain value at the last item popped before that cycle"""
    from era_zkevm_test_harness_amd import native

    _, offs, w = _build(ctx, sizes, seed, capacity)
    groups = -(-capacity // 64)
    ck = w.get(native.RAM_GP_CKPT)
    inst = w.get(native.RAM_INSTANCES)
    assert ck.shape == (inst.size, groups, 4)
    lz, rz = w.get(native.RAM_LHS_Z).reshape(-1), w.get(native.RAM_RHS_Z).reshape(-1)
    exp = np.zeros_like(ck)
    k = 0
    for b, n in enumerate(sizes):
        lo = int(offs[b])
        zl, zr = lz[2 * lo:2 * (lo + n)].reshape(2, n), rz[2 * lo:2 * (lo + n)].reshape(2, n)
        for _ in range(-(-n // capacity)):
            rec = inst[k]
            first, m = int(rec["first_item"]), int(rec["num_items"])
            exp[k, 0, 0:2] = rec["hidden_fsm_input"]["lhs_accumulator"]
            exp[k, 0, 2:4] = rec["hidden_fsm_input"]["rhs_accumulator"]
            for g in range(1, groups):
                at = first + min(64 * g - 1, m - 1)
                exp[k, g, 0:2] = zl[:, at]
                exp[k, g, 2:4] = zr[:, at]
            k += 1
    assert k == inst.size
    assert np.array_equal(ck, exp), np.argwhere(ck != exp)[:8]
    w.free()


def test_checkpoint_accessor(ctx):
    _check_checkpoints(ctx, [250], 500, 100)
    _check_checkpoints(ctx, THREE_BLOCKS, 500, 100)
