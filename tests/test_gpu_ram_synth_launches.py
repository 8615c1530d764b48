"""A warm `zkw_ram_synthesize` is four launches: the gather, row C, ONE Poseidon2 launch (grid z = the side) and row D, whose
boundary block writes the multiplicity column and clears the histogram. The tile prefixes of row C's counter are the builder's
(`ZKW_RAM_ND_PREFIX`), and a call of up to 32 instances carries its job table in the kernels' arguments. The smallest shapes at
which each of these can go wrong. Every case compares every cell of every trace with `oracle.ram_synthesize` and requires
0 violations from the GPU checker."""
import numpy as np
import pytest

from era_zkevm_test_harness_amd import synthetic
from era_zkevm_test_harness_amd.ram_circuit import min_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


def _queue(n, seed, heap_writes):
    """a consistent memory queue with `heap_writes` nondeterministic heap writes (timestamp 0, page 10, distinct cells), spread over
    the queue's positions (as tests/test_gpu_ram_gp_checkpoints.py, which puts two of them first)"""
    q = synthetic.ram_trace(n, seed=seed, pages=3, indices=16)
    k = min(n, heap_writes)
    at = np.random.default_rng(seed).permutation(n)[:k]
    q["page"][at] = 10
    q["index"][at] = 1000 + np.arange(k)
    q["timestamp"][at] = 0
    q["rw_flag"][at] = 1
    q["value_is_pointer"][at] = 0
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


def nd_flags(sorted_q):
    """the circuit's nondeterministic-write flag of every item of a sorted queue"""
    return ((sorted_q["timestamp"] == 0) & (sorted_q["page"] == 10) & (sorted_q["rw_flag"] != 0) & (sorted_q["value_is_pointer"] == 0))


def nd_prefix_of(sorted_q, capacity):
    """[instances][ceil(capacity / 256)]: the flags of the instance's cycles before each tile of 256 cycles"""
    f = nd_flags(sorted_q).astype(np.int64)
    tiles = -(-capacity // 256)
    out = []
    for lo in range(0, f.size, capacity):
        c = np.zeros(tiles * 256, np.int64)
        m = min(capacity, f.size - lo)
        c[:m] = f[lo:lo + m]
        per_tile = c.reshape(tiles, 256).sum(axis=1)
        out.append(np.concatenate([[0], np.cumsum(per_tile)[:-1]]))
    return np.array(out, np.uint32).reshape(-1, tiles)


class Case:
    """one builder pass over the blocks `sizes` and the oracle's traces of every instance, computed once"""

    def __init__(self, ctx, oracle, sizes, seed, capacity, heap_writes, n_rows=None):
        self.capacity, self.n_rows = capacity, n_rows or _rows(capacity)
        self.qs = [_queue(n, seed + b, heap_writes) for b, n in enumerate(sizes)]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        if len(sizes) == 1:
            self.w = ctx.compute_ram_circuit_snapshots(self.qs[0], capacity, 2)
        else:
            self.w = ctx.compute_ram_circuit_snapshots(np.concatenate(self.qs), capacity, 2, block_offsets=offs)
        self.o = [oracle.ram_build_instances(q, capacity, 2) for q in self.qs]
        self.exp = []
        for o in self.o:
            self.exp += [oracle.ram_synthesize(o, i, capacity, self.n_rows) for i in range(o["instances"].size)]
        assert self.w.num_instances == len(self.exp)

    def check(self, ctx, t, instance, slot, what):
        _assert_equal(t.get(slot), self.exp[instance], f"{what}, instance {instance} in slot {slot}")
        bad, first = ctx.check_if_satisfied_ram(t, slot, self.capacity)
        assert bad == 0, (what, instance, first)

    def run(self, ctx, calls, n_slots, what):
        """`calls` = (first instance, instances, first slot); the traces are compared after the last call"""
        from era_zkevm_test_harness_amd import native

        t = native.Trace(ctx, self.n_rows, n_slots)
        slot_of = {}
        for first, n, first_slot in calls:
            ctx.synthesize_ram(self.w, t, first, n, first_slot)
            for k in range(n):
                slot_of[first + k] = (first_slot + k) % n_slots
        assert sorted(slot_of) == list(range(len(self.exp))) and len(set(slot_of.values())) == len(self.exp)
        for k in range(len(self.exp)):
            self.check(ctx, t, k, slot_of[k], what)
        t.free()

    def free(self):
        self.w.free()


# ------------------------------------------------------------------------------------------------ the builder's tile prefixes, row C's counters
# (blocks, capacity): one block of 2 x capacity + 37 items, and a batch of two blocks of unequal size; capacity 300 = two tiles, the
# second partial (44 cycles), capacity 256 = one full tile. 30 % of the items are nondeterministic writes.
PREFIX_CASES = {
    "capacity_300_one_block": ([637], 300),
    "capacity_256_one_block": ([549], 256),
    "capacity_300_two_blocks": ([637, 350], 300),
    "capacity_256_two_blocks": ([549, 300], 256),
}


@pytest.mark.parametrize("name", list(PREFIX_CASES))
def test_nd_prefix_and_row_c_counters(ctx, oracle, name):
    from era_zkevm_test_harness_amd import native

    sizes, capacity = PREFIX_CASES[name]
    c = Case(ctx, oracle, sizes, 900, capacity, heap_writes=sizes[0] * 3 // 10)
    # what the case is for, asserted on the oracle's side: in the first block the writes fall into at least two instances, one of them
    # with a nonzero count entering it, and (two tiles) into both tiles of one instance
    exp = np.concatenate([nd_prefix_of(o["sorted_q"], capacity) for o in c.o])
    f0 = nd_flags(c.o[0]["sorted_q"])
    per_inst = [int(f0[lo:lo + capacity].sum()) for lo in range(0, f0.size, capacity)]
    assert sum(1 for x in per_inst if x) >= 2, per_inst
    assert any(int(r["hidden_fsm_input"]["num_nondeterministic_writes"]) > 0 for r in c.o[0]["instances"])
    if capacity > 256:
        assert any(f0[lo:lo + 256].any() and f0[lo + 256:lo + capacity].any() for lo in range(0, f0.size, capacity)), "both tiles of one instance"
    got = c.w.get(native.RAM_ND_PREFIX)
    assert got.dtype == np.uint32 and got.shape == exp.shape == (len(c.exp), -(-capacity // 256))
    assert np.array_equal(got, exp), (got, exp)
    # RC_C_P_cnt / RC_C_cnt of every cycle (and the rest of every trace); one call over every block
    c.run(ctx, [(0, len(c.exp), 0)], len(c.exp), name)
    c.free()


# ------------------------------------------------------------------------------------------------ both Poseidon2 regions in one launch
# capacity 64: the region stride is the capacity, one full group per side; 65: stride 128, a second group of one live cycle and 63 gap
# rows; 300: four full groups and a partial one. The last instance of each is padded.
MERGED_CASES = {"capacity_64": ([100], 64), "capacity_65": ([100], 65), "capacity_300": ([450], 300)}


@pytest.mark.parametrize("name", list(MERGED_CASES))
def test_merged_poseidon_launch(ctx, oracle, name):
    sizes, capacity = MERGED_CASES[name]
    c = Case(ctx, oracle, sizes, 910, capacity, heap_writes=5)
    assert int(c.o[0]["instances"][-1]["num_items"]) < capacity  # padded
    c.run(ctx, [(0, len(c.exp), 0)], len(c.exp), name)
    c.free()


# ------------------------------------------------------------------------------------------------ the histogram is zero between calls
def test_histogram_is_cleared_by_the_call_that_reads_it(ctx, oracle):
    """three calls in a row into the same two slots with different instances, a call with one slot's tag forgotten among clean ones
    (the cold path: the tail launch), a warm call again: the multiplicity column, and every other cell, after each"""
    from era_zkevm_test_harness_amd import native

    c = Case(ctx, oracle, [64 * 7 + 20], 920, 64, heap_writes=9)
    assert len(c.exp) == 8
    t = native.Trace(ctx, c.n_rows, 2)
    for first in (0, 2, 4):
        ctx.synthesize_ram(c.w, t, first, 2, 0)
        for k in range(2):
            c.check(ctx, t, first + k, k, f"warm call at {first}")
    assert t.device_ptr(1)  # the caller may have written through it: slot 1 is not clean any more, slot 0 is
    ctx.synthesize_ram(c.w, t, 6, 2, 0)
    for k in range(2):
        c.check(ctx, t, 6 + k, k, "one cold slot among clean ones")
    ctx.synthesize_ram(c.w, t, 3, 2, 0)
    for k in range(2):
        c.check(ctx, t, 3 + k, k, "warm again")
    t.free()
    c.free()


# ------------------------------------------------------------------------------------------------ the job table
@pytest.fixture(scope="module")
def case_33(ctx, oracle):
    c = Case(ctx, oracle, [33 * 64], 930, 64, heap_writes=40, n_rows=1024)
    assert len(c.exp) == 33
    yield c
    c.free()


@pytest.mark.parametrize("calls", [[(0, 33, 0)], [(0, 32, 0), (32, 1, 32)]], ids=["33_uploaded", "32_inline_then_1"])
def test_job_table_inline_and_uploaded(ctx, case_33, calls):
    """32 jobs travel in the kernels' arguments, 33 as an uploaded table"""
    case_33.run(ctx, calls, 33, str(calls))


def test_inline_job_table_in_a_call_split_at_the_sorted_window(ctx, oracle, monkeypatch):
    """ZKW_Z_WINDOW_ITEMS is read when a witness is allocated: with a sorted window of one block's size the call over three blocks
    is split at block boundaries into three calls, each with its own table"""
    monkeypatch.setenv("ZKW_Z_WINDOW_ITEMS", "1")
    c = Case(ctx, oracle, [130, 70, 210], 940, 64, heap_writes=12)
    monkeypatch.delenv("ZKW_Z_WINDOW_ITEMS")
    assert len(c.exp) == 3 + 2 + 4
    c.run(ctx, [(0, 9, 0)], 9, "split at the sorted window")
    c.free()


# ------------------------------------------------------------------------------------------------ the batched path
def test_blocks_synthesize_ram_traces_equal_the_oracle(ctx, oracle):
    """zkw_blocks_run + zkw_blocks_synthesize (the blocks' contexts belong to a batch: merged launches, the job tables in the upload
    arena): the RAM traces handed out are the oracle's over each block's whole memory queue"""
    import threading

    from era_zkevm_test_harness_amd import block as blk, native as nv

    caps = {blk.DECOMMITS_SORTER: 5, blk.CODE_DECOMMITTER: 7, blk.LOG_DEMUXER: 64, blk.KECCAK256: 3, blk.SHA256: 4, blk.ECRECOVER: 2,
            blk.RAM_PERMUTATION: 1000, blk.STORAGE_SORTER: 40, blk.EVENTS_SORTER: 16, blk.L1_MESSAGES_SORTER: 9, blk.L1_MESSAGES_HASHER: 48}
    bs = [synthetic.block_after_vm(seed=70 + k, n_vm_memory=400 + 700 * k, n_storage=20) for k in range(2)]
    n_rows = 1 << 18
    exp = {}
    for bi, b in enumerate(bs):
        a = blk.create_artifacts_after_vm(ctx, b, caps)
        o = oracle.ram_build_instances(a["memory_queries"], caps[blk.RAM_PERMUTATION], 0)
        for i in range(o["instances"].size):
            exp[(bi, i)] = oracle.ram_synthesize(o, i, caps[blk.RAM_PERMUTATION], n_rows)
        for wit in a["witnesses"].values():
            wit.free()
    assert len(exp) >= 3  # one block with one instance, one with more
    many = nv.Block.run_many(0, bs, caps)
    lib = nv.load()
    cols = next(iter(exp.values())).shape[0]  # the circuit's own columns (a ring is as wide as the widest type)
    seen, lock = [], threading.Lock()

    def cb(bi, t, i, tr, s, pi):
        if t != blk.RAM_PERMUTATION:
            return
        a = np.zeros((cols, n_rows), np.uint64)
        nv._check(lib.zkw_trace_get(tr, s, 0, cols, a.ctypes.data))
        _assert_equal(a, exp[(bi, i)], f"block {bi}, RAM instance {i}")
        with lock:
            seen.append((bi, i))

    nv.Block.synthesize_many(many, n_rows, ring_slots=2, callback=cb)
    assert sorted(seen) == sorted(exp)
    for m in many:
        m.free()
