"""The RAM builder keeps no grand-product chain: a group pass multiplies the factors of every 64 cycles of every instance up and
counts the nondeterministic writes of every tile of 256 cycles, a scan pass per block turns both into `ZKW_RAM_GP_CKPT`,
`ZKW_RAM_ND_PREFIX` and the instances' accumulators and write counts. One batch per capacity, through
`zkw_ram_build_instances_batch`, at the sizes where a group, a tile or an instance ends: the instance records byte for byte
against the oracle's, the checkpoints against the chains that `ZKW_RAM_LHS_Z` / `_RHS_Z` compute on their own, the counts
against numpy."""
import numpy as np
import pytest

from era_zkevm_test_harness_amd import synthetic

pytestmark = pytest.mark.gpu
HEAP_PAGE = 10


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


def nd_targets(n, capacity):
    """sorted positions of a block that must hold a nondeterministic write: cycles 255, 256, 257 and the last cycle of every
    instance (where the instance has them)"""
    at = set()
    for lo in range(0, n, capacity):
        m = min(capacity, n - lo)
        at |= {lo + c for c in (255, 256, 257, m - 1) if c < m}
    return sorted(at)


def queue(n, capacity, seed):
    """A consistent memory queue of n items on the heap page whose SORTED order is known by construction: cells of one to three
    items (a write first, then reads and writes in timestamp order), a new cell at every target position, whose first write gets
    timestamp 0: a nondeterministic write, every other one of them a pointer (the FSM counts those, the circuit does not). Returns
    the queue in timestamp order and the sorted positions of the nondeterministic writes."""
    rng = np.random.default_rng(seed)
    targets = nd_targets(n, capacity)
    start = np.zeros(n, bool)  # the first item of a cell, in sorted order
    start[0] = True
    start[targets] = True
    start |= rng.random(n) < 0.5
    cell = np.cumsum(start) - 1
    s = np.zeros(n, synthetic.MEM_QUERY)
    s["page"] = HEAP_PAGE
    s["index"] = 7 + 3 * cell
    s["rw_flag"] = start | (rng.random(n) < 0.3)
    # timestamps: a random order of the queue in which every cell's items keep their sorted order
    key = rng.random(n)
    for lo in np.flatnonzero(start):
        hi = lo + 1
        while hi < n and not start[hi]:
            hi += 1
        key[lo:hi] = np.sort(key[lo:hi])
    order = np.argsort(key, kind="stable")  # queue position -> sorted position
    s["timestamp"][order] = 1 + np.arange(n, dtype=np.uint32)
    s["timestamp"][targets] = 0
    val = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    ptr = rng.random(n) < 0.2
    ptr[targets] = (np.arange(len(targets)) + seed) % 2 == 1
    for i in range(n):
        if not s["rw_flag"][i]:
            val[i], ptr[i] = val[i - 1], ptr[i - 1]
    s["value"] = val
    s["value_is_pointer"] = ptr
    return s[order], np.array(targets)


def block_sizes(capacity):
    """k x capacity - 1, k x capacity, k x capacity + 1 for k = 1 and 3, a block shorter than one capacity, a block of one item"""
    sizes = [k * capacity + d for k in (1, 3) for d in (-1, 0, 1)] + [max(1, capacity // 2), 1]
    return [n for n in sizes if n > 0]


def stable_sorted(q):
    return q[np.lexsort((q["timestamp"], q["index"], q["page"]))]


@pytest.mark.parametrize("capacity", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_against_oracle_chains_and_counts(ctx, oracle, capacity):
    from era_zkevm_test_harness_amd import native

    sizes = block_sizes(capacity)
    assert len(set(sizes)) >= 3 and len({-(-n // capacity) for n in sizes}) >= 2
    made = [queue(n, capacity, 7000 + 10 * capacity + b) for b, n in enumerate(sizes)]
    qs = [q for q, _ in made]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    w = ctx.compute_ram_circuit_snapshots(np.concatenate(qs), capacity, 2, block_offsets=offs)
    groups, tiles = -(-capacity // 64), -(-capacity // 256)
    n_inst = sum(-(-n // capacity) for n in sizes)
    inst = w.get(native.RAM_INSTANCES)
    ck = w.get(native.RAM_GP_CKPT)
    ndp = w.get(native.RAM_ND_PREFIX)
    assert w.num_instances == inst.size == n_inst
    assert ck.shape == (n_inst, groups, 4) and ndp.shape == (n_inst, tiles) and ndp.dtype == np.uint32

    # the instance records, byte for byte
    exp_inst = [oracle.ram_build_instances(q, capacity, 2)["instances"] for q in qs]
    k = 0
    for b, e in enumerate(exp_inst):
        got = inst[k:k + e.size]
        assert got.tobytes() == e.tobytes(), (capacity, "block", b, [i for i in range(e.size) if got[i].tobytes() != e[i].tobytes()])
        k += e.size
    assert k == n_inst

    # the checkpoints: the chains' values at the cycle before each group (1 before the block's first cycle)
    lz, rz = w.get(native.RAM_LHS_Z).reshape(-1), w.get(native.RAM_RHS_Z).reshape(-1)
    exp_ck = np.zeros_like(ck)
    exp_ndp = np.zeros_like(ndp)
    kinds = set()
    k = 0
    for b, n in enumerate(sizes):
        lo = int(offs[b])
        z = np.concatenate([lz[2 * lo:2 * (lo + n)].reshape(2, n), rz[2 * lo:2 * (lo + n)].reshape(2, n)])  # [4][n]
        sq = stable_sorted(qs[b])
        heap_write = (sq["rw_flag"] != 0) & (sq["timestamp"] == 0) & (sq["page"] == HEAP_PAGE)
        # what the inputs are for: the writes sit where they were put, both kinds of them
        assert np.array_equal(np.flatnonzero(heap_write), made[b][1])
        kinds |= set(sq["value_is_pointer"][heap_write] != 0)
        fsm = heap_write.astype(np.int64)
        circuit = (heap_write & (sq["value_is_pointer"] == 0)).astype(np.int64)
        for first in range(0, n, capacity):
            m = min(capacity, n - first)
            for g in range(groups):
                at = first + min(64 * g, m) - 1  # the last item popped before cycle 64 g
                exp_ck[k, g] = z[:, at] if at >= 0 else 1
            c = np.zeros(tiles * 256, np.int64)
            c[:m] = circuit[first:first + m]
            exp_ndp[k] = np.concatenate([[0], np.cumsum(c.reshape(tiles, 256).sum(axis=1))[:-1]])
            assert int(inst[k]["first_item"]) == first and int(inst[k]["num_items"]) == m
            assert int(inst[k]["hidden_fsm_input"]["num_nondeterministic_writes"]) == fsm[:first].sum()
            assert int(inst[k]["hidden_fsm_output"]["num_nondeterministic_writes"]) == fsm[:first + m].sum()
            k += 1
    assert k == n_inst and kinds == {False, True}
    assert np.array_equal(ck, exp_ck), (capacity, np.argwhere(ck != exp_ck)[:8])
    assert np.array_equal(ndp, exp_ndp), (capacity, np.argwhere(ndp != exp_ndp)[:8])
    w.free()
