"""GPU: zkw_storage_tree_advance_witness / _by_queries (csrc/storage_witness_kernels.cuh, "advance") — the witness tree of the state AFTER
a batch of writes, computed on the device from the witness tree before it — and the flow it is for: ONE table for the slots of K
consecutive blocks, the other K - 1 pre-states derived from it, all blocks in one zkw_blocks_run. The yardsticks are the full device tree
after the same insert, the oracle's sequential tree, the host model of tests/storage_witness_model.py and hashlib's Blake2s; an advanced
table's own output is never one. Every comparison is byte-exact. The world is tests/test_gpu_storage_witness_tree.py's."""
import threading

import numpy as np
import pytest

from era_zkevm_test_harness_amd import synthetic
from tests import storage_witness_model as model
from tests.test_gpu_storage_witness_tree import CAPS, SAP, _dedup_queries, _flip, _rebase_storage, _rows, _sap_record, _storage_keys

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


class _World:
    """1 000 leaves, a table of 270 present + 205 absent keys and the oracle's answers for it in the initial state — computed once, unchanged"""


def _oracle_answers(tree, keys):
    n = len(keys)
    idx, val, paths = np.zeros(n, np.uint64), np.zeros((n, 32), np.uint8), np.zeros((n, 256, 32), np.uint8)
    for i, k in enumerate(keys):
        ix, v, paths[i] = tree.get_leaf(k)
        idx[i], val[i] = ix, np.frombuffer(v, np.uint8)
    return idx, val, paths


@pytest.fixture(scope="module")
def world(oracle):
    from era_zkevm_test_harness_amd import native as nv

    rng = np.random.default_rng(23)
    a, b, c = rng.bytes(32), rng.bytes(32), rng.bytes(32)
    run = [bytes([i]) + c[1:] for i in range(64)]  # 64 keys under one node of height 6
    edge = [bytes(32), b"\xff" * 32, a, _flip(a, 0), b, _flip(b, 255)] + run
    w = _World()
    w.a, w.b, w.run = a, b, run
    # log queries whose derived keys are in the table (15 present, 25 absent) and 20 whose keys are not
    w.q = np.ascontiguousarray(synthetic.storage_application_trace(60, seed=3)[0], dtype=nv.LOG_QUERY)
    w.qkeys = [oracle.derive_final_address(x) for x in w.q]
    w.leaves = [rng.bytes(32) for _ in range(1000 - len(edge) - 15)] + w.qkeys[:15] + edge
    w.values = [rng.bytes(32) for _ in w.leaves]
    w.tree = oracle.Tree()
    for k, v in zip(w.leaves, w.values):
        w.tree.insert_leaf(k, v)
    x, y = rng.bytes(32), rng.bytes(32)
    w.sib0, w.sib255 = [x, _flip(x, 0)], [y, _flip(y, 255)]  # absent pairs: siblings at level 0, and keys that differ in bit 255 only
    neighbours = [_flip(run[0], 6), _flip(run[63], 255), _flip(a, 1), _flip(bytes(32), 0), _flip(b"\xff" * 32, 255)]  # absent, next to present keys
    present = [w.leaves[i] for i in rng.choice(1000 - len(edge) - 15, size=185, replace=False)] + w.qkeys[:15] + edge
    absent = [rng.bytes(32) for _ in range(171)] + w.qkeys[15:40] + w.sib0 + w.sib255 + neighbours
    assert not set(absent) & set(w.leaves)
    w.keys, w.n_present = present + absent, len(present)
    assert (w.n_present, len(absent), len(set(w.keys))) == (270, 205, 475)
    w.idx, w.val, w.paths = _oracle_answers(w.tree, w.keys)
    assert w.idx[:w.n_present].all() and not w.idx[w.n_present:].any()
    for i in (0, w.n_present - 1, w.n_present, len(w.keys) - 1):  # the table's entries are proofs, by hashlib alone
        assert model.fold(w.keys[i], w.idx[i], w.val[i].tobytes(), w.paths[i]) == w.tree.root
    w.model = model.Table(w.keys, w.idx, w.val, w.paths, w.tree.root, w.tree.next_enumeration_index)
    w.order = [w.keys[i] for i in rng.permutation(len(w.keys))]  # the order the tables are asked in
    w.outside = [rng.bytes(32), _flip(w.keys[0], 3)]
    assert not set(w.outside) & set(w.keys) and not set(w.qkeys[40:]) & set(w.keys)
    for arr in (w.idx, w.val, w.paths):
        arr.setflags(write=False)
    return w


def _fresh(nv, ctx, oracle, w, capacity=1280):
    """the world's tree once more on both sides, for a test that writes"""
    tree = oracle.Tree()
    for k, v in zip(w.leaves, w.values):
        tree.insert_leaf(k, v)
    t = nv.StorageTreeDevice(ctx, capacity)
    t.insert(_rows(w.leaves), _rows(w.values))
    assert t.root == tree.root == w.tree.root
    return tree, t


def _extracted(nv, ctx, w):
    t = nv.StorageTreeDevice(ctx, 1024)
    t.insert(_rows(w.leaves), _rows(w.values))
    wt = t.extract_witness(w.keys)
    t.free()
    return wt


def _from_proofs(nv, ctx, tree, keys):
    idx, val, paths = _oracle_answers(tree, keys)
    return nv.StorageTreeDevice.from_proofs(ctx, _rows(keys) if keys else np.zeros((0, 32), np.uint8), idx, val, paths, tree.root, tree.next_enumeration_index)


def _same(got, want, what=""):
    for k, (g, x) in enumerate(zip(got, want)):
        assert np.asarray(g).tobytes() == np.asarray(x).tobytes(), (what, ("index", "value", "paths")[k])


def _is_state_of(wt, keys, t, tree, m=None):
    """the witness tree answers `keys` as the full device tree, the oracle's tree and (if given) the host model do, and describes their state"""
    got = wt.get_leaves(keys)
    _same(got, t.get_leaves(keys), "full device tree")
    _same(got, _oracle_answers(tree, keys), "oracle")
    assert wt.is_witness and wt.root == t.root == tree.root
    assert wt.next_enumeration_index == t.next_enumeration_index == tree.next_enumeration_index
    if m is not None:
        _same(got, m.answers(keys), "host model")
        assert (wt.root, wt.next_enumeration_index, wt.num_leaves) == (m.root, m.next_enumeration_index, m.num_leaves)
    return got


def _insert(t, tree, pairs):
    t.insert(_rows([k for k, _ in pairs]), _rows([v for _, v in pairs]))
    for k, v in pairs:
        tree.insert_leaf(k, v)


def _advance(wt, pairs):
    return wt.advance(_rows([k for k, _ in pairs]), _rows([v for _, v in pairs]))


def test_parity_over_a_chain(ctx, world, oracle):
    """three batches, each applied to the previous OUTPUT"""
    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(5)
    tree, t = _fresh(nv, ctx, oracle, w)
    present, absent = w.keys[:w.n_present], w.keys[w.n_present:]
    wt, m = t.extract_witness(w.keys), w.model
    # 1: rewrites of present keys, one of them three times
    b1 = [(present[i], rng.bytes(32)) for i in rng.choice(w.n_present, size=40, replace=False)]
    thrice = present[77]
    b1[3:3], b1[20:20] = [(thrice, rng.bytes(32))], [(thrice, rng.bytes(32))]
    b1.append((thrice, rng.bytes(32)))
    # 2: inserts of absent table keys — siblings at level 0, a pair that differs in bit 255 only, one key three times, a zero value — between rewrites
    b2 = [(absent[i], rng.bytes(32)) for i in rng.choice(171, size=30, replace=False)]
    b2[4:4] = [(w.sib0[1], rng.bytes(32)), (present[5], rng.bytes(32)), (w.sib255[0], rng.bytes(32))]
    b2[15:15] = [(absent[180], rng.bytes(32)), (w.sib0[0], rng.bytes(32)), (absent[180], rng.bytes(32))]
    b2 += [(absent[200], bytes(32)), (w.sib255[1], rng.bytes(32)), (absent[180], rng.bytes(32)), (present[200], rng.bytes(32))]
    # 3: the query form, reads mixed in, present and absent slots
    q3 = w.q[:40][rng.permutation(40)].copy()
    assert 0 < int(q3["rw_flag"].sum()) < 40
    written = set()
    for batch in (b1, b2, q3):
        n_before, next_before = wt.num_leaves, wt.next_enumeration_index
        if isinstance(batch, list):
            pairs = batch
            new = _advance(wt, pairs)
            t.insert(_rows([k for k, _ in pairs]), _rows([v for _, v in pairs]))
        else:
            pairs = [(oracle.derive_final_address(x), model.written_value(x)) for x in batch if x["rw_flag"]]
            new = wt.advance_by_queries(batch)
            t.apply_queries(batch)
        for k, v in pairs:
            tree.insert_leaf(k, v)
        m = m.advance(pairs)
        got = _is_state_of(new, w.order, t, tree, m)
        n_new = len({k for k, _ in pairs} - set(present) - written)
        written |= {k for k, _ in pairs}
        assert new.capacity == len(w.keys) and new.num_leaves == n_before + n_new and new.next_enumeration_index == next_before + n_new
        # a path of the output folded with hashlib reaches the new root: a written entry, an unwritten present one, an unwritten absent one
        pos = {k: i for i, k in enumerate(w.order)}
        untouched = [k for k in present if k not in written][0], [k for k in absent if k not in written][0]
        for k in (pairs[0][0],) + untouched:
            i = pos[k]
            assert model.fold(k, got[0][i], got[1][i].tobytes(), got[2][i]) == tree.root
        assert got[0][pos[untouched[1]]] == 0
        wt.free()
        wt = new
    assert wt.get_leaves([absent[200]])[0][0] != 0  # the zero value took an index
    wt.free()
    t.free()


def test_smallest_shapes(ctx, world, oracle):
    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(7)
    tree, t = _fresh(nv, ctx, oracle, w)

    def case(keys, pairs):
        """the table of `keys` in the current state, advanced by `pairs`, against the trees after the same insert and the model"""
        wt = t.extract_witness(_rows(keys)) if keys else t.extract_witness(np.zeros((0, 32), np.uint8))
        m = model.Table(keys, *_oracle_answers(tree, keys), tree.root, tree.next_enumeration_index)
        before = wt.get_leaves(keys) if keys else None
        new = _advance(wt, pairs) if pairs else wt.advance(np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8))
        if pairs:
            _insert(t, tree, pairs)
        if keys:
            after = _is_state_of(new, keys, t, tree, m.advance(pairs))
            _same(wt.get_leaves(keys), before, "the input")  # the input is as it was
        else:
            before = after = None
            assert (new.root, new.next_enumeration_index) == (tree.root, tree.next_enumeration_index)
        assert (new.capacity, new.num_leaves) == (len(keys), sum(1 for k in keys if tree.get_leaf(k)[0]))
        wt.free()
        new.free()
        return before, after

    present = w.keys[:w.n_present]
    case([present[0]], [(present[0], rng.bytes(32))])  # one entry, written once
    case([w.keys[-9]], [(w.keys[-9], rng.bytes(32))])  # ... an absent one
    for key, bit in ((w.a, 0), (w.b, 255)):  # two entries whose keys differ in one bit, one written: the other's path changes at that level only
        before, after = case([key, _flip(key, bit)], [(key, rng.bytes(32))])
        assert before[0][1] == after[0][1] and before[1][1].tobytes() == after[1][1].tobytes()
        assert np.nonzero((before[2][1] != after[2][1]).any(axis=1))[0].tolist() == [bit]
        assert np.nonzero((before[2][0] != after[2][0]).any(axis=1))[0].tolist() == []  # the written key's siblings stay
    before, after = case(present[10:20] + w.keys[-3:], [])  # n == 0: an equal table
    _same(after, before, "n == 0")
    case([], [])  # no entries, no writes
    case(w.run + [w.keys[-1], present[30]], [(k, rng.bytes(32)) for k in w.run])  # all 64 keys under the height-6 node in one call
    t.free()


def test_multi_launch_fold(ctx):
    """more written keys than one workgroup folds (ST_PERSISTENT_MAX = 1 024): a launch per height, against the full tree"""
    from era_zkevm_test_harness_amd import native as nv

    rng = np.random.default_rng(11)
    leaves = [rng.bytes(32) for _ in range(900)]
    t = nv.StorageTreeDevice(ctx, 2048)
    t.insert(_rows(leaves), _rows([rng.bytes(32) for _ in leaves]))
    keys = leaves[:700] + [rng.bytes(32) for _ in range(600)]
    wt = t.extract_witness(_rows(keys))
    assert wt.capacity == 1300 and wt.num_leaves == 700
    pick = rng.choice(1300, size=1100, replace=False)
    pairs = [(keys[i], rng.bytes(32)) for i in pick] + [(keys[i], rng.bytes(32)) for i in pick[:50]]
    new = _advance(wt, pairs)
    t.insert(_rows([k for k, _ in pairs]), _rows([v for _, v in pairs]))
    n_new = int((pick >= 700).sum())
    assert (new.root, new.next_enumeration_index, new.num_leaves, new.capacity) == (t.root, 901 + n_new, 700 + n_new, 1300)
    assert t.num_leaves == 900 + n_new
    asked = [keys[i] for i in rng.permutation(1300)]
    _same(new.get_leaves(asked), t.get_leaves(asked), "full device tree")
    for x in (wt, new, t):
        x.free()


def test_source_of_the_table_and_pointer_mode(ctx, world, oracle):
    """a table from proofs and one cut out of the full tree advance to equal tables; host and device pointer mode give equal results"""
    import torch

    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(13)
    pairs = [(w.keys[i], rng.bytes(32)) for i in rng.integers(0, len(w.keys), size=60)]
    q = w.q[:40]
    m1, m2 = w.model.advance(pairs), w.model.advance_by_queries(q, oracle.derive_final_address)
    c2 = nv.Context(0)
    c2.set_pointer_mode(nv.PTR_DEVICE)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_k, d_v, d_q, d_asked = up(_rows([k for k, _ in pairs])).reshape(-1, 32), up(_rows([v for _, v in pairs])).reshape(-1, 32), up(q), up(_rows(w.order)).reshape(-1, 32)
    torch.cuda.synchronize(dev)
    for source in (_from_proofs(nv, ctx, w.tree, w.keys), _extracted(nv, ctx, w)):
        for m, host, device in ((m1, lambda: _advance(source, pairs), lambda: source.advance(d_k, d_v, ctx=c2)),
                                (m2, lambda: source.advance_by_queries(q), lambda: source.advance_by_queries(d_q, ctx=c2))):
            h, d = host(), device()
            got = h.get_leaves(w.order)
            _same(got, m.answers(w.order), "host model")
            _same([x.cpu().numpy() for x in d.get_leaves(d_asked)], got, "device pointer mode")
            for x in (h, d):
                assert (x.root, x.next_enumeration_index, x.num_leaves, x.capacity) == (m.root, m.next_enumeration_index, m.num_leaves, len(w.keys))
                x.free()
        _same(source.get_leaves(w.order), w.model.answers(w.order), "the input")
        source.free()
    c2.close()


def test_errors(ctx, world, oracle):
    """each error returns nothing, the input answers as before, and the device goes on working"""
    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(17)
    wt = _from_proofs(nv, ctx, w.tree, w.keys)
    before = wt.get_leaves(w.order)

    def rejected(call):
        with pytest.raises(nv.ZkwError) as ei:
            call()
        assert ei.value.code == nv.ERR_INVALID
        return str(ei.value)

    # a written key outside the table: the position in the caller's order
    for pos, n in ((0, 1), (2, 5), (37, 38)):
        pairs = [(w.keys[i], rng.bytes(32)) for i in rng.integers(0, len(w.keys), size=n)]
        pairs[pos] = (w.outside[0], rng.bytes(32))
        if pos + 1 < n:
            pairs[-1] = (w.outside[1], rng.bytes(32))  # a later one does not change the answer
        assert f"position {pos} " in rejected(lambda: _advance(wt, pairs))
    # the query form: a READ of a key outside the table is no error, a write is, at the QUERY's position
    q = np.concatenate([w.q[:40], w.q[40:44]])
    q["rw_flag"][40:] = 0
    q["rw_flag"][:6] = [0, 1, 0, 0, 1, 1]
    ok = wt.advance_by_queries(q)
    _same(ok.get_leaves(w.order), w.model.advance_by_queries(q[:40], oracle.derive_final_address).answers(w.order), "host model")
    ok.free()
    q["rw_flag"][42] = 1
    assert int(q["rw_flag"][:42].sum()) < 42  # the position is the query's, not the write's
    assert "position 42 " in rejected(lambda: wt.advance_by_queries(q))
    # a full tree as the input
    t = nv.StorageTreeDevice(ctx, 16)
    t.insert(_rows(w.leaves[:4]), _rows(w.values[:4]))
    rejected(lambda: t.advance(_rows(w.leaves[:1]), _rows(w.values[:1])))
    rejected(lambda: t.advance_by_queries(q[:3]))
    assert t.num_leaves == 4
    t.free()
    _same(wt.get_leaves(w.order), before, "the input")
    assert (wt.root, wt.next_enumeration_index, wt.num_leaves, wt.capacity) == (w.tree.root, 1001, w.n_present, len(w.keys))
    pairs = [(w.keys[3], rng.bytes(32))]
    again = _advance(wt, pairs)  # the device goes on working
    _same(again.get_leaves(w.order), w.model.advance(pairs).answers(w.order), "host model")
    again.free()
    wt.free()


def test_context_of_another_device(ctx, world):
    import torch

    from era_zkevm_test_harness_amd import native as nv

    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    w = world
    wt = _from_proofs(nv, ctx, w.tree, w.keys[:8])
    other = nv.Context(1)
    for call in (lambda: wt.advance(_rows(w.keys[:1]), _rows(w.keys[:1]), ctx=other), lambda: wt.advance_by_queries(w.q[:2], ctx=other)):
        with pytest.raises(nv.ZkwError) as ei:
            call()
        assert ei.value.code == nv.ERR_INVALID
    _same(wt.get_leaves(w.keys[:8]), _oracle_answers(w.tree, w.keys[:8]), "the input")
    other.close()
    wt.free()


# ---- the block path: ONE table for K consecutive blocks --------------------------------------------------------------
def _four_blocks():
    return [synthetic.block_after_vm(seed=70, n_vm_memory=900, n_storage=50),
            synthetic.block_after_vm(seed=71, n_vm_memory=1200, n_storage=70, n_events=0),
            synthetic.block_after_vm(seed=72, n_vm_memory=700, n_storage=0, n_storage_cells=1),
            synthetic.block_after_vm(seed=73, n_vm_memory=1000, n_storage=40, n_storage_cells=12, n_l1_messages=0)]


def _two_blocks_on_the_same_slots():
    state = {}
    shapes = (dict(seed=70, n_vm_memory=900, n_storage=50), dict(seed=70, n_vm_memory=1000, n_storage=50, n_l1_messages=0))
    return [_rebase_storage(synthetic.block_after_vm(**sh), state) for sh in shapes]


@pytest.mark.parametrize("make_blocks, seed", [(_four_blocks, 31), (_two_blocks_on_the_same_slots, 37)], ids=["four_blocks", "same_slots"])
def test_consecutive_blocks_over_one_table(ctx, oracle, make_blocks, seed):
    """test_consecutive_blocks_in_one_call's and _on_the_same_slots' blocks with ONE table — the union of all blocks' slots in the initial
    state, cut out of the full tree or (the stateless host) built from the oracle's proofs — and every later pre-state made by
    advance_by_queries with the block's deduplicated queue: all blocks in one zkw_blocks_run = one block at a time on the full tree"""
    from era_zkevm_test_harness_amd import native as nv

    blocks = make_blocks()
    keys = [_storage_keys(oracle, b) for b in blocks]
    union = [k for ks in keys for k in ks]
    rng = np.random.default_rng(seed)
    initial = [(rng.bytes(32), rng.bytes(32)) for _ in range(10)]
    dedup = [_dedup_queries(nv, b) for b in blocks]
    # the truth: one block at a time on the full tree
    t = nv.StorageTreeDevice(ctx, 256)
    t.insert(_rows([k for k, _ in initial]), _rows([v for _, v in initial]))
    first_extracted = t.extract_witness(_rows(union))
    truth, roots = [], [t.root]
    for b in blocks:
        B = nv.Block(0, b, CAPS, storage_tree_device=t)
        truth.append(_sap_record(nv, B))
        B.apply_storage(t)
        B.free()
        roots.append(t.root)
    assert t.num_leaves > 10 and len(set(roots)) >= 2
    final = t.get_leaves(sorted(set(union)))
    t.free()
    tree = oracle.Tree()
    for k, v in initial:
        tree.insert_leaf(k, v)
    first_proven = _from_proofs(nv, ctx, tree, sorted(set(union)))
    for first in (first_extracted, first_proven):
        assert first.capacity == len(set(union)) and first.root == roots[0]
        tables = [first]
        for d in dedup:
            tables.append(tables[-1].advance_by_queries(d))
        assert [x.root for x in tables] == roots
        _same(tables[-1].get_leaves(sorted(set(union))), final, "full device tree")
        many = nv.Block.run_many(0, blocks, CAPS, storage_tree_device=tables[:-1])
        for k, mb in enumerate(many):
            rec = _sap_record(nv, mb)
            assert rec.keys() == truth[k].keys()
            for key in truth[k]:
                assert rec[key] == truth[k][key], (k, key)
        bad, lock, local, checkers = [], threading.Lock(), threading.local(), []

        def cb(bi, ty, i, tr, s, pi):
            if ty != SAP:
                return
            if not hasattr(local, "ctx"):  # a checker context per calling thread (include/zkw.h, zkw_blocks_synthesize)
                local.ctx = nv.Context(0)
                with lock:
                    checkers.append(local.ctx)
            v = many[bi].check_satisfied(SAP, tr, s, ctx=local.ctx)[0]
            with lock:
                bad.append((bi, i, v))

        nv.Block.synthesize_many(many, 1 << 18, ring_slots=1, callback=cb)
        assert sorted((bi, i) for bi, i, _v in bad) == [(bi, i) for bi, mb in enumerate(many) for i in range(mb.num_instances(SAP))]
        assert not any(v for *_x, v in bad), [x for x in bad if x[2]][:5]
        for c in checkers:
            c.close()
        nv.Block.free_many(many)
        for x in tables:
            x.free()
