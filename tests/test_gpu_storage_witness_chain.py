"""GPU: zkw_storage_tree_advance_witness_chain / _chain_pairs (csrc/storage_witness_kernels.cuh, "chain") — the pre-states of K consecutive
blocks out of ONE table in one call, each as a table of the block's own keys, and the final state of the union. The yardsticks are the host
model of tests/storage_witness_chain_model.py (the sequential Table.advance per block, restricted to the block's keys), the full device tree
after the same writes, the oracle's sequential tree and K - 1 sequential advance_by_queries calls; the call's own output is never one. Every
comparison is byte-exact. The world and the helpers are tests/test_gpu_storage_witness_advance.py's.

derive_final_address is a hash, so a QUERY cannot be aimed at a chosen key: the shapes that need chosen keys (level-0 siblings, keys that
differ in bit 255 only, 600 of 700 entries) go through the pair form, which runs the same kernels with every pair a write; reads, the
empty and the reads-only block, K = 260 and the block path go through the query form."""
import threading

import numpy as np
import pytest

from tests import storage_witness_chain_model as chain_model
from tests import storage_witness_model as model
from tests.test_gpu_storage_witness_advance import (_extracted, _four_blocks, _fresh, _from_proofs, _oracle_answers, _same, _two_blocks_on_the_same_slots,
                                                    ctx, world)  # noqa: F401  (ctx, world: fixtures)
from tests.test_gpu_storage_witness_tree import CAPS, SAP, _dedup_queries, _flip, _rows, _sap_record, _storage_keys

pytestmark = pytest.mark.gpu


def _queries(w, picks, rng):
    """records of the world's queries: picks = (query number, is_write) or (query number, is_write, value bytes)"""
    q = w.q[np.array([p[0] for p in picks], dtype=np.int64)].copy()
    for r, p in zip(q, picks):
        value = p[2] if len(p) > 2 else rng.bytes(32)
        r["rw_flag"] = 1 if p[1] else 0
        r["written_value"] = np.frombuffer(value, ">u4")[::-1]
    return q


def _pairs_args(blocks):
    return [(_rows([k for k, _v in b]) if b else np.zeros((0, 32), np.uint8), _rows([v for _k, v in b]) if b else np.zeros((0, 32), np.uint8)) for b in blocks]


def _model_blocks(oracle, blocks, pairs):
    return [[(k, v, True) for k, v in b] for b in blocks] if pairs else [chain_model.block_of(b, oracle.derive_final_address) for b in blocks]


def _is_table(t, m, rng):
    """the witness tree `t` is the model's table `m`: the same keys, the same answers in a shuffled order, the same description"""
    keys = sorted(m.entries)
    assert t.is_witness and (t.capacity, t.num_leaves, t.root, t.next_enumeration_index) == (len(keys), m.num_leaves, m.root, m.next_enumeration_index)
    if keys:
        asked = [keys[i] for i in rng.permutation(len(keys))]
        _same(t.get_leaves(asked), m.answers(asked), "host model")


def _chain(oracle, wt, m, blocks, rng, pairs=False, final=False):
    """advance_chain of `blocks` on `wt` (whose state the model table `m` holds) checked against the model; returns (outs, final table, models)"""
    keys = sorted(m.entries)
    before = wt.get_leaves(keys)
    got = (wt.advance_chain_pairs(_pairs_args(blocks), final=True) if pairs else wt.advance_chain(blocks, final=True)) if final else (
        (wt.advance_chain_pairs(_pairs_args(blocks)) if pairs else wt.advance_chain(blocks)), None)
    outs, last = got
    m_outs, m_last = chain_model.chain(m, _model_blocks(oracle, blocks, pairs))
    assert len(outs) == len(blocks)
    for t, mo in zip(outs, m_outs):
        _is_table(t, mo, rng)
    assert sum(t.capacity for t in outs) == sum(len(mo.entries) for mo in m_outs)  # HBM: the blocks' own keys, not K x the union
    if last is not None:
        _is_table(last, m_last, rng)
    _same(wt.get_leaves(keys), before, "the input")  # the input answers as before
    _same(before, m.answers(keys), "the input")
    return outs, last, (m_outs, m_last)


def _free(*tables):
    for t in tables:
        if isinstance(t, (list, tuple)):
            _free(*t)
        elif t is not None:
            t.free()


def test_tightest_dependencies(ctx, world, oracle):
    """K = 2, block 0 writes x, block 1 its sibling at level 0 — block 1's fold at level 0 reads the cell block 0 updated one step earlier —
    and the same with keys that differ in bit 255 only, the last step; both keys absent before. A table of exactly the two keys, and the two
    inside the 475-key world."""
    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(101)
    for x, y in (w.sib0, w.sib255):
        for keys, m in (([x, y], model.Table([x, y], *_oracle_answers(w.tree, [x, y]), w.tree.root, w.tree.next_enumeration_index)), (w.keys, w.model)):
            wt = _from_proofs(nv, ctx, w.tree, keys)
            for first, second in ((x, y), (y, x)):
                outs, last, (m_outs, _m) = _chain(oracle, wt, m, [[(first, rng.bytes(32))], [(second, rng.bytes(32))]], rng, pairs=True, final=True)
                assert outs[0].capacity == outs[1].capacity == 1 and outs[0].root == w.tree.root != outs[1].root != last.root
                assert (last.num_leaves, last.next_enumeration_index) == (m.num_leaves + 2, 1003)
                idx, _val, paths = outs[1].get_leaves([second])
                bit = 0 if x is w.sib0[0] else 255
                assert idx[0] == 0 and paths[0][bit].tobytes() == m_outs[1].entries[second][2][bit] != m.entries[second][2][bit]  # block 0's new leaf / subtree
                _free(outs, last)
            wt.free()


def test_single_block_single_entry(ctx, world, oracle):
    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(103)
    for k in (w.keys[0], w.keys[-9]):  # a present entry, an absent one
        m = model.Table([k], *_oracle_answers(w.tree, [k]), w.tree.root, w.tree.next_enumeration_index)
        wt = _from_proofs(nv, ctx, w.tree, [k])
        outs, last, _m = _chain(oracle, wt, m, [[(k, rng.bytes(32))]], rng, pairs=True, final=True)
        assert outs[0].root == w.tree.root != last.root and last.capacity == 1
        _free(outs, last, wt)


def test_empty_and_reads_only_blocks_carry_the_state(ctx, world, oracle):
    """K = 3: writes and reads, an empty block, a reads-only block"""
    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(107)
    wt = _from_proofs(nv, ctx, w.tree, w.keys)
    blocks = [_queries(w, [(i, i % 3 != 0) for i in range(12)] + [(30, True)], rng), _queries(w, [], rng), _queries(w, [(i, False) for i in (30, 2, 17, 2)], rng)]
    outs, last, _m = _chain(oracle, wt, w.model, blocks, rng, final=True)
    assert outs[1].capacity == 0 and outs[2].capacity == 3
    assert w.tree.root == outs[0].root != outs[1].root == outs[2].root == last.root
    assert outs[0].next_enumeration_index < outs[1].next_enumeration_index == outs[2].next_enumeration_index == last.next_enumeration_index
    _free(outs, last, wt)


def test_one_key_written_in_every_block(ctx, world, oracle):
    """K = 4: the key is absent at the start, takes its index in block 0 and keeps it; block 1 writes it three times, block 2 the zero value"""
    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(109)
    a, other, present = w.keys[-20], w.keys[-21], w.keys[7]
    v = lambda: rng.bytes(32)  # noqa: E731
    blocks = [[(other, v()), (a, v())], [(a, v()), (present, v()), (a, v()), (a, v())], [(a, bytes(32))], [(a, v()), (other, v())]]
    wt = _from_proofs(nv, ctx, w.tree, w.keys)
    outs, last, _m = _chain(oracle, wt, w.model, blocks, rng, pairs=True, final=True)
    got = [t.get_leaves([a]) for t in outs + [last]]
    assert [int(g[0][0]) for g in got] == [0, 1002, 1002, 1002, 1002]
    assert got[2][1].tobytes() == blocks[1][-1][1] and got[3][1].tobytes() == bytes(32) and got[4][1].tobytes() == blocks[3][0][1]
    assert [t.next_enumeration_index for t in outs + [last]] == [1001, 1003, 1003, 1003, 1003]
    _free(outs, last, wt)


def test_read_of_a_key_an_earlier_block_wrote(ctx, world, oracle):
    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(113)
    value = rng.bytes(32)
    blocks = [_queries(w, [(20, True, value), (3, False)], rng), _queries(w, [(4, True), (25, True)], rng), _queries(w, [(20, False), (5, True)], rng)]
    wt = _from_proofs(nv, ctx, w.tree, w.keys)
    outs, _last, (m_outs, _m) = _chain(oracle, wt, w.model, blocks, rng)
    idx, val, paths = outs[2].get_leaves([w.qkeys[20]])
    assert w.model.entries[w.qkeys[20]][0] == 0 and idx[0] == 1001 and val[0].tobytes() == value  # absent before block 0: the new index and value
    assert paths[0].tobytes() == b"".join(m_outs[2].entries[w.qkeys[20]][2]) != b"".join(w.model.entries[w.qkeys[20]][2])  # and block 1's siblings
    assert model.fold(w.qkeys[20], idx[0], value, paths[0]) == outs[2].root
    _free(outs, wt)


def test_final_state_and_a_second_chain(ctx, world, oracle):
    """final=True = the model's last table = the full device tree and the oracle's tree after all blocks, over all 475 keys; a chain started from
    it continues; and every table = what sequential advance_by_queries calls on the union give"""
    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(127)
    tree, t = _fresh(nv, ctx, oracle, w)
    blocks = [_queries(w, [(int(i), bool(rng.integers(0, 3))) for i in rng.integers(0, 40, size=n)], rng) for n in (25, 1, 40, 0, 13)]
    wt = _from_proofs(nv, ctx, w.tree, w.keys)
    outs, last, (_mo, m_last) = _chain(oracle, wt, w.model, blocks[:3], rng, final=True)
    seq = wt
    for k, b in enumerate(blocks[:3]):  # K - 1 sequential calls on the union table (and one more for the final state)
        mine = sorted({oracle.derive_final_address(x) for x in b})
        _same(outs[k].get_leaves(mine), seq.get_leaves(mine), "advance_by_queries")
        assert (outs[k].root, outs[k].next_enumeration_index) == (seq.root, seq.next_enumeration_index)
        nxt = seq.advance_by_queries(b)
        if seq is not wt:
            seq.free()
        seq = nxt
        t.apply_queries(b)
        for x in b:
            if x["rw_flag"]:
                tree.insert_leaf(oracle.derive_final_address(x), model.written_value(x))
    got = last.get_leaves(w.order)
    for what, want in (("advance_by_queries", seq.get_leaves(w.order)), ("full device tree", t.get_leaves(w.order)), ("oracle", _oracle_answers(tree, w.order))):
        _same(got, want, what)
    assert last.root == seq.root == t.root == tree.root and last.next_enumeration_index == t.next_enumeration_index == tree.next_enumeration_index
    assert last.capacity == len(w.keys)
    outs2, last2, _m2 = _chain(oracle, last, m_last, blocks[3:], rng, final=True)
    for b in blocks[3:]:
        t.apply_queries(b)
    _same(last2.get_leaves(w.order), t.get_leaves(w.order), "full device tree")
    assert last2.root == t.root
    _free(outs, outs2, last, last2, seq, wt, t)


def test_window_slides_off_both_ends(ctx, world, oracle):
    """K = 260 blocks of one or two queries over a 40-key table: more blocks than heights"""
    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(131)
    keys = w.qkeys[:40]
    m = model.Table(keys, *_oracle_answers(w.tree, keys), w.tree.root, w.tree.next_enumeration_index)
    wt = _from_proofs(nv, ctx, w.tree, keys)
    blocks = [_queries(w, [(int(i), bool(rng.integers(0, 4))) for i in rng.integers(0, 40, size=1 + k % 2)], rng) for k in range(260)]
    outs, last, _m = _chain(oracle, wt, m, blocks, rng, final=True)
    assert len({t.root for t in outs}) > 100
    _free(outs, last, wt)


def test_fold_over_several_workgroups(ctx):
    """one block that writes 600 of 700 entries, then a block that rewrites 50 of them, against the full device tree"""
    from era_zkevm_test_harness_amd import native as nv

    rng = np.random.default_rng(137)
    leaves = [rng.bytes(32) for _ in range(900)]
    t = nv.StorageTreeDevice(ctx, 2048)
    t.insert(_rows(leaves), _rows([rng.bytes(32) for _ in leaves]))
    keys = leaves[:400] + [rng.bytes(32) for _ in range(300)]
    wt = t.extract_witness(_rows(keys))
    pick = rng.choice(700, size=600, replace=False)
    blocks = [[(keys[i], rng.bytes(32)) for i in pick], [(keys[i], rng.bytes(32)) for i in pick[100:150]]]
    outs, last = wt.advance_chain_pairs(_pairs_args(blocks), final=True)
    assert [x.capacity for x in outs] == [600, 50] and last.capacity == 700
    n_new = int((pick >= 400).sum())
    for k, b in enumerate(blocks):
        mine = [x for x, _v in b]
        _same(outs[k].get_leaves(mine), t.get_leaves(mine), "full device tree")
        assert (outs[k].root, outs[k].next_enumeration_index) == (t.root, t.next_enumeration_index)
        assert outs[k].num_leaves == sum(1 for i in t.get_leaves(mine, paths=False)[0] if i)
        t.insert(_rows(mine), _rows([v for _x, v in b]))
    asked = [keys[i] for i in rng.permutation(700)]
    _same(last.get_leaves(asked), t.get_leaves(asked), "full device tree")
    assert (last.root, last.next_enumeration_index, last.num_leaves) == (t.root, 901 + n_new, 400 + n_new)
    _free(outs, last, wt, t)


def test_sources_and_pointer_modes(ctx, world, oracle):
    """a table from proofs and an extracted one, the host and the device pointer mode: equal tables"""
    import torch

    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(139)
    blocks = [_queries(w, [(int(i), bool(rng.integers(0, 2))) for i in rng.integers(0, 40, size=n)], rng) for n in (9, 0, 17)]
    c2 = nv.Context(0)
    c2.set_pointer_mode(nv.PTR_DEVICE)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_blocks, d_order = [up(b) for b in blocks], up(_rows(w.order)).reshape(-1, 32)
    torch.cuda.synchronize(dev)
    for source in (_from_proofs(nv, ctx, w.tree, w.keys), _extracted(nv, ctx, w)):
        outs, last, (m_outs, _m) = _chain(oracle, source, w.model, blocks, rng, final=True)
        d_outs, d_last = source.advance_chain(d_blocks, ctx=c2, final=True)
        for h, d, mo in zip(outs + [last], d_outs + [d_last], m_outs + [None]):
            assert (h.capacity, h.num_leaves, h.root, h.next_enumeration_index) == (d.capacity, d.num_leaves, d.root, d.next_enumeration_index)
            asked = w.order if mo is None else sorted(mo.entries)
            if asked:
                d_asked = d_order if mo is None else up(_rows(asked)).reshape(-1, 32)
                torch.cuda.synchronize(dev)
                _same([x.cpu().numpy() for x in d.get_leaves(d_asked)], h.get_leaves(asked), "device pointer mode")
        _free(outs, last, d_outs, d_last, source)
    c2.close()


def test_errors(ctx, world, oracle):
    """each error returns nothing, the input answers as before, and a correct call succeeds afterwards"""
    from era_zkevm_test_harness_amd import native as nv

    w = world
    rng = np.random.default_rng(149)
    wt = _from_proofs(nv, ctx, w.tree, w.keys)
    good = [_queries(w, [(1, True), (2, False)], rng), _queries(w, [(2, True)], rng)]

    def rejected(call):
        with pytest.raises(nv.ZkwError) as ei:
            call()
        assert ei.value.code == nv.ERR_INVALID
        _same(wt.get_leaves(w.order), w.model.answers(w.order), "the input")
        outs, _last, _m = _chain(oracle, wt, w.model, good, rng)  # the device goes on working
        _free(outs)
        return str(ei.value)

    # a READ and a write outside the table (queries 40.. of the world), the first of two in (block, position) order
    for is_write in (False, True):
        blocks = [_queries(w, [(0, True), (5, False)], rng), _queries(w, [], rng), _queries(w, [(7, True), (9, False), (41, is_write), (3, True)], rng),
                  _queries(w, [(45, True), (2, True)], rng)]
        text = rejected(lambda: wt.advance_chain(blocks))
        assert "block 2," in text and "position 2)" in text, text
    blocks = [_queries(w, [(44, False)], rng), _queries(w, [(43, True)], rng)]
    text = rejected(lambda: wt.advance_chain(blocks, final=True))
    assert "block 0," in text and "position 0)" in text, text
    text = rejected(lambda: wt.advance_chain_pairs(_pairs_args([[(w.keys[0], rng.bytes(32))], [(w.keys[1], rng.bytes(32)), (w.outside[0], rng.bytes(32))]])))
    assert "block 1," in text and "position 1)" in text, text
    # a full tree as the input, no blocks, bad offsets
    t = nv.StorageTreeDevice(ctx, 16)
    t.insert(_rows(w.leaves[:4]), _rows(w.values[:4]))
    rejected(lambda: t.advance_chain(good))
    assert t.num_leaves == 4
    t.free()
    rejected(lambda: wt.advance_chain([]))
    import ctypes as C

    lib = nv.load()
    q = np.concatenate(good)
    out = (C.c_void_p * 2)()
    for offsets in ((1, 2, 3), (0, 3, 2)):
        offs = (C.c_uint64 * 3)(*offsets)
        rejected(lambda: nv._check(lib.zkw_storage_tree_advance_witness_chain(wt.handle, ctx.handle, q.ctypes.data_as(C.c_void_p), offs, 2, out, None)))
        assert not out[0] and not out[1]
    wt.free()


@pytest.mark.parametrize("make_blocks, seed", [(_four_blocks, 31), (_two_blocks_on_the_same_slots, 37)], ids=["four_blocks", "same_slots"])
def test_consecutive_blocks_over_one_chain(ctx, oracle, make_blocks, seed):
    """test_consecutive_blocks_over_one_table's blocks with every pre-state made by ONE advance_chain of the blocks' deduplicated queues over
    the table of the union of their slots: all blocks in one zkw_blocks_run = one block at a time on the full tree, and the instances are
    satisfied"""
    from era_zkevm_test_harness_amd import native as nv

    blocks = make_blocks()
    union = sorted({k for b in blocks for k in _storage_keys(oracle, b)})
    rng = np.random.default_rng(seed)
    initial = [(rng.bytes(32), rng.bytes(32)) for _ in range(10)]
    dedup = [_dedup_queries(nv, b) for b in blocks]
    # the truth: one block at a time on the full tree
    t = nv.StorageTreeDevice(ctx, 256)
    t.insert(_rows([k for k, _ in initial]), _rows([v for _, v in initial]))
    first = t.extract_witness(_rows(union))
    truth, roots = [], [t.root]
    for b in blocks:
        B = nv.Block(0, b, CAPS, storage_tree_device=t)
        truth.append(_sap_record(nv, B))
        B.apply_storage(t)
        B.free()
        roots.append(t.root)
    final = t.get_leaves(union)
    t.free()
    tables, last = first.advance_chain(dedup, final=True)
    assert [x.root for x in tables] + [last.root] == roots
    assert [x.capacity for x in tables] == [len({oracle.derive_final_address(q) for q in d}) for d in dedup] and last.capacity == len(union)
    _same(last.get_leaves(union), final, "full device tree")
    many = nv.Block.run_many(0, blocks, CAPS, storage_tree_device=tables)
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
    _free(tables, last, first)
