"""GPU: the device-resident storage tree (zkw_storage_tree, csrc/zkw_storage_tree.hip) and the block path that reads it instead of
calling back to the host (zkw_block_inputs.storage_tree_device). The yardstick is the oracle's tree (oracle.Tree: the reference's
InMemoryStorageTree restated in C, sequential inserts) and, for the block cases, the callback path over that tree; every comparison is
byte-exact."""
import hashlib
import threading

import numpy as np
import pytest

from era_zkevm_test_harness_amd import synthetic

pytestmark = pytest.mark.gpu

CAPS = {2: 5, 3: 7, 4: 64, 5: 3, 6: 4, 7: 2, 8: 1000, 9: 40, 10: 5, 11: 16, 12: 9, 13: 48}  # tests/test_gpu_block.py's, by circuit type
SAP = 10


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


def _rows(list_of_bytes):
    return np.frombuffer(b"".join(list_of_bytes), np.uint8).reshape(-1, 32)


def _oracle_answers(tree, keys):
    idx = np.zeros(len(keys), np.uint64)
    val = np.zeros((len(keys), 32), np.uint8)
    paths = np.zeros((len(keys), 256, 32), np.uint8)
    for i, k in enumerate(keys):
        ix, v, paths[i] = tree.get_leaf(k)
        idx[i], val[i] = ix, np.frombuffer(v, np.uint8)
    return idx, val, paths


def _same_answers(t, tree, keys):
    idx, val, paths = t.get_leaves(keys)
    eidx, eval_, epaths = _oracle_answers(tree, keys)
    assert np.array_equal(idx, eidx)
    assert val.tobytes() == eval_.tobytes()
    assert paths.tobytes() == epaths.tobytes()
    return idx, val, paths


def _same_state(t, tree):
    assert t.root == tree.root
    assert t.next_enumeration_index == tree.next_enumeration_index


def _flip(key, bit):
    k = bytearray(key)
    k[bit // 8] ^= 1 << (bit % 8)
    return bytes(k)


def test_empty_tree(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv

    t = nv.StorageTreeDevice(ctx, 16)
    tree = oracle.Tree()
    assert t.root == tree.root and t.num_leaves == 0 and t.next_enumeration_index == 1
    keys = [bytes(32), b"\xff" * 32, np.random.default_rng(5).bytes(32)]
    idx, val, paths = _same_answers(t, tree, keys)
    assert not idx.any() and not val.any()
    empty = [hashlib.blake2s(bytes(40), digest_size=32).digest()]
    for _ in range(255):
        empty.append(hashlib.blake2s(empty[-1] * 2, digest_size=32).digest())
    for i in range(3):
        assert paths[i].tobytes() == b"".join(empty)
    t.free()


@pytest.mark.parametrize("n", [1, 2, 1000, 20000])
def test_build_in_one_call(ctx, oracle, n):
    from era_zkevm_test_harness_amd import native as nv

    rng = np.random.default_rng(100 + n)
    keys = [rng.bytes(32) for _ in range(n)]
    values = [rng.bytes(32) for _ in range(n)]
    tree = oracle.Tree()
    for k, v in zip(keys, values):
        tree.insert_leaf(k, v)
    t = nv.StorageTreeDevice(ctx, n)
    t.insert(_rows(keys), _rows(values))
    _same_state(t, tree)
    assert t.num_leaves == n
    present = [keys[i] for i in rng.choice(n, size=min(n, 200), replace=False)]
    absent = [rng.bytes(32) for _ in range(200)]
    idx, _val, _p = _same_answers(t, tree, present + absent)
    assert idx[:len(present)].all() and not idx[len(present):].any()
    t.free()


def test_shaped_keys(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv

    rng = np.random.default_rng(7)
    a, b, c = rng.bytes(32), rng.bytes(32), rng.bytes(32)
    run = [bytes([i]) + c[1:] for i in range(64)]  # 64 keys that share their top 250 bits (bits 0..5 vary)
    rep = rng.bytes(32)
    keys = [bytes(32), b"\xff" * 32, a, _flip(a, 0), b, _flip(b, 255)] + run + [rep, rng.bytes(32), rep, rep]
    values = [rng.bytes(32) for _ in keys]
    tree = oracle.Tree()
    for k, v in zip(keys, values):
        tree.insert_leaf(k, v)
    t = nv.StorageTreeDevice(ctx, 128)
    t.insert(_rows(keys), _rows(values))
    _same_state(t, tree)
    distinct = list(dict.fromkeys(keys))
    assert t.num_leaves == len(distinct) == len(keys) - 2
    neighbours = [_flip(run[0], 6), _flip(run[63], 255), _flip(rep, 0), _flip(rep, 255), _flip(bytes(32), 0), _flip(b"\xff" * 32, 255)]
    assert not set(neighbours) & set(distinct)
    idx0, val0, _p = _same_answers(t, tree, distinct + neighbours + [rng.bytes(32) for _ in range(20)])
    assert val0[distinct.index(rep)].tobytes() == values[-1]  # the last value of the repeated key, the index of its first occurrence
    assert int(idx0[distinct.index(rep)]) == keys.index(rep) + 1
    # a second call: five existing keys rewritten, five new ones
    rewritten = [bytes(32), a, run[17], rep, _flip(b, 255)]
    fresh = [rng.bytes(32) for _ in range(4)] + [_flip(a, 1)]
    keys2 = [k for pair in zip(rewritten, fresh) for k in pair]
    values2 = [rng.bytes(32) for _ in keys2]
    for k, v in zip(keys2, values2):
        tree.insert_leaf(k, v)
    t.insert(_rows(keys2), _rows(values2))
    _same_state(t, tree)
    assert t.num_leaves == len(distinct) + 5
    idx1, val1, _p = _same_answers(t, tree, distinct + fresh + neighbours + [_flip(k, 0) for k in fresh[:4]] + [_flip(k, 255) for k in fresh[:4]])
    assert np.array_equal(idx1[:len(distinct)], idx0[:len(distinct)])  # every key kept its index, the rewritten ones included
    for k in rewritten:
        assert val1[distinct.index(k)].tobytes() == values2[keys2.index(k)]
    assert sorted(int(x) for x in idx1[len(distinct):len(distinct) + 5]) == list(range(len(distinct) + 1, len(distinct) + 6))
    t.free()


def test_paths_are_proofs(ctx):
    """independent of the library and of the oracle: folding a returned (index, value, path) with hashlib reaches the root"""
    from era_zkevm_test_harness_amd import native as nv

    rng = np.random.default_rng(11)
    n = 3000
    keys = [rng.bytes(32) for _ in range(n)]
    t = nv.StorageTreeDevice(ctx, 4096)
    t.insert(_rows(keys), _rows([rng.bytes(32) for _ in range(n)]))
    asked = [keys[i] for i in rng.choice(n, size=80, replace=False)] + [rng.bytes(32) for _ in range(20)]
    idx, val, paths = t.get_leaves(asked)
    root = t.root
    h = lambda b: hashlib.blake2s(b, digest_size=32).digest()  # noqa: E731
    for i, key in enumerate(asked):
        k = int.from_bytes(key, "little")
        cur = h(int(idx[i]).to_bytes(8, "big") + val[i].tobytes())
        for level in range(256):
            sib = paths[i, level].tobytes()
            cur = h(sib + cur) if (k >> level) & 1 else h(cur + sib)
        assert cur == root, i
    assert idx[:80].all() and not idx[80:].any()
    t.free()


def test_three_batches_equal_one_sequence(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv

    rng = np.random.default_rng(13)
    keys = [rng.bytes(32) for _ in range(1500)]
    keys[700:720] = keys[100:120]     # keys of the first batch come again in the second ...
    keys[1400:1410] = keys[690:700]   # ... and of the second in the third
    values = [rng.bytes(32) for _ in keys]
    tree = oracle.Tree()
    t = nv.StorageTreeDevice(ctx, 2048)
    for lo, hi in ((0, 500), (500, 1300), (1300, 1500)):
        for k, v in zip(keys[lo:hi], values[lo:hi]):
            tree.insert_leaf(k, v)
        t.insert(_rows(keys[lo:hi]), _rows(values[lo:hi]))
        _same_state(t, tree)
    assert t.num_leaves == 1470
    _same_answers(t, tree, keys[::7] + [rng.bytes(32) for _ in range(30)])
    one = nv.StorageTreeDevice(ctx, 2048)  # and the same list in ONE call
    one.insert(_rows(keys), _rows(values))
    _same_state(one, tree)
    one.free()
    t.free()


def test_errors_leave_the_tree_alone(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv

    rng = np.random.default_rng(17)
    keys = [rng.bytes(32) for _ in range(12)]
    values = [rng.bytes(32) for _ in range(12)]
    t = nv.StorageTreeDevice(ctx, 10)
    t.insert(_rows(keys[:8]), _rows(values[:8]))
    root, nxt = t.root, t.next_enumeration_index
    with pytest.raises(nv.ZkwError) as ei:
        t.insert(_rows(keys[6:12]), _rows(values[6:12]))  # two rewrites + four new leaves: 12 > 10
    assert ei.value.code == nv.ERR_OOM
    assert (t.root, t.next_enumeration_index, t.num_leaves) == (root, nxt, 8)
    tree = oracle.Tree()
    for k, v in zip(keys[:8], values[:8]):
        tree.insert_leaf(k, v)
    _same_state(t, tree)
    _same_answers(t, tree, keys)
    t.insert(_rows(keys[6:10]), _rows(values[6:10]))  # what fits still goes in
    assert t.num_leaves == 10
    with pytest.raises(nv.ZkwError) as ei:
        nv.StorageTreeDevice(ctx, 0)
    assert ei.value.code == nv.ERR_INVALID
    b = synthetic.block_after_vm(seed=1)
    with pytest.raises(nv.ZkwError) as ei:
        nv.Block(0, b, CAPS, storage_tree=lambda q: (np.zeros(q.size, np.uint64), np.zeros((q.size, 256, 32), np.uint8)),
                 storage_initial_root=bytes(32), storage_next_enumeration_index=1, storage_tree_device=t)
    assert ei.value.code == nv.ERR_INVALID and "storage_tree" in str(ei.value)
    t.free()


def test_device_pointer_mode_answer_and_apply_queries(oracle):
    """a context in device pointer mode: torch tensors in and out; zkw_storage_tree_answer_queries / _apply_queries over log queries that
    are in device memory — derive_final_address, get_leaf and the block's writes without a host in between"""
    import torch

    from era_zkevm_test_harness_amd import native as nv

    c = nv.Context(0)
    c.set_pointer_mode(nv.PTR_DEVICE)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    q, existing = synthetic.storage_application_trace(120, seed=3)
    q = np.ascontiguousarray(q, dtype=nv.LOG_QUERY)
    rng = np.random.default_rng(19)
    pairs = [(rng.bytes(32), rng.bytes(32)) for _ in range(300)]
    pairs += [(oracle.derive_final_address(q[i]), _value_of(q[i])) for i in range(q.size) if existing[i]]
    tree = oracle.Tree()
    for k, v in pairs:
        tree.insert_leaf(k, v)
    t = nv.StorageTreeDevice(c, 512)
    t.insert(up(_rows([k for k, _ in pairs])).reshape(-1, 32), up(_rows([v for _, v in pairs])).reshape(-1, 32))
    _same_state(t, tree)
    keys = [oracle.derive_final_address(x) for x in q]
    eidx, eval_, epaths = _oracle_answers(tree, keys)
    idx, val, paths = t.get_leaves(up(_rows(keys)).reshape(-1, 32))
    assert np.array_equal(idx.cpu().numpy().astype(np.uint64), eidx) and val.cpu().numpy().tobytes() == eval_.tobytes()
    assert paths.cpu().numpy().tobytes() == epaths.tobytes()
    d_q = up(q)
    d_idx = torch.zeros(q.size, dtype=torch.int64, device=dev)
    d_paths = torch.zeros((q.size, 256, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    t.answer_queries(c, d_q.data_ptr(), q.size, d_idx.data_ptr(), d_paths.data_ptr())
    c.synchronize()
    assert np.array_equal(d_idx.cpu().numpy().astype(np.uint64), eidx) and d_paths.cpu().numpy().tobytes() == epaths.tobytes()
    t.apply_queries(d_q)
    for x in q:
        if x["rw_flag"]:
            tree.insert_leaf(oracle.derive_final_address(x), b"".join(int(w).to_bytes(4, "big") for w in x["written_value"][::-1]))
    _same_state(t, tree)
    assert q["rw_flag"].any() and not q["rw_flag"].all()
    t.free()
    c.close()


# ---- the block path ------------------------------------------------------------------------------------------------
def _value_of(q):
    return b"".join(int(x).to_bytes(4, "big") for x in q["read_value"][::-1])


def _dedup_queries(nv, block):
    """the deduplicated storage queue of a block: what its storage application will ask the tree about"""
    B = nv.Block(0, block, CAPS)
    dedup = B.witness_get(9, nv.STO_RESULT_QUERIES, np.uint8).view(nv.LOG_QUERY).copy()
    qt = B.witness_get(9, nv.STO_RESULT_NEW_TAILS, np.uint64).reshape(-1, 4).copy()
    B.free()
    return dedup, qt


def _pre_block_leaves(oracle, dedup, seed):
    """tests/test_gpu_block.py::_tree_for as a list of pairs: ten unrelated leaves, then what the block's first reads expect"""
    rng = np.random.default_rng(seed)
    pairs = [(rng.bytes(32), rng.bytes(32)) for _ in range(10)]
    pairs += [(oracle.derive_final_address(q), _value_of(q)) for q in dedup if q["read_value"].any()]
    return pairs


def _callback_over(oracle, tree):
    def answers(q):
        idx = np.zeros(q.size, np.uint64)
        paths = np.zeros((q.size, 256, 32), np.uint8)
        for i in range(q.size):
            idx[i], _, paths[i] = tree.get_leaf(oracle.derive_final_address(q[i]))
        return idx, paths
    return answers


def _sap_record(nv, B):
    r = {w: B.witness_get(SAP, w, np.uint8).tobytes() for w in (nv.SAP_DERIVED_KEYS, nv.SAP_MERKLE_PATHS, nv.SAP_LEAF_INDEXES, nv.SAP_ROOTS, nv.SAP_INSTANCES)}
    r["pi"] = B.public_inputs(SAP).tobytes()
    enc, states = B.recursion_queue(SAP)
    r["rq"] = enc.tobytes() + states.tobytes()
    r["n"] = B.num_instances(SAP)
    return r


def _block_on_both_trees(nv, oracle, block, t, tree):
    """the block over the device tree and over the callback on the oracle's tree (same pre-block state): the records of both, compared"""
    Bd = nv.Block(0, block, CAPS, storage_tree_device=t)
    Bc = nv.Block(0, block, CAPS, storage_tree=_callback_over(oracle, tree), storage_initial_root=tree.root,
                  storage_next_enumeration_index=tree.next_enumeration_index)
    rd, rc = _sap_record(nv, Bd), _sap_record(nv, Bc)
    assert rd.keys() == rc.keys()
    for key in rc:
        assert rd[key] == rc[key], key
    Bc.free()
    return Bd, rd


@pytest.mark.parametrize("seed", [1, 4])
def test_block_single_and_chained(ctx, oracle, seed):
    from era_zkevm_test_harness_amd import native as nv

    block = synthetic.block_after_vm(seed=seed)
    dedup, qt = _dedup_queries(nv, block)
    pairs = _pre_block_leaves(oracle, dedup, seed)
    tree = oracle.Tree()
    for k, v in pairs:
        tree.insert_leaf(k, v)
    t = nv.StorageTreeDevice(ctx, 1024)
    t.insert(_rows([k for k, _ in pairs]), _rows([v for _, v in pairs]))
    _same_state(t, tree)
    B, rec = _block_on_both_trees(nv, oracle, block, t, tree)
    o = oracle.storage_application_build(tree, dedup, qt, CAPS[SAP])  # (advances the oracle's tree)
    assert rec[nv.SAP_ROOTS] == o["roots"].tobytes()
    assert rec["n"] == o["instances"].size >= 2
    # chaining: the block's writes into the device tree
    B.apply_storage(t)
    assert t.root == tree.root == o["roots"][-1].tobytes()
    assert t.next_enumeration_index == tree.next_enumeration_index
    B.free()
    # a second block on the advanced trees; what its first reads expect is merged in on both sides
    block2 = synthetic.block_after_vm(seed=seed + 30, n_storage=90, n_storage_cells=20)
    dedup2, qt2 = _dedup_queries(nv, block2)
    extra = [(oracle.derive_final_address(q), _value_of(q)) for q in dedup2 if q["read_value"].any()]
    for k, v in extra:
        tree.insert_leaf(k, v)
    t.insert(_rows([k for k, _ in extra]), _rows([v for _, v in extra]))
    _same_state(t, tree)
    B2, rec2 = _block_on_both_trees(nv, oracle, block2, t, tree)
    o2 = oracle.storage_application_build(tree, dedup2, qt2, CAPS[SAP])
    assert rec2[nv.SAP_ROOTS] == o2["roots"].tobytes() and rec2["n"] == o2["instances"].size >= 2
    B2.apply_storage(t)
    _same_state(t, tree)
    B2.free()
    t.free()


def test_many_blocks_with_device_trees(ctx, oracle):
    """eight blocks of different shapes through zkw_blocks_run, their storage queries answered from device trees inside the fibers (one shared
    tree where the blocks' slots do not contradict each other, a tree of its own otherwise; one block without storage queries, one without
    a tree): type 10 of every block as zkw_block_run gives it alone, and every type-10 trace zkw_blocks_synthesize hands out satisfied"""
    from era_zkevm_test_harness_amd import native as nv

    shapes = [synthetic.block_after_vm(seed=60, n_vm_memory=900, n_storage=50),
              synthetic.block_after_vm(seed=61, n_vm_memory=1400, n_storage=70, n_events=0),
              synthetic.block_after_vm(seed=62, n_vm_memory=700, n_storage=40, n_l1_messages=0),
              synthetic.block_after_vm(seed=63, n_vm_memory=1100, n_storage=0, n_storage_cells=1),
              synthetic.block_after_vm(seed=64, n_vm_memory=800, n_storage=30, n_precompile_calls=(0, 0, 0)),
              synthetic.block_after_vm(seed=65, n_vm_memory=1000, n_storage=20, n_events=0, n_l1_messages=0),
              synthetic.block_after_vm(seed=66, n_vm_memory=1300, n_storage=90, n_decommits=40, n_bytecodes=9),
              synthetic.block_after_vm(seed=67, n_vm_memory=600, n_storage=10, n_events=3, n_l1_messages=1, n_precompile_calls=(1, 0, 2))]
    NO_TREE = 5
    shared_slots, shared_users, own = {}, [], {}
    for k, sh in enumerate(shapes):
        if k == NO_TREE:
            continue
        dedup, _qt = _dedup_queries(nv, sh)
        slots = {oracle.derive_final_address(q): _value_of(q) for q in dedup}  # (a zero value: the slot must be empty before the block)
        if all(shared_slots.get(key, v) == v for key, v in slots.items()):
            shared_slots.update(slots)
            shared_users.append(k)
        else:
            own[k] = slots
    assert len(shared_users) >= 2

    def tree_of(slots, seed):
        rng = np.random.default_rng(seed)
        pairs = [(rng.bytes(32), rng.bytes(32)) for _ in range(10)] + [(key, v) for key, v in slots.items() if any(v)]
        t = nv.StorageTreeDevice(ctx, 1024)
        t.insert(_rows([key for key, _ in pairs]), _rows([v for _, v in pairs]))
        return t

    shared = tree_of(shared_slots, 1)
    trees = [None if k == NO_TREE else shared if k in shared_users else tree_of(own[k], 2 + k) for k in range(len(shapes))]
    many = nv.Block.run_many(0, shapes, CAPS, storage_tree_device=trees)
    total_sap = 0
    for k, (sh, m) in enumerate(zip(shapes, many)):
        if trees[k] is None:
            assert m.num_instances(SAP) == 0 and m.public_inputs(SAP) is None
            continue
        one = nv.Block(0, sh, CAPS, storage_tree_device=trees[k])
        rm, ro = _sap_record(nv, m), _sap_record(nv, one)
        for key in ro:
            assert rm[key] == ro[key], (k, key)
        assert rm["n"] >= 1
        total_sap += rm["n"]
        one.free()
    assert many[3].num_instances(SAP) == 1  # no storage queries: the dummy instance
    bad, lock, local, checkers = [], threading.Lock(), threading.local(), []

    def cb(bi, t, i, tr, s, pi):
        if t != SAP:
            return
        if not hasattr(local, "ctx"):  # a checker context per calling thread (include/zkw.h, zkw_blocks_synthesize)
            local.ctx = nv.Context(0)
            with lock:
                checkers.append(local.ctx)
        v = many[bi].check_satisfied(SAP, tr, s, ctx=local.ctx)[0]
        with lock:
            bad.append((bi, i, v))

    n = nv.Block.synthesize_many(many, 1 << 18, ring_slots=1, callback=cb)
    order = (4, 8, 10, 2, 3, 5, 6, 7, 9, 11, 12, 13)
    assert n == sum(m.num_instances(t) for m in many for t in order)
    assert len(bad) == total_sap >= 8 and not any(v for *_x, v in bad), [x for x in bad if x[2]][:5]
    assert sorted((bi, i) for bi, i, _v in bad) == [(bi, i) for bi, m in enumerate(many) for i in range(m.num_instances(SAP))]
    for c in checkers:
        c.close()
    nv.Block.free_many(many)
    for t in set(x for x in trees if x is not None):
        t.free()
