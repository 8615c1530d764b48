"""The refused calls of the eight witness builders and of the storage-tree tables, as native.py delivers them: error code and full message,
the handle passed by reference still NULL, and a correct build on the same context right afterwards equal to the oracle array for array.

Two kinds. A refusal of an ARGUMENT returns before anything is read or queued (the size limits go through a raw call with a one-element
array and the count alone at the limit). A refusal AFTER ALLOCATION drops a witness whose buffers queued kernels have written: each is
made three times in a row before the good build, which takes the dropped buffers out of the allocation cache again — a buffer handed
back while queued work still wrote it would show there.

Inputs: the smallest ones tests/test_gpu_ram_path.py and tests/test_gpu_storage_witness_*.py use for the same refusals. A count inside a
message comes from how the input was made (one record changed: one record in violation), for the storage log from a restatement of the
reference's asserts. A failed launch or allocation cannot be provoked on a shared machine and is not tried."""
import ctypes as C

import numpy as np
import pytest

from era_zkevm_test_harness_amd import synthetic
from tests import storage_witness_chain_model as chain_model
from tests import storage_witness_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


def _handles_of(ei):
    """the handles the wrapper that raised passed by reference: its witness object (`w`, `t`) or its array of table handles"""
    found, tb = [], ei.tb
    while tb is not None:
        if tb.tb_frame.f_code.co_filename.endswith("native.py"):
            for name, v in tb.tb_frame.f_locals.items():
                if name in ("w", "t") and hasattr(v, "handle"):
                    found.append(v.handle.value)
                elif name == "handles":
                    found.extend(v[i] for i in range(len(v)))
                elif name == "last" and isinstance(v, C.c_void_p):
                    found.append(v.value)
        tb = tb.tb_next
    return found


def _refused(call, code, msg, handle=None):
    """`handle`: the c_void_p a raw call passed by reference; a wrapper's own is found in its frame"""
    from era_zkevm_test_harness_amd import native

    with pytest.raises(native.ZkwError) as ei:
        call()
    assert ei.value.code == code
    assert str(ei.value) == f"libzkw error {code}: {msg}"
    handles = [handle.value] if handle is not None else _handles_of(ei)
    assert handles and not any(handles), handles


def _raw(symbol, *args):
    """(call, handle) of a raw call of a builder entry whose last argument is the handle by reference"""
    from era_zkevm_test_harness_amd import native

    h = C.c_void_p(None)
    return (lambda: native._check(getattr(native.load(), symbol)(*args, C.byref(h)))), h


def _fields_equal(a, b, path=""):
    if a.dtype.names:
        for f in a.dtype.names:
            _fields_equal(a[f], b[f], f"{path}.{f}")
    else:
        assert a.tobytes() == b.tobytes(), path


def _witness_equal(w, o, arrays, instances):
    for what, key in arrays:
        assert np.array_equal(w.get(what), o[key]), key
    gi = w.get(instances)
    assert gi.size == o["instances"].size
    _fields_equal(gi, o["instances"])
    w.free()


def _one(dtype):
    return np.zeros(1, dtype)


# ------------------------------------------------------------------------------------------------ the four sorters
def test_decommit_sorter(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv

    q = synthetic.decommit_trace(40, 3, seed=2)
    build = ctx.compute_decommitts_sorter_circuit_snapshots
    _refused(lambda: build(q, 0), nv.ERR_INVALID, "zkw_decommit_sorter_prepare: bad argument")
    _refused(lambda: build(q[:0], 16), nv.ERR_INVALID, "VM should have made some code decommits (sort_decommit_requests.rs:38-41)")
    call, h = _raw("zkw_decommit_sorter_build", ctx.handle, nv._np_ptr(_one(nv.DECOMMIT_QUERY)), 1 << 32, 16, None)
    _refused(call, nv.ERR_INVALID, "too many requests", h)
    bad = q.copy()
    bad["memory_page"][-1] += 1
    for _ in range(3):
        _refused(lambda: build(bad, 16), nv.ERR_CHECK_FAILED, "decommit requests with the same hash disagree on page or are not "
                 "timestamp-ordered (sort_decommit_requests.rs:99-114)")
    _witness_equal(build(q, 16), oracle.decommit_sorter_build(q, 16),
                   ((nv.DEC_SORTED_QUERIES, "sorted_q"), (nv.DEC_UNSORTED_ENC, "unsorted_enc"), (nv.DEC_SORTED_ENC, "sorted_enc"),
                    (nv.DEC_UNSORTED_TAILS, "unsorted_tails"), (nv.DEC_SORTED_TAILS, "sorted_tails"), (nv.DEC_DEDUP_QUERIES, "dedup_q"),
                    (nv.DEC_DEDUP_TAILS, "dedup_tails"), (nv.DEC_CHALLENGES, "challenges"), (nv.DEC_LHS_Z, "lhs_z"), (nv.DEC_RHS_Z, "rhs_z")),
                   nv.DEC_INSTANCES)


def test_events_sorter(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv

    q = synthetic.events_trace(10, 0.0, seed=3)
    build = ctx.compute_events_dedup_and_sort
    _refused(lambda: build(q, 0), nv.ERR_INVALID, "zkw_events_sorter_build: bad argument")
    call, h = _raw("zkw_events_sorter_build", ctx.handle, nv._np_ptr(_one(nv.LOG_QUERY)), 1 << 31, 16, None)
    _refused(call, nv.ERR_INVALID, "too many log queries", h)
    bad = q.copy()
    bad["rollback"][4] = 1  # ten forward events with their own timestamps: this one alone is a rollback without its forward event
    for _ in range(3):
        _refused(lambda: build(bad, 16), nv.ERR_CHECK_FAILED, "event queue is not a sequence of forward events each optionally followed by "
                 "its own rollback (events_sort_dedup.rs:344-356, 512-533): 1 violations")
    _witness_equal(build(q, 16), oracle.events_sorter_build(q, 16),
                   ((nv.EVT_SORTED_QUERIES, "sorted_q"), (nv.EVT_UNSORTED_ENC, "unsorted_enc"), (nv.EVT_SORTED_ENC, "sorted_enc"),
                    (nv.EVT_UNSORTED_OLD_TAILS, "unsorted_old_tails"), (nv.EVT_UNSORTED_NEW_TAILS, "unsorted_new_tails"),
                    (nv.EVT_SORTED_OLD_TAILS, "sorted_old_tails"), (nv.EVT_SORTED_NEW_TAILS, "sorted_new_tails"),
                    (nv.EVT_RESULT_QUERIES, "result_q"), (nv.EVT_RESULT_NEW_TAILS, "result_new_tails"), (nv.EVT_CHALLENGES, "challenges"),
                    (nv.EVT_LHS_Z, "lhs_z"), (nv.EVT_RHS_Z, "rhs_z")), nv.EVT_INSTANCES)


def test_log_demux(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv

    q = synthetic.mixed_log_queue(50, seed=1)
    build = ctx.compute_logs_demux
    _refused(lambda: build(q, 0), nv.ERR_INVALID, "zkw_log_demux_build: bad argument")
    call, h = _raw("zkw_log_demux_build", ctx.handle, nv._np_ptr(_one(nv.LOG_QUERY)), 1 << 31, 16, None)
    _refused(call, nv.ERR_INVALID, "too many log queries", h)
    bad = q.copy()
    bad["aux_byte"][7] = 9  # every record is routed on its own: this one alone has no route
    for _ in range(3):
        _refused(lambda: build(bad, 16), nv.ERR_CHECK_FAILED, "1 log queries have an aux byte / shard / rollback combination the "
                 "reference treats as unreachable (log_demux.rs:174-249)")
    _witness_equal(build(q, 16), oracle.log_demux_build(q, 16),
                   ((nv.DMX_IN_ENC, "in_enc"), (nv.DMX_IN_OLD_TAILS, "in_old_tails"), (nv.DMX_IN_NEW_TAILS, "in_new_tails"),
                    (nv.DMX_OUT_QUERIES, "out_q"), (nv.DMX_OUT_ENC, "out_enc"), (nv.DMX_OUT_OLD_TAILS, "out_old_tails"),
                    (nv.DMX_OUT_NEW_TAILS, "out_new_tails"), (nv.DMX_OUT_OFFSETS, "out_offsets")), nv.DMX_INSTANCES)


def _storage_log_violations(q):
    """the asserts of sort_storage_access.rs:64-203 over a storage log in queue order (shard 0), counted per record as the builder counts
    them: a cell that starts with a rollback, every record below depth zero, and a cell that ends at depth zero on another value than it
    started from"""
    cells = {}
    for r in q:
        cells.setdefault((r["address"].tobytes(), r["key"].tobytes()), []).append(r)
    bad = 0
    for records in cells.values():
        depth, reads_at_zero = 0, 0
        bad += int(records[0]["rw_flag"] and records[0]["rollback"])
        for r in records:
            depth += (-1 if r["rollback"] else 1) if r["rw_flag"] else 0
            bad += depth < 0
            reads_at_zero += (not r["rw_flag"]) and depth == 0
        last = records[-1]
        current = last["written_value"] if last["rw_flag"] and not last["rollback"] else last["read_value"]
        if (depth > 0 or reads_at_zero) and depth == 0:
            bad += current.tobytes() != records[0]["read_value"].tobytes()
    return bad


def test_storage_sorter(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv

    q = synthetic.storage_trace(40, 3, seed=9, p_rollback=0.0)
    assert _storage_log_violations(q) == 0
    build = ctx.compute_storage_dedup_and_sort
    _refused(lambda: build(q, 0), nv.ERR_INVALID, "zkw_storage_sorter_build: bad argument")
    call, h = _raw("zkw_storage_sorter_build", ctx.handle, nv._np_ptr(_one(nv.LOG_QUERY)), 1 << 31, 16)
    _refused(call, nv.ERR_INVALID, "too many log queries", h)
    bad = q.copy()
    bad["rw_flag"][0], bad["rollback"][0] = 1, 1  # a rollback with nothing to roll back
    violations = _storage_log_violations(bad)
    assert violations >= 2  # the cell starts with a rollback, and that record is below depth zero
    for _ in range(3):
        _refused(lambda: build(bad, 16), nv.ERR_CHECK_FAILED, f"storage log is not a consistent history ({violations} violations of the asserts at "
                 "sort_storage_access.rs:64-203)")
    _witness_equal(build(q, 16), oracle.storage_sorter_build(q, 16),
                   ((nv.STO_SORTED_QUERIES, "sorted_q"), (nv.STO_SORTED_EXT_TS, "sorted_ext_ts"), (nv.STO_UNSORTED_ENC, "unsorted_enc"),
                    (nv.STO_LHS_ENC, "lhs_enc"), (nv.STO_SORTED_ENC, "sorted_enc"), (nv.STO_UNSORTED_OLD_TAILS, "unsorted_old_tails"),
                    (nv.STO_UNSORTED_NEW_TAILS, "unsorted_new_tails"), (nv.STO_SORTED_OLD_TAILS, "sorted_old_tails"),
                    (nv.STO_SORTED_NEW_TAILS, "sorted_new_tails"), (nv.STO_RESULT_QUERIES, "result_q"),
                    (nv.STO_RESULT_NEW_TAILS, "result_new_tails"), (nv.STO_CHALLENGES, "challenges"), (nv.STO_LHS_Z, "lhs_z"),
                    (nv.STO_RHS_Z, "rhs_z")), nv.STO_INSTANCES)


# ------------------------------------------------------------------------------------------------ decommitter, precompiles, storage application
def test_decommitter(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv
    from tests.test_oracle_ram import _bytecodes

    req, tails, words, woff = _bytecodes(oracle, 1, seed=6)
    mem_in = np.zeros(1, oracle.QUEUE_STATE12)
    mem_in["tail"] = synthetic.random_field_elements(9, (12,))
    mem_in["length"] = 77
    build = ctx.compute_decommitter_circuit_snapshots
    _refused(lambda: build(req, tails, words, woff, 0, mem_in), nv.ERR_INVALID, "zkw_decommitter_build: bad argument")
    _refused(lambda: build(req[:0], tails[:0], words, woff[:1], 4, mem_in), nv.ERR_INVALID, "zkw_decommitter_build: bad argument")
    _refused(lambda: build(req, tails, words, woff[[0, 0]], 4, mem_in), nv.ERR_INVALID, "request 0 has no bytecode (decommit_code.rs:236)")
    bad = words.copy()
    bad[-1, 3] ^= 0x10  # one request, one bit of its bytecode: its digest is another one
    for _ in range(3):
        _refused(lambda: build(req, tails, bad, woff, 4, mem_in), nv.ERR_CHECK_FAILED, "1 bytecodes do not match their decommit request "
                 "(length parity, word count or SHA-256 digest, decommit_code.rs:241-244, 323-337)")
    _witness_equal(build(req, tails, words, woff, 4, mem_in), oracle.decommitter_build(req, tails, words, woff, 4, mem_in),
                   ((nv.DCM_MEM_QUERIES, "mem_q"), (nv.DCM_MEM_ENC, "mem_enc"), (nv.DCM_MEM_TAILS, "mem_tails"),
                    (nv.DCM_ROUND_STATES, "round_states")), nv.DCM_INSTANCES)


def test_precompile(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv

    req, mq = synthetic.precompile_trace(0, 10, seed=5)
    new = oracle.queue_push_chain_log(oracle.encode_log_queries(req))[1]
    mem_in = np.zeros(1, nv.QUEUE_STATE12)
    build = ctx._precompile
    _refused(lambda: build(0, req, new, mq, 0, mem_in), nv.ERR_INVALID, "zkw_precompile_build: bad argument")
    _refused(lambda: build(0, req[:0], new[:0], mq, 3, mem_in), nv.ERR_INVALID, "memory queries without a precompile request")
    _refused(lambda: build(0, req, new, mq[:-1], 3, mem_in), nv.ERR_INVALID, f"the requests need {mq.size} memory queries, {mq.size - 1} given")
    bad = mq.copy()
    bad["rw_flag"][-1] = 0  # the last request's write is a read: that request alone does not fit its ABI
    for _ in range(3):
        _refused(lambda: build(0, req, new, bad, 3, mem_in), nv.ERR_CHECK_FAILED, "1 requests whose memory queries do not fit their ABI "
                 "(read/write flags, word index or count: the asserts of the round walks)")
    w, o = build(0, req, new, mq, 3, mem_in), oracle.precompile_build(0, req, new, mq, 3, mem_in)
    assert w.num_instances == o["instances"].size
    assert w.get(nv.PRC_KECCAK_ROUNDS).tobytes() == o["keccak_rounds"].tobytes()
    _witness_equal(w, o, ((nv.PRC_MEM_ENC, "mem_enc"), (nv.PRC_MEM_TAILS, "mem_tails")), nv.PRC_INSTANCES)


def test_storage_application(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv
    from sap_case import storage_application_case

    n = 50
    q, tails, tree, idx, paths = storage_application_case(oracle, n, seed=3)
    root0, next0 = tree.root, tree.next_enumeration_index
    build = ctx.decompose_into_storage_application_witnesses
    for capacity in (0, 1):
        _refused(lambda: build(q, tails, idx, paths, root0, next0, capacity), nv.ERR_INVALID, "zkw_storage_application_build: bad argument")
    one = [nv._np_ptr(a) for a in (_one(nv.LOG_QUERY), np.zeros(4, np.uint64), np.zeros(1, np.uint64), np.zeros(256 * 32, np.uint8))]
    root = np.frombuffer(root0, np.uint8).copy()
    call, h = _raw("zkw_storage_application_build", ctx.handle, one[0], one[1], 1 << 31, one[2], one[3], nv._np_ptr(root), next0, 33)
    _refused(call, nv.ERR_INVALID, "too many storage queries", h)
    # the LAST query: no later one walks over what it wrote, so it alone contradicts the tree
    bad_paths = paths.copy()
    bad_paths[n - 1, 100, 5] ^= 1
    bad_q = q.copy()
    bad_q["read_value"][n - 1][0] ^= 1
    message = ("1 storage queries contradict the tree: the pre-state proof does not lead to the initial root, the read value is not the "
               "leaf's (storage_application.rs:221,276), or a slot occurs twice")
    for _ in range(3):
        _refused(lambda: build(q, tails, idx, bad_paths, root0, next0, 33), nv.ERR_CHECK_FAILED, message)
    for _ in range(3):
        _refused(lambda: build(bad_q, tails, idx, paths, root0, next0, 33), nv.ERR_CHECK_FAILED, message)
    w = build(q, tails, idx, paths, root0, next0, 33)
    o = oracle.storage_application_build(tree, q, tails, 33)  # mutates the tree
    _witness_equal(w, o, ((nv.SAP_DERIVED_KEYS, "derived_keys"), (nv.SAP_LEAF_INDEXES, "leaf_indexes"), (nv.SAP_ROOTS, "roots"),
                          (nv.SAP_MERKLE_PATHS, "merkle_paths")), nv.SAP_INSTANCES)


# ------------------------------------------------------------------------------------------------ RAM
def test_ram(ctx, oracle):
    from era_zkevm_test_harness_amd import native as nv
    from tests.test_gpu_ram_path import _assert_witness_equal

    q = synthetic.ram_trace(64, seed=1064)
    w = nv.RamWitness(ctx)
    build = lambda queries, capacity: ctx.compute_ram_circuit_snapshots(queries, capacity, 3, witness=w)
    _refused(lambda: build(q, 0), nv.ERR_INVALID, "zkw_ram_build_instances_batch: bad argument", w.handle)
    _refused(lambda: build(q[:0], 64), nv.ERR_INVALID, "block 0 is empty: the VM must have made memory requests (W/ram_permutation.rs:43-46)", w.handle)
    offsets, nd = np.array([0, 1 << 32], np.uint64), np.zeros(1, np.uint32)
    call, h = _raw("zkw_ram_build_instances_batch", ctx.handle, nv._np_ptr(_one(nv.MEM_QUERY)), nv._np_ptr(offsets), 1, 64, nv._np_ptr(nd))
    _refused(call, nv.ERR_INVALID, "more than 2^32-1 queries in one batch", h)
    build(q, 64)
    o = oracle.ram_build_instances(q, 64, 3)
    assert w.num_instances == o["instances"].size
    _assert_witness_equal(w, o, nv)
    w.free()


# ------------------------------------------------------------------------------------------------ storage-tree tables
def _rows(items):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, 32)


def test_storage_tree_tables(ctx, oracle):
    """from_proofs with a bad path, advance and advance_chain with a key outside the table (tests/test_gpu_storage_witness_tree.py, _advance.py,
    _chain.py), each followed by the correct call against the host models"""
    from era_zkevm_test_harness_amd import native as nv
    from tests.test_gpu_storage_witness_advance import _oracle_answers, _same

    rng = np.random.default_rng(28)
    tree = oracle.Tree()
    leaves = [rng.bytes(32) for _ in range(20)]
    for k in leaves:
        tree.insert_leaf(k, rng.bytes(32))
    keys = leaves[:6] + [rng.bytes(32) for _ in range(3)]  # six present, three absent
    outside = rng.bytes(32)
    idx, val, paths = _oracle_answers(tree, keys)
    root, nxt = tree.root, tree.next_enumeration_index
    m = model.Table(keys, idx, val, paths, root, nxt)

    forged = paths.copy()
    forged[4, 128, 7] ^= 0x10
    for _ in range(3):
        _refused(lambda: nv.StorageTreeDevice.from_proofs(ctx, _rows(keys), idx, val, forged, root, nxt), nv.ERR_INVALID,
                 "zkw_storage_tree_create_witness: entry 4 is not a proof for this root: its Merkle path does not lead to the root")
    wt = nv.StorageTreeDevice.from_proofs(ctx, _rows(keys), idx, val, paths, root, nxt)
    _same(wt.get_leaves(keys), m.answers(keys), "host model")

    pairs = [(keys[1], rng.bytes(32)), (keys[7], rng.bytes(32)), (keys[1], rng.bytes(32))]
    stray = pairs[:2] + [(outside, rng.bytes(32))]
    for _ in range(3):
        _refused(lambda: wt.advance(_rows([k for k, _v in stray]), _rows([v for _k, v in stray])), nv.ERR_INVALID,
                 "zkw_storage_tree_advance_witness: the key written at position 2 is not in the witness tree")
    after = wt.advance(_rows([k for k, _v in pairs]), _rows([v for _k, v in pairs]))
    m_after = m.advance(pairs)
    _same(after.get_leaves(keys), m_after.answers(keys), "host model")
    assert (after.root, after.next_enumeration_index, after.num_leaves) == (m_after.root, m_after.next_enumeration_index, m_after.num_leaves)
    after.free()

    blocks = [pairs[:2], pairs[2:]]
    args = lambda bs: [(_rows([k for k, _v in b]), _rows([v for _k, v in b])) for b in bs]
    for _ in range(3):
        _refused(lambda: wt.advance_chain_pairs(args([pairs[:2], [pairs[2], (outside, rng.bytes(32))]]), final=True), nv.ERR_INVALID,
                 "zkw_storage_tree_advance_witness_chain_pairs: the key at (block 1, position 1) is not in the witness tree")
    outs, last = wt.advance_chain_pairs(args(blocks), final=True)
    m_outs, m_last = chain_model.chain(m, [[(k, v, True) for k, v in b] for b in blocks])
    for t, mo in zip(outs + [last], m_outs + [m_last]):
        asked = sorted(mo.entries)
        assert (t.capacity, t.num_leaves, t.root, t.next_enumeration_index) == (len(asked), mo.num_leaves, mo.root, mo.next_enumeration_index)
        _same(t.get_leaves(asked), mo.answers(asked), "host model")
        t.free()
    _same(wt.get_leaves(keys), m.answers(keys), "the input")
    wt.free()
