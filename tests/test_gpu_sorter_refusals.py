"""The refused calls of the four sorter circuits' synthesis and of the seven non-RAM witness accessors: error code and full message,
nothing written, and the slot still good for a correct call afterwards. Every refusal returns before any launch.

Sizes: the smallest case of each circuit's own synthesis test. Row counts from the generated specs (region stride 64 at capacity 8):
rows needed = rows per cycle x 64 + the boundary rows = 7 x 64 + 54, 13 x 64 + 56, 12 x 64 + 33, 22 x 64 + 54."""
import ctypes as C

import numpy as np
import pytest

from era_zkevm_test_harness_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


def _refused(call, msg):
    from era_zkevm_test_harness_amd import native

    with pytest.raises(native.ZkwError) as ei:
        call()
    assert ei.value.code == native.ERR_INVALID
    assert str(ei.value) == f"libzkw error {native.ERR_INVALID}: {msg}"


def _decommit(ctx, oracle):
    q = synthetic.decommit_trace(5, 5, seed=5)
    return dict(name="decommit_sorter", capacity=8, n_rows=512, need=502, cols=None, short_cols=None, q=q,
                build_at=lambda cap: ctx.compute_decommitts_sorter_circuit_snapshots(q, cap), synth=ctx.synthesize_decommit_sorter,
                o=oracle.decommit_sorter_build(q, 8), oracle_synth=oracle.decommit_sorter_synthesize, width=149)


def _events(ctx, oracle):
    q = synthetic.events_trace(3, 1.0, seed=3)
    return dict(name="events_sorter", capacity=8, n_rows=2048, need=888, cols=None, short_cols=None, q=q,
                build_at=lambda cap: ctx.compute_events_dedup_and_sort(q, cap), synth=ctx.synthesize_events_sorter,
                o=oracle.events_sorter_build(q, 8), oracle_synth=oracle.events_sorter_synthesize, width=139)


def _demux(ctx, oracle):
    q = synthetic.mixed_log_queue(5, seed=5)
    return dict(name="log_demux", capacity=8, n_rows=1024, need=801, cols=151, q=q,
                short_cols=(150, "trace has 150 columns, the LogDemuxer needs 151 (zkw_trace_create_with_columns)"),
                build_at=lambda cap: ctx.compute_logs_demux(q, cap), synth=ctx.synthesize_log_demux,
                o=oracle.log_demux_build(q, 8), oracle_synth=oracle.log_demux_synthesize, width=151)


def _storage(ctx, oracle):
    q = synthetic.storage_trace(7, 2, seed=7)
    return dict(name="storage_sorter", capacity=8, n_rows=2048, need=1462, cols=None, q=q,
                short_cols=(148, "trace has 148 columns, the StorageSorter needs 149"),
                build_at=lambda cap: ctx.compute_storage_dedup_and_sort(q, cap), synth=ctx.synthesize_storage_sorter,
                o=oracle.storage_sorter_build(q, 8), oracle_synth=oracle.storage_sorter_synthesize, width=149)


def _demux_with_other_params(ctx, q, capacity):
    """a demux witness whose routing constants are not ZKW_DEMUX_PARAMS_DEFAULT (another ecrecover address: those logs are dropped, not violations)"""
    from era_zkevm_test_harness_amd import native

    class Params(C.Structure):
        _fields_ = [("aux", C.c_uint8 * 4), ("keccak256_address", C.c_uint32), ("sha256_address", C.c_uint32), ("ecrecover_address", C.c_uint32)]

    p = Params((C.c_uint8 * 4)(0, 1, 2, 3), 0x8010, 0x02, 0x05)
    assert C.sizeof(p) == 16
    w = native.DemuxWitness(ctx)
    q = np.ascontiguousarray(q, dtype=native.LOG_QUERY)
    native._check(native.load().zkw_log_demux_build(ctx.handle, native._np_ptr(q), q.size, capacity, C.cast(C.byref(p), C.c_void_p), C.byref(w.handle)))
    return w


@pytest.mark.parametrize("case", [_decommit, _events, _demux, _storage])
def test_synthesis_refusals(ctx, oracle, case):
    from era_zkevm_test_harness_amd import native

    c = case(ctx, oracle)
    capacity, n_rows, synth = c["capacity"], c["n_rows"], c["synth"]
    w = c["build_at"](capacity)
    n_inst = int(w.num_instances)
    assert n_inst == c["o"]["instances"].size == 1
    expected = c["oracle_synth"](c["o"], 0, capacity, n_rows)

    t = native.Trace(ctx, n_rows, 1, n_cols=c["cols"])

    def good():
        synth(w, t, 0, 1, 0)
        assert np.array_equal(t.get(0)[:c["width"]], expected)

    def refused_in_t(call, msg):
        before = t.get(0)
        _refused(call, msg)
        assert np.array_equal(t.get(0), before)
        good()  # the refused call left the slot's tag "unknown" or true: a correct call still gives the oracle's trace

    good()
    refused_in_t(lambda: synth(w, t, 1, 1, 0), "instance range out of bounds")
    refused_in_t(lambda: synth(w, t, 0, 2, 0), "instance range out of bounds")
    if c["name"] == "log_demux":
        other = _demux_with_other_params(ctx, c["q"], capacity)
        refused_in_t(lambda: synth(other, t, 0, 1, 0),
                     "the LogDemuxer circuit hard-wires ZKW_DEMUX_PARAMS_DEFAULT; this witness was built with other routing constants")
        other.free()
    t.free()

    def refused_elsewhere(trace, call, msg):
        before = [trace.get(s) for s in range(trace.n_slots)]
        _refused(call, msg)
        for s in range(trace.n_slots):
            assert np.array_equal(trace.get(s), before[s])
        trace.free()

    # more instances than slots: the same queue at capacity 2 (several instances) and a ring one slot short
    wm = c["build_at"](2)
    n_many = int(wm.num_instances)
    assert n_many >= 3
    t2 = native.Trace(ctx, n_rows, n_many - 1, n_cols=c["cols"])
    refused_elsewhere(t2, lambda: synth(wm, t2, 0, n_many, 0), f"more instances ({n_many}) than trace slots ({n_many - 1})")
    wm.free()

    need = c["need"]
    short = need - 2 if need % 2 == 0 else need - 1  # even: only the row count is wrong
    ts = native.Trace(ctx, short, 1, n_cols=c["cols"])
    refused_elsewhere(ts, lambda: synth(w, ts, 0, 1, 0), f"capacity {capacity} needs {need} rows, trace has {short}")
    to = native.Trace(ctx, n_rows + 1, 1, n_cols=c["cols"])
    refused_elsewhere(to, lambda: synth(w, to, 0, 1, 0), "trace length must be even (it is a power of two in every circuit)")
    if c["short_cols"]:
        n_cols, msg = c["short_cols"]
        tc = native.Trace(ctx, n_rows, 1, n_cols=n_cols)
        refused_elsewhere(tc, lambda: synth(w, tc, 0, 1, 0), msg)
    w.free()


def _w_decommit(ctx, oracle):
    return ctx.compute_decommitts_sorter_circuit_snapshots(synthetic.decommit_trace(5, 5, seed=5), 8)


def _w_events(ctx, oracle):
    return ctx.compute_events_dedup_and_sort(synthetic.events_trace(3, 1.0, seed=3), 8)


def _w_demux(ctx, oracle):
    return ctx.compute_logs_demux(synthetic.mixed_log_queue(5, seed=5), 8)


def _w_storage(ctx, oracle):
    return ctx.compute_storage_dedup_and_sort(synthetic.storage_trace(7, 2, seed=7), 8)


def _w_decommitter(ctx, oracle):
    from tests.test_oracle_ram import _bytecodes

    req, tails, words, woff = _bytecodes(oracle, 1, seed=6)
    return ctx.compute_decommitter_circuit_snapshots(req, tails, words, woff, 4, np.zeros(1, oracle.QUEUE_STATE12))


def _w_precompile(ctx, oracle):
    from era_zkevm_test_harness_amd import native

    req, mq = synthetic.precompile_trace(0, 1, seed=7, max_rounds=6)
    new = oracle.queue_push_chain_log(oracle.encode_log_queries(req))[1]
    return ctx._precompile(0, req, new, mq, 1, np.zeros(1, native.QUEUE_STATE12))


def _w_storage_application(ctx, oracle):
    from sap_case import storage_application_case

    q, tails, tree, idx, paths = storage_application_case(oracle, 1, seed=12)
    return ctx.decompose_into_storage_application_witnesses(q, tails, idx, paths, tree.root, tree.next_enumeration_index, 33)


# (C symbol prefix, builder, largest valid `what`, what zkw_*_witness_get answers to what = -1)
ACCESSORS = [("decommit", _w_decommit, 12, "empty"),  # the decommit sorter's get looks the array up first: a negative `what` is an empty array
             ("events", _w_events, 14, "refused"), ("demux", _w_demux, 10, "refused"), ("storage", _w_storage, 16, "refused"),
             ("decommitter", _w_decommitter, 5, "refused"), ("precompile", _w_precompile, 4, "refused"),
             ("storage_application", _w_storage_application, 4, "refused")]


@pytest.mark.parametrize("prefix,build,last,negative", ACCESSORS, ids=[a[0] for a in ACCESSORS])
def test_witness_accessor_refusals(ctx, oracle, prefix, build, last, negative):
    from era_zkevm_test_harness_amd import native

    lib = native.load()
    w = build(ctx, oracle)
    n_bytes = getattr(lib, f"zkw_{prefix}_witness_bytes")
    get = getattr(lib, f"zkw_{prefix}_witness_get")

    def err(rc, msg):
        assert rc == native.ERR_INVALID and lib.zkw_last_error().decode() == msg

    assert n_bytes(w.handle, -1) == 0 and n_bytes(w.handle, last + 1) == 0
    buf = np.zeros(64, np.uint8)
    err(get(w.handle, last + 1, native._np_ptr(buf), buf.size), f"unknown array {last + 1}")
    if negative == "refused":
        err(get(w.handle, -1, native._np_ptr(buf), buf.size), "unknown array -1")
    else:
        assert get(w.handle, -1, native._np_ptr(buf), buf.size) == native.OK and not buf.any()
    err(get(w.handle, 0, None, 1 << 30), f"zkw_{prefix}_witness_get: null argument")
    err(get(None, 0, native._np_ptr(buf), buf.size), f"zkw_{prefix}_witness_get: null argument")
    some = 0
    for what in range(last + 1):
        b = n_bytes(w.handle, what)
        out = np.zeros(max(b, 1), np.uint8)
        assert get(w.handle, what, native._np_ptr(out), b) == native.OK, what
        if b:
            some += 1
            err(get(w.handle, what, native._np_ptr(out), b - 1), f"need {b} bytes, got {b - 1}")
    assert some  # (an array may be empty: a keccak witness has no SHA-256 rounds)
    w.free()
