"""The profile of one call of each host unit: which spans a call records and how many launches each counts, exactly.

Every launch statement opens its own span (csrc/zkw_ctx.h: LaunchAt), under the kernel's name unless the statement names another one
(`span_as`), with none for the inner launches of the radix sort and of the prefix scans (`no_span`: they run under the caller's
"radix_sort" span) — and an empty grid launches nothing but still records its span and counts one launch. The roofline of bench.py and
the tools/probe_* scripts read these names and counts, so a launch that loses its span, gains one or changes its name shows here.

The tables below were recorded by running this file against a library built from the commit BEFORE the launch statements were folded
(loaded through ZKW_LIB), where it passed first; times are only required to be non-negative. Inputs: the smallest ones the unit's own GPU
test uses.

The refusal of a context of a batch by `launch_direct` / `direct_only` cannot be reached from Python: such a context exists only inside
zkw_blocks_run, whose fibers call none of the directly launched kernels."""
import json

import numpy as np
import pytest

from era_zkevm_test_harness_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    c.profile_enable(True)
    yield c
    c.close()


def _rows32(items):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, 32) if items else np.zeros((0, 32), np.uint8)


def _decommit_sorter(ctx, oracle):
    """build, synthesis and check_satisfied of the decommit sorter (tests/test_gpu_sorter_refusals.py: capacity 8 in 512 rows)"""
    from era_zkevm_test_harness_amd import native

    w = ctx.compute_decommitts_sorter_circuit_snapshots(synthetic.decommit_trace(5, 5, seed=5), 8)
    t = native.Trace(ctx, 512, 1)
    ctx.synthesize_decommit_sorter(w, t, 0, 1, 0)
    assert ctx.check_if_satisfied(2, t, 0, 8)[0] == 0
    return [t, w]


def _ram(ctx, oracle):
    """build and synthesis of the RAM permutation (tests/test_gpu_ram_synth_launches.py: 100 items at capacity 64)"""
    from era_zkevm_test_harness_amd import native
    from era_zkevm_test_harness_amd.ram_circuit import min_rows

    w = ctx.compute_ram_circuit_snapshots(synthetic.ram_trace(100, seed=910, pages=3, indices=16), 64, 0)
    n_rows = 256
    while n_rows < min_rows(64):
        n_rows *= 2
    t = native.Trace(ctx, n_rows, 2)
    ctx.synthesize_ram(w, t, 0, 2, 0)
    return [t, w]


def _keccak(ctx, oracle):
    """build, synthesis and check_satisfied of the Keccak precompile (tests/test_gpu_netlist_circuits.py: 6 requests at capacity 6)"""
    from era_zkevm_test_harness_amd import native

    req, mq = synthetic.precompile_trace(0, 6, seed=3, max_rounds=4)
    tails = oracle.queue_push_chain_log(oracle.encode_log_queries(req))[1]
    w = ctx._precompile(0, req, tails, mq, 6, np.zeros(1, native.QUEUE_STATE12))
    t = native.Trace(ctx, 1 << 18, 1, n_cols=native.KC_COLS)
    ctx.synthesize_keccak_round_function(w, t, 0, 1, 0)
    assert ctx.check_if_satisfied(5, t, 0, 6)[0] == 0
    return [t, w]


def _storage_tree(ctx, oracle):
    """two leaves: one workgroup folds all the levels (tests/test_gpu_storage_tree.py, n = 2)"""
    from era_zkevm_test_harness_amd import native

    rng = np.random.default_rng(102)
    keys, values = [rng.bytes(32) for _ in range(2)], [rng.bytes(32) for _ in range(2)]
    t = native.StorageTreeDevice(ctx, 2)
    t.insert(_rows32(keys), _rows32(values))
    assert t.num_leaves == 2
    return [t]


def _storage_witness_without_writes(ctx, oracle):
    """a witness tree advanced by NO writes (tests/test_gpu_storage_witness_advance.py, "n == 0"): k_swa_locate, k_swa_leaves and
    k_swa_fold have empty grids"""
    from era_zkevm_test_harness_amd import native

    rng = np.random.default_rng(103)
    keys, values = [rng.bytes(32) for _ in range(4)], [rng.bytes(32) for _ in range(4)]
    t = native.StorageTreeDevice(ctx, 16)
    t.insert(_rows32(keys), _rows32(values))
    wt = t.extract_witness(_rows32(keys[:2] + [rng.bytes(32)]))
    ctx.synchronize()
    ctx.profile_reset()  # the advance alone
    new = wt.advance(_rows32([]), _rows32([]))
    assert new.root == t.root
    return [new, wt, t]


def _kzg_verify(ctx, oracle):
    """a verifier and one true claim on a setup of known tau (tests/test_gpu_kzg_verify.py, n = 1)"""
    from era_zkevm_test_harness_amd import native
    from tests import kzg_model as km, kzg_open_model as om, kzg_pairing_model as pm

    tau, coeffs, z = 0x4844, [5, 7, 11], 12345
    ev = lambda at: sum(c * pow(at, i, km.R) for i, c in enumerate(coeffs)) % km.R
    le32 = lambda v: np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)
    v = native.KzgVerifier(ctx, pm.g2_compress(pm.g2_mul(tau, pm.G2_GEN)))
    commitment = km.compress(km.mul_naive(ev(tau), pm.g1_gen()))
    out = v.verify(np.frombuffer(commitment, np.uint8), le32(z), le32(ev(z)), np.frombuffer(om.proof_by_tau(coeffs, z, tau), np.uint8))
    assert [int(x) for x in out] == [1]
    return [v]


def _callstack(ctx, oracle):
    """tests/test_gpu_ram_path.py: 50 operations, depth 3"""
    ops, e = synthetic.callstack_trace(50, seed=50, max_depth=3, final_unwind=False)
    ctx.callstack_simulate(ops, e)
    return []


def _commit(ctx, oracle):
    """NTT and Merkle tree (tests/test_gpu_commit.py: 5 columns of 2^6 values extended twice, 2 sets of 11 columns of 32 leaves)"""
    P = 2**64 - 2**32 + 1
    rng = np.random.default_rng(6)
    ctx.lde(rng.integers(0, P, (5, 64), dtype=np.uint64), 2)
    ctx.merkle_tree_with_cap(rng.integers(0, P, (2, 11, 32), dtype=np.uint64), 4)
    return []


# {case: (call, {span: launches})}
CASES = {
    "decommit_sorter": (_decommit_sorter, {
        "k_chain_full": 1, "k_check_links": 1, "k_check_lookups": 1, "k_check_mult": 1, "k_check_rows": 1, "k_commit_encodings": 1,
        "k_decommit_dedup": 1, "k_decommit_fresh_prefix": 1, "k_decommit_gather_encode": 1, "k_decommit_instances": 1,
        "k_decommit_last_fresh": 1, "k_decommit_sort_keys": 1, "k_ds_commitments": 1, "k_ds_fill_poseidon": 3, "k_ds_fill_row_A": 1,
        "k_ds_fill_row_B": 1, "k_ds_fill_row_C": 1, "k_ds_fill_row_D": 1, "k_ds_fill_tail": 1, "k_ds_fresh_prefix": 1,
        "k_encode_decommit": 1, "k_fs_challenges": 1, "k_gather_u64_by_u32": 4, "k_gp_apply": 1, "k_gp_local": 1, "k_gp_tiles": 1,
        "radix_sort": 5}),
    "ram": (_ram, {
        "k_chain_full": 1, "k_commit_encodings": 1, "k_fs_challenges": 1, "k_gather_encode": 1, "k_ram_commitments": 1, "k_ram_fill_C": 1,
        "k_ram_fill_D": 1, "k_ram_fill_poseidon": 2, "k_ram_fill_tail": 1, "k_ram_gp_groups": 1, "k_ram_gp_scan": 1, "k_ram_instances": 1,
        "k_ram_key_ranges": 1, "k_ram_packed_keys": 1, "radix_sort": 1}),
    "keccak": (_keccak, {
        "k_chain_full": 1, "k_closed_form_commitments": 1, "k_commit_encodings": 1, "k_encode_mem": 1, "k_nl_check_steps": 1,
        "k_nl_check_tail": 1, "k_nl_fill": 1, "k_nl_finish": 1, "k_nl_hist": 1, "k_nl_prepare": 1, "k_nlcf_check": 1, "k_nlcf_ties": 1,
        "k_nlq_check": 1, "k_nlq_feed": 1, "k_nlq_fill": 1, "k_precompile_counts": 1, "k_precompile_instances": 1, "k_precompile_walk": 1}),
    "storage_tree": (_storage_tree, {
        "k_st_emit": 1, "k_st_empty": 1, "k_st_gather_word": 4, "k_st_heads": 1, "k_st_iota": 1, "k_st_leaves": 1, "k_st_levels": 1,
        "k_st_mark": 1, "k_st_new_rank": 1, "radix_sort": 4}),
    # k_swa_locate, k_swa_leaves and k_swa_fold: empty grids, a span and one launch each all the same
    "storage_witness_without_writes": (_storage_witness_without_writes, {
        "k_swa_compact": 1, "k_swa_fold": 1, "k_swa_leaves": 1, "k_swa_locate": 1, "k_swa_paths": 1, "k_swa_wrank": 1}),
    "kzg_verify": (_kzg_verify, {"k_kzg_g2_prepare": 1, "k_kzg_verify_pairing": 1, "k_kzg_verify_points": 1}),
    "callstack": (_callstack, {
        "k_stack_depth": 1, "k_stack_emit": 1, "k_stack_level": 3, "k_stack_links": 1, "k_stack_prefix": 1, "k_stack_push_keys": 1,
        "radix_sort": 1}),
    "commit": (_commit, {"k_merkle_leaves": 2, "k_merkle_nodes": 4, "k_ntt_single": 3}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_profile_of_one_call(ctx, oracle, name):
    call, expected = CASES[name]
    ctx.synchronize()
    ctx.profile_reset()
    made = call(ctx, oracle)
    ctx.synchronize()
    prof = ctx.profile()
    for x in made:
        x.free()
    print("PROFILE", name, json.dumps({k: int(v[1]) for k, v in sorted(prof.items())}))
    assert {k: int(v[1]) for k, v in prof.items()} == expected
    assert all(v[0] >= 0 for v in prof.values()), prof
