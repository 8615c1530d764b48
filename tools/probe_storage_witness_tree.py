"""Witness trees (zkw_storage_tree_create_witness / _extract_witness) measured on one MI355X -> profiles/r11/storage_witness_tree.json.

    python tools/probe_storage_witness_tree.py --parent-lib PATH/libzkw.so [--out profiles/r11/storage_witness_tree.json] [--skip batched]

--parent-lib: libzkw.so built from the PARENT commit (the comparisons below are against it; native.py loads it through ZKW_LIB).
Every GPU step is a child process of its own under its own time limit; the steps run one after another and the first one that fails
(or runs out of time) ends the probe — nothing is started on the GPU after it. A step prints one JSON object as its last line.

  tables         from_proofs and extract_witness for 66 and 512 entries: wall clock around the synchronised call, warm, median of five; then
                 one profiled call each (zkw_profile: HIP events around every launch) for the split into sort, gather, verification; what
                 is left of the wall clock is the upload of the proofs (8 264 B per entry) and the host side. Verification as Blake2s
                 compressions per second against the plain-32-bit VALU ceiling
  gate           the storage_application span of zkw_block_timings, production-shape block (30 slots, 66 walks): the full tree on the PARENT
                 library and the witness tree on this one, five child processes each IN TURN (a warm-up run and one timed run per process)
  batched        64 production blocks through run_prepared + synthesize_many: one shared full tree per shape on the PARENT library, one
                 witness tree per block on this one, three child processes each in turn (a warm-up round and one timed round per process);
                 the batch's own launch accounting (ZKW_BATCH_LOG: in all, and per kernel for the lookup — K blocks' lookups of a stage
                 as ONE merged launch carrying K jobs); the witness trees' HBM per block
  advance        zkw_storage_tree_advance_witness_by_queries (-> profiles/r12/storage_witness_advance.json; needs no parent library:
                 `--skip tables --skip gate --skip batched --out profiles/r12/storage_witness_advance.json`): 66 entries / 30 writes,
                 512 / 256 and 1 920 / 30 (the union of 64 blocks' slots), wall clock around the synchronised call, warm, median of five,
                 and one profiled call for the split; against the route the parent commit offers for the same step — extract_witness +
                 apply_queries on a full tree of 2^20 leaves (code this library has unchanged), five runs, with its min-max spread; then
                 the tables of 64 consecutive blocks of 30 slots each: one extraction of the union + 63 advances against 64 x (extraction +
                 apply_queries), and their HBM
  chain          zkw_storage_tree_advance_witness_chain (-> profiles/r13/storage_witness_chain.json; needs no parent library:
                 `--skip tables --skip gate --skip batched --skip advance --out profiles/r13/storage_witness_chain.json`): K = 64, 16, 4
                 and 1 consecutive blocks of 30 slots each, every slot written, over the table of the 64 blocks' union (1 920 entries).
                 In one process, wall clock around the synchronised calls, warm, five runs each: the chain call without and with the
                 final state, and the parent commit's route on the same table (code this library has unchanged) — K - 1 calls of
                 advance_by_queries for the K pre-states, K calls for the final state too — with its min-max spread; one profiled chain
                 call for the split; the HBM of both routes
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS_PER_COMPRESSION = 10 * 8 * 14 + 40  # tools/probe_storage_tree.py
BYTES_PER_ENTRY = 32 + 8 + 32 + 256 * 32


def _valu_ceiling():
    with open(os.path.join(ROOT, "profiles", "r05", "valu_ceiling.json")) as f:
        c = json.load(f)
    add = next(x for x in c["classes"] if x["class"] == "v_add_u32")
    return add["best_wave_insts_per_s"] * 64


def _native():
    """the binding; on a step that runs against the parent commit's library (ZKW_LIB) only the functions that library exports are
    bound — native.load() types every declared symbol, and the parent has none of the witness trees' three"""
    from era_zkevm_test_harness_amd import native as nv

    if os.environ.get("ZKW_LIB"):
        import ctypes

        import torch  # noqa: F401  (first, as native.load() does: one HIP runtime in the process)

        lib = ctypes.CDLL(nv.LIB_PATH)
        missing = [name for name, _res, _args in nv.SYMBOLS if not hasattr(lib, name)]
        assert all("witness" in name for name in missing), missing
        nv.SYMBOLS[:] = [x for x in nv.SYMBOLS if x[0] not in missing]
    return nv


def _time_ms(fn, sync):
    sync()
    t0 = time.perf_counter()
    r = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, r


def step_tables():
    import numpy as np

    from era_zkevm_test_harness_amd import native as nv

    ctx = nv.Context(0)
    rng = np.random.default_rng(41)
    leaves = rng.integers(0, 256, size=(1 << 16, 32), dtype=np.uint8)
    full = nv.StorageTreeDevice(ctx, 1 << 16)
    full.insert(leaves, rng.integers(0, 256, size=(1 << 16, 32), dtype=np.uint8))
    out = {"full_tree_leaves": 1 << 16, "bytes_per_entry": BYTES_PER_ENTRY}
    ceiling = _valu_ceiling() / OPS_PER_COMPRESSION
    for n in (66, 512):
        keys = np.concatenate([leaves[rng.choice(1 << 16, size=n // 2, replace=False)], rng.integers(0, 256, size=(n - n // 2, 32), dtype=np.uint8)])
        idx, val, paths = full.get_leaves(keys)
        root, nxt = full.root, full.next_enumeration_index
        make = {"from_proofs": lambda: nv.StorageTreeDevice.from_proofs(ctx, keys, idx, val, paths, root, nxt),
                "extract_witness": lambda: full.extract_witness(keys)}
        for name, fn in make.items():
            fn().free()  # warm: scratch, buffers
            walls = []
            for _ in range(5):
                ms, t = _time_ms(fn, ctx.synchronize)
                walls.append(ms)
                t.free()
            ctx.profile_enable(True)
            ctx.profile_reset()
            fn().free()
            prof = ctx.profile()
            ctx.profile_enable(False)
            kern = {k: round(v[0], 4) for k, v in prof.items()} if isinstance(prof, dict) else prof
            rec = {"wall_ms": [round(x, 4) for x in walls], "median_wall_ms": round(statistics.median(walls), 4), "kernels_ms_profiled_run": kern}
            if name == "from_proofs" and isinstance(prof, dict):
                v_ms = prof["k_sw_verify"][0]
                comp = n * 257
                rec["verification"] = {"compressions": comp, "ms": round(v_ms, 4), "compressions_per_s": comp / (v_ms * 1e-3),
                                       "valu_ceiling_compressions_per_s": ceiling, "fraction_of_valu_ceiling": round(comp / (v_ms * 1e-3) / ceiling, 5)}
                rec["upload_bytes"] = n * BYTES_PER_ENTRY
            out[f"{name}_{n}"] = rec
    full.free()
    return out


def step_advance():
    import numpy as np

    from era_zkevm_test_harness_amd import native as nv, synthetic

    ctx = nv.Context(0)
    rng = np.random.default_rng(43)
    n_full = 1 << 20
    K, slots = 64, 30
    q = np.ascontiguousarray(synthetic.storage_application_trace(K * slots, seed=5)[0], dtype=nv.LOG_QUERY)
    q["rw_flag"] = 1
    qkeys = np.frombuffer(b"".join(synthetic.derive_final_address(x) for x in q), np.uint8).reshape(-1, 32)
    leaves = rng.integers(0, 256, size=(n_full - K * slots, 32), dtype=np.uint8)
    leaves[:K * slots // 2] = qkeys[::2]  # every other slot exists before the first block
    full = nv.StorageTreeDevice(ctx, n_full)
    full.insert(leaves, rng.integers(0, 256, size=leaves.shape, dtype=np.uint8))
    out = {"full_tree_leaves": int(full.num_leaves), "bytes_per_entry": BYTES_PER_ENTRY, "shapes": {}}

    def profiled(fn):
        ctx.profile_enable(True)
        ctx.profile_reset()
        fn()
        prof = ctx.profile()
        ctx.profile_enable(False)
        return {k: round(v[0], 4) for k, v in prof.items()} if isinstance(prof, dict) else prof

    for entries, writes in ((66, 30), (512, 256), (1920, 30)):
        keys, batch = qkeys[:entries], q[:writes]
        table = full.extract_witness(keys)
        table.advance_by_queries(batch).free()  # warm: scratch, buffers
        new = []
        for _ in range(5):
            ms, t = _time_ms(lambda: table.advance_by_queries(batch), ctx.synchronize)
            new.append(ms)
            t.free()
        split = profiled(lambda: table.advance_by_queries(batch).free())
        table.free()
        # the parent's route for the same step: the next block's table cut out of the full tree, then the block's writes applied to it
        full.extract_witness(keys).free()
        parent, parts = [], []
        for _ in range(5):
            ms_x, t = _time_ms(lambda: full.extract_witness(keys), ctx.synchronize)
            ms_a, _r = _time_ms(lambda: full.apply_queries(batch), ctx.synchronize)
            t.free()
            parent.append(ms_x + ms_a)
            parts.append([round(ms_x, 4), round(ms_a, 4)])
        spread = max(parent) - min(parent)
        mn, mp = statistics.median(new), statistics.median(parent)
        out["shapes"][f"{entries}_entries_{writes}_writes"] = {
            "advance_by_queries_wall_ms": [round(x, 4) for x in new], "advance_median_ms": round(mn, 4), "advance_kernels_ms_profiled_run": split,
            "parent_route_wall_ms": [round(x, 4) for x in parent], "parent_route_extract_apply_ms": parts, "parent_route_median_ms": round(mp, 4),
            "parent_route_min_max_spread_ms": round(spread, 4), "below_parent_median_minus_spread": bool(mn < mp - spread),
            "table_hbm_bytes": entries * BYTES_PER_ENTRY}
    # the tables of K consecutive blocks: block k writes slots [30 k, 30 k + 30)
    union = qkeys[:K * slots]

    def by_advance():
        tables = [full.extract_witness(union)]
        for k in range(K - 1):
            tables.append(tables[-1].advance_by_queries(q[k * slots:(k + 1) * slots]))
        return tables

    for t in by_advance():
        t.free()
    ms_adv, tables = _time_ms(by_advance, ctx.synchronize)
    hbm_adv = sum(t.capacity for t in tables) * BYTES_PER_ENTRY
    for t in tables:
        t.free()

    def by_extraction():
        tables = []
        for k in range(K):
            tables.append(full.extract_witness(qkeys[k * slots:(k + 1) * slots]))
            full.apply_queries(q[k * slots:(k + 1) * slots])
        return tables

    ms_ext, tables = _time_ms(by_extraction, ctx.synchronize)
    hbm_ext = sum(t.capacity for t in tables) * BYTES_PER_ENTRY
    for t in tables:
        t.free()
    out["tables_of_64_blocks"] = {"one_extraction_63_advances_ms": round(ms_adv, 3), "tables_hbm_bytes": hbm_adv,
                                  "per_block_extraction_and_apply_on_the_full_tree_ms": round(ms_ext, 3), "per_block_tables_hbm_bytes": hbm_ext,
                                  "full_tree_hbm_bytes": n_full * nv.StorageTreeDevice.bytes_per_leaf()}
    full.free()
    return out


def step_chain():
    import numpy as np

    from era_zkevm_test_harness_amd import native as nv, synthetic

    ctx = nv.Context(0)
    rng = np.random.default_rng(47)
    n_full, K_max, slots = 1 << 16, 64, 30
    q = np.ascontiguousarray(synthetic.storage_application_trace(K_max * slots, seed=5)[0], dtype=nv.LOG_QUERY)
    q["rw_flag"] = 1
    qkeys = np.frombuffer(b"".join(synthetic.derive_final_address(x) for x in q), np.uint8).reshape(-1, 32)
    leaves = rng.integers(0, 256, size=(n_full - K_max * slots, 32), dtype=np.uint8)
    leaves[:K_max * slots // 2] = qkeys[::2]  # every other slot exists before the first block
    full = nv.StorageTreeDevice(ctx, n_full)
    full.insert(leaves, rng.integers(0, 256, size=leaves.shape, dtype=np.uint8))
    union = full.extract_witness(qkeys)
    full.free()
    entries = int(union.capacity)
    out = {"union_entries": entries, "slots_per_block": slots, "bytes_per_entry": BYTES_PER_ENTRY, "blocks": {}}

    def free(x):
        for t in x if isinstance(x, (list, tuple)) else [x]:
            free(t) if isinstance(t, (list, tuple)) else t.free()

    def sequential(blocks, calls):
        tables = [union]
        for b in blocks[:calls]:
            tables.append(tables[-1].advance_by_queries(b))
        return tables[1:]

    def five(fn):
        free(fn())  # warm: scratch, buffers
        walls = []
        for _ in range(5):
            ms, r = _time_ms(fn, ctx.synchronize)
            walls.append(ms)
            free(r)
        return walls

    for K in (64, 16, 4, 1):
        blocks = [q[k * slots:(k + 1) * slots] for k in range(K)]
        rec = {}
        for what, final in (("pre_states", False), ("pre_states_and_final", True)):
            new = five(lambda: union.advance_chain(blocks, final=final))
            parent = five(lambda: sequential(blocks, K if final else K - 1))
            spread = max(parent) - min(parent)
            mn, mp = statistics.median(new), statistics.median(parent)
            rec[what] = {"chain_wall_ms": [round(x, 4) for x in new], "chain_median_ms": round(mn, 4),
                         "sequential_calls": K if final else K - 1, "sequential_wall_ms": [round(x, 4) for x in parent], "sequential_median_ms": round(mp, 4),
                         "sequential_min_max_spread_ms": round(spread, 4), "below_sequential_median_minus_spread": bool(mn < mp - spread)}
        ctx.profile_enable(True)
        ctx.profile_reset()
        tables = union.advance_chain(blocks)
        prof = ctx.profile()
        ctx.profile_enable(False)
        rec["chain_kernels_ms_launches_profiled_run"] = {k: [round(v[0], 4), int(v[1])] for k, v in prof.items()} if isinstance(prof, dict) else prof
        own = sum(t.capacity for t in tables)
        free(tables)
        rec["hbm_bytes"] = {"chain_tables": own * BYTES_PER_ENTRY, "chain_working_copy_of_the_union": entries * BYTES_PER_ENTRY,
                            "chain_scratch": 4 * (5 * K * entries + entries + 2 * K * slots + 20 * min(K * slots, K * entries) + 21 * K + 23),
                            "sequential_tables": K * entries * BYTES_PER_ENTRY}
        out["blocks"][str(K)] = rec
    union.free()
    return out


def _production_block_and_pairs(nv, synthetic, np, seed):
    """(generated on the host in tens of seconds: the probe's child processes share one copy per seed in the temporary directory, keyed on
    the generator's source so that a copy from another version of it is never read)"""
    import hashlib
    import pickle
    import tempfile

    with open(synthetic.__file__, "rb") as f:
        version = hashlib.sha256(f.read()).hexdigest()[:16]
    cache = os.path.join(tempfile.gettempdir(), f"zkw_probe_production_block_{seed}_{version}_{os.getuid()}.pkl")
    if os.path.exists(cache):
        with open(cache, "rb") as f:
            blk, dedup = pickle.load(f)
    else:
        blk = synthetic.block_production(seed=seed)
        first = nv.Block(0, blk)
        dedup = first.witness_get(9, nv.STO_RESULT_QUERIES, np.uint8).view(nv.LOG_QUERY).copy()
        first.free()
        with open(cache + ".tmp", "wb") as f:
            pickle.dump((blk, dedup), f)
        os.replace(cache + ".tmp", cache)
    rng = np.random.default_rng(seed)
    pairs = [(rng.bytes(32), rng.bytes(32)) for _ in range(10)]
    pairs += [(synthetic.derive_final_address(q), b"".join(int(x).to_bytes(4, "big") for x in q["read_value"][::-1])) for q in dedup if q["read_value"].any()]
    return blk, dedup, pairs


def step_gate_one(witness):
    """one process: the production block once untimed, once timed; the storage_application span"""
    import numpy as np

    from era_zkevm_test_harness_amd import synthetic

    nv = _native()
    ctx = nv.Context(0)
    blk, dedup, pairs = _production_block_and_pairs(nv, synthetic, np, 1)
    t = nv.StorageTreeDevice(ctx, 1024)
    t.insert([k for k, _ in pairs], [v for _, v in pairs])
    tree = t.extract_witness([synthetic.derive_final_address(q) for q in dedup]) if witness else t
    spans = []
    for _ in range(2):
        B = nv.Block(0, blk, storage_tree_device=tree)
        spans.append(next(e - s for name, s, e in B.timings() if name == "storage_application"))
        pi = B.public_inputs(10).tobytes()
        B.free()
    return {"tree_queries": int(dedup.size), "span_ms": spans[1], "warmup_span_ms": spans[0], "pi_sha": __import__("hashlib").sha256(pi).hexdigest()[:16]}


def step_batched_one(witness):
    import numpy as np
    import torch

    from era_zkevm_test_harness_amd import synthetic

    nv = _native()
    ctx = nv.Context(0)
    K = 64
    blocks, trees = [], []
    for seed in (1, 2, 3, 4):
        blk, dedup, pairs = _production_block_and_pairs(nv, synthetic, np, seed)
        t = nv.StorageTreeDevice(ctx, 1024)
        t.insert([k for k, _ in pairs], [v for _, v in pairs])
        blocks.append(nv.Block.queues_to_device(blk, 0))
        trees.append((t, [synthetic.derive_final_address(q) for q in dedup]))
    if witness:
        per_block = [trees[k % 4][0].extract_witness(trees[k % 4][1]) for k in range(K)]  # one of its own per block
        hbm = [w.capacity * BYTES_PER_ENTRY for w in per_block]
    else:
        per_block = [trees[k % 4][0] for k in range(K)]
        hbm = []
    tpl = nv.Block.prepare_many(0, [blocks[k % 4] for k in range(K)], None, storage_tree_device=per_block)
    rounds = []
    for rnd in range(2):  # the first fills the caches: untimed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        many = nv.Block.run_prepared(0, tpl)
        t1 = time.perf_counter()
        inst = nv.Block.synthesize_many(many, 1 << 20, ring_slots=1)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        nv.Block.free_many(many)
        rounds.append({"builders_ms": round((t1 - t0) * 1e3, 1), "synthesis_ms": round((t2 - t1) * 1e3, 1), "blocks_per_s": round(K / (t2 - t0), 2), "instances": inst})
    return {"blocks": K, "timed_round": rounds[1], "warmup_round": rounds[0], "witness_tree_hbm_bytes_per_block": sorted(set(hbm))}


def run_step(name):
    if name == "tables":
        return step_tables()
    if name == "advance":
        return step_advance()
    if name == "chain":
        return step_chain()
    if name in ("gate_full", "gate_witness"):
        return step_gate_one(name == "gate_witness")
    if name in ("batched_full", "batched_witness"):
        return step_batched_one(name == "batched_witness")
    raise SystemExit(f"unknown step {name}")


def _spread_gate(parent, new, higher_is_better):
    spread = max(parent) - min(parent)
    mp, mn = statistics.median(parent), statistics.median(new)
    holds = mn >= mp - spread if higher_is_better else mn <= mp + spread
    return {"parent_median": round(mp, 3), "new_median": round(mn, 3), "parent_min_max_spread": round(spread, 3), "within_parent_spread": bool(holds)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "storage_witness_tree.json"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--step")
    ap.add_argument("--skip", action="append", default=[])
    a = ap.parse_args()
    if a.step:
        print(json.dumps(run_step(a.step)))
        return 0
    if not {"gate", "batched"} <= set(a.skip):
        assert a.parent_lib and os.path.exists(a.parent_lib), "--parent-lib: libzkw.so of the parent commit"
    plan = [("tables", "tables", False, 240)]
    plan += [x for _ in range(5) for x in (("gate", "gate_full", True, 240), ("gate", "gate_witness", False, 240))]
    plan += [x for _ in range(3) for x in (("batched", "batched_full", True, 420), ("batched", "batched_witness", False, 420))]
    plan += [("advance", "advance", False, 420), ("chain", "chain", False, 300)]
    result = {"source": "tools/probe_storage_witness_tree.py on one MI355X; wall-clock times around synchronised calls", "steps": {}}
    rc = 0

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    for group, step, on_parent, limit in plan:
        if group in a.skip:
            continue
        env = dict(os.environ)
        if on_parent:
            env["ZKW_LIB"] = os.path.abspath(a.parent_lib)
        if group == "batched":
            env["ZKW_BATCH_LOG"] = "1"
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            result["steps"].setdefault(step, []).append({"failed": f"no result within {limit} s"})
            rc = 124
        else:
            if p.returncode != 0:
                result["steps"].setdefault(step, []).append({"failed": f"exit status {p.returncode}", "stderr_tail": p.stderr[-2000:]})
                rc = p.returncode
        if rc:
            result["stopped_at"] = step  # nothing was started after the step that failed
            break
        rec = json.loads(p.stdout.strip().splitlines()[-1])
        if group == "batched":  # the batch's own accounting: the line of the timed round's zkw_blocks_run (the last builders' batch)
            logs = re.findall(r"\[zkw batch\] (\d+) fibers, (\d+) flushes, (\d+) merged launches carrying (\d+) jobs, (\d+) chain launches", p.stderr)
            rec["batch_log"] = [dict(zip(("fibers", "flushes", "merged_launches", "jobs", "chain_launches"), map(int, x))) for x in logs]
            # per kernel (this build's library prints it): the lookups of the K blocks' stage as merged launches and the jobs they carried;
            # the builders' batch is the call with K x 7 or more fibers, the last of them the timed round's
            per = re.findall(r"\[zkw batch\]   (k_sw_lookup|k_st_query): (\d+) merged launches carrying (\d+) jobs", p.stderr)
            rec["lookup_launches"] = [{"kernel": k, "merged_launches": int(a_), "jobs": int(b_)} for k, a_, b_ in per]
        result["steps"].setdefault(step, []).append(rec)
        print(step, json.dumps(rec), flush=True)
        save()
    s = result["steps"]
    if not rc and "gate" not in a.skip:
        result["gate_storage_application_span_ms"] = dict(_spread_gate([x["span_ms"] for x in s["gate_full"]], [x["span_ms"] for x in s["gate_witness"]], False),
                                                          parent_full_tree=[round(x["span_ms"], 3) for x in s["gate_full"]],
                                                          witness_tree=[round(x["span_ms"], 3) for x in s["gate_witness"]])
    if not rc and "batched" not in a.skip:
        result["gate_batched_blocks_per_s"] = dict(_spread_gate([x["timed_round"]["blocks_per_s"] for x in s["batched_full"]],
                                                                [x["timed_round"]["blocks_per_s"] for x in s["batched_witness"]], True),
                                                   parent_shared_full_tree=[x["timed_round"]["blocks_per_s"] for x in s["batched_full"]],
                                                   witness_tree_per_block=[x["timed_round"]["blocks_per_s"] for x in s["batched_witness"]])
    save()
    return rc


if __name__ == "__main__":
    sys.exit(main())
