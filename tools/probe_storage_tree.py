"""The device-resident storage tree (zkw_storage_tree) measured on one MI355X -> profiles/r07/storage_tree.json.

    python tools/probe_storage_tree.py [--out profiles/r07/storage_tree.json] [--skip batched]

Every GPU step is a child process of its own under its own time limit; the steps run one after another and the first one that fails
(or runs out of time) ends the probe — nothing is started on the GPU after it. A step prints one JSON object as its last line.

  build_2p16, build_2p20   one insert of n random leaves into an empty tree (cold: the context's sort scratch is allocated on the way;
                           warm: a second tree of the same size on the same context), HBM of the tree, the Blake2s compressions the
                           build makes (counted on the host from the sorted keys) per second against the plain-32-bit VALU ceiling
  queries_2p20             zkw_storage_tree_answer_queries for 66 and 512 log queries against the 2^20 tree, an apply of 512 writes
  gate                     the storage_application span of zkw_block_timings, production-shape block: device tree vs the callback path
                           with precomputed answers (the callback only copies them), five runs each
  batched                  64 production blocks through run_prepared + synthesize_many with trees (type 10 built) and without
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("build_2p16", 120), ("build_2p20", 240), ("queries_2p20", 240), ("gate", 400), ("batched", 400)]
# plain 32-bit VALU operations of one Blake2s compression: 10 rounds x 8 G x 14 (a G is 6 additions, 4 xors, 4 rotations) + the
# initialisation and the feed-forward
OPS_PER_COMPRESSION = 10 * 8 * 14 + 40


def _valu_ceiling():
    """plain 32-bit lane operations per second (profiles/r05/valu_ceiling.json: v_add_u32 wave instructions x 64 lanes)"""
    with open(os.path.join(ROOT, "profiles", "r05", "valu_ceiling.json")) as f:
        c = json.load(f)
    add = next(x for x in c["classes"] if x["class"] == "v_add_u32")
    return add["best_wave_insts_per_s"] * 64


def _random_rows(n, seed):
    import numpy as np

    return np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)


def _compressions_of_build(keys):
    """leaf hashes + one node hash per non-empty node of every height 1..256, from the keys alone"""
    import numpy as np

    w = np.ascontiguousarray(keys).view("<u8").reshape(-1, 4)
    order = np.lexsort((w[:, 0], w[:, 1], w[:, 2], w[:, 3]))
    s = w[order]
    x = s[1:] ^ s[:-1]
    top = np.full(x.shape[0], -1, np.int64)  # highest differing bit of neighbours
    for word in range(4):
        v = x[:, word].copy()
        nz = v != 0
        bit = np.zeros(v.shape[0], np.int64)
        for sh in (32, 16, 8, 4, 2, 1):
            big = (v >> np.uint64(sh)) != 0
            bit += np.where(big, sh, 0)
            v = np.where(big, v >> np.uint64(sh), v)
        top = np.where(nz, 64 * word + bit, top)
    assert (top >= 0).all(), "distinct keys"
    n = s.shape[0]
    hist = np.bincount(top, minlength=256)
    starts_at_least = np.cumsum(hist[::-1])[::-1]  # [h] = leaves i >= 1 with top >= h
    return int(n + sum(1 + int(starts_at_least[h]) if h < 256 else 1 for h in range(1, 257)))


def _time_ms(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def step_build(log2n):
    import numpy as np

    from era_zkevm_test_harness_amd import native as nv

    n = 1 << log2n
    ctx = nv.Context(0)
    keys, values = _random_rows(n, 1000 + log2n), _random_rows(n, 2000 + log2n)
    comp = _compressions_of_build(keys)
    times = []
    for _ in range(3):  # the first is cold (scratch, buffers from hipMalloc), the others find everything in the library's caches
        t = nv.StorageTreeDevice(ctx, n)
        times.append(_time_ms(lambda: t.insert(keys, values), ctx.synchronize))
        root = t.root
        t.free()
    warm = min(times[1:])
    rate = comp / (warm * 1e-3)
    ceiling = _valu_ceiling() / OPS_PER_COMPRESSION
    return {"leaves": n, "insert_ms_cold": round(times[0], 3), "insert_ms_warm": [round(x, 3) for x in times[1:]],
            "includes": "host -> device copy of the pairs (64 B per leaf), the 256-bit sort, every height, the root back on the host",
            "hbm_bytes": n * nv.StorageTreeDevice.bytes_per_leaf(), "bytes_per_leaf": nv.StorageTreeDevice.bytes_per_leaf(),
            "blake2s_compressions": comp, "compressions_per_s": rate, "valu_ceiling_compressions_per_s": ceiling,
            "fraction_of_valu_ceiling": round(rate / ceiling, 4), "root": root.hex(), "n_distinct": int(np.unique(keys, axis=0).shape[0])}


def step_queries():
    import numpy as np
    import torch

    from era_zkevm_test_harness_amd import native as nv, synthetic

    n = 1 << 20
    ctx = nv.Context(0)
    t = nv.StorageTreeDevice(ctx, n + 4096)
    t.insert(_random_rows(n, 1020), _random_rows(n, 2020))
    dev = torch.device("cuda", 0)
    out = {"tree_leaves": n}
    dctx = nv.Context(0)
    dctx.set_pointer_mode(nv.PTR_DEVICE)
    for nq in (66, 512):
        q, _existing = synthetic.storage_application_trace(nq, seed=nq)
        q = np.ascontiguousarray(q, dtype=nv.LOG_QUERY)
        d_q = torch.from_numpy(q.view(np.uint8).reshape(-1).copy()).to(dev)
        d_idx = torch.zeros(nq, dtype=torch.int64, device=dev)
        d_paths = torch.zeros((nq, 256, 32), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        call = lambda: t.answer_queries(dctx, d_q.data_ptr(), nq, d_idx.data_ptr(), d_paths.data_ptr())  # noqa: E731
        ms = sorted(_time_ms(call, dctx.synchronize) for _ in range(21))
        out[f"answer_{nq}_queries_ms"] = {"median": round(ms[10], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4),
                                          "what": "launch + kernel + synchronize, one call: derive_final_address, %d lower bounds of ~20 steps, %d KB of paths" % (nq * 257, nq * 8)}
    applies = []
    for rep in range(5):
        q, _existing = synthetic.storage_application_trace(512, seed=700 + rep, existing_fraction=0.0, write_fraction=1.0)
        q = np.ascontiguousarray(q, dtype=nv.LOG_QUERY)
        q["address"][:, 0] = 7000 + rep  # other slots every time: 512 new leaves per apply
        applies.append(_time_ms(lambda: t.apply_queries(q), ctx.synchronize))
    out["apply_512_writes_ms"] = {"first": round(applies[0], 3), "median_of_rest": round(statistics.median(applies[1:]), 3),
                                  "what": "512 new leaves into the 2^20 tree: the sort of tree + batch and a rebuild of every height (the cost of a build)"}
    out["leaves_after"] = t.num_leaves
    assert t.num_leaves == n + 5 * 512
    t.free()
    return out


def _production_block_and_trees(nv, synthetic, np, seed):
    blk = synthetic.block_production(seed=seed)
    first = nv.Block(0, blk)
    dedup = first.witness_get(9, nv.STO_RESULT_QUERIES, np.uint8).view(nv.LOG_QUERY).copy()
    first.free()
    host_tree, answers = synthetic.storage_tree_for(dedup, seed=seed)
    rng = np.random.default_rng(seed)  # the same leaves in the same order (synthetic.storage_tree_for)
    pairs = [(rng.bytes(32), rng.bytes(32)) for _ in range(10)]
    pairs += [(synthetic.derive_final_address(q), b"".join(int(x).to_bytes(4, "big") for x in q["read_value"][::-1])) for q in dedup if q["read_value"].any()]
    return blk, dedup, host_tree, answers, pairs


def step_gate():
    import numpy as np

    from era_zkevm_test_harness_amd import native as nv, synthetic

    ctx = nv.Context(0)
    blk, dedup, host_tree, answers, pairs = _production_block_and_trees(nv, synthetic, np, 1)
    t = nv.StorageTreeDevice(ctx, 1024)
    t.insert([k for k, _ in pairs], [v for _, v in pairs])
    assert t.root == host_tree.root and t.next_enumeration_index == host_tree.next_enumeration_index
    idx, paths = answers(dedup)  # precomputed: the callback below only hands them over

    def run(device_tree):
        if device_tree:
            B = nv.Block(0, blk, storage_tree_device=t)
        else:
            B = nv.Block(0, blk, storage_tree=lambda q: (idx, paths), storage_initial_root=host_tree.root,
                         storage_next_enumeration_index=host_tree.next_enumeration_index)
        span = next(e - s for name, s, e in B.timings() if name == "storage_application")
        rec = (B.witness_get(10, nv.SAP_INSTANCES, np.uint8).tobytes(), B.public_inputs(10).tobytes())
        B.free()
        return span, rec

    (_w0, rec_cb), (_w1, rec_dev) = run(False), run(True)  # untimed: warm both paths
    assert rec_cb == rec_dev, "the two paths disagree"
    cb, dv = [], []
    for _ in range(5):  # in turn, so that a drift of the machine hits both
        cb.append(run(False)[0])
        dv.append(run(True)[0])
    spread = max(max(cb) - min(cb), max(dv) - min(dv))
    med_cb, med_dv = statistics.median(cb), statistics.median(dv)
    return {"block": "synthetic.block_production(seed=1)", "tree_queries": int(dedup.size), "span": "storage_application (zkw_block_timings), ms",
            "callback_precomputed_ms": [round(x, 3) for x in cb], "device_tree_ms": [round(x, 3) for x in dv],
            "median_callback_ms": round(med_cb, 3), "median_device_tree_ms": round(med_dv, 3), "larger_min_max_spread_ms": round(spread, 3),
            "gate": "median_device_tree <= median_callback + larger spread", "gate_holds": bool(med_dv <= med_cb + spread),
            "note": "the callback path is the parent commit's code, unchanged, in the same library; its Python callback returns arrays prepared before the run"}


def step_batched():
    import numpy as np
    import torch

    from era_zkevm_test_harness_amd import native as nv, synthetic

    ctx = nv.Context(0)
    K = 64
    blocks, trees = [], []
    for seed in (1, 2, 3, 4):
        blk, _dedup, host_tree, _answers, pairs = _production_block_and_trees(nv, synthetic, np, seed)
        t = nv.StorageTreeDevice(ctx, 1024)
        t.insert([k for k, _ in pairs], [v for _, v in pairs])
        assert t.root == host_tree.root
        blocks.append(nv.Block.queues_to_device(blk, 0))
        trees.append(t)
    out = {"blocks_per_batch": K, "n_rows": 1 << 20}
    for name, with_trees in (("without_trees", False), ("with_trees", True)):
        tpl = nv.Block.prepare_many(0, [blocks[k % 4] for k in range(K)], None, storage_tree_device=[trees[k % 4] for k in range(K)] if with_trees else None)
        walls, inst = [], 0
        for rnd in range(3):  # the first fills the caches: untimed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            many = nv.Block.run_prepared(0, tpl)
            t1 = time.perf_counter()
            inst = nv.Block.synthesize_many(many, 1 << 20, ring_slots=1)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            per_block = sum(many[0].num_instances(t_) for t_ in (4, 8, 10, 2, 3, 5, 6, 7, 9, 11, 12, 13))
            nv.Block.free_many(many)
            if rnd:
                walls.append({"builders_ms": round((t1 - t0) * 1e3, 1), "synthesis_ms": round((t2 - t1) * 1e3, 1), "blocks_per_s": round(K / (t2 - t0), 2)})
        out[name] = {"rounds": walls, "instances_per_batch": inst, "instances_per_block": per_block}
    for t in trees:
        t.free()
    return out


def run_step(name):
    if name == "build_2p16":
        return step_build(16)
    if name == "build_2p20":
        return step_build(20)
    if name == "queries_2p20":
        return step_queries()
    if name == "gate":
        return step_gate()
    if name == "batched":
        return step_batched()
    raise SystemExit(f"unknown step {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "storage_tree.json"))
    ap.add_argument("--step")
    ap.add_argument("--skip", action="append", default=[])
    a = ap.parse_args()
    if a.step:
        print(json.dumps(run_step(a.step)))
        return 0
    result = {"source": "tools/probe_storage_tree.py on one MI355X; wall-clock times around synchronised calls", "steps": {}}
    rc = 0
    for name, limit in STEPS:
        if name in a.skip:
            result["steps"][name] = {"skipped": True}
            continue
        t0 = time.perf_counter()
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            result["steps"][name] = {"failed": f"no result within {limit} s"}
            rc = 124
            break
        if p.returncode != 0:
            result["steps"][name] = {"failed": f"exit status {p.returncode}", "stderr_tail": p.stderr[-2000:]}
            rc = p.returncode
            break
        result["steps"][name] = json.loads(p.stdout.strip().splitlines()[-1])
        result["steps"][name]["step_wall_s"] = round(time.perf_counter() - t0, 1)
        print(name, json.dumps(result["steps"][name]), flush=True)
    if rc:
        result["stopped_at"] = name  # nothing was started after the step that failed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
