// zkw_storage_tree.hip — zkw_storage_tree behind include/zkw.h: the reference's `tree: impl BinarySparseStorageTree`
// (src/external_calls.rs:81, src/witness/tree/mod.rs:42-99) as a structure of the library, resident in HBM. Kernels and the layout:
// storage_tree_kernels.cuh. Every call that changes the tree ends with the new root on the host (one small readback), so a call that
// only reads — zkw_storage_tree_answer_queries from the storage branch of any number of blocks — needs no ordering with the tree's stream.
// A WITNESS tree (storage_witness_kernels.cuh) is the same handle with `witness` set: a sorted table of get_leaf answers for one state,
// built once (zkw_storage_tree_create_witness / _extract_witness), read like a tree, never changed; zkw_storage_tree_advance_witness makes
// the table of the NEXT state out of it, as a new handle.
#include "zkw_ctx.h"
#include "storage_witness_kernels.cuh"
#include "radix_sort.cuh"
#include "scan_kernels.cuh"

struct zkw_storage_tree {
    zkw_ctx* ctx = nullptr;
    size_t cap = 0, n = 0;
    u64 next_index = 1;
    // leaves, double buffered: an insert writes the merged leaves to the other side and flips
    u32* keys[2] = {nullptr, nullptr};
    u64* index[2] = {nullptr, nullptr};
    u32* values[2] = {nullptr, nullptr};
    int cur = 0;
    u32 *nodes = nullptr, *empty = nullptr, *d = nullptr, *nxt = nullptr, *root_dev = nullptr;
    uint8_t root[32] = {}, empty_root[32] = {};
    // a witness tree: keys[0] / index[0] / values[0] are the table's sorted entries (cap of them, n with a nonzero index) and `paths` their
    // Merkle paths; nothing else is allocated
    bool witness = false;
    u32* paths = nullptr;
    void release() {
        void* ptrs[] = {keys[0], keys[1], index[0], index[1], values[0], values[1], nodes, empty, d, nxt, root_dev, paths};
        for (void* p : ptrs)
            if (p) dev_free(p);
    }
    StView view() const { return StView{keys[cur], index[cur], values[cur], nodes, empty, (u64)n, (u64)cap}; }
    SwView table() const { return SwView{keys[0], index[0], values[0], paths, (u64)cap}; }
};

// bytes of HBM per leaf of capacity: the nodes (256 x 32), two sides of key / index / value (2 x 72), d and nxt (2 x 4)
static constexpr size_t ST_BYTES_PER_LEAF = 256 * 32 + 2 * (32 + 8 + 32) + 8;

extern "C" size_t zkw_storage_tree_bytes_per_leaf(void) { return ST_BYTES_PER_LEAF; }

extern "C" int zkw_storage_tree_create(zkw_ctx* ctx, size_t capacity_leaves, zkw_storage_tree** out) {
    if (!ctx || !out || capacity_leaves == 0) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_create: bad argument");
    if (capacity_leaves >= (1ull << 31)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_create: at most 2^31 - 1 leaves");
    if (ctx->batch) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_create: the context belongs to a batch of blocks");
    HIP_TRY(hipSetDevice(ctx->device));
    *out = nullptr;
    Building<zkw_storage_tree> t(ctx);
    t->cap = capacity_leaves;
    for (int s = 0; s < 2; s++) {
        t.alloc(&t->keys[s], t->cap * 32);
        t.alloc(&t->index[s], t->cap * 8);
        t.alloc(&t->values[s], t->cap * 32);
    }
    t.alloc(&t->nodes, t->cap * (size_t)ST_DEPTH * 32);
    t.alloc(&t->empty, (ST_DEPTH + 1) * 32);
    t.alloc(&t->d, t->cap * 4);
    t.alloc(&t->nxt, t->cap * 4);
    t.alloc(&t->root_dev, 32);
    if (t.err != hipSuccess) {
        (void)hipGetLastError();
        return fail(ZKW_ERR_OOM, "zkw_storage_tree_create: %zu leaves need %zu bytes of device memory: %s", capacity_leaves,
                    capacity_leaves * ST_BYTES_PER_LEAF, hipGetErrorString(t.err));
    }
    ZKW_LAUNCH(ctx, k_st_empty, 1, 64, t->empty);
    ZKW_TRY(ctx->read_small(t->empty_root, t->empty + 8 * ST_DEPTH, 32));
    memcpy(t->root, t->empty_root, 32);
    t.commit(out);
    return ZKW_OK;
}

extern "C" void zkw_storage_tree_free(zkw_storage_tree* t) { witness_free(t); }

extern "C" int zkw_storage_tree_root(const zkw_storage_tree* t, uint8_t out[32]) {
    if (!t || !out) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_root: null argument");
    memcpy(out, t->root, 32);
    return ZKW_OK;
}
extern "C" uint64_t zkw_storage_tree_next_enumeration_index(const zkw_storage_tree* t) { return t ? t->next_index : 0; }
extern "C" int zkw_storage_tree_set_next_enumeration_index(zkw_storage_tree* t, uint64_t next) {
    if (!t || next == 0) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_set_next_enumeration_index: bad argument (index 0 is the empty leaf's)");
    if (t->witness) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_set_next_enumeration_index: a witness tree does not change");
    t->next_index = next;
    return ZKW_OK;
}
extern "C" size_t zkw_storage_tree_num_leaves(const zkw_storage_tree* t) { return t ? t->n : 0; }
extern "C" size_t zkw_storage_tree_capacity(const zkw_storage_tree* t) { return t ? t->cap : 0; }
extern "C" int zkw_storage_tree_is_witness(const zkw_storage_tree* t) { return t && t->witness; }
int zkw_storage_tree_device(const zkw_storage_tree* t) { return t ? t->ctx->device : -1; }

// every height over the leaves of side `cur`, then the root to the host
static int st_rebuild(zkw_storage_tree* t) {
    zkw_ctx* ctx = t->ctx;
    if (t->n == 0) {
        memcpy(t->root, t->empty_root, 32);
        return ZKW_OK;
    }
    StBuild b{t->keys[t->cur], t->index[t->cur], t->values[t->cur], t->nodes, t->empty, t->d, t->nxt, t->root_dev, (u64)t->n, (u64)t->cap};
    const unsigned g64 = blocks_for(t->n, 64);
    ZKW_LAUNCH(ctx, k_st_leaves, g64, 64, b);
    static_assert(ZKW_STORAGE_TREE_DEPTH == ST_DEPTH, "the tree kernels walk 256 levels");
    if (t->n <= ST_PERSISTENT_MAX) {
        ZKW_LAUNCH(ctx, k_st_levels, 1, ST_PERSISTENT_THREADS, b);
    } else {
        for (int L = 0; L < ST_DEPTH; L++) ZKW_LAUNCH(ctx, k_st_level, g64, 64, b, L);
    }
    return ctx->read_small(t->root, t->root_dev, 32);
}

// the stable sort by key of the N entries of `g` (the tree's leaves, then a batch): four passes of 64 bits, least significant first, over
// a permutation. *perm = the scratch buffer that holds the result.
static int st_sort_merged(zkw_ctx* ctx, const StMerge& g, size_t N, const u32** perm) {
    u32 *perm0 = nullptr, *perm1 = nullptr;
    u64 *k64a = nullptr, *k64b = nullptr;
    void* tmp = nullptr;
    const size_t tmp_bytes = radix_temp_bytes(N);
    ZKW_TRY(ctx->scratch_t<u32>("st_perm0", N, &perm0));
    ZKW_TRY(ctx->scratch_t<u32>("st_perm1", N, &perm1));
    ZKW_TRY(ctx->scratch_t<u64>("st_k64a", N, &k64a));
    ZKW_TRY(ctx->scratch_t<u64>("st_k64b", N, &k64b));
    ZKW_TRY(ctx->scratch("st_sort_tmp", tmp_bytes + 256, &tmp));
    const unsigned grid = blocks_for(N, 256);
    ZKW_LAUNCH(ctx, k_st_iota, grid, 256, perm0, (u64)N);
    u32 *pc = perm0, *pn = perm1;
    for (int w = 0; w < 4; w++) {
        ZKW_LAUNCH(ctx, k_st_gather_word, grid, 256, g, (const u32*)pc, w, (u64)N, k64a);
        { Prof _p(ctx, "radix_sort"); ZKW_TRY(radix_sort_pairs<u64>(ctx, tmp, tmp_bytes, k64a, k64b, pc, pn, N, 64)); }
        u32* x = pc; pc = pn; pn = x;
    }
    *perm = pc;
    return ZKW_OK;
}
// a bare key set as the "batch" of an empty tree
static StMerge st_keys_only(const u32* d_keys, size_t n) { return StMerge{nullptr, nullptr, nullptr, d_keys, nullptr, 0, (u64)n, 0}; }

// m pairs in device memory, inserted one after another in array order (insert_many_leafs, tree/mod.rs:65-81)
static int st_insert_device(zkw_storage_tree* t, const u32* d_keys, const u32* d_values, size_t m) {
    zkw_ctx* ctx = t->ctx;
    if (m == 0) return ZKW_OK;
    const size_t N = t->n + m;
    if (N >= (1ull << 32) - 1) return fail(ZKW_ERR_OOM, "zkw_storage_tree: %zu leaves and %zu pairs are more than one insert sorts", t->n, m);
    u32 *new_first = nullptr, *new_rank = nullptr, *heads = nullptr;
    ZKW_TRY(ctx->scratch_t<u32>("st_new_first", m, &new_first));
    ZKW_TRY(ctx->scratch_t<u32>("st_new_rank", m + 1, &new_rank));
    ZKW_TRY(ctx->scratch_t<u32>("st_heads", N + 1, &heads));
    const int cur = t->cur, oth = cur ^ 1;
    StMerge g{t->keys[cur], t->index[cur], t->values[cur], d_keys, d_values, (u64)t->n, (u64)m, t->next_index};
    const unsigned grid = blocks_for(N, 256);
    const u32* pc = nullptr;
    ZKW_TRY(st_sort_merged(ctx, g, N, &pc));
    // which batch entries bring a new leaf, and their ranks in array order
    ZKW_LAUNCH(ctx, k_st_mark, grid, 256, g, pc, (u64)N, new_first);
    ZKW_TRY(flag_prefix(ctx, "k_st_new_rank", StArrayFlag{new_first}, m, new_rank));
    u32 n_new = 0;
    ZKW_TRY(ctx->read_small(&n_new, new_rank + m, sizeof n_new));
    if (t->n + n_new > t->cap)  // nothing of the tree has been written yet
        return fail(ZKW_ERR_OOM, "zkw_storage_tree: %zu leaves + %u new ones exceed the capacity of %zu", t->n, n_new, t->cap);
    ZKW_TRY(flag_prefix(ctx, "k_st_heads", StHeadFlag{g, pc}, N, heads));
    ZKW_LAUNCH(ctx, k_st_emit, grid, 256, g, pc, (u64)N, (const u32*)heads, (const u32*)new_rank, t->keys[oth], t->index[oth], t->values[oth]);
    t->cur = oth;
    t->n += n_new;
    t->next_index += n_new;
    return st_rebuild(t);
}

extern "C" int zkw_storage_tree_insert(zkw_storage_tree* t, const uint8_t* keys, const uint8_t* values, size_t n) {
    if (!t || (n && (!keys || !values))) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_insert: null argument");
    if (t->witness) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_insert: a witness tree does not change");
    zkw_ctx* ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *d_k = nullptr, *d_v = nullptr;
    ZKW_TRY(ctx->in("st_in_keys", keys, n * 32, &d_k));
    ZKW_TRY(ctx->in("st_in_values", values, n * 32, &d_v));
    return st_insert_device(t, reinterpret_cast<const u32*>(d_k), reinterpret_cast<const u32*>(d_v), n);
}

// `missing`: the flag word of k_sw_lookup, or NULL; a full tree answers every key and leaves it alone
static int st_query(zkw_ctx* ctx, const zkw_storage_tree* t, const StQuery& q, size_t n, u32* missing = nullptr) {
    if (t->witness) {
        ZKW_LAUNCH(ctx, k_sw_lookup, n, ST_DEPTH, t->table(), q, missing);
        return ZKW_OK;
    }
    ZKW_LAUNCH(ctx, k_st_query, n, ST_DEPTH, t->view(), q);
    return ZKW_OK;
}

extern "C" int zkw_storage_tree_get_leaves(const zkw_storage_tree* t, const uint8_t* keys, size_t n, uint64_t* leaf_indexes, uint8_t* values,
                                           uint8_t* merkle_paths) {
    if (!t || (n && !keys)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_get_leaves: null argument");
    if (n >= (1ull << 31)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_get_leaves: too many keys");
    zkw_ctx* ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return ZKW_OK;
    const uint8_t* d_k = nullptr;
    ZKW_TRY(ctx->in("st_q_keys", keys, n * 32, &d_k));
    u64* d_idx = nullptr;
    uint8_t *d_val = nullptr, *d_paths = nullptr;
    if (leaf_indexes) ZKW_TRY(ctx->out("st_q_idx", leaf_indexes, n, &d_idx));
    if (values) ZKW_TRY(ctx->out("st_q_values", values, n * 32, &d_val));
    if (merkle_paths) ZKW_TRY(ctx->out("st_q_paths", merkle_paths, n * ST_DEPTH * 32, &d_paths));
    StQuery q{nullptr, reinterpret_cast<const u32*>(d_k), d_idx, reinterpret_cast<u32*>(d_val), reinterpret_cast<u32*>(d_paths)};
    if (t->witness) {  // a key outside the table is the caller's error (in device pointer mode the kernel has written the caller's buffers by then)
        u32 *d_missing = nullptr, missing = 0;
        ZKW_TRY(ctx->scratch_t<u32>("sw_missing", 1, &d_missing));
        HIP_TRY(ctx->memset_async(d_missing, 0, sizeof(u32)));
        ZKW_TRY(st_query(ctx, t, q, n, d_missing));
        ZKW_TRY(ctx->read_small(&missing, d_missing, sizeof missing));
        if (missing) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_get_leaves: the key at position %zu is not in the witness tree", n - missing);
    } else {
        ZKW_TRY(st_query(ctx, t, q, n));
    }
    if (leaf_indexes) ZKW_TRY(ctx->finish_out(leaf_indexes, d_idx, n));
    if (values) ZKW_TRY(ctx->finish_out(values, d_val, n * 32));
    if (merkle_paths) ZKW_TRY(ctx->finish_out(merkle_paths, d_paths, n * ST_DEPTH * 32));
    return ctx->sync_if_host();
}

extern "C" int zkw_storage_tree_answer_queries(const zkw_storage_tree* t, zkw_ctx* ctx, const zkw_log_query* queries, size_t n,
                                               uint64_t* leaf_indexes, uint8_t* merkle_paths) {
    if (!t || !ctx || (n && !queries)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_answer_queries: null argument");
    if (ctx->device != t->ctx->device) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_answer_queries: the tree lives on device %d, the context on device %d", t->ctx->device, ctx->device);
    if (n >= (1ull << 31)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_answer_queries: too many queries");
    if (n == 0) return ZKW_OK;
    StQuery q{queries, nullptr, leaf_indexes, nullptr, reinterpret_cast<u32*>(merkle_paths)};
    return st_query(ctx, t, q, n);
}

// the same with the flag word of a witness tree's lookup (zkw_internal.h): d_missing is zeroed here, ahead of the lookup, on ctx's stream
int zkw_storage_tree_answer_queries_flagged(const zkw_storage_tree* t, zkw_ctx* ctx, const zkw_log_query* queries, size_t n, uint64_t* leaf_indexes,
                                            uint8_t* merkle_paths, uint32_t* d_missing) {
    if (!t || !ctx || !d_missing || (n && !queries)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_answer_queries: null argument");
    if (ctx->device != t->ctx->device) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_answer_queries: the tree lives on device %d, the context on device %d", t->ctx->device, ctx->device);
    if (n >= (1ull << 31)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_answer_queries: too many queries");
    HIP_TRY(ctx->memset_async(d_missing, 0, sizeof(u32)));
    if (n == 0) return ZKW_OK;
    StQuery q{queries, nullptr, leaf_indexes, nullptr, reinterpret_cast<u32*>(merkle_paths)};
    return st_query(ctx, t, q, n, d_missing);
}

// queries in DEVICE memory (zkw_internal.h: zkw_block_apply_storage hands over the block's own deduplicated queue)
int zkw_storage_tree_apply_queries_device(zkw_storage_tree* t, const zkw_log_query* d_queries, size_t n) {
    if (!t || (n && !d_queries)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_apply_queries: null argument");
    if (t->witness) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_apply_queries: a witness tree does not change");
    if (n >= (1ull << 31)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_apply_queries: too many queries");
    zkw_ctx* ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return ZKW_OK;
    u32 *rank = nullptr, *wk = nullptr, *wv = nullptr;
    ZKW_TRY(ctx->scratch_t<u32>("st_ap_rank", n + 1, &rank));
    ZKW_TRY(ctx->scratch_t<u32>("st_ap_keys", n * 8, &wk));
    ZKW_TRY(ctx->scratch_t<u32>("st_ap_values", n * 8, &wv));
    ZKW_TRY(flag_prefix(ctx, "k_st_write_rank", StWriteFlag{d_queries}, n, rank));
    ZKW_LAUNCH(ctx, k_st_writes, blocks_for(n, 64), 64, d_queries, (u64)n, (const u32*)rank, wk, wv);
    u32 m = 0;
    ZKW_TRY(ctx->read_small(&m, rank + n, sizeof m));
    return st_insert_device(t, wk, wv, m);
}

extern "C" int zkw_storage_tree_apply_queries(zkw_storage_tree* t, const zkw_log_query* queries, size_t n) {
    if (!t || (n && !queries)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_apply_queries: null argument");
    if (t->witness) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_apply_queries: a witness tree does not change");
    zkw_ctx* ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const zkw_log_query* d_q = nullptr;
    ZKW_TRY(ctx->in("st_ap_queries", queries, n, &d_q));
    return zkw_storage_tree_apply_queries_device(t, d_q, n);
}

// ------------------------------------------------------------------------------------------------ witness trees
// `t` becomes an empty table for up to `entries` entries (the caller commits it once the table is complete)
static int sw_alloc(Building<zkw_storage_tree>& t, size_t entries, const char* who) {
    t->witness = true;
    t->cap = entries;
    t.alloc(&t->keys[0], entries * 32);
    t.alloc(&t->index[0], entries * 8);
    t.alloc(&t->values[0], entries * 32);
    t.alloc(&t->paths, entries * (size_t)ST_DEPTH * 32);
    if (t.err != hipSuccess) {
        (void)hipGetLastError();
        return fail(ZKW_ERR_OOM, "%s: %zu entries need %zu bytes of device memory: %s", who, entries, entries * (size_t)(ST_DEPTH * 32 + 72), hipGetErrorString(t.err));
    }
    return ZKW_OK;
}

static const char* sw_reason(u32 status) {
    if (status & SW_BAD_INDEX) return "its leaf index is not below the next enumeration index";
    if (status & SW_BAD_EMPTY) return "index 0 (an absent key) with a nonzero value";
    if (status & SW_BAD_ROOT) return "its Merkle path does not lead to the root";
    return "its key repeats an earlier entry's";
}

extern "C" int zkw_storage_tree_create_witness(zkw_ctx* ctx, const uint8_t* keys, const uint64_t* leaf_indexes, const uint8_t* values,
                                               const uint8_t* merkle_paths, size_t n, const uint8_t root[32], uint64_t next_enumeration_index,
                                               zkw_storage_tree** out) {
    if (!ctx || !out || !root || (n && (!keys || !leaf_indexes || !values || !merkle_paths)))
        return fail(ZKW_ERR_INVALID, "zkw_storage_tree_create_witness: null argument");
    if (next_enumeration_index == 0) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_create_witness: the next enumeration index is at least 1 (index 0 is the empty leaf's)");
    if (n >= (1ull << 31)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_create_witness: at most 2^31 - 1 entries");
    if (ctx->batch) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_create_witness: the context belongs to a batch of blocks");
    HIP_TRY(hipSetDevice(ctx->device));
    *out = nullptr;
    const uint8_t *d_k = nullptr, *d_v = nullptr, *d_p = nullptr;
    const uint64_t* d_i = nullptr;
    ZKW_TRY(ctx->in("sw_in_keys", keys, n * 32, &d_k));
    ZKW_TRY(ctx->in("sw_in_index", leaf_indexes, n, &d_i));
    ZKW_TRY(ctx->in("sw_in_values", values, n * 32, &d_v));
    ZKW_TRY(ctx->in("sw_in_paths", merkle_paths, n * (size_t)ST_DEPTH * 32, &d_p));
    u32 *status = nullptr, *meta = nullptr;  // meta[0] = the first bad entry, meta[1] = entries with a nonzero index
    ZKW_TRY(ctx->scratch_t<u32>("sw_status", n + 1, &status));
    ZKW_TRY(ctx->scratch_t<u32>("sw_meta", 2, &meta));
    Building<zkw_storage_tree> t(ctx);
    ZKW_TRY(sw_alloc(t, n, "zkw_storage_tree_create_witness"));
    memcpy(t->root, root, 32);
    t->next_index = next_enumeration_index;
    u32 h_meta[2] = {~0u, 0};
    HIP_TRY(ctx->memset_async(meta, 0xFF, sizeof(u32)));
    HIP_TRY(ctx->memset_async(meta + 1, 0, sizeof(u32)));
    if (n) {
        SwEntries e{reinterpret_cast<const u32*>(d_k), d_i, reinterpret_cast<const u32*>(d_v), reinterpret_cast<const u32*>(d_p), (u64)n, next_enumeration_index, {}};
        memcpy(e.root, root, 32);
        ZKW_LAUNCH(ctx, k_sw_verify, blocks_for(n, 64), 64, e, status, meta);
        const u32* perm = nullptr;
        ZKW_TRY(st_sort_merged(ctx, st_keys_only(e.keys, n), n, &perm));
        ZKW_LAUNCH(ctx, k_sw_gather, n, ST_DEPTH, e, perm, SwTable{t->keys[0], t->index[0], t->values[0], t->paths}, status, meta);
        ZKW_LAUNCH(ctx, k_sw_count, blocks_for(n, 256), 256, (const u64*)t->index[0], (u64)n, meta + 1);
        ZKW_TRY(ctx->read_small(h_meta, meta, sizeof h_meta));
    }
    if (h_meta[0] != ~0u) {
        u32 st = 0;
        ZKW_TRY(ctx->read_small(&st, status + h_meta[0], sizeof st));
        return fail(ZKW_ERR_INVALID, "zkw_storage_tree_create_witness: entry %u is not a proof for this root: %s", h_meta[0], sw_reason(st));
    }
    t->n = h_meta[1];
    t.commit(out);
    return ZKW_OK;
}

extern "C" int zkw_storage_tree_extract_witness(const zkw_storage_tree* tree, zkw_ctx* ctx, const uint8_t* keys, size_t n, zkw_storage_tree** out) {
    if (!tree || !ctx || !out || (n && !keys)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_extract_witness: null argument");
    if (tree->witness) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_extract_witness: the source is a witness tree; a witness is cut out of a full tree");
    if (ctx->device != tree->ctx->device) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_extract_witness: the tree lives on device %d, the context on device %d", tree->ctx->device, ctx->device);
    if (n >= (1ull << 31)) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_extract_witness: at most 2^31 - 1 keys");
    if (ctx->batch) return fail(ZKW_ERR_INVALID, "zkw_storage_tree_extract_witness: the context belongs to a batch of blocks");
    HIP_TRY(hipSetDevice(ctx->device));
    *out = nullptr;
    const uint8_t* d_k = nullptr;
    ZKW_TRY(ctx->in("sw_in_keys", keys, n * 32, &d_k));
    const u32* d_keys = reinterpret_cast<const u32*>(d_k);
    // the distinct keys in order: the sort, then a count of the runs' heads
    u32 unique = 0, *heads = nullptr;
    const u32* perm = nullptr;
    if (n) {
        ZKW_TRY(ctx->scratch_t<u32>("st_heads", n + 1, &heads));
        ZKW_TRY(st_sort_merged(ctx, st_keys_only(d_keys, n), n, &perm));
        ZKW_TRY(flag_prefix(ctx, "k_st_heads", StHeadFlag{st_keys_only(d_keys, n), perm}, n, heads));
        ZKW_TRY(ctx->read_small(&unique, heads + n, sizeof unique));
    }
    Building<zkw_storage_tree> t(ctx);
    ZKW_TRY(sw_alloc(t, unique, "zkw_storage_tree_extract_witness"));
    memcpy(t->root, tree->root, 32);
    t->next_index = tree->next_index;
    u32 count = 0;
    if (unique) {
        u32* d_count = nullptr;
        ZKW_TRY(ctx->scratch_t<u32>("sw_meta", 2, &d_count));
        HIP_TRY(ctx->memset_async(d_count, 0, sizeof(u32)));
        ZKW_LAUNCH(ctx, k_sw_unique_keys, blocks_for(n, 256), 256, d_keys, perm, (const u32*)heads, (u64)n, t->keys[0]);
        // the full tree's answers straight into the table
        ZKW_TRY(st_query(ctx, tree, StQuery{nullptr, t->keys[0], t->index[0], t->values[0], t->paths}, unique));
        ZKW_LAUNCH(ctx, k_sw_count, blocks_for(unique, 256), 256, (const u64*)t->index[0], (u64)unique, d_count);
        ZKW_TRY(ctx->read_small(&count, d_count, sizeof count));
    }
    t->n = count;
    t.commit(out);
    return ZKW_OK;
}

// ------------------------------------------------------------------------------------------------ advancing a witness tree
// the writes `wr` (device memory) applied to the state `src` holds: storage_witness_kernels.cuh, "advance". One readback at the end: the
// flag word of a key outside the table, |W|, the new leaves and the root together.
static int sw_advance(const char* who, const zkw_storage_tree* src, zkw_ctx* ctx, const SwaWrites& wr, zkw_storage_tree** out) {
    const size_t entries = src->cap, n = (size_t)wr.n;
    const size_t bound = std::min(entries, n);  // >= the written entries
    u32 *first = nullptr, *meta = nullptr, *ent = nullptr, *new_rank = nullptr, *wrank = nullptr, *wlist = nullptr, *wval = nullptr, *up = nullptr, *d = nullptr, *nxt = nullptr;
    u64* widx = nullptr;
    ZKW_TRY(ctx->scratch_t<u32>("swa_first", entries, &first));
    ZKW_TRY(ctx->scratch_t<u32>("swa_meta_last", SWA_META_WORDS + entries, &meta));
    ZKW_TRY(ctx->scratch_t<u32>("swa_ent", n, &ent));
    ZKW_TRY(ctx->scratch_t<u32>("swa_new_rank", n + 1, &new_rank));
    ZKW_TRY(ctx->scratch_t<u32>("swa_wrank", entries + 1, &wrank));
    ZKW_TRY(ctx->scratch_t<u32>("swa_wlist", bound, &wlist));
    ZKW_TRY(ctx->scratch_t<u64>("swa_widx", bound, &widx));
    ZKW_TRY(ctx->scratch_t<u32>("swa_wval", bound * 8, &wval));
    ZKW_TRY(ctx->scratch_t<u32>("swa_d", bound, &d));
    ZKW_TRY(ctx->scratch_t<u32>("swa_nxt", bound, &nxt));
    ZKW_TRY(ctx->scratch_t<u32>("swa_up", bound * (size_t)(ST_DEPTH + 1) * 8, &up));
    u32* last = meta + SWA_META_WORDS;
    Building<zkw_storage_tree> t(ctx);
    ZKW_TRY(sw_alloc(t, entries, who));
    u32 h_meta[SWA_META_WORDS] = {};
    if (entries) HIP_TRY(ctx->memset_async(first, 0xFF, entries * sizeof(u32)));
    HIP_TRY(ctx->memset_async(meta, 0, (SWA_META_WORDS + entries) * sizeof(u32)));
    const SwView tv = src->table();
    const SwaFold f{tv, wlist, up, d, nxt, meta, (u64)bound};
    ZKW_LAUNCH(ctx, k_swa_locate, blocks_for(n, 64), 64, tv, wr, ent, first, last, meta);
    ZKW_TRY(flag_prefix(ctx, "k_swa_new_rank", SwaNewFlag{ent, first, tv.index}, n, new_rank));
    ZKW_TRY(flag_prefix(ctx, "k_swa_wrank", SwaWrittenFlag{first}, entries, wrank));
    ZKW_LAUNCH(ctx, k_swa_compact, blocks_for(entries, 256), 256, (const u32*)first, (const u32*)wrank, (const u32*)new_rank, (u64)entries, (u64)n, wlist, meta);
    ZKW_LAUNCH(ctx, k_swa_leaves, blocks_for(bound, 64), 64, f, wr, (const u32*)first, (const u32*)last, (const u32*)new_rank, src->next_index, widx, wval);
    if (bound <= ST_PERSISTENT_MAX) {
        ZKW_LAUNCH(ctx, k_swa_fold, bound ? 1 : 0, ST_PERSISTENT_THREADS, f);  // (no writes: nothing is launched, the span is still recorded)
    } else {
        for (int L = 0; L < ST_DEPTH; L++) ZKW_LAUNCH(ctx, k_swa_level, blocks_for(bound, 64), 64, f, L);
    }
    ZKW_LAUNCH(ctx, k_swa_paths, entries, ST_DEPTH, f, (const u32*)first, (const u32*)wrank, (const u64*)widx, (const u32*)wval, SwTable{t->keys[0], t->index[0], t->values[0], t->paths});
    ZKW_TRY(ctx->read_small(h_meta, meta, sizeof h_meta));
    if (h_meta[SWA_META_MISSING])
        return fail(ZKW_ERR_INVALID, "%s: the key written at position %zu is not in the witness tree", who, n - h_meta[SWA_META_MISSING]);
    memcpy(t->root, h_meta[SWA_META_NW] ? reinterpret_cast<const uint8_t*>(h_meta + SWA_META_ROOT) : src->root, 32);
    t->n = src->n + h_meta[SWA_META_NEW];
    t->next_index = src->next_index + h_meta[SWA_META_NEW];
    t.commit(out);
    return ZKW_OK;
}

static int sw_advance_check(const char* who, const zkw_storage_tree* w, zkw_ctx* ctx, size_t n, zkw_storage_tree** out) {
    if (!w || !ctx || !out) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    if (!w->witness) return fail(ZKW_ERR_INVALID, "%s: the source is a full tree; it takes zkw_storage_tree_insert / _apply_queries", who);
    if (ctx->device != w->ctx->device) return fail(ZKW_ERR_INVALID, "%s: the tree lives on device %d, the context on device %d", who, w->ctx->device, ctx->device);
    if (n >= (1ull << 31)) return fail(ZKW_ERR_INVALID, "%s: at most 2^31 - 1 writes", who);
    if (ctx->batch) return fail(ZKW_ERR_INVALID, "%s: the context belongs to a batch of blocks", who);
    *out = nullptr;
    return ZKW_OK;
}

extern "C" int zkw_storage_tree_advance_witness(const zkw_storage_tree* witness, zkw_ctx* ctx, const uint8_t* keys, const uint8_t* values, size_t n,
                                                zkw_storage_tree** out) {
    static const char who[] = "zkw_storage_tree_advance_witness";
    if (n && (!keys || !values)) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    ZKW_TRY(sw_advance_check(who, witness, ctx, n, out));
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *d_k = nullptr, *d_v = nullptr;
    ZKW_TRY(ctx->in("swa_in_keys", keys, n * 32, &d_k));
    ZKW_TRY(ctx->in("swa_in_values", values, n * 32, &d_v));
    return sw_advance(who, witness, ctx, SwaWrites{nullptr, reinterpret_cast<const u32*>(d_k), reinterpret_cast<const u32*>(d_v), (u64)n}, out);
}

extern "C" int zkw_storage_tree_advance_witness_by_queries(const zkw_storage_tree* witness, zkw_ctx* ctx, const zkw_log_query* queries, size_t n,
                                                           zkw_storage_tree** out) {
    static const char who[] = "zkw_storage_tree_advance_witness_by_queries";
    if (n && !queries) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    ZKW_TRY(sw_advance_check(who, witness, ctx, n, out));
    HIP_TRY(hipSetDevice(ctx->device));
    const zkw_log_query* d_q = nullptr;
    ZKW_TRY(ctx->in("swa_in_queries", queries, n, &d_q));
    // (n == 0: no query is read, and SwaWrites with queries == NULL is the pair form with no pair)
    return sw_advance(who, witness, ctx, SwaWrites{d_q, nullptr, nullptr, (u64)n}, out);
}

// ------------------------------------------------------------------------------------------------ a chain of K blocks in one call
// storage_witness_kernels.cuh, "chain". Two readbacks: the blocks' entry counts with the miss word (the K tables are allocated after
// it), and the roots and counts at the end. The 256 + K - 1 steps of the wavefront are plain launches on ctx's stream.
static int sw_chain(const char* who, const zkw_storage_tree* src, zkw_ctx* ctx, SwaWrites wr, const std::vector<u32>& offs, zkw_storage_tree** out,
                    zkw_storage_tree** final_state) {
    const size_t K = offs.size() - 1, E = src->cap, N = offs[K], KE = K * E;
    const size_t bound = std::min(N, KE);  // >= the written (block, entry) pairs
    u32 *flags = nullptr, *trank = nullptr, *wrank = nullptr, *cfirst = nullptr, *ent = nullptr, *new_rank = nullptr, *wl = nullptr, *h = nullptr, *hdr = nullptr,
        *fin = nullptr, *d_offs = nullptr;
    ZKW_TRY(ctx->scratch_t<u32>("swc_flags", 3 * KE, &flags));
    ZKW_TRY(ctx->scratch_t<u32>("swc_trank", KE + 1, &trank));
    ZKW_TRY(ctx->scratch_t<u32>("swc_wrank", KE + 1, &wrank));
    ZKW_TRY(ctx->scratch_t<u32>("swc_cfirst", E, &cfirst));
    ZKW_TRY(ctx->scratch_t<u32>("swc_ent", N, &ent));
    ZKW_TRY(ctx->scratch_t<u32>("swc_new_rank", N + 1, &new_rank));
    ZKW_TRY(ctx->scratch_t<u32>("swc_wlists", 4 * bound, &wl));
    ZKW_TRY(ctx->scratch_t<u32>("swc_heights", 16 * bound, &h));
    const size_t hdr_words = SWC_HDR_WORDS + 2 * (K + 1), fin_words = 10 * K + 1;
    ZKW_TRY(ctx->scratch_t<u32>("swc_hdr", hdr_words, &hdr));
    ZKW_TRY(ctx->scratch_t<u32>("swc_fin", fin_words, &fin));
    ZKW_TRY(ctx->upload("swc_offs", offs, &d_offs));
    u32 *touched = flags, *first = flags + KE, *last = flags + 2 * KE, *tbase = hdr + SWC_HDR_WORDS, *wbase = tbase + K + 1;
    const SwView tv = src->table();
    SwcChain c{tv.keys, SwTable{}, nullptr, touched, first, trank, wrank, tbase, wbase, wl, wl + bound, wl + 2 * bound, wl + 3 * bound, h, fin, (u64)E, (u64)bound, (u32)K};
    // locate, ranks, and the first readback
    std::vector<u32> h_hdr(hdr_words);
    {
        if (KE) {
            HIP_TRY(ctx->memset_async(touched, 0, KE * sizeof(u32)));
            HIP_TRY(ctx->memset_async(first, 0xFF, KE * sizeof(u32)));
            HIP_TRY(ctx->memset_async(last, 0, KE * sizeof(u32)));
            HIP_TRY(ctx->memset_async(cfirst, 0xFF, E * sizeof(u32)));
        }
        HIP_TRY(ctx->memset_async(hdr, 0, hdr_words * sizeof(u32)));
        HIP_TRY(ctx->memset_async(fin, 0, fin_words * sizeof(u32)));
        ZKW_LAUNCH(ctx, k_swc_locate, blocks_for(N, 64), 64, tv, SwcQueries{wr, d_offs, (u32)K}, ent, touched, first, last, cfirst, hdr);
        ZKW_TRY(flag_prefix(ctx, "k_swc_trank", SwcTouchedFlag{touched}, KE, trank));
        ZKW_TRY(flag_prefix(ctx, "k_swc_wrank", SwaWrittenFlag{first}, KE, wrank));
        ZKW_TRY(flag_prefix(ctx, "k_swc_new_rank", SwcNewFlag{ent, cfirst, tv.index}, N, new_rank));
        ZKW_LAUNCH(ctx, k_swc_compact, blocks_for(std::max(KE, K + 1), 256), 256, c, tbase, wbase);
        ZKW_TRY(ctx->read_small(h_hdr.data(), hdr, hdr_words * sizeof(u32)));
    }
    if (h_hdr[SWC_HDR_MISSING]) {
        const size_t p = N - h_hdr[SWC_HDR_MISSING];
        size_t k = 0;
        while (offs[k + 1] <= p) k++;
        return fail(ZKW_ERR_INVALID, "%s: the key at (block %zu, position %zu) is not in the witness tree", who, k, p - offs[k]);
    }
    const u32 *h_tbase = h_hdr.data() + SWC_HDR_WORDS, *h_wbase = h_tbase + K + 1;
    // the K tables and the working copy
    std::vector<Building<zkw_storage_tree>> made;
    made.reserve(K + 1);
    for (size_t k = 0; k <= K; k++) {
        made.emplace_back(ctx);
        ZKW_TRY(sw_alloc(made[k], k < K ? h_tbase[k + 1] - h_tbase[k] : E, who));
    }
    Building<zkw_storage_tree>& work = made[K];
    std::vector<u32> h_fin(fin_words);
    std::vector<SwTable> tabs(K);
    for (size_t k = 0; k < K; k++) tabs[k] = SwTable{made[k]->keys[0], made[k]->index[0], made[k]->values[0], made[k]->paths};
    SwTable* d_tabs = nullptr;
    ZKW_TRY(ctx->upload("swc_tables", tabs, &d_tabs));
    c.outs = d_tabs;
    c.work = SwTable{work->keys[0], work->index[0], work->values[0], work->paths};
    if (E) {
        HIP_TRY(ctx->copy_async(work->keys[0], tv.keys, E * 32, hipMemcpyDeviceToDevice));
        Prof _p(ctx, "swc_copy_paths");
        HIP_TRY(ctx->copy_async(work->paths, tv.paths, E * (size_t)ST_DEPTH * 32, hipMemcpyDeviceToDevice));
    }
    ZKW_LAUNCH(ctx, k_swc_walk, blocks_for(E, 64), 64, c, wr, tv.index, tv.values, (const u32*)last, (const u32*)cfirst, (const u32*)new_rank, src->next_index);
    const unsigned fold_wgs = blocks_for(h_wbase[K], 256), all_wgs = fold_wgs + blocks_for(KE, 256);
    if (h_tbase[K])  // (a chain without a query captures and folds nothing)
        for (int s = 0; s < ST_DEPTH + (int)K - 1; s++) ZKW_LAUNCH(ctx, k_swc_step, all_wgs, 256, c, fold_wgs, s);
    ZKW_TRY(ctx->read_small(h_fin.data(), fin, fin_words * sizeof(u32)));
    // roots and indices are carried over the blocks: a block without writes leaves the state as it is
    uint8_t root[32];
    memcpy(root, src->root, 32);
    u64 next = src->next_index;
    for (size_t k = 0; k <= K; k++) {
        Building<zkw_storage_tree>& t = made[k];
        memcpy(t->root, root, 32);
        t->next_index = next;
        t->n = h_fin[9 * K + k];
        if (k < K && h_wbase[k + 1] != h_wbase[k]) memcpy(root, h_fin.data() + 8 * k, 32);
        if (k < K) next += h_fin[8 * K + k];
    }
    if (final_state) work.commit(final_state);  // (else the working copy goes when `made` does)
    for (size_t k = 0; k < K; k++) made[k].commit(&out[k]);
    return ZKW_OK;
}

// the argument checks of both forms; offs = the offsets as the kernels take them
static int sw_chain_check(const char* who, const zkw_storage_tree* w, zkw_ctx* ctx, bool have_input, const uint64_t* block_offsets, size_t n_blocks,
                          zkw_storage_tree** out, zkw_storage_tree** final_state, std::vector<u32>* offs) {
    if (!w || !ctx || !block_offsets || !out) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    if (n_blocks == 0) return fail(ZKW_ERR_INVALID, "%s: no blocks", who);
    if (block_offsets[0] != 0) return fail(ZKW_ERR_INVALID, "%s: block_offsets[0] is %llu, not 0", who, (unsigned long long)block_offsets[0]);
    for (size_t k = 0; k < n_blocks; k++)
        if (block_offsets[k + 1] < block_offsets[k]) return fail(ZKW_ERR_INVALID, "%s: block_offsets decrease at block %zu", who, k);
    const uint64_t n = block_offsets[n_blocks];
    if (n && !have_input) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    if (!w->witness) return fail(ZKW_ERR_INVALID, "%s: the source is a full tree; it takes zkw_storage_tree_insert / _apply_queries", who);
    if (ctx->device != w->ctx->device) return fail(ZKW_ERR_INVALID, "%s: the tree lives on device %d, the context on device %d", who, w->ctx->device, ctx->device);
    if (ctx->batch) return fail(ZKW_ERR_INVALID, "%s: the context belongs to a batch of blocks", who);
    if (n >= (1ull << 31)) return fail(ZKW_ERR_INVALID, "%s: at most 2^31 - 1 queries", who);
    if ((uint64_t)n_blocks * std::max<uint64_t>(w->cap, 1) >= (1ull << 31)) return fail(ZKW_ERR_INVALID, "%s: %zu blocks x %zu entries are 2^31 or more", who, n_blocks, w->cap);
    for (size_t k = 0; k < n_blocks; k++) out[k] = nullptr;
    if (final_state) *final_state = nullptr;
    offs->assign(block_offsets, block_offsets + n_blocks + 1);
    return ZKW_OK;
}

extern "C" int zkw_storage_tree_advance_witness_chain(const zkw_storage_tree* witness, zkw_ctx* ctx, const zkw_log_query* queries, const uint64_t* block_offsets,
                                                      size_t n_blocks, zkw_storage_tree** out, zkw_storage_tree** final_state) {
    static const char who[] = "zkw_storage_tree_advance_witness_chain";
    std::vector<u32> offs;
    ZKW_TRY(sw_chain_check(who, witness, ctx, queries != nullptr, block_offsets, n_blocks, out, final_state, &offs));
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = offs[n_blocks];
    const zkw_log_query* d_q = nullptr;
    ZKW_TRY(ctx->in("swc_in_queries", queries, n, &d_q));
    // (n == 0: no query is read, and SwaWrites with queries == NULL is the pair form with no pair)
    return sw_chain(who, witness, ctx, SwaWrites{d_q, nullptr, nullptr, (u64)n}, offs, out, final_state);
}

extern "C" int zkw_storage_tree_advance_witness_chain_pairs(const zkw_storage_tree* witness, zkw_ctx* ctx, const uint8_t* keys, const uint8_t* values,
                                                            const uint64_t* block_offsets, size_t n_blocks, zkw_storage_tree** out, zkw_storage_tree** final_state) {
    static const char who[] = "zkw_storage_tree_advance_witness_chain_pairs";
    std::vector<u32> offs;
    ZKW_TRY(sw_chain_check(who, witness, ctx, keys && values, block_offsets, n_blocks, out, final_state, &offs));
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = offs[n_blocks];
    const uint8_t *d_k = nullptr, *d_v = nullptr;
    ZKW_TRY(ctx->in("swc_in_keys", keys, n * 32, &d_k));
    ZKW_TRY(ctx->in("swc_in_values", values, n * 32, &d_v));
    return sw_chain(who, witness, ctx, SwaWrites{nullptr, reinterpret_cast<const u32*>(d_k), reinterpret_cast<const u32*>(d_v), (u64)n}, offs, out, final_state);
}
