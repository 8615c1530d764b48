// storage_tree_kernels.cuh — the library's own BinarySparseStorageTree, resident in HBM (include/zkw.h, zkw_storage_tree).
//
// Reference: InMemoryStorageTree<256, 32, 8, Blake2s256, ZkSyncStorageLeaf>, src/witness/tree/mod.rs:101-384 behind the trait at
// :42-99. The reference keeps a hash map (level, masked key) -> node and walks 256 levels per leaf, one leaf after another. Here:
//   * the leaves are kept SORTED by key as a 256-bit number (word 7 of the eight little-endian words is the most significant: bit 255 =
//     the split at the root) next to (enumeration index, value);
//   * a non-empty node at height L covers a contiguous range of sorted leaves — those that share key >> L — and is stored at the rank of
//     the range's first leaf: nodes[L][first]. 256 x capacity x 32 B = 8 KiB per leaf, what ONE Merkle path of the leaf weighs;
//   * build (k_st_leaves, then k_st_level per height or k_st_levels for a small tree): d[i] = the highest bit where leaf i differs from
//     leaf i - 1, so i starts a range at height h iff d[i] >= h; nxt[i] = the start of the next range at the current height. A node at
//     height L + 1 has at most two children at height L: its own start a, and m = nxt[a] when d[m] == L. No search, no sort per level:
//     a thread per leaf, idle once its leaf is no longer a range start;
//   * query (k_st_query): a workgroup per key, a thread per level: the sibling at level L is the node of the prefix
//     (key ^ (1 << L)) >> L; its range starts at the lower bound of that prefix among the sorted keys, and is empty — the level's
//     empty-subtree hash — when the leaf found there has another prefix;
//   * insert (k_st_iota .. k_st_emit around radix_sort_pairs and flag_prefix): tree leaves and batch are sorted together, stably, the
//     tree's leaves first; a run of equal keys keeps its head's enumeration index (a batch head: the next free index + its rank among
//     the batch's NEW first occurrences in array order) and its tail's value — "inserted one after another", without the chain.
// Everything a block's storage branch runs (k_st_query) is a kernel BODY (zkw_launch.h): inside zkw_blocks_run the K blocks' queries
// leave as one launch. Blake2s, the leaf hash and derive_final_address are storage_application_kernels.cuh's.
#pragma once
#include "storage_application_kernels.cuh"

namespace zkw {

constexpr int ST_DEPTH = 256;

// the tree as a reading kernel sees it
struct StView {
    const u32* keys;    // [n][8]
    const u64* index;   // [n]
    const u32* values;  // [n][8]: the value's 32 bytes as little-endian words
    const u32* nodes;   // [256][cap][8]: height 0 = the leaf hashes
    const u32* empty;   // [257][8]: the empty subtree of every height; [256] = the empty tree's root
    u64 n, cap;
};

// -1 / 0 / 1 as a < b / a == b / a > b, 256-bit numbers of eight little-endian words
__device__ __forceinline__ int st_cmp(const u32* __restrict__ a, const u32* b) {
    for (int w = 7; w >= 0; w--) {
        const u32 x = a[w], y = b[w];
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}
// the highest bit where a and b differ, -1 when they are equal
__device__ __forceinline__ int st_top_diff(const u32* __restrict__ a, const u32* b) {
    for (int w = 7; w >= 0; w--) {
        const u32 x = a[w] ^ b[w];
        if (x) return 32 * w + 31 - __clz(x);
    }
    return -1;
}
// the first leaf whose key is not below `target` (n when there is none)
__device__ __forceinline__ u64 st_lower_bound(const StView& t, const u32* target) {
    u64 lo = 0, hi = t.n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (st_cmp(t.keys + 8 * mid, target) < 0) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------ query
struct StQuery {
    const zkw_log_query* queries;  // the keys are derive_final_address of these, or (NULL) ...
    const u32* keys;               // ... given: [n][8]
    u64* leaf_indexes;             // [n] or NULL
    u32* values;                   // [n][8] or NULL
    u32* paths;                    // [n][256][8] or NULL
};

// grid = the keys, 256 threads: thread L answers level L. get_leaf, tree/mod.rs:219-240
static __device__ __forceinline__ void k_st_query(const VB& vb, StView t, StQuery q) {
    __shared__ u32 s_key[8];
    const u64 i = vb.x;
    const int L = threadIdx.x;
    if (q.queries) {
        if (L == 0) {
            u32 k[8];
            sap_derive_key(q.queries + i, k);
#pragma unroll
            for (int w = 0; w < 8; w++) s_key[w] = k[w];
        }
    } else if (L < 8) {
        s_key[L] = q.keys[8 * i + L];
    }
    __syncthreads();
    u32 key[8];
#pragma unroll
    for (int w = 0; w < 8; w++) key[w] = s_key[w];
    if (L == 0 && (q.leaf_indexes || q.values)) {
        const u64 j = st_lower_bound(t, key);
        const bool hit = j < t.n && st_cmp(t.keys + 8 * j, key) == 0;
        if (q.leaf_indexes) q.leaf_indexes[i] = hit ? t.index[j] : 0;
        if (q.values)
            for (int w = 0; w < 8; w++) q.values[8 * i + w] = hit ? t.values[8 * j + w] : 0;
    }
    if (!q.paths) return;
    // the sibling subtree at level L: the key with bit L flipped and the bits below cleared
    const int wl = L >> 5;
#pragma unroll
    for (int w = 0; w < 8; w++)
        if (w < wl) key[w] = 0;
        else if (w == wl) key[w] = (key[w] ^ (1u << (L & 31))) & ~((1u << (L & 31)) - 1u);
    const u64 j = st_lower_bound(t, key);
    const bool hit = j < t.n && st_top_diff(t.keys + 8 * j, key) < L;  // the leaf found shares the prefix above bit L - 1
    const uint4* src = reinterpret_cast<const uint4*>(hit ? t.nodes + ((u64)L * t.cap + j) * 8 : t.empty + 8 * L);
    uint4* dst = reinterpret_cast<uint4*>(q.paths + (i * ST_DEPTH + L) * 8);
    dst[0] = src[0];
    dst[1] = src[1];
}

// ------------------------------------------------------------------------------------------------ build
struct StBuild {
    const u32* keys;    // [n][8] sorted, distinct
    const u64* index;   // [n]
    const u32* values;  // [n][8]
    u32* nodes;         // [256][cap][8]
    const u32* empty;   // [257][8]
    u32* d;             // [n]: highest bit where leaf i differs from leaf i - 1 (256 for leaf 0)
    u32* nxt;           // [n]: for a range start of the current height, the start of the next range
    u32* root;          // [8]
    u64 n, cap;
};

// the empty subtrees (tree/mod.rs:159-198): one thread, 257 compressions, once per tree
static __device__ __forceinline__ void k_st_empty(const VB& vb, u32* __restrict__ empty) {
    if (threadIdx.x != 0 || vb.x != 0) return;
    u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cur[8], nx[8];
    sap_leaf_hash_bytes(0, zero, cur);
    for (int L = 0; L <= ST_DEPTH; L++) {
        for (int k = 0; k < 8; k++) empty[8 * L + k] = cur[k];
        sap_node_hash(cur, cur, nx);
        for (int k = 0; k < 8; k++) cur[k] = nx[k];
    }
}

static __device__ __forceinline__ void k_st_leaves(const VB& vb, StBuild b) {
    const u64 i = (u64)vb.x * blockDim.x + threadIdx.x;
    if (i >= b.n) return;
    u32 v[8], h[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = b.values[8 * i + k];
    sap_leaf_hash_bytes(b.index[i], v, h);
#pragma unroll
    for (int k = 0; k < 8; k++) b.nodes[8 * i + k] = h[k];
    b.d[i] = i ? (u32)st_top_diff(b.keys + 8 * i, b.keys + 8 * (i - 1)) : (u32)ST_DEPTH;
    b.nxt[i] = (u32)(i + 1);
}

// height L + 1 from height L for leaf i (see the header comment); the node of height 256 is the root
__device__ __forceinline__ void st_level_step(const StBuild& b, int L, u64 i) {
    if (b.d[i] <= (u32)L) return;  // not the first leaf of a node of height L + 1
    const u32 m = b.nxt[i];
    const bool has_sibling = m < b.n && b.d[m] == (u32)L;  // the next node of height L lies under the same parent
    const bool right = (b.keys[8 * i + (L >> 5)] >> (L & 31)) & 1;  // this node is the right child: the left one is empty (the leaves are sorted)
    const u32* mine = b.nodes + ((u64)L * b.cap + i) * 8;
    const u32* other = has_sibling ? b.nodes + ((u64)L * b.cap + m) * 8 : b.empty + 8 * L;
    u32 l[8], r[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const u32 a = mine[k], c = other[k];
        l[k] = right ? c : a;
        r[k] = right ? a : c;
    }
    sap_node_hash(l, r, o);
    u32* out = L + 1 == ST_DEPTH ? b.root : b.nodes + ((u64)(L + 1) * b.cap + i) * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = o[k];
    if (has_sibling) b.nxt[i] = b.nxt[m];  // (m starts no node of height L + 1: nobody writes nxt[m] at this height)
}

static __device__ __forceinline__ void k_st_level(const VB& vb, StBuild b, int L) {
    const u64 i = (u64)vb.x * blockDim.x + threadIdx.x;
    if (i < b.n) st_level_step(b, L, i);
}

// all heights in one launch for a tree one workgroup holds: a barrier (and a device-scope fence: the hashes travel through global memory)
// per height instead of a kernel boundary, as k_sap_levels does
constexpr int ST_PERSISTENT_THREADS = 256;
constexpr u64 ST_PERSISTENT_MAX = 4 * ST_PERSISTENT_THREADS;
static __device__ __forceinline__ void k_st_levels(const VB& vb, StBuild b) {
    for (int L = 0; L < ST_DEPTH; L++) {
        for (u64 i = threadIdx.x; i < b.n; i += ST_PERSISTENT_THREADS) st_level_step(b, L, i);
        __threadfence();
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ insert
// the tree's leaves [0, n_old) followed by the batch [0, m): entry s of the concatenation
struct StMerge {
    const u32* old_keys; const u64* old_index; const u32* old_values;
    const u32* new_keys; const u32* new_values;
    u64 n_old, m, next_index;
    __device__ __forceinline__ const u32* key(u32 s) const { return s < n_old ? old_keys + 8 * (u64)s : new_keys + 8 * ((u64)s - n_old); }
    __device__ __forceinline__ const u32* value(u32 s) const { return s < n_old ? old_values + 8 * (u64)s : new_values + 8 * ((u64)s - n_old); }
};

static __device__ __forceinline__ void k_st_iota(const VB& vb, u32* __restrict__ perm, u64 n) {
    const u64 i = (u64)vb.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = (u32)i;
}
// 64-bit digit `w` (0 = least significant) of the keys in the order `perm`
static __device__ __forceinline__ void k_st_gather_word(const VB& vb, StMerge g, const u32* __restrict__ perm, int w, u64 n, u64* __restrict__ out) {
    const u64 i = (u64)vb.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32* k = g.key(perm[i]);
    out[i] = (u64)k[2 * w] | ((u64)k[2 * w + 1] << 32);
}
// is sorted position r the first of its run of equal keys: the flag of flag_prefix (scan_kernels.cuh)
struct StHeadFlag {
    StMerge g;
    const u32* perm;
    __device__ __forceinline__ u32 operator()(size_t r) const { return r == 0 || st_cmp(g.key(perm[r]), g.key(perm[r - 1])) != 0; }
};
struct StArrayFlag {
    const u32* a;
    __device__ __forceinline__ u32 operator()(size_t i) const { return a[i]; }
};
// new_first[j] = batch entry j is the first occurrence of a key the tree does not hold (the sort is stable and the tree's leaves come
// first: a run with a tree leaf has that leaf at its head)
static __device__ __forceinline__ void k_st_mark(const VB& vb, StMerge g, const u32* __restrict__ perm, u64 n, u32* __restrict__ new_first) {
    const u64 r = (u64)vb.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const u32 s = perm[r];
    if (s >= g.n_old) new_first[s - g.n_old] = StHeadFlag{g, perm}(r);
}
// heads[r] = runs that start before sorted position r. The head of a run gives its key and enumeration index, its tail the value.
static __device__ __forceinline__ void k_st_emit(const VB& vb, StMerge g, const u32* __restrict__ perm, u64 n, const u32* __restrict__ heads,
                                                 const u32* __restrict__ new_rank, u32* __restrict__ out_keys, u64* __restrict__ out_index,
                                                 u32* __restrict__ out_values) {
    const u64 r = (u64)vb.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const u32 s = perm[r];
    const u32 run = heads[r + 1] - 1;  // the run position r belongs to = the leaf's rank in the new tree
    if (heads[r + 1] != heads[r]) {
        const u32* k = g.key(s);
#pragma unroll
        for (int w = 0; w < 8; w++) out_keys[8 * (u64)run + w] = k[w];
        out_index[run] = s < g.n_old ? g.old_index[s] : g.next_index + new_rank[s - g.n_old];
    }
    if (r + 1 == n || heads[r + 2] != heads[r + 1]) {
        const u32* v = g.value(s);
#pragma unroll
        for (int w = 0; w < 8; w++) out_values[8 * (u64)run + w] = v[w];
    }
}

// the writes of a block's deduplicated queue as (key, value) pairs, in queue order (storage_application.rs:221-283): write_rank[i] =
// writes before query i
struct StWriteFlag {
    const zkw_log_query* q;
    __device__ __forceinline__ u32 operator()(size_t i) const { return q[i].rw_flag != 0; }
};
static __device__ __forceinline__ void k_st_writes(const VB& vb, const zkw_log_query* __restrict__ q, u64 n, const u32* __restrict__ write_rank,
                                                   u32* __restrict__ out_keys, u32* __restrict__ out_values) {
    const u64 i = (u64)vb.x * blockDim.x + threadIdx.x;
    if (i >= n || !q[i].rw_flag) return;
    const u64 o = write_rank[i];
    u32 k[8];
    sap_derive_key(q + i, k);
#pragma unroll
    for (int w = 0; w < 8; w++) {
        out_keys[8 * o + w] = k[w];
        out_values[8 * o + w] = bswap32(q[i].written_value[7 - w]);  // the U256's big-endian bytes
    }
}

}  // namespace zkw
