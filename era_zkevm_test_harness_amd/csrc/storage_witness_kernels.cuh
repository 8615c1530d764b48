// storage_witness_kernels.cuh — a WITNESS tree: the answers get_leaf gives for a set of keys in ONE state of a storage tree, and nothing
// else (include/zkw.h, zkw_storage_tree_create_witness / _extract_witness). What the reference reads per slot through `get_leaf` and
// checks with `verify_inclusion_proxy` (storage_application.rs:217-266), as a table in HBM:
//   * the entries SORTED by key (the 256-bit order of storage_tree_kernels.cuh), next to (enumeration index, value, Merkle path):
//     keys [n][8], index [n], values [n][8], paths [n][256][8] — 8 264 bytes per entry, immutable once built;
//   * lookup (k_sw_lookup): a workgroup of 256 per query; thread 0 derives the key and finds it by lower bound, the 256 threads copy
//     the 8 KB path as contiguous 32-byte stores. A key outside the table gets the sentinel index and a zero path, and raises the
//     caller's flag word. It is a kernel BODY (zkw_launch.h): the K blocks' lookups of a stage leave as one launch, each job with
//     its own table;
//   * verification (k_sw_verify): an entry per lane — a fold is 256 dependent Blake2s compressions with nothing to share inside an
//     entry — over the entries in the CALLER's order: one status word per entry, the first bad position by atomicMin;
//   * the sort is the tree's (four 64-bit radix_sort_pairs passes over a permutation, k_st_gather_word in between); k_sw_gather then
//     moves every entry ONCE to its sorted place (8 KB per entry, a workgroup per entry) and marks a key that repeats.
// Blake2s, the leaf hash and derive_final_address are storage_application_kernels.cuh's; st_cmp and StQuery storage_tree_kernels.cuh's.
#pragma once
#include "storage_tree_kernels.cuh"

namespace zkw {

constexpr u64 SW_MISSING = ~0ull;  // leaf_indexes[i] of a query whose key the table does not hold
// status word of an entry (0 = a valid proof)
constexpr u32 SW_BAD_INDEX = 1;   // leaf_index >= next_enumeration_index
constexpr u32 SW_BAD_EMPTY = 2;   // index 0 (an absent key) with a nonzero value
constexpr u32 SW_BAD_ROOT = 4;    // the fold of the path does not reach the root
constexpr u32 SW_BAD_REPEAT = 8;  // the key of an earlier entry

// the table as a reading kernel sees it
struct SwView {
    const u32* keys;    // [n][8] sorted, distinct
    const u64* index;   // [n]
    const u32* values;  // [n][8]
    const u32* paths;   // [n][256][8]
    u64 n;
};

// grid = the queries, 256 threads. `missing` (or NULL): one zeroed word of the caller's; a query at position i whose key the table does
// not hold raises it to at least (number of queries - i), so afterwards 0 = every key was found, else the FIRST such position is
// (number of queries - *missing).
static __device__ __forceinline__ void k_sw_lookup(const VB& vb, SwView t, StQuery q, u32* __restrict__ missing) {
    __shared__ u64 s_j;
    const u64 i = vb.x;
    const int L = threadIdx.x;
    if (L == 0) {
        u32 key[8];
        if (q.queries) {
            sap_derive_key(q.queries + i, key);
        } else {
#pragma unroll
            for (int w = 0; w < 8; w++) key[w] = q.keys[8 * i + w];
        }
        u64 lo = 0, hi = t.n;
        while (lo < hi) {
            const u64 mid = (lo + hi) >> 1;
            if (st_cmp(t.keys + 8 * mid, key) < 0) lo = mid + 1; else hi = mid;
        }
        const bool hit = lo < t.n && st_cmp(t.keys + 8 * lo, key) == 0;
        s_j = hit ? lo : SW_MISSING;
        if (q.leaf_indexes) q.leaf_indexes[i] = hit ? t.index[lo] : SW_MISSING;
        if (q.values)
            for (int w = 0; w < 8; w++) q.values[8 * i + w] = hit ? t.values[8 * lo + w] : 0;
        if (!hit && missing) atomicMax(missing, vb.nx - vb.x);
    }
    if (!q.paths) return;
    __syncthreads();
    const u64 j = s_j;
    uint4 a = make_uint4(0, 0, 0, 0), b = a;
    if (j != SW_MISSING) {
        const uint4* src = reinterpret_cast<const uint4*>(t.paths + (j * ST_DEPTH + L) * 8);
        a = src[0];
        b = src[1];
    }
    uint4* dst = reinterpret_cast<uint4*>(q.paths + (i * ST_DEPTH + L) * 8);
    dst[0] = a;
    dst[1] = b;
}

// the entries as the caller gave them
struct SwEntries {
    const u32* keys;    // [n][8]
    const u64* index;   // [n]
    const u32* values;  // [n][8]
    const u32* paths;   // [n][256][8]
    u64 n, next_index;
    u32 root[8];
};

// verify_inclusion_proxy (storage_application.rs:230,266) of entry s = the lane: the leaf hash of (index, value) folded up the 256
// siblings by the key's bits must be the root. status[s] = what is wrong with it; first_bad = the least s with a nonzero status.
static __device__ __forceinline__ void k_sw_verify(const VB& vb, const SwEntries& e, u32* __restrict__ status, u32* __restrict__ first_bad) {
    const u64 s = (u64)vb.x * blockDim.x + threadIdx.x;
    if (s >= e.n) return;
    const u64 index = e.index[s];
    u32 v[8], h[8], o[8];
    u32 any = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) { v[k] = e.values[8 * s + k]; any |= v[k]; }
    u32 bad = 0;
    if (index >= e.next_index) bad |= SW_BAD_INDEX;
    if (index == 0 && any) bad |= SW_BAD_EMPTY;
    sap_leaf_hash_bytes(index, v, h);
    const uint4* path = reinterpret_cast<const uint4*>(e.paths + s * ST_DEPTH * 8);
    for (int w = 0; w < 8; w++) {
        u32 bits = e.keys[8 * s + w];
        for (int b = 0; b < 32; b++, bits >>= 1) {
            const uint4 p0 = path[2 * (32 * w + b)], p1 = path[2 * (32 * w + b) + 1];
            const u32 sib[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
            const bool right = bits & 1;  // this node is the right child
            u32 l[8], r[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                l[k] = right ? sib[k] : h[k];
                r[k] = right ? h[k] : sib[k];
            }
            sap_node_hash(l, r, o);
#pragma unroll
            for (int k = 0; k < 8; k++) h[k] = o[k];
        }
    }
    u32 diff = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) diff |= h[k] ^ e.root[k];
    if (diff) bad |= SW_BAD_ROOT;
    status[s] = bad;
    if (bad) atomicMin(first_bad, (u32)s);
}

// the table's arrays, writable
struct SwTable {
    u32* keys;
    u64* index;
    u32* values;
    u32* paths;
};

// grid = the sorted positions, 256 threads: entry perm[r] to place r; thread L moves level L of the path. An entry whose key equals
// its predecessor's repeats it (the sort is stable: the predecessor came first in the caller's order too).
static __device__ __forceinline__ void k_sw_gather(const VB& vb, SwEntries e, const u32* __restrict__ perm, SwTable out, u32* __restrict__ status,
                                                   u32* __restrict__ first_bad) {
    const u64 r = vb.x;
    const int L = threadIdx.x;
    const u64 s = perm[r];
    const uint4* src = reinterpret_cast<const uint4*>(e.paths + (s * ST_DEPTH + L) * 8);
    uint4* dst = reinterpret_cast<uint4*>(out.paths + (r * ST_DEPTH + L) * 8);
    dst[0] = src[0];
    dst[1] = src[1];
    if (L < 8) {
        out.keys[8 * r + L] = e.keys[8 * s + L];
        out.values[8 * r + L] = e.values[8 * s + L];
    }
    if (L == 0) {
        out.index[r] = e.index[s];
        if (r && st_cmp(e.keys + 8 * s, e.keys + 8 * (u64)perm[r - 1]) == 0) {
            atomicOr(status + s, SW_BAD_REPEAT);
            atomicMin(first_bad, (u32)s);
        }
    }
}

// extract: the distinct keys of a sorted key set, in order (heads[r] = runs of equal keys that start before sorted position r)
static __device__ __forceinline__ void k_sw_unique_keys(const VB& vb, const u32* __restrict__ keys, const u32* __restrict__ perm, const u32* __restrict__ heads,
                                                        u64 n, u32* __restrict__ out_keys) {
    const u64 r = (u64)vb.x * blockDim.x + threadIdx.x;
    if (r >= n || heads[r + 1] == heads[r]) return;
    const u32* k = keys + 8 * (u64)perm[r];
    const u64 o = heads[r];
#pragma unroll
    for (int w = 0; w < 8; w++) out_keys[8 * o + w] = k[w];
}

// the entries with a nonzero enumeration index: the table's num_leaves
static __device__ __forceinline__ void k_sw_count(const VB& vb, const u64* __restrict__ index, u64 n, u32* __restrict__ count) {
    const u64 i = (u64)vb.x * blockDim.x + threadIdx.x;
    if (i < n && index[i] != 0) atomicAdd(count, 1u);
}

// ------------------------------------------------------------------------------------------------ advance
// zkw_storage_tree_advance_witness / _by_queries: a NEW table with the same keys in the state after a call's writes. A write changes its
// key's own path and the siblings that hang off it, and the written keys' old paths hold every sibling hash that does not change. So:
//   * locate (k_swa_locate): a thread per position p of the call — pair p, or query p when it writes: the key's entry by lower bound;
//     first[entry] / last[entry] = the least / greatest writing position (atomicMin / atomicMax); a key outside the table raises the
//     `missing` word as k_sw_lookup does. Two flag_prefix passes follow: over the positions (p is the first write of an entry with
//     index 0: its rank among the NEW leaves, in array order) and over the entries (written: the rank w in the written set W, which
//     is sorted by key because the table is);
//   * k_swa_compact, k_swa_leaves: wlist[w] = the entry, its new (index, value), the new leaf hash and d[w] = the highest bit where
//     written key w differs from written key w - 1;
//   * fold (k_swa_fold for |W| <= ST_PERSISTENT_MAX, else k_swa_level per height): the build of storage_tree_kernels.cuh over W alone.
//     The written keys under one node of height L are a contiguous range of W; the node's hash is kept at the range's first key:
//     up[L][a], level-major [257][bound][8]. Height L + 1 of range start a = H(up[L][a], s) ordered by the sides, where s =
//     up[L][m] when the next range m = nxt[a] lies under the same parent (d[m] == L), else the sibling subtree holds no written key
//     and s = the OLD path[L] of a's entry. up[256][0] = the new root;
//   * paths (k_swa_paths): a workgroup per entry of the table, thread L: the sibling subtree at level L is a prefix; the first
//     written key not below it starts that node's range if it shares the prefix, and the new path[L] = up[L][that], else the old one.
//     The same pass copies the key and writes the new index and value: the table is copied once.
// Nothing is read back before the end: grids are sized by bound = min(positions, entries) >= |W|, the kernels read |W| from meta.
constexpr u32 SWA_NONE = ~0u;        // first[e] of an entry no position writes
constexpr int SWA_META_MISSING = 0;  // k_sw_lookup's convention: 0, or (positions - the first position whose key the table lacks)
constexpr int SWA_META_NW = 1;       // |W|
constexpr int SWA_META_NEW = 2;      // entries that become present
constexpr int SWA_META_ROOT = 4;     // [8]: up[256][0]
constexpr int SWA_META_WORDS = 16;   // `last` follows in the same zeroed buffer

// the call's writes: the queries with rw_flag set, or (queries == NULL) n pairs
struct SwaWrites {
    const zkw_log_query* queries;
    const u32* keys;    // [n][8]
    const u32* values;  // [n][8]
    u64 n;
    __device__ __forceinline__ bool writes(u64 p) const { return !queries || queries[p].rw_flag != 0; }
    __device__ __forceinline__ u32 value_word(u64 p, int w) const { return queries ? bswap32(queries[p].written_value[7 - w]) : values[8 * p + w]; }
};

static __device__ __forceinline__ void k_swa_locate(const VB& vb, SwView t, SwaWrites wr, u32* __restrict__ ent, u32* __restrict__ first,
                                                    u32* __restrict__ last, u32* __restrict__ meta) {
    const u64 p = (u64)vb.x * blockDim.x + threadIdx.x;
    if (p >= wr.n) return;
    if (!wr.writes(p)) { ent[p] = SWA_NONE; return; }
    u32 key[8];
    if (wr.queries) {
        sap_derive_key(wr.queries + p, key);
    } else {
#pragma unroll
        for (int w = 0; w < 8; w++) key[w] = wr.keys[8 * p + w];
    }
    u64 lo = 0, hi = t.n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (st_cmp(t.keys + 8 * mid, key) < 0) lo = mid + 1; else hi = mid;
    }
    const bool hit = lo < t.n && st_cmp(t.keys + 8 * lo, key) == 0;
    ent[p] = hit ? (u32)lo : SWA_NONE;
    if (hit) {
        atomicMin(first + lo, (u32)p);
        atomicMax(last + lo, (u32)p);
    } else {
        atomicMax(meta + SWA_META_MISSING, (u32)(wr.n - p));
    }
}
// position p is the first write of an entry that is absent so far
struct SwaNewFlag {
    const u32 *ent, *first;
    const u64* index;
    __device__ __forceinline__ u32 operator()(size_t p) const {
        const u32 e = ent[p];
        return e != SWA_NONE && first[e] == (u32)p && index[e] == 0;
    }
};
struct SwaWrittenFlag {
    const u32* first;
    __device__ __forceinline__ u32 operator()(size_t e) const { return first[e] != SWA_NONE; }
};

// what the fold works on; `bound` = the pitch of up's levels
struct SwaFold {
    SwView t;
    const u32* wlist;  // [|W|]: the written entries, ascending
    u32* up;           // [257][bound][8]
    u32* d;            // [|W|]
    u32* nxt;          // [|W|]
    u32* meta;
    u64 bound;
};

// wrank[e] = written entries before e; new_rank[p] = new leaves before position p
static __device__ __forceinline__ void k_swa_compact(const VB& vb, const u32* __restrict__ first, const u32* __restrict__ wrank, const u32* __restrict__ new_rank,
                                                     u64 entries, u64 positions, u32* __restrict__ wlist, u32* __restrict__ meta) {
    const u64 e = (u64)vb.x * blockDim.x + threadIdx.x;
    if (e >= entries) return;
    if (first[e] != SWA_NONE) wlist[wrank[e]] = (u32)e;
    if (e == 0) {
        meta[SWA_META_NW] = wrank[entries];
        meta[SWA_META_NEW] = new_rank[positions];
    }
}

// written key w: its new index and value (widx, wval: what k_swa_paths writes into the table), the leaf hash, d and nxt
static __device__ __forceinline__ void k_swa_leaves(const VB& vb, SwaFold f, SwaWrites wr, const u32* __restrict__ first, const u32* __restrict__ last,
                                                    const u32* __restrict__ new_rank, u64 next_index, u64* __restrict__ widx, u32* __restrict__ wval) {
    const u64 w = (u64)vb.x * blockDim.x + threadIdx.x;
    if (w >= f.meta[SWA_META_NW]) return;
    const u64 e = f.wlist[w];
    const u64 old = f.t.index[e], index = old ? old : next_index + new_rank[first[e]];
    const u64 p = last[e];
    u32 v[8], h[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = wr.value_word(p, k);
    sap_leaf_hash_bytes(index, v, h);
    widx[w] = index;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        wval[8 * w + k] = v[k];
        f.up[8 * w + k] = h[k];
    }
    f.d[w] = w ? (u32)st_top_diff(f.t.keys + 8 * e, f.t.keys + 8 * (u64)f.wlist[w - 1]) : (u32)ST_DEPTH;
    f.nxt[w] = (u32)(w + 1);
}

// the node of height L + 1 over `mine` (height L, the range that starts at written entry e): its sibling is `other`, the next range's
// node (then `mine` is the left child: W is sorted), or NULL: the entry's old path[L], on the side the key's bit L says
__device__ __forceinline__ void swa_parent(const SwView& t, int L, u64 e, const u32* mine, const u32* other, u32 o[8]) {
    bool right = false;
    uint4 s0, s1;
    if (other) {
        s0 = make_uint4(other[0], other[1], other[2], other[3]);
        s1 = make_uint4(other[4], other[5], other[6], other[7]);
    } else {
        const uint4* sib = reinterpret_cast<const uint4*>(t.paths + (e * ST_DEPTH + L) * 8);
        s0 = sib[0];
        s1 = sib[1];
        right = (t.keys[8 * e + (L >> 5)] >> (L & 31)) & 1;
    }
    const u32 c[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    u32 l[8], r[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const u32 a = mine[k];
        l[k] = right ? c[k] : a;
        r[k] = right ? a : c[k];
    }
    sap_node_hash(l, r, o);
}

// one height per launch: grid = the written keys, 64 threads
static __device__ __forceinline__ void k_swa_level(const VB& vb, SwaFold f, int L) {
    const u64 i = (u64)vb.x * blockDim.x + threadIdx.x;
    const u32 nw = f.meta[SWA_META_NW];
    if (i >= nw || f.d[i] <= (u32)L) return;  // not the first written key of a node of height L + 1
    const u32 m = f.nxt[i];
    const bool has_sibling = m < nw && f.d[m] == (u32)L;
    u32 o[8];
    swa_parent(f.t, L, f.wlist[i], f.up + ((u64)L * f.bound + i) * 8, has_sibling ? f.up + ((u64)L * f.bound + m) * 8 : nullptr, o);
    u32* out = f.up + ((u64)(L + 1) * f.bound + i) * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = o[k];
    if (L + 1 == ST_DEPTH)
        for (int k = 0; k < 8; k++) f.meta[SWA_META_ROOT + k] = o[k];
    if (has_sibling) f.nxt[i] = f.nxt[m];  // (m starts no node of height L + 1: nobody writes nxt[m] at this height)
}

// all heights in one launch, one workgroup, |W| <= ST_PERSISTENT_MAX: the current height's hashes, d, nxt and wlist live in LDS, so
// the barrier per height needs no device-scope fence (k_st_levels pays one per height: its hashes travel through global memory);
// up[] is only written here, for k_swa_paths. A slot is read by its own thread and by the one range start to its left, which
// then computes while the slot's owner does not: in place, one barrier per height.
static __device__ __forceinline__ void k_swa_fold(const VB& vb, SwaFold f) {
    __shared__ u32 s_h[ST_PERSISTENT_MAX][8];
    __shared__ u32 s_d[ST_PERSISTENT_MAX], s_nxt[ST_PERSISTENT_MAX], s_e[ST_PERSISTENT_MAX];
    const u32 nw = f.meta[SWA_META_NW];
    if (nw > ST_PERSISTENT_MAX) return;  // (the driver sizes by bound >= |W|)
    for (u32 i = threadIdx.x; i < nw; i += ST_PERSISTENT_THREADS) {
#pragma unroll
        for (int k = 0; k < 8; k++) s_h[i][k] = f.up[8 * (u64)i + k];
        s_d[i] = f.d[i];
        s_nxt[i] = i + 1;
        s_e[i] = f.wlist[i];
    }
    __syncthreads();
    for (int L = 0; L < ST_DEPTH; L++) {
        for (u32 i = threadIdx.x; i < nw; i += ST_PERSISTENT_THREADS) {
            if (s_d[i] <= (u32)L) continue;
            const u32 m = s_nxt[i];
            const bool has_sibling = m < nw && s_d[m] == (u32)L;
            u32 o[8];
            swa_parent(f.t, L, s_e[i], s_h[i], has_sibling ? s_h[m] : nullptr, o);
            u32* out = f.up + ((u64)(L + 1) * f.bound + i) * 8;
#pragma unroll
            for (int k = 0; k < 8; k++) { s_h[i][k] = o[k]; out[k] = o[k]; }
            if (L + 1 == ST_DEPTH)
                for (int k = 0; k < 8; k++) f.meta[SWA_META_ROOT + k] = o[k];
            if (has_sibling) s_nxt[i] = s_nxt[m];
        }
        __syncthreads();
    }
}

// grid = the entries, 256 threads: thread L writes level L of entry e's new path
static __device__ __forceinline__ void k_swa_paths(const VB& vb, SwaFold f, const u32* __restrict__ first, const u32* __restrict__ wrank,
                                                   const u64* __restrict__ widx, const u32* __restrict__ wval, SwTable out) {
    const u64 e = vb.x;
    const int L = threadIdx.x;
    const u32 nw = f.meta[SWA_META_NW];
    u32 key[8];
#pragma unroll
    for (int w = 0; w < 8; w++) key[w] = f.t.keys[8 * e + w];
    if (L < 8) {
        const bool written = first[e] != SWA_NONE;
        out.keys[8 * e + L] = f.t.keys[8 * e + L];
        out.values[8 * e + L] = written ? wval[8 * (u64)wrank[e] + L] : f.t.values[8 * e + L];
        if (L == 0) out.index[e] = written ? widx[wrank[e]] : f.t.index[e];
    }
    // the sibling subtree at level L: the key with bit L flipped and the bits below cleared (k_st_query)
    const int wl = L >> 5;
#pragma unroll
    for (int w = 0; w < 8; w++)
        if (w < wl) key[w] = 0;
        else if (w == wl) key[w] = (key[w] ^ (1u << (L & 31))) & ~((1u << (L & 31)) - 1u);
    u32 lo = 0, hi = nw;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (st_cmp(f.t.keys + 8 * (u64)f.wlist[mid], key) < 0) lo = mid + 1; else hi = mid;
    }
    const bool hit = lo < nw && st_top_diff(f.t.keys + 8 * (u64)f.wlist[lo], key) < L;  // a written key under the sibling: lo starts its range
    const uint4* src = reinterpret_cast<const uint4*>(hit ? f.up + ((u64)L * f.bound + lo) * 8 : f.t.paths + (e * ST_DEPTH + L) * 8);
    uint4* dst = reinterpret_cast<uint4*>(out.paths + (e * ST_DEPTH + L) * 8);
    dst[0] = src[0];
    dst[1] = src[1];
}

// ------------------------------------------------------------------------------------------------ chain
// zkw_storage_tree_advance_witness_chain: the pre-states of K consecutive blocks out of ONE table over (at least) the union of their
// slots, in one call. out[k] is a table of block k's OWN keys in the state after blocks 0 .. k - 1; one working copy of the union is
// advanced in place and becomes the final state. The key set is fixed, so an entry never moves: E = the table's entries, N = the
// queries of all blocks, flat index (k, e) = k E + e.
//   * locate (k_swc_locate): a thread per position p of all blocks (a query, or a pair of the pair form: always a write): its block by binary search over the offsets, its entry by lower
//     bound; READS are located too (the block will look them up). touched[k E + e] = 1; a write leaves first / last[k E + e]
//     (atomicMin / atomicMax of the global position) and cfirst[e] = the first writing position of the whole chain; a miss raises
//     meta[0] to at least N - p, so the first bad (block, position) falls out;
//   * ranks: flag_prefix over the K E touched flags (trank: where (k, e) goes in out[k], already sorted because the union is), over
//     the K E written flags (wrank: the written lists W_k back to back, `bound` = min(N, K E) slots) and over the positions (new_rank:
//     the first write of the chain to an entry whose index is 0). k_swc_compact leaves wlist / wblk and the per-block bases tbase,
//     wbase [K + 1] next to the miss word: the FIRST readback, which sizes the K tables;
//   * walk (k_swc_walk): a thread per entry walks k = 0 .. K - 1 with its current (index, value): writes them with the key into
//     out[k] where block k touches the entry, then applies block k's last write and leaves the new leaf hash, d and nxt at its slot
//     of W_k. Counts the new leaves per block and the present entries per table; its last state goes into the working table;
//   * the wavefront (k_swc_step, one launch per step s = 0 .. 256 + K - 2): block k is at height L = s - k.
//       fold: a range start of W_k at height L makes its parent (swa_parent) from its hash and the next range's when that lies under
//       the same parent, else the WORKING table's path[L] of its entry. Two heights per block (ping-pong on L & 1); height 256 is
//       block k's root.
//       update and capture: thread (k, e) reads the working cell path[e][L]; if block k touches e the old cell is out[k]'s path[L];
//       if a key of W_k lies under e's sibling subtree at L (k_swa_paths' lower bound over W_k) that node's hash replaces the cell.
//     The fold reads a cell only where no written key of block k lies under the sibling — where the update does not write. The
//     other blocks of the step are at other levels, and blocks < k were at level L in earlier steps: a step is race-free in place.
// Scratch, in 32-bit words: 5 K E + 2 (touched, first, last, trank, wrank) + E (cfirst) + 2 N + 1 (ent, new_rank) + 20 bound (wlist,
// wblk, d, nxt, two heights of 8 words) + 2 K + 18 (the first readback) + 10 K + 1 (the second: roots, new leaves, present entries)
// + 9 K + 1 (the offsets and the K tables' pointers) = 5 K E + E + 2 N + 20 bound + 21 K + 23.
constexpr int SWC_HDR_MISSING = 0;  // k_sw_lookup's convention over the N positions of the chain
constexpr int SWC_HDR_WORDS = 16;   // tbase [K + 1] and wbase [K + 1] follow

// all blocks' queries (or pairs: each one a write) back to back; offs [K + 1] in device memory
struct SwcQueries {
    SwaWrites wr;
    const u32* offs;
    u32 blocks;
};

static __device__ __forceinline__ void k_swc_locate(const VB& vb, SwView t, SwcQueries cq, u32* __restrict__ ent, u32* __restrict__ touched,
                                                    u32* __restrict__ first, u32* __restrict__ last, u32* __restrict__ cfirst, u32* __restrict__ hdr) {
    const u64 p = (u64)vb.x * blockDim.x + threadIdx.x;
    if (p >= cq.wr.n) return;
    u32 k = 0, kh = cq.blocks;  // the last block that starts at or before p (an empty block starts where the next one does)
    while (kh - k > 1) {
        const u32 mid = (k + kh) >> 1;
        if (cq.offs[mid] <= p) k = mid; else kh = mid;
    }
    u32 key[8];
    if (cq.wr.queries) {
        sap_derive_key(cq.wr.queries + p, key);
    } else {
#pragma unroll
        for (int w = 0; w < 8; w++) key[w] = cq.wr.keys[8 * p + w];
    }
    u64 lo = 0, hi = t.n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (st_cmp(t.keys + 8 * mid, key) < 0) lo = mid + 1; else hi = mid;
    }
    const bool hit = lo < t.n && st_cmp(t.keys + 8 * lo, key) == 0;
    ent[p] = hit ? (u32)lo : SWA_NONE;
    if (!hit) {
        atomicMax(hdr + SWC_HDR_MISSING, (u32)(cq.wr.n - p));
        return;
    }
    const u64 i = (u64)k * t.n + lo;
    touched[i] = 1;
    if (cq.wr.writes(p)) {
        atomicMin(first + i, (u32)p);
        atomicMax(last + i, (u32)p);
        atomicMin(cfirst + lo, (u32)p);
    }
}
struct SwcTouchedFlag {
    const u32* touched;
    __device__ __forceinline__ u32 operator()(size_t i) const { return touched[i] != 0; }
};
// position p is the first write of the chain to an entry that is absent before block 0
struct SwcNewFlag {
    const u32 *ent, *cfirst;
    const u64* index;
    __device__ __forceinline__ u32 operator()(size_t p) const {
        const u32 e = ent[p];
        return e != SWA_NONE && cfirst[e] == (u32)p && index[e] == 0;
    }
};

// what the walk and the wavefront work on
struct SwcChain {
    const u32* keys;      // [E][8]: the union's keys
    SwTable work;         // the working copy of the union: the state after the blocks that have passed a level
    const SwTable* outs;  // [K]
    const u32 *touched, *first, *trank, *wrank;  // [K E], the ranks [K E + 1]
    const u32 *tbase, *wbase;                    // [K + 1]
    u32 *wlist, *wblk, *d, *nxt;                 // [bound]: W_0, W_1, ... back to back
    u32* h;                                      // [2][bound][8]: height L of a block at h[L & 1]
    u32* fin;                                    // [8 K] roots, [K] new leaves, [K + 1] present entries (the last: the final table's)
    u64 entries, bound;
    u32 blocks;
};

static __device__ __forceinline__ void k_swc_compact(const VB& vb, SwcChain c, u32* __restrict__ tbase, u32* __restrict__ wbase) {
    const u64 i = (u64)vb.x * blockDim.x + threadIdx.x;
    if (i <= c.blocks) {
        tbase[i] = c.trank[i * c.entries];
        wbase[i] = c.wrank[i * c.entries];
    }
    if (i >= (u64)c.blocks * c.entries || c.first[i] == SWA_NONE) return;
    const u32 w = c.wrank[i];
    c.wlist[w] = (u32)(i % c.entries);
    c.wblk[w] = (u32)(i / c.entries);
}

static __device__ __forceinline__ void k_swc_walk(const VB& vb, const SwcChain& c, SwaWrites wr, const u64* __restrict__ index0,
                                                  const u32* __restrict__ values0, const u32* __restrict__ last, const u32* __restrict__ cfirst,
                                                  const u32* __restrict__ new_rank, u64 next_index) {
    const u64 e = (u64)vb.x * blockDim.x + threadIdx.x;
    if (e >= c.entries) return;
    u64 index = index0[e];
    u32 key[8], v[8], h[8];
#pragma unroll
    for (int w = 0; w < 8; w++) { key[w] = c.keys[8 * e + w]; v[w] = values0[8 * e + w]; }
    for (u32 k = 0; k < c.blocks; k++) {
        const u64 i = (u64)k * c.entries + e;
        if (!c.touched[i]) continue;
        const SwTable o = c.outs[k];
        const u64 j = c.trank[i] - c.tbase[k];
        o.index[j] = index;
#pragma unroll
        for (int w = 0; w < 8; w++) { o.keys[8 * j + w] = key[w]; o.values[8 * j + w] = v[w]; }
        if (index) atomicAdd(c.fin + 9 * (u64)c.blocks + k, 1u);
        if (c.first[i] == SWA_NONE) continue;
        if (index == 0) {
            index = next_index + new_rank[cfirst[e]];
            atomicAdd(c.fin + 8 * (u64)c.blocks + k, 1u);
        }
        const u64 p = last[i];
#pragma unroll
        for (int w = 0; w < 8; w++) v[w] = wr.value_word(p, w);
        sap_leaf_hash_bytes(index, v, h);
        const u32 w = c.wrank[i];
#pragma unroll
        for (int q = 0; q < 8; q++) c.h[8 * (u64)w + q] = h[q];
        c.d[w] = w > c.wbase[k] ? (u32)st_top_diff(c.keys + 8 * e, c.keys + 8 * (u64)c.wlist[w - 1]) : (u32)ST_DEPTH;
        c.nxt[w] = w + 1;
    }
    c.work.index[e] = index;
#pragma unroll
    for (int w = 0; w < 8; w++) c.work.values[8 * e + w] = v[w];
    if (index) atomicAdd(c.fin + 10 * (u64)c.blocks, 1u);
}

// one step of the wavefront: the first `fold_wgs` workgroups fold (a thread per slot of the written lists), the others update and
// capture (a thread per (entry, block), the blocks of an entry side by side: their cells at levels s - k are neighbours in memory)
static __device__ __forceinline__ void k_swc_step(const VB& vb, const SwcChain& c, u32 fold_wgs, int s) {
    if (vb.x < fold_wgs) {
        const u64 i = (u64)vb.x * blockDim.x + threadIdx.x;
        if (i >= c.wbase[c.blocks]) return;
        const u32 k = c.wblk[i];
        const int L = s - (int)k;
        if (L < 0 || L >= ST_DEPTH || c.d[i] <= (u32)L) return;  // not the first written key of a node of height L + 1
        const u32 m = c.nxt[i];
        const bool has_sibling = m < c.wbase[k + 1] && c.d[m] == (u32)L;
        const u32* cur = c.h + (u64)(L & 1) * c.bound * 8;
        u32 o[8];
        swa_parent(SwView{c.keys, nullptr, nullptr, c.work.paths, c.entries}, L, c.wlist[i], cur + 8 * i, has_sibling ? cur + 8 * (u64)m : nullptr, o);
        u32* out = c.h + ((u64)((L + 1) & 1) * c.bound + i) * 8;
#pragma unroll
        for (int q = 0; q < 8; q++) out[q] = o[q];
        if (L + 1 == ST_DEPTH)
            for (int q = 0; q < 8; q++) c.fin[8 * (u64)k + q] = o[q];
        if (has_sibling) c.nxt[i] = c.nxt[m];  // (k_swa_level: m starts no node of height L + 1)
        return;
    }
    const u64 u = (u64)(vb.x - fold_wgs) * blockDim.x + threadIdx.x;
    if (u >= c.entries * c.blocks) return;
    const u64 e = u / c.blocks;
    const u32 k = (u32)(u % c.blocks);
    const int L = s - (int)k;
    if (L < 0 || L >= ST_DEPTH) return;
    const u64 i = (u64)k * c.entries + e;
    const bool touched = c.touched[i] != 0;
    const u32 w0 = c.wbase[k], w1 = c.wbase[k + 1];
    if (!touched && w0 == w1) return;
    uint4* cell = reinterpret_cast<uint4*>(c.work.paths + (e * ST_DEPTH + L) * 8);
    if (touched) {
        uint4* dst = reinterpret_cast<uint4*>(c.outs[k].paths + ((u64)(c.trank[i] - c.tbase[k]) * ST_DEPTH + L) * 8);
        dst[0] = cell[0];
        dst[1] = cell[1];
    }
    if (w0 == w1) return;
    // the sibling subtree at level L: the key with bit L flipped and the bits below cleared (k_swa_paths)
    u32 key[8];
    const int wl = L >> 5;
#pragma unroll
    for (int w = 0; w < 8; w++) {
        const u32 x = c.keys[8 * e + w];
        key[w] = w < wl ? 0u : w == wl ? (x ^ (1u << (L & 31))) & ~((1u << (L & 31)) - 1u) : x;
    }
    u32 lo = w0, hi = w1;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (st_cmp(c.keys + 8 * (u64)c.wlist[mid], key) < 0) lo = mid + 1; else hi = mid;
    }
    if (lo < w1 && st_top_diff(c.keys + 8 * (u64)c.wlist[lo], key) < L) {  // a written key of block k under the sibling: lo starts its range
        const uint4* src = reinterpret_cast<const uint4*>(c.h + ((u64)(L & 1) * c.bound + lo) * 8);
        cell[0] = src[0];
        cell[1] = src[1];
    }
}

}  // namespace zkw
