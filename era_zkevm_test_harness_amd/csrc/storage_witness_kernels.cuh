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

}  // namespace zkw
