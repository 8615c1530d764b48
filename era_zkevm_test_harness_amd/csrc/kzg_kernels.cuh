// kzg_kernels.cuh — the EIP-4844 blob witness (generate_eip4844_witness, src/utils.rs:119-231 of the reference; kzg/src/lib.rs) on gfx950:
// KZG commitment over a fixed-base table, the blob's Keccak-256, and the opening p(z) with the three short hashes around it.
//
// The setup is the monomial one, S[k] = [tau^k] G1. zkw_kzg_settings_create keeps T[w][k] = 2^(8 w) S[k] (w < 32, affine, 96 bytes an
// entry: 12.6 MB for 4 096 points), so byte w of coefficient k, when it is d != 0, sends T[w][k] into bucket d and
//     commitment = sum_d d * B_d,   B_d = sum of the table entries sent to d
// with ONE set of 255 buckets per polynomial: no per-window passes, no doublings, no window Horner (the reference's compute_commitment
// runs 4 096 double-and-add multiplications one after another, kzg/src/lib.rs:193-215). sum_d d B_d = sum_j 2^j (sum over d with bit j
// set of B_d): eight sums side by side and seven doublings instead of a 255-step running sum on one lane.
//   k_kzg_decompress   a lane per setup point: decompression, the curve and subgroup checks, T[0][k]
//   k_kzg_table        a lane per (w >= 1, k): 8 w doublings of S[k] and one Fermat inversion (runs once per settings handle)
//   k_kzg_check        a lane per coefficient: below r? (zkw_kzg_commit only; a blob's elements are below 2^248)
//   k_kzg_accumulate   a wave per (bucket, polynomial): each lane walks a strided share of the scalar bytes, adds the entries of its
//                      digit (mixed additions), the 64 partial sums fold through LDS
//   k_kzg_finish       two workgroups per polynomial, a wave per bit j: two buckets per lane, a fold through LDS
//   k_kzg_compress     a lane per polynomial: the seven doublings, to affine, the 48 compressed bytes
//   k_kzg_linear_hash  a wave per blob: the serial 934-block Keccak-256 sponge, a lane of the state per lane of the wave
//   k_kzg_tail         a workgroup per blob: versioned hash (SHA-256), z, the opening y = p(z) in Fr (lane t: Horner over its 16
//                      elements, weighted by (z^16)^(255 - t), summed through LDS), the output hash
// Every kernel is a body for both launch forms (zkw_launch.h).
#pragma once
#include "bls12_381.cuh"
#include "decommitter_kernels.cuh"  // sha256_compress, keccak_f1600 and the 25-lane round of k_linear_keccak256

namespace zkw {

enum : u32 { KZG_WINDOWS = 32, KZG_MAX_POINTS = 4096, KZG_BLOB_ELEMENTS = 4096, KZG_BLOB_BYTES = 4096 * 31, KZG_BUCKETS = 256 };
// zkw_eip4844_record (include/zkw.h), by byte offset
enum : u32 { KZG_REC_LINEAR = 0, KZG_REC_VERSIONED = 32, KZG_REC_OUTPUT = 64, KZG_REC_Z = 96, KZG_REC_Y = 112, KZG_REC_COMMITMENT = 144, KZG_REC_BYTES = 192 };
// a WAVE per bucket: with 256 lanes a lane found ~2 entries and the fold of the 256 partial sums (eight levels of Jacobian additions, 16
// products each, against 11 for a mixed addition) was most of the work at many blobs per call (profiles/r14)
enum : int { KZG_ACC_THREADS = 64, KZG_FIN_THREADS = 256, KZG_TAIL_THREADS = 256 };

// where a polynomial's scalar bytes are: coefficients of 32 little-endian bytes (zkw_kzg_commit), or a blob whose element i (31 bytes) is
// the coefficient of X^(4095 - i)
struct KzgSrc {
    const uint8_t* base;
    u32 n_coeffs, blob;
};

static __device__ __forceinline__ void k_kzg_decompress(const VB& vb, const uint8_t* __restrict__ in, u32 n, bls::G1Aff* __restrict__ table,
                                                        u32* __restrict__ status) {
    const u32 k = vb.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    bls::G1Aff p;
    int st = bls::decompress(in + 48 * (size_t)k, &p);
    if (st == bls::G1_OK && !bls::is_inf(p) && !bls::in_subgroup(p)) st = bls::G1_NOT_IN_SUBGROUP;
    if (st != bls::G1_OK) p = bls::G1Aff{bls::zero<bls::FqT>(), bls::zero<bls::FqT>()};
    table[k] = p;
    status[k] = (u32)st;
}

static __device__ __forceinline__ void k_kzg_table(const VB& vb, bls::G1Aff* __restrict__ table, u32 n) {
    const u32 k = vb.x * blockDim.x + threadIdx.x, w = vb.y + 1;
    if (k >= n || w >= KZG_WINDOWS) return;
    bls::G1Jac p = bls::to_jac(table[k]);
#pragma unroll 1
    for (u32 i = 0; i < 8 * w; i++) p = bls::jdbl(p);
    table[(size_t)w * n + k] = bls::to_affine(p);
}

// flag: the position of the first coefficient that is not below r (atomicMin; ~0 = none)
static __device__ __forceinline__ void k_kzg_check(const VB& vb, const uint8_t* __restrict__ coeffs, u32 total, u32* __restrict__ flag) {
    const u32 i = vb.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    u32 w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint8_t* b = coeffs + 32 * (size_t)i + 4 * j;
        w[j] = (u32)b[0] | ((u32)b[1] << 8) | ((u32)b[2] << 16) | ((u32)b[3] << 24);
    }
    if (!bls::below_modulus<bls::FrT>(w)) atomicMin(flag, i);
}

// the sum of the G partial sums of each group of G consecutive lanes (BS / G groups), in the group's first lane. lds: BS / 2 points
template <int G> static __device__ __forceinline__ bls::G1Jac kzg_group_sum(bls::G1Jac acc, bls::G1Jac* lds) {
    const int l = threadIdx.x % G;
    bls::G1Jac* mine = lds + (threadIdx.x / G) * (G / 2);
#pragma unroll 1
    for (int s = G / 2; s >= 1; s >>= 1) {
        if (l >= s && l < 2 * s) mine[l - s] = acc;
        __syncthreads();
        if (l < s) acc = bls::jadd(acc, mine[l]);
        __syncthreads();
    }
    return acc;
}

// grid (255, n_polys), a wave each. buckets: [n_polys][256] (entry 0 unused)
static __device__ __forceinline__ void k_kzg_accumulate(const VB& vb, KzgSrc src, u32 poly_stride, const bls::G1Aff* __restrict__ table, u32 n_points,
                                                        bls::G1Jac* __restrict__ buckets) {
    __shared__ bls::G1Jac lds[KZG_ACC_THREADS / 2];
    const u32 d = vb.x + 1, width = src.blob ? 31u : 32u, n_bytes = src.n_coeffs * width;
    const uint8_t* bytes = src.base + (size_t)vb.y * poly_stride;
    bls::G1Jac acc = bls::jac_inf();
    u32 q = threadIdx.x;
#pragma unroll 1
    for (;;) {
        while (q < n_bytes && bytes[q] != d) q += KZG_ACC_THREADS;  // (cheap and divergent; the additions below run once per found entry)
        if (q >= n_bytes) break;
        const u32 i = src.blob ? q / 31u : q >> 5, w = src.blob ? q % 31u : q & 31u;
        const u32 k = src.blob ? src.n_coeffs - 1 - i : i;  // k < n_coeffs <= n_points, w < 32
        acc = bls::jmadd(acc, table[(size_t)w * n_points + k]);
        q += KZG_ACC_THREADS;
    }
    acc = kzg_group_sum<KZG_ACC_THREADS>(acc, lds);
    if (threadIdx.x == 0) buckets[(size_t)vb.y * KZG_BUCKETS + d] = acc;
}

// grid (n_polys, 2): four bits a workgroup (four waves: a wave alone on its SIMD, as in k_kzg_accumulate; a Jacobian addition holds
// ~240 registers). sums: [n_polys][8], sums[j] = the sum of the buckets whose digit has bit j set
static __device__ __forceinline__ void k_kzg_finish(const VB& vb, const bls::G1Jac* __restrict__ buckets, bls::G1Jac* __restrict__ sums) {
    __shared__ bls::G1Jac lds[KZG_FIN_THREADS / 2];
    const u32 j = 4 * vb.y + (threadIdx.x >> 6), l = threadIdx.x & 63;  // a wave sums the 128 buckets whose digit has bit j set
    const bls::G1Jac* b = buckets + (size_t)vb.x * KZG_BUCKETS;
    const u32 low = (1u << j) - 1, m1 = l + 64;  // the m-th digit with bit j set (m < 128): m with a 1 inserted at bit j
    const u32 d0 = ((l >> j) << (j + 1)) | (1u << j) | (l & low), d1 = ((m1 >> j) << (j + 1)) | (1u << j) | (m1 & low);
    bls::G1Jac acc = b[d0];
    {
        const bls::G1Jac other = b[d1];
        acc = bls::jadd(acc, other);
    }
    acc = kzg_group_sum<64>(acc, lds);
    if (l == 0) sums[(size_t)vb.x * 8 + j] = acc;
}

// a lane per polynomial: sum_j 2^j sums[j] by seven doublings, to affine (one Fermat inversion), the 48 compressed bytes at
// out + poly * out_stride. The chain is serial, so the polynomials of a call share a wave: 64 of them cost what one costs
static __device__ __forceinline__ void k_kzg_compress(const VB& vb, const bls::G1Jac* __restrict__ sums, u32 n_polys, uint8_t* __restrict__ out, u32 out_stride) {
    const u32 poly = vb.x * blockDim.x + threadIdx.x;
    if (poly >= n_polys) return;
    const bls::G1Jac* s = sums + (size_t)poly * 8;
    bls::G1Jac acc = s[7];
#pragma unroll 1
    for (int bit = 6; bit >= 0; bit--) acc = bls::jadd(bls::jdbl(acc), s[bit]);
    bls::compress(bls::to_affine(acc), out + (size_t)poly * out_stride);
}

// grid n_blobs, 64 lanes: Keccak-256 of the blob's 126 976 bytes = 933 full blocks and one of 88 bytes + padding. Lane t = x + 5 y < 25
// holds lane (x, y) of the state (the round of k_linear_keccak256, decommitter_kernels.cuh); the next block's words are loaded ahead of
// this block's rounds
static __device__ __forceinline__ void k_kzg_linear_hash(const VB& vb, const uint8_t* __restrict__ blobs, uint8_t* __restrict__ out, u32 out_stride) {
    const int t = threadIdx.x;
    const uint8_t* blob = blobs + (size_t)vb.x * KZG_BLOB_BYTES;
    const int x = t % 5, y = t / 5;
    const int src_pi = (x + 3 * y) % 5 + 5 * x;
    const int rot_pi = t < 25 ? c_keccak_rot[src_pi] : 0;
    constexpr u32 LAST = KZG_BLOB_BYTES / 136;  // 933: the block that holds the last 88 bytes
    const bool aligned = (reinterpret_cast<uintptr_t>(blobs) & 7) == 0;  // one 8-byte load per word (a caller's device pointer may be odd)
    auto word_of = [&](u32 blk) -> u64 {  // (t < 17) word t of block blk
        u64 v = 0;
        const u32 off = blk * 136 + 8 * (u32)t;
        if (aligned) {  // (a blob is a multiple of 8 bytes: a word lies inside it or behind it)
            if (off < KZG_BLOB_BYTES) v = *reinterpret_cast<const u64*>(blob + off);
        } else {
#pragma unroll
            for (u32 i = 0; i < 8; i++)
                if (off + i < KZG_BLOB_BYTES) v |= (u64)blob[off + i] << (8 * i);
        }
        if (blk == LAST && off == KZG_BLOB_BYTES) v ^= 1;               // pad10*1: the first byte after the message
        if (blk == LAST && t == 16) v ^= 0x8000000000000000ull;       // and the block's last bit
        return v;
    };
    u64 a = 0, next = t < 17 ? word_of(0) : 0;
#pragma unroll 1
    for (u32 blk = 0; blk <= LAST; blk++) {
        a ^= next;
        if (t < 17 && blk < LAST) next = word_of(blk + 1);
#pragma unroll 1
        for (int round = 0; round < 24; round++) {
            const u64 c = a ^ __shfl(a, (t + 5) % 25) ^ __shfl(a, (t + 10) % 25) ^ __shfl(a, (t + 15) % 25) ^ __shfl(a, (t + 20) % 25);
            const u64 dd = __shfl(c, (x + 4) % 5) ^ rol64(__shfl(c, (x + 1) % 5), 1);
            const u64 ap = a ^ dd;
            const u64 bm = rol64(__shfl(ap, src_pi), rot_pi);
            const u64 b1 = __shfl(bm, (x + 1) % 5 + 5 * y), b2 = __shfl(bm, (x + 2) % 5 + 5 * y);
            a = bm ^ (~b1 & b2);
            if (t == 0) a ^= c_keccak_rc[round];
        }
    }
    const u64 w = __shfl(a, (t >> 3) & 3);
    if (t < 32) out[(size_t)vb.x * out_stride + t] = (uint8_t)(w >> (8 * (t & 7)));
}

static __device__ __forceinline__ u64 kzg_bswap64(u64 v) { return __builtin_bswap64(v); }
static __device__ __forceinline__ void kzg_put64(uint8_t* out, u64 v) {  // little-endian bytes
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = (uint8_t)(v >> (8 * i));
}
static __device__ __forceinline__ u64 kzg_get64(const uint8_t* in) {
    u64 v = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) v |= (u64)in[i] << (8 * i);
    return v;
}

// grid n_blobs. rec: the blob's record with linear_hash and commitment already written (k_kzg_linear_hash, k_kzg_compress)
static __device__ __forceinline__ void k_kzg_tail(const VB& vb, const uint8_t* __restrict__ blobs, uint8_t* __restrict__ recs) {
    __shared__ bls::Fr lds_sum[KZG_TAIL_THREADS / 2];
    __shared__ u64 lds_z[2], lds_versioned[4];
    const int t = threadIdx.x;
    const uint8_t* blob = blobs + (size_t)vb.x * KZG_BLOB_BYTES;
    uint8_t* rec = recs + (size_t)vb.x * KZG_REC_BYTES;
    if (t == 0) {
        // versioned hash: SHA-256 of the 48 commitment bytes (one block), byte 0 replaced by 0x01
        u32 st[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u}, w[16];
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const uint8_t* b = rec + KZG_REC_COMMITMENT + 4 * i;
            w[i] = ((u32)b[0] << 24) | ((u32)b[1] << 16) | ((u32)b[2] << 8) | (u32)b[3];
        }
        w[12] = 0x80000000u; w[13] = 0; w[14] = 0; w[15] = 48 * 8;
        sha256_compress(st, w);
        u64 v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = (u64)__builtin_bswap32(st[2 * i]) | ((u64)__builtin_bswap32(st[2 * i + 1]) << 32);
        v[0] = (v[0] & ~0xFFull) | 0x01;
        // z: bytes 16..32 of Keccak-256(linear_hash || versioned_hash), big-endian
        u64 a[25];
#pragma unroll
        for (int i = 0; i < 25; i++) a[i] = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) { a[i] = kzg_get64(rec + KZG_REC_LINEAR + 8 * i); a[4 + i] = v[i]; }
        a[8] ^= 1;
        a[16] ^= 0x8000000000000000ull;
        keccak_f1600(a);
#pragma unroll
        for (int i = 0; i < 4; i++) { kzg_put64(rec + KZG_REC_VERSIONED + 8 * i, v[i]); lds_versioned[i] = v[i]; }
        kzg_put64(rec + KZG_REC_Z, a[2]);
        kzg_put64(rec + KZG_REC_Z + 8, a[3]);
        lds_z[0] = a[2];
        lds_z[1] = a[3];
    }
    __syncthreads();
    // the opening y = sum_i e_i z^(4095 - i). z stays in Montgomery form and the running values plain: mul(plain, Montgomery) is plain
    bls::Fr z = bls::zero<bls::FrT>();
    {
        const u64 lo = kzg_bswap64(lds_z[1]), hi = kzg_bswap64(lds_z[0]);
        z.w[0] = (u32)lo; z.w[1] = (u32)(lo >> 32); z.w[2] = (u32)hi; z.w[3] = (u32)(hi >> 32);
    }
    const bls::Fr zm = bls::to_mont(z);
    bls::Fr acc = bls::zero<bls::FrT>();
#pragma unroll 1
    for (int i = 0; i < 16; i++) {
        const uint8_t* b = blob + 31 * (size_t)(16 * t + i);
        bls::Fr e;
#pragma unroll
        for (int j = 0; j < 8; j++) e.w[j] = (u32)b[4 * j] | ((u32)b[4 * j + 1] << 8) | ((u32)b[4 * j + 2] << 16) | (j < 7 ? (u32)b[4 * j + 3] << 24 : 0u);
        acc = bls::add(bls::mul<bls::FrT>(acc, zm), e);
    }
    bls::Fr z16 = zm;
#pragma unroll 1
    for (int i = 0; i < 4; i++) z16 = bls::sqr(z16);
    bls::Fr pw = bls::one<bls::FrT>();  // (z^16)^(255 - t)
    const u32 ex = 255u - (u32)t;
#pragma unroll 1
    for (int bit = 7; bit >= 0; bit--) {
        pw = bls::sqr(pw);
        const bls::Fr with = bls::mul<bls::FrT>(pw, z16);
        pw = bls::select((ex >> bit) & 1, with, pw);
    }
    acc = bls::mul<bls::FrT>(acc, pw);
#pragma unroll 1
    for (int s = KZG_TAIL_THREADS / 2; s >= 1; s >>= 1) {
        if (t >= s && t < 2 * s) lds_sum[t - s] = acc;
        __syncthreads();
        if (t < s) acc = bls::add(acc, lds_sum[t]);
        __syncthreads();
    }
    if (t != 0) return;
    // y as 32 big-endian bytes; output hash = Keccak-256(versioned_hash || z || y): 80 bytes, one block
    u64 a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        a[i] = lds_versioned[i];
        a[6 + i] = kzg_bswap64((u64)acc.w[6 - 2 * i] | ((u64)acc.w[7 - 2 * i] << 32));
        kzg_put64(rec + KZG_REC_Y + 8 * i, a[6 + i]);
    }
    a[4] = lds_z[0];
    a[5] = lds_z[1];
    a[10] ^= 1;
    a[16] ^= 0x8000000000000000ull;
    keccak_f1600(a);
#pragma unroll
    for (int i = 0; i < 4; i++) kzg_put64(rec + KZG_REC_OUTPUT + 8 * i, a[i]);
}

}  // namespace zkw
