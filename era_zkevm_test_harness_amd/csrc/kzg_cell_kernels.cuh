// kzg_cell_kernels.cuh — EIP-7594 (PeerDAS) cells and cell proofs of a blob on gfx950, on top of kzg_open_kernels.cuh: the extended blob of
// 8 192 evaluations cut into 128 cells of 64 elements, and one KZG multi-opening proof per cell by FK20 (Feist, Khovratovich: "Fast
// amortized KZG proofs") over a Fourier transform of G1 points.
//
// With W = 7^((r - 1) / 8192), w = W^2 the blob's root and w128 = w^32: extended evaluation e[j] = p(W^brp13(j)); cell k = e[64 k .. 64 k + 63],
// the 64 roots of X^64 - c_k, c_k = w128^brp7(k); proof[k] = [q_k(tau)] G1 for q_k = p div (X^64 - c_k) = sum_j c_k^j floor(p / X^(64 (j + 1))).
// So with h_j = [floor(p / X^(64 (j + 1)))(tau)] G1 (j < 63) the 128 proofs are ONE transform, P[u] = sum_j w128^(u j) h_j, proof[k] = P[brp7(k)],
// and the h_j are 64 Toeplitz products (offset i < 64: c_i[d] = p[4095 - i - 64 d] against x_i[m] = S[4031 - i - 64 m]) done as circular
// products of length 128 in the transformed domain: H[j] = sum_i C_i[j] X_i[j], h = G1_IFFT(H). The X_i = G1_FFT(x_i) are the setup side
// (zkw_kzg_cell_settings: a byte-window table 2^(8 w) X_i[j], k_kzg_table as it is), the C_i = Fr_FFT(t_i) / 128 the blob side.
//   k_kzg_g1_fft          a wave per transform of n <= 128 points, Jacobian in LDS, a lane per butterfly, decimation in frequency; the
//                         product by a twiddle is [k1] P + [k2] phi(P) over 128 doublings, two bits of each half a step (kzg_cell_tables.cuh:
//                         the twiddles split on the host)
//   k_kzg_g1_lift, k_kzg_g1_compress   the byte forms around it: affine -> Jacobian; Jacobian -> 48 compressed bytes, a lane per point
//   k_kzg_cell_setup_x, k_kzg_cell_setup_affine   settings: the vectors x_i from S; the X_i[j] to affine as row 0 of the table, [j][i]
//   k_kzg_cell_wpow       W^k, k < 4096
//   k_kzg_cells           a workgroup per (blob, half): cells 64..127 = the blob's forward transform of the coefficients scaled by W^k;
//                         cells 0..63 = the blob itself (copied) or the unscaled transform (pubdata form)
//   k_kzg_cell_toeplitz   a wave per (offset i, blob): t_i from the coefficients, kzg_fr_ntt128 in LDS, C_i / 128 as scalar bytes [j][i]
//   k_kzg_cell_msm        a workgroup per (j, blob): the 64 x 32 digits of C_.[j] in LDS, a LANE per bucket d (it walks the digits for the next
//                         one equal to d and adds the table entry), the 255 buckets through LDS into the eight bit sums of k_kzg_finish
//   k_kzg_cell_horner     a lane per (j, blob): H[j] = sum_b 2^b sums[b], kept Jacobian
// As in kzg_open_kernels.cuh the Fr twiddles are in Montgomery form and the running values PLAIN. Every kernel is a body for both launch forms.
#pragma once
#include "kzg_open_kernels.cuh"
#include "kzg_cell_tables.cuh"

namespace zkw {

enum : u32 { KZG_CELLS = 128, KZG_CELL_ELEMENTS = 64, KZG_CELL_BYTES = 64 * 32, KZG_CELLS_BYTES = 128 * 64 * 32, KZG_CELL_POINTS = 8192, KZG_G1_FFT_MAX = 128 };
enum : int { KZG_G1_FFT_THREADS = 64, KZG_CELL_FR_THREADS = 256, KZG_CELL_MSM_THREADS = 256 };

static __device__ __forceinline__ u32 kzg_brp(u32 v, u32 bits) { return bits ? __brev(v) >> (32 - bits) : 0u; }

// A lane's window table for kzg_g1_mul_split: entry a + 4 b - 1 = [a] q + [b] phi(q) for a, b < 4 (not both 0), 15 Jacobian points of 36
// words, word w of entry e at tab[(36 e + w) * 64] (tab already points at the lane's column: the lanes of a wave read and write side by side)
enum : u32 { KZG_G1_TAB_ENTRIES = 15, KZG_G1_TAB_WORDS = 15 * 36 * 64 };
static __device__ __forceinline__ void kzg_g1_tab_put(u32* tab, u32 e, const bls::G1Jac& p) {
#pragma unroll
    for (int w = 0; w < 12; w++) {
        tab[(36 * e + w) * 64] = p.X.w[w];
        tab[(36 * e + 12 + w) * 64] = p.Y.w[w];
        tab[(36 * e + 24 + w) * 64] = p.Z.w[w];
    }
}
static __device__ __forceinline__ bls::G1Jac kzg_g1_tab_get(const u32* tab, u32 e) {
    bls::G1Jac p;
#pragma unroll
    for (int w = 0; w < 12; w++) {
        p.X.w[w] = tab[(36 * e + w) * 64];
        p.Y.w[w] = tab[(36 * e + 12 + w) * 64];
        p.Z.w[w] = tab[(36 * e + 24 + w) * 64];
    }
    return p;
}

// [k] q for row = (k1, k2) of c_kzg_g1_twiddle, k = k1 + k2 lambda and phi(q) = (beta X, Y, Z) = [lambda] q: one walk over both halves two
// bits at a time (Straus) — 64 steps of two doublings and ONE addition of the table entry the four bits name, against 128 steps of one
// doubling and one addition for single bits and 255 for the unsplit scalar. Uniform control flow (a zero digit pair adds the point at
// infinity; every case of jadd is complete). tab: the lane's column of a table in global memory (15 x 36 words a lane is more than a
// wave can keep in registers, and in LDS it would cost the kernel its occupancy)
static __device__ __forceinline__ bls::G1Jac kzg_g1_mul_split(const bls::G1Jac& q, const u32* __restrict__ row, u32* tab) {
    {
        const bls::Fq beta = kzg_g1_beta();
        bls::G1Jac m = q;  // [a] q and [a] phi(q), a = 1, 2, 3
#pragma unroll 1
        for (u32 a = 1; a < 4; a++) {
            if (a == 2) m = bls::jdbl(q);
            if (a == 3) m = bls::jadd(m, q);
            kzg_g1_tab_put(tab, a - 1, m);
            kzg_g1_tab_put(tab, 4 * a - 1, bls::G1Jac{bls::mul<bls::FqT>(m.X, beta), m.Y, m.Z});
        }
#pragma unroll 1
        for (u32 e = 5; e < 16; e++) {
            if ((e & 3) == 0) continue;
            kzg_g1_tab_put(tab, e - 1, bls::jadd(kzg_g1_tab_get(tab, (e & 3) - 1), kzg_g1_tab_get(tab, (e & 12) - 1)));
        }
    }
    bls::G1Jac acc = bls::jac_inf();
#pragma unroll 1
    for (int wi = 3; wi >= 0; wi--) {
        const u32 k1 = row[wi], k2 = row[4 + wi];
#pragma unroll 1
        for (int bit = 30; bit >= 0; bit -= 2) {
            const u32 e = ((k1 >> bit) & 3) | (((k2 >> bit) & 3) << 2);
            bls::G1Jac a = kzg_g1_tab_get(tab, e ? e - 1 : 0);
            a.Z = bls::select(e != 0, a.Z, bls::zero<bls::FqT>());
            acc = bls::jadd(bls::jdbl(bls::jdbl(acc)), a);
        }
    }
    return acc;
}

// grid n_ffts, one wave. in, out: [n_ffts][n] Jacobian points in natural order, n = 2^log_n <= 128 (in == out is fine: a transform is read whole
// before it is written). out[u] = sum_j w_n^(u j) in[j], w_n = w128^(128 / n); inverse: w_n^-1 = w128^(128 - 128 / n) and, with `scale`, the
// factor 1 / n (one more product per point). tab: KZG_G1_TAB_WORDS words per transform for the lanes' window tables. upper_inf: in[j] for
// j >= n / 2 is taken as the point at infinity (FK20 drops the upper half of the circular products). A stage of half-width h pairs x[i] with x[i + h]: (u, v) -> (u + v, [w_n^(j n / 2 h)] (u - v)), j = i mod h; the
// result is in bit-reversed order in LDS and leaves in natural order
static __device__ __forceinline__ void k_kzg_g1_fft(const VB& vb, const bls::G1Jac* __restrict__ in, bls::G1Jac* __restrict__ out, u32* tab, u32 log_n,
                                                    u32 inverse, u32 scale, u32 upper_inf) {
    __shared__ bls::G1Jac x[KZG_G1_FFT_MAX];
    const u32 t = threadIdx.x, n = 1u << log_n, half_n = n >> 1;
    u32* mine = tab + (size_t)vb.x * KZG_G1_TAB_WORDS + t;  // t < 64
    const bls::G1Jac* src = in + (size_t)vb.x * n;
#pragma unroll 1
    for (u32 k = t; k < n; k += KZG_G1_FFT_THREADS) {  // k < n <= 128
        if (upper_inf && log_n && k >= half_n) x[k] = bls::jac_inf();
        else x[k] = src[k];
    }
    __syncthreads();
#pragma unroll 1
    for (u32 s = 0; s < log_n; s++) {
        const u32 half = half_n >> s;
        if (t < half_n) {
            const u32 j = t & (half - 1), i0 = ((t >> (log_n - 1 - s)) << (log_n - s)) | j, i1 = i0 + half;  // i1 <= n - 1
            const bls::G1Jac u = x[i0], v = x[i1];
            x[i0] = bls::jadd(u, v);
            bls::G1Jac d = bls::jadd(u, bls::G1Jac{v.X, bls::neg(v.Y), v.Z});
            if (s + 1 < log_n) {  // (the last stage's only twiddle is 1)
                u32 e = (j << s) * (KZG_G1_FFT_MAX >> log_n);  // < 64
                if (inverse) e = (KZG_G1_FFT_MAX - e) & (KZG_G1_FFT_MAX - 1);
                d = kzg_g1_mul_split(d, c_kzg_g1_twiddle[e], mine);
            }
            x[i1] = d;
        }
        __syncthreads();
    }
    bls::G1Jac* dst = out + (size_t)vb.x * n;
#pragma unroll 1
    for (u32 k = t; k < n; k += KZG_G1_FFT_THREADS) {
        bls::G1Jac v = x[k];
        if (scale && log_n) v = kzg_g1_mul_split(v, c_kzg_g1_twiddle[KZG_G1_FFT_MAX + log_n], mine);
        dst[kzg_brp(k, log_n)] = v;
    }
}

// a lane per point
static __device__ __forceinline__ void k_kzg_g1_lift(const VB& vb, const bls::G1Aff* __restrict__ in, u32 n, bls::G1Jac* __restrict__ out) {
    const u32 k = vb.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const bls::Fq ax = in[k].x, ay = in[k].y;
    out[k].X = ax;
    out[k].Y = ay;
    out[k].Z = bls::is_zero(ax) && bls::is_zero(ay) ? bls::zero<bls::FqT>() : bls::one<bls::FqT>();
}

// a lane per point: to affine (one Fermat inversion a lane; the lanes of a wave invert side by side) and the 48 compressed bytes. With
// `by_cell`, point u of each run of 128 goes to place brp7(u) of that run: proof[k] = P[brp7(k)]
static __device__ __forceinline__ void k_kzg_g1_compress(const VB& vb, const bls::G1Jac* __restrict__ in, u32 n, u32 by_cell, uint8_t* __restrict__ out) {
    const u32 k = vb.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const u32 to = by_cell ? (k & ~127u) | kzg_brp(k & 127u, 7) : k;
    bls::compress(bls::to_affine(in[k]), out + 48 * (size_t)to);
}

// settings: x[i][m] = S[4031 - i - 64 m] for m < 63, infinity for 63 <= m < 128 (S: row 0 of the settings' table, 4 096 affine points)
static __device__ __forceinline__ void k_kzg_cell_setup_x(const VB& vb, const bls::G1Aff* __restrict__ s, bls::G1Jac* __restrict__ x) {
    const u32 idx = vb.x * blockDim.x + threadIdx.x;
    if (idx >= KZG_CELL_POINTS) return;
    const u32 i = idx >> 7, m = idx & 127u;
    x[idx] = m < 63 ? bls::to_jac(s[4031u - i - 64u * m]) : bls::jac_inf();  // 4031 - 63 - 64 * 62 = 0
}

// settings: X[i][j] (Jacobian) -> table[j * 64 + i] (affine; infinity is (0, 0) and contributes nothing to a sum)
static __device__ __forceinline__ void k_kzg_cell_setup_affine(const VB& vb, const bls::G1Jac* __restrict__ x, bls::G1Aff* __restrict__ table) {
    const u32 idx = vb.x * blockDim.x + threadIdx.x;
    if (idx >= KZG_CELL_POINTS) return;
    const u32 i = idx >> 7, j = idx & 127u;
    table[j * 64u + i] = bls::to_affine(x[idx]);
}

// wpow[k] = W^k (Montgomery form), k < 4096
static __device__ __forceinline__ void k_kzg_cell_wpow(const VB& vb, bls::Fr* __restrict__ wpow) {
    const u32 k = vb.x * blockDim.x + threadIdx.x;
    if (k >= 4096) return;
    const bls::Fr w = kzg_cell_w();
    bls::Fr pw = bls::one<bls::FrT>();
#pragma unroll 1
    for (int bit = 11; bit >= 0; bit--) {  // (kzg_fr_pow(w, k, 12) written out: see there)
        pw = bls::sqr(pw);
        const bls::Fr with = bls::mul<bls::FrT>(pw, w);
        pw = bls::select((k >> bit) & 1, with, pw);
    }
    wpow[k] = pw;
}

// grid (n_blobs, 2), 512 lanes, KZG_NTT_LDS bytes of dynamic LDS. cells: [n_blobs][128][2048], any address. Half 1 (cells 64..127): element j
// = p(W w^brp12(j)), kzg_fr_ntt4096 on the coefficients scaled by W^k. Half 0 (cells 0..63): the blob's own evaluation form —
// copied from `evals` ([n_blobs][131072], any address) when that is given, else the same transform unscaled. The polynomial is read through
// src (a blob of 31-byte elements or rows of 32 little-endian bytes), blob b at src.base + b * poly_stride
static __device__ __forceinline__ void k_kzg_cells(const VB& vb, KzgSrc src, u32 poly_stride, const uint8_t* __restrict__ evals, const bls::Fr* __restrict__ tw,
                                                   const bls::Fr* __restrict__ wpow, uint8_t* __restrict__ cells) {
    extern __shared__ __attribute__((aligned(16))) uint4 kzg_cells_lds[];
    uint4* x = kzg_cells_lds;
    const u32 t = threadIdx.x;
    uint8_t* out = cells + (size_t)vb.x * KZG_CELLS_BYTES + (size_t)vb.y * KZG_EVAL_BYTES;
    const bool aligned = (reinterpret_cast<uintptr_t>(cells) & 3) == 0;  // (a caller's device pointer may be odd)
    if (vb.y == 0 && evals) {
        const uint8_t* ev = evals + (size_t)vb.x * KZG_EVAL_BYTES;
        if (aligned && (reinterpret_cast<uintptr_t>(evals) & 3) == 0) {
#pragma unroll 1
            for (u32 i = t; i < KZG_EVAL_BYTES / 4; i += KZG_NTT_THREADS) reinterpret_cast<u32*>(out)[i] = reinterpret_cast<const u32*>(ev)[i];
        } else {
#pragma unroll 1
            for (u32 i = t; i < KZG_EVAL_BYTES; i += KZG_NTT_THREADS) out[i] = ev[i];
        }
        return;
    }
    const uint8_t* bytes = src.base + (size_t)vb.x * poly_stride;
#pragma unroll 1
    for (u32 k = t; k < 4096; k += KZG_NTT_THREADS) {  // x[k]: the coefficient of X^k, times W^k in the upper half
        bls::Fr c = kzg_coeff_from_top(src, bytes, 4095 - k);
        if (vb.y) c = bls::mul<bls::FrT>(c, wpow[k]);
        kzg_lds_put(x, k, c);
    }
    __syncthreads();
    kzg_fr_ntt4096(x, t, tw);
    kzg_store_be32_rows(x, t, out, aligned);
}

// grid (16, n_blobs), 256 lanes: wave v of workgroup g takes offset i = 4 g + v. t_i[0] = p[4095 - i], t_i[1..65] = 0, t_i[66 + m] = p[127 - i + 64 m]
// (m < 62); C_i = Fr_FFT_128(t_i) with w128 = w^32 (tw: k_kzg_twiddles' table of w^j) by kzg_fr_ntt128, times 1 / 128 — the
// factor of the inverse G1 transform that follows the sums, taken here where it is one product in Fr. c: [n_blobs][128][64][32], the scalar
// C_i[j] as 32 little-endian bytes at row j, column i: the 2 048 digit bytes of a sum H[j] are contiguous (32-byte aligned)
static __device__ __forceinline__ void k_kzg_cell_toeplitz(const VB& vb, KzgSrc src, u32 poly_stride, const bls::Fr* __restrict__ tw, uint8_t* __restrict__ c) {
    __shared__ __attribute__((aligned(16))) uint4 lds[4 * 2 * KZG_CELLS];
    const u32 wave = threadIdx.x >> 6, l = threadIdx.x & 63u, i = 4 * vb.x + wave;  // i < 64
    uint4* x = lds + wave * 2 * KZG_CELLS;
    const uint8_t* bytes = src.base + (size_t)vb.y * poly_stride;
    // p[k] = the (4095 - k)-th coefficient from the top. Lane l holds t[l] and t[64 + l]
    bls::Fr lo = bls::zero<bls::FrT>(), hi = bls::zero<bls::FrT>();
    if (l == 0) lo = kzg_coeff_from_top(src, bytes, i);
    if (l >= 2) hi = kzg_coeff_from_top(src, bytes, 3968u + i - 64u * (l - 2));  // 4095 - (127 - i + 64 m), m = l - 2 <= 61: >= 64 + i
    kzg_lds_put(x, l, lo);
    kzg_lds_put(x, 64 + l, hi);
    __syncthreads();
    kzg_fr_ntt128(x, l, tw);
    // 1 / 128 in Montgomery form is 2^256 / 2^7 = 2^249, which is below r as it stands
    bls::Fr inv_width = bls::zero<bls::FrT>();
    inv_width.w[7] = 1u << 25;
    uint4* out = reinterpret_cast<uint4*>(c + (size_t)vb.y * KZG_CELLS * 2048);
#pragma unroll
    for (u32 h = 0; h < 2; h++) {
        const u32 pos = l + 64 * h, j = kzg_brp(pos, 7);
        kzg_lds_put(out, j * 64 + i, bls::mul<bls::FrT>(kzg_lds_get(x, pos), inv_width));
    }
}

// grid (128, n_blobs), 256 lanes: H[j] of blob vb.y as 255 buckets, lane d owning bucket d. The 2 048 digit bytes (scalar i's byte w at
// 32 i + w) sit in LDS; a lane walks them a word at a time for the next byte equal to d (the zero-byte test on the word xor d d d d: its
// lowest flag is exact) and adds table[w][j][i] = 2^(8 w) X_i[j], so a wave pays for its busiest lane's entries (8 on average) and no fold
// follows: the buckets go through LDS into k_kzg_finish's eight bit sums, sums[b] = the sum of the buckets whose digit has bit b set — a
// wave per bit, two passes. c: k_kzg_cell_toeplitz's rows; table: [32][8192] affine; sums: [n_blobs][128][8].
// The walk and the fold are written once, kzg_cell_msm_sum, for every table of byte windows: sum number `sum` over the 64 entries that
// `at(w, i)` (w < 32, i < 64) places in `table` — here column j of the cell settings, in kzg_cell_verify_kernels.cuh the first 64 columns of
// the settings themselves
struct KzgCellColumns {
    u32 j;
    __device__ __forceinline__ size_t operator()(u32 w, u32 i) const { return (size_t)w * KZG_CELL_POINTS + j * 64u + i; }  // w < 32, j < 128, i < 64
};
template <class At>
static __device__ __forceinline__ void kzg_cell_msm_sum(size_t sum, At at, const uint8_t* __restrict__ c, const bls::G1Aff* __restrict__ table, bls::G1Jac* __restrict__ sums) {
    __shared__ __attribute__((aligned(16))) u32 digits[512];
    __shared__ bls::G1Jac bucket[KZG_BUCKETS];
    __shared__ bls::G1Jac fold[KZG_CELL_MSM_THREADS / 2];
    const u32 t = threadIdx.x;
    if (t < 128) reinterpret_cast<uint4*>(digits)[t] = reinterpret_cast<const uint4*>(c + sum * 2048)[t];
    __syncthreads();
    bls::G1Jac acc = bls::jac_inf();
    const u32 pattern = t * 0x01010101u;
    u32 q = t ? 0u : 2048u;  // the next position to look at (bucket 0 collects nothing)
#pragma unroll 1
    for (;;) {
#pragma unroll 1
        while (q < 2048) {
            const u32 v = (digits[q >> 2] ^ pattern) | ((1u << (8 * (q & 3))) - 1);  // (the bytes below q count as no match)
            const u32 z = (v - 0x01010101u) & ~v & 0x80808080u;
            if (z) {
                q = (q & ~3u) + ((u32)(__ffs((int)z) - 1) >> 3);
                break;
            }
            q = (q & ~3u) + 4;
        }
        if (q >= 2048) break;
        acc = bls::jmadd(acc, table[at(q & 31u, q >> 5)]);
        q++;
    }
    bucket[t] = acc;
    __syncthreads();
    const u32 l = t & 63u;
#pragma unroll 1
    for (u32 pass = 0; pass < 2; pass++) {
        const u32 b = 4 * pass + (t >> 6), low = (1u << b) - 1, m1 = l + 64;  // the m-th digit with bit b set (m < 128): m with a 1 inserted at bit b
        const u32 d0 = ((l >> b) << (b + 1)) | (1u << b) | (l & low), d1 = ((m1 >> b) << (b + 1)) | (1u << b) | (m1 & low);
        bls::G1Jac a = bucket[d0];
        {
            const bls::G1Jac other = bucket[d1];
            a = bls::jadd(a, other);
        }
        a = kzg_group_sum<64>(a, fold);
        if (l == 0) sums[sum * 8 + b] = a;
    }
}
static __device__ __forceinline__ void k_kzg_cell_msm(const VB& vb, const uint8_t* __restrict__ c, const bls::G1Aff* __restrict__ table, bls::G1Jac* __restrict__ sums) {
    kzg_cell_msm_sum((size_t)vb.y * KZG_CELLS + vb.x, KzgCellColumns{vb.x}, c, table, sums);
}

// a lane per sum: H = sum_b 2^b sums[b] by seven doublings, kept Jacobian
static __device__ __forceinline__ void k_kzg_cell_horner(const VB& vb, const bls::G1Jac* __restrict__ sums, u32 n, bls::G1Jac* __restrict__ h) {
    const u32 k = vb.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const bls::G1Jac* s = sums + (size_t)k * 8;
    bls::G1Jac acc = s[7];
#pragma unroll 1
    for (int bit = 6; bit >= 0; bit--) acc = bls::jadd(bls::jdbl(acc), s[bit]);
    h[k] = acc;
}

}  // namespace zkw
