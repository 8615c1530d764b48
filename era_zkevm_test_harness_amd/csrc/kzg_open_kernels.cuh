// kzg_open_kernels.cuh — the two KZG proofs of an EIP-4844 blob (compute_proof and compute_proof_poly, kzg/src/lib.rs:218-256, 285-288,
// 360-383 of the reference) on gfx950, on top of kzg_kernels.cuh.
//
// In the monomial form this library keeps, the proof of p(z) = y is the commitment of q(X) = (p(X) - y) / (X - z), and the coefficients
// of q are the intermediate values of the Horner walk that evaluates p at z: with the coefficients highest first, a_0 .. a_(n-1),
//     v_0 = a_0,  v_h = v_(h-1) z + a_h:   q = sum_h v_h X^(n-2-h) (h < n - 1),   y = v_(n-1)
// for EVERY z — on the evaluation domain or off it, no inversion. So an opening is one scan in Fr and one more run of the commitment
// (kzg_commit_device over the rows of q). The blob proof is the opening at a Fiat-Shamir challenge over the blob in evaluation form:
//   k_kzg_quotient        a workgroup per polynomial: lane t runs Horner over its chunk of L coefficients from zero, the 256 chunk values
//                         become carries by a Kogge-Stone scan of H_t = H_(t-1) z^L + a_(t-1) through LDS (eight steps, the multipliers
//                         z^(L 2^s) by squaring), then every lane repeats its chunk from its carry and stores each value as a row of q
//   k_kzg_twiddles        a lane per j < 2048: w^j by square-and-multiply (per call, into context scratch)
//   k_kzg_blob_ntt        a workgroup per blob: the 4 096 coefficients in 128 KiB of dynamic LDS, twelve decimation-in-frequency stages
//                         on natural-order input, so that position i of the result is p(w^brp12(i)): the blob's evaluation form as is
//   k_kzg_blob_intt       a workgroup per blob, the way back: the evaluation form (range-checked while it is loaded) to the 4 096
//                         coefficients, the same twelve stages undone last first with the same table, then 1 / 4096
//   k_kzg_blob_challenge  a wave per blob: SHA-256 over "FSBLOBVERIFY_V1_" || 4096 || evaluation form || commitment (2 050 blocks),
//                         reduced below r
//   k_kzg_proofs_out      the 2 n compressed proofs into the n records
// The transforms in Fr of this header and of kzg_cell_kernels.cuh and kzg_recover_kernels.cuh are written ONCE, here: kzg_fr_ntt4096 and
// kzg_fr_intt4096 (the twelve stages and the twelve undone), kzg_fr_ntt128 (seven stages, a wave), kzg_fr_pow (the recovery kernels') and kzg_store_be32_rows.
// As in k_kzg_tail, z and the twiddles are in Montgomery form and the running values PLAIN: mul(plain, Montgomery) is plain, so no
// element is converted on the way in or out. Every kernel is a body for both launch forms (zkw_launch.h).
#pragma once
#include "kzg_kernels.cuh"

namespace zkw {

// zkw_eip4844_proof_record (include/zkw.h), by byte offset
enum : u32 { KZG_PRF_OPENING = 0, KZG_PRF_BLOB = 48, KZG_PRF_CHALLENGE = 96, KZG_PRF_VALUE = 128, KZG_PRF_BYTES = 160 };
enum : u32 { KZG_EVAL_BYTES = 4096 * 32, KZG_FS_BLOCKS = 2050 };  // the challenge's preimage: 32 + 131 072 + 48 bytes, padded
enum : int { KZG_QUO_THREADS = 256, KZG_NTT_THREADS = 512, KZG_NTT_LDS = 4096 * 32 };
// how a point z is stored: 32 little-endian bytes (zkw_kzg_open), the 16 big-endian bytes of a record's evaluation_point, or the 32
// big-endian bytes of a blob_challenge
enum : u32 { KZG_Z_LE32 = 0, KZG_Z_BE16 = 1, KZG_Z_BE32 = 2 };

// w = 7^((r - 1) / 4096) mod r in Montgomery form: a primitive 4 096th root of unity of Fr (kzg/src/lib.rs:39-47)
static __device__ __forceinline__ bls::Fr kzg_omega() {
    return bls::Fr{{0x09458a39u, 0xf2df262cu, 0x99dff177u, 0x048cdf5bu, 0xc7cce57bu, 0x16857bc5u, 0xa4a915aeu, 0x043b3dbcu}};
}

// the h-th coefficient of a polynomial, HIGHEST first (h = 0: the leading one)
static __device__ __forceinline__ bls::Fr kzg_coeff_from_top(const KzgSrc& src, const uint8_t* bytes, u32 h) {
    bls::Fr e;
    if (src.blob) {
        const uint8_t* b = bytes + 31 * (size_t)h;
#pragma unroll
        for (int j = 0; j < 8; j++) e.w[j] = (u32)b[4 * j] | ((u32)b[4 * j + 1] << 8) | ((u32)b[4 * j + 2] << 16) | (j < 7 ? (u32)b[4 * j + 3] << 24 : 0u);
    } else {
        const uint8_t* b = bytes + 32 * (size_t)(src.n_coeffs - 1 - h);
#pragma unroll
        for (int j = 0; j < 8; j++) e.w[j] = (u32)b[4 * j] | ((u32)b[4 * j + 1] << 8) | ((u32)b[4 * j + 2] << 16) | ((u32)b[4 * j + 3] << 24);
    }
    return e;
}

static __device__ __forceinline__ void kzg_put_be32(uint8_t* out, const bls::Fr& v) {  // 32 big-endian bytes, any address
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const u32 w = v.w[7 - m];
        out[4 * m] = (uint8_t)(w >> 24);
        out[4 * m + 1] = (uint8_t)(w >> 16);
        out[4 * m + 2] = (uint8_t)(w >> 8);
        out[4 * m + 3] = (uint8_t)w;
    }
}

// ---- what the transforms in Fr share (this header, kzg_cell_kernels.cuh, kzg_recover_kernels.cuh) ---------------------------------------
// base^e for e < 2^bits, by square-and-multiply with uniform control flow (Montgomery form). The recovery kernels call it; k_kzg_twiddles
// and k_kzg_cell_wpow keep the same loop written out with a constant count: called through here the compiler counts their loop another way
// (the same work in other instructions), and a refactor moves no instruction
static __device__ __forceinline__ bls::Fr kzg_fr_pow(const bls::Fr& base, u32 e, int bits) {
    bls::Fr pw = bls::one<bls::FrT>();
#pragma unroll 1
    for (int bit = bits - 1; bit >= 0; bit--) {
        pw = bls::sqr(pw);
        const bls::Fr with = bls::mul<bls::FrT>(pw, base);
        pw = bls::select((e >> bit) & 1, with, pw);
    }
    return pw;
}

static __device__ __forceinline__ bls::Fr kzg_lds_get(const uint4* x, u32 i) {
    const uint4 a = x[2 * i], b = x[2 * i + 1];
    return bls::Fr{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
static __device__ __forceinline__ void kzg_lds_put(uint4* x, u32 i, const bls::Fr& v) {
    x[2 * i] = uint4{v.w[0], v.w[1], v.w[2], v.w[3]};
    x[2 * i + 1] = uint4{v.w[4], v.w[5], v.w[6], v.w[7]};
}

// The twelve decimation-in-frequency stages over x[0 .. 4095] (plain elements in LDS, 16-byte aligned), lane t of KZG_NTT_THREADS, tw =
// k_kzg_twiddles' table; every lane of the workgroup calls it, behind a barrier after the last write of x, and it ends on a barrier. Stage s
// has half-width h = 2048 >> s and pairs x[i0] with x[i1 = i0 + h]: butterfly b < 2048 has j = b mod h and i0 = (b div h) 2 h + j, and
// (u, v) -> (u + v, (u - v) w^(j 2048 / h)) = tw[j << s]. Natural order in, bit-reversed order out: position i holds the value at w^brp12(i)
static __device__ __forceinline__ void kzg_fr_ntt4096(uint4* x, u32 t, const bls::Fr* __restrict__ tw) {
#pragma unroll 1
    for (u32 s = 0; s < 12; s++) {
        const u32 half = 2048u >> s;
#pragma unroll 1
        for (u32 b = t; b < 2048; b += KZG_NTT_THREADS) {
            const u32 j = b & (half - 1), i0 = ((b >> (11 - s)) << (12 - s)) | j, i1 = i0 + half;  // i1 <= 4095
            const bls::Fr u = kzg_lds_get(x, i0), v = kzg_lds_get(x, i1);
            kzg_lds_put(x, i0, bls::add(u, v));
            bls::Fr d = bls::sub(u, v);
            if (s < 11) d = bls::mul<bls::FrT>(d, tw[j << s]);  // (the last stage's only twiddle is 1)
            kzg_lds_put(x, i1, d);
        }
        __syncthreads();
    }
}
// The same twelve stages undone last first, under the same conditions: bit-reversed order in, natural order out, every element 4 096 times
// the inverse transform (the caller's one product by 1 / 4096). A forward stage sent (u, v) to (a, b) = (u + v, (u - v) w^e), e = j 2048 / h,
// so (2 u, 2 v) = (a + b w^-e, a - b w^-e), and w^-e = -w^(2048 - e) (w^2048 = -1): the same table with add and sub exchanged, for e = 0
// entry 0 with them as they are
static __device__ __forceinline__ void kzg_fr_intt4096(uint4* x, u32 t, const bls::Fr* __restrict__ tw) {
#pragma unroll 1
    for (u32 s = 12; s-- > 0;) {
        const u32 half = 2048u >> s;
#pragma unroll 1
        for (u32 b = t; b < 2048; b += KZG_NTT_THREADS) {
            const u32 j = b & (half - 1), i0 = ((b >> (11 - s)) << (12 - s)) | j, i1 = i0 + half;  // i1 <= 4095
            const bls::Fr u = kzg_lds_get(x, i0);
            bls::Fr m = kzg_lds_get(x, i1);
            if (s < 11) m = bls::mul<bls::FrT>(m, tw[(2048u - (j << s)) & 2047u]);  // (the first stage undone has no twiddle but 1)
            const bls::Fr with = bls::add(u, m), without = bls::sub(u, m);
            kzg_lds_put(x, i0, bls::select(j == 0, with, without));
            kzg_lds_put(x, i1, bls::select(j == 0, without, with));
        }
        __syncthreads();
    }
}
// The seven stages of the same form over x[0 .. 127], one wave, lane l < 64 a butterfly, with w128 = w^32 from the same table: natural
// order in, position q = the value at w128^brp7(q) out. Every lane of the WORKGROUP calls it (each stage ends on the workgroup's barrier)
static __device__ __forceinline__ void kzg_fr_ntt128(uint4* x, u32 l, const bls::Fr* __restrict__ tw) {
#pragma unroll 1
    for (u32 s = 0; s < 7; s++) {
        const u32 half = 64u >> s;
        const u32 j = l & (half - 1), i0 = ((l >> (6 - s)) << (7 - s)) | j, i1 = i0 + half;  // i1 <= 127
        const bls::Fr u = kzg_lds_get(x, i0), v = kzg_lds_get(x, i1);
        kzg_lds_put(x, i0, bls::add(u, v));
        bls::Fr d = bls::sub(u, v);
        if (s < 6) d = bls::mul<bls::FrT>(d, tw[(j << s) * 32u]);  // w128^(j 2^s) = w^(32 j 2^s), index <= 32 * 63
        kzg_lds_put(x, i1, d);
        __syncthreads();
    }
}
// x[0 .. 4095] out as rows of 32 big-endian bytes, lane t of KZG_NTT_THREADS: word stores when the rows are 4-byte aligned
static __device__ __forceinline__ void kzg_store_be32_rows(const uint4* x, u32 t, uint8_t* out, bool aligned) {
#pragma unroll 1
    for (u32 i = t; i < 4096; i += KZG_NTT_THREADS) {
        const bls::Fr v = kzg_lds_get(x, i);
        if (aligned) {
            u32* o = reinterpret_cast<u32*>(out + 32 * (size_t)i);
#pragma unroll
            for (int m = 0; m < 8; m++) o[m] = __builtin_bswap32(v.w[7 - m]);
        } else {
            kzg_put_be32(out + 32 * (size_t)i, v);
        }
    }
}

// grid n_polys, 256 lanes. Polynomial j: its coefficients at src.base + j * poly_stride, its point at z + j * z_stride (z_form), the
// n_coeffs - 1 rows of its quotient (32 little-endian bytes each, row k = the coefficient of X^k) at rows + j * rows_stride (32-byte
// aligned), its value at y + j * y_stride (y may be null; big- or little-endian bytes). The point must be below r.
static __device__ __forceinline__ void k_kzg_quotient(const VB& vb, KzgSrc src, u32 poly_stride, const uint8_t* __restrict__ z, u32 z_stride, u32 z_form,
                                                      uint8_t* __restrict__ rows, u32 rows_stride, uint8_t* __restrict__ y, u32 y_stride, u32 y_be) {
    __shared__ bls::Fr lds[KZG_QUO_THREADS];
    const u32 t = threadIdx.x, n = src.n_coeffs;
    const uint8_t* bytes = src.base + (size_t)vb.x * poly_stride;
    const u32 L = n ? (n + KZG_QUO_THREADS - 1) / KZG_QUO_THREADS : 1u;  // a lane's chunk: [lo, hi), empty past the end
    const u32 lo = t * L < n ? t * L : n, hi = lo + L < n ? lo + L : n;
    bls::Fr zp = bls::zero<bls::FrT>();
    {
        const uint8_t* b = z + (size_t)vb.x * z_stride;
        if (z_form == KZG_Z_LE32) {
#pragma unroll
            for (int j = 0; j < 8; j++) zp.w[j] = (u32)b[4 * j] | ((u32)b[4 * j + 1] << 8) | ((u32)b[4 * j + 2] << 16) | ((u32)b[4 * j + 3] << 24);
        } else {
            const u32 words = z_form == KZG_Z_BE16 ? 4u : 8u;
#pragma unroll
            for (u32 j = 0; j < 8; j++)
                if (j < words) {
                    const uint8_t* p = b + 4 * (words - 1 - j);
                    zp.w[j] = ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | (u32)p[3];
                }
        }
    }
    const bls::Fr zm = bls::to_mont(zp);
    bls::Fr acc = bls::zero<bls::FrT>();
#pragma unroll 1
    for (u32 h = lo; h < hi; h++) acc = bls::add(bls::mul<bls::FrT>(acc, zm), kzg_coeff_from_top(src, bytes, h));
    bls::Fr m = zm;  // z^L, then z^(L 2^s)
#pragma unroll 1
    for (int bit = 30 - __clz((int)L); bit >= 0; bit--) {
        m = bls::sqr(m);
        if ((L >> bit) & 1) m = bls::mul<bls::FrT>(m, zm);
    }
    // inclusive scan S_t = sum_(j <= t) a_j (z^L)^(t - j) over the lanes whose chunks are full (a later lane's sum is never used)
#pragma unroll 1
    for (u32 d = 1; d < KZG_QUO_THREADS; d <<= 1) {
        lds[t] = acc;
        __syncthreads();
        if (t >= d) acc = bls::add(acc, bls::mul<bls::FrT>(lds[t - d], m));
        __syncthreads();
        m = bls::sqr(m);
    }
    lds[t] = acc;
    __syncthreads();
    acc = t ? lds[t - 1] : bls::zero<bls::FrT>();  // the carry: Horner's value ahead of this lane's chunk
    uint8_t* mine = rows + (size_t)vb.x * rows_stride;
    uint8_t* yo = y ? y + (size_t)vb.x * y_stride : nullptr;
#pragma unroll 1
    for (u32 h = lo; h < hi; h++) {
        acc = bls::add(bls::mul<bls::FrT>(acc, zm), kzg_coeff_from_top(src, bytes, h));
        if (h + 1 < n) {
            uint4* row = reinterpret_cast<uint4*>(mine + 32 * (size_t)(n - 2 - h));
            row[0] = uint4{acc.w[0], acc.w[1], acc.w[2], acc.w[3]};
            row[1] = uint4{acc.w[4], acc.w[5], acc.w[6], acc.w[7]};
        } else if (yo) {
            if (y_be) kzg_put_be32(yo, acc);
            else {
#pragma unroll
                for (int j = 0; j < 32; j++) yo[j] = (uint8_t)(acc.w[j >> 2] >> (8 * (j & 3)));
            }
        }
    }
    if (n == 0 && t == 0 && yo) {  // the zero polynomial of no coefficients
#pragma unroll 1
        for (int j = 0; j < 32; j++) yo[j] = 0;
    }
}

// tw[j] = w^j (Montgomery form), j < 2048
static __device__ __forceinline__ void k_kzg_twiddles(const VB& vb, bls::Fr* __restrict__ tw) {
    const u32 j = vb.x * blockDim.x + threadIdx.x;
    if (j >= 2048) return;
    const bls::Fr w = kzg_omega();
    bls::Fr pw = bls::one<bls::FrT>();
#pragma unroll 1
    for (int bit = 10; bit >= 0; bit--) {  // (kzg_fr_pow(w, j, 11) written out: see there)
        pw = bls::sqr(pw);
        const bls::Fr with = bls::mul<bls::FrT>(pw, w);
        pw = bls::select((j >> bit) & 1, with, pw);
    }
    tw[j] = pw;
}

// grid n_blobs, 512 lanes, KZG_NTT_LDS bytes of dynamic LDS. evals: [n_blobs][4096][32] big-endian, element i = p(w^brp12(i)) for
// p(X) = sum_i e_i X^(4095 - i): kzg_fr_ntt4096 on the coefficients leaves the transform in bit-reversed order, which is the order the
// blob's evaluation form has
static __device__ __forceinline__ void k_kzg_blob_ntt(const VB& vb, const uint8_t* __restrict__ blobs, const bls::Fr* __restrict__ tw, uint8_t* __restrict__ evals) {
    extern __shared__ __attribute__((aligned(16))) uint4 kzg_ntt_lds[];
    uint4* x = kzg_ntt_lds;
    const u32 t = threadIdx.x;
    const KzgSrc src{blobs + (size_t)vb.x * KZG_BLOB_BYTES, KZG_BLOB_ELEMENTS, 1};
#pragma unroll 1
    for (u32 k = t; k < 4096; k += KZG_NTT_THREADS) kzg_lds_put(x, k, kzg_coeff_from_top(src, src.base, 4095 - k));  // x[k]: the coefficient of X^k
    __syncthreads();
    kzg_fr_ntt4096(x, t, tw);
    uint8_t* out = evals + (size_t)vb.x * KZG_EVAL_BYTES;
    const bool aligned = (reinterpret_cast<uintptr_t>(evals) & 3) == 0;  // (a caller's device pointer may be odd)
    kzg_store_be32_rows(x, t, out, aligned);
}

// 32 big-endian bytes as plain words: eight word loads when the address allows, byte loads otherwise
static __device__ __forceinline__ bls::Fr kzg_get_be32(const uint8_t* b, bool aligned) {
    bls::Fr e;
    if (aligned) {
        const u32* p = reinterpret_cast<const u32*>(b);
#pragma unroll
        for (int m = 0; m < 8; m++) e.w[7 - m] = __builtin_bswap32(p[m]);
    } else {
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const uint8_t* p = b + 4 * (7 - m);
            e.w[m] = ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | (u32)p[3];
        }
    }
    return e;
}

// The way back: grid n_blobs, 512 lanes, KZG_NTT_LDS bytes of dynamic LDS. evals: [n_blobs][4096][32] big-endian, element i = p(w^brp12(i)),
// any address. coeffs: [n_blobs][4096][32] little-endian, row k = the coefficient of X^k (KzgSrc{.., 4096, 0}: what k_kzg_quotient and
// k_kzg_accumulate read), 16-byte aligned. kzg_fr_intt4096 on the evaluation form as it is (bit-reversed order in, natural order out); the
// twelve factors of two leave with one product by 1 / 4096 per element on the way out.
// status[blob]: 0, or 1 + e for the LOWEST element index e that is not below r (k_kzg_blob_eval's form); such a blob is not transformed.
// points (may be null): [n_blobs][32] big-endian; status[n_blobs + blob] = 1 when the blob's point is not below r, else 0
static __device__ __forceinline__ void k_kzg_blob_intt(const VB& vb, const uint8_t* __restrict__ evals, const bls::Fr* __restrict__ tw, uint8_t* __restrict__ coeffs,
                                                       const uint8_t* __restrict__ points, u32 n_blobs, u32* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint4 kzg_ntt_lds[];
    __shared__ u32 s_bad;
    uint4* x = kzg_ntt_lds;
    const u32 t = threadIdx.x;
    if (t == 0) s_bad = ~0u;
    __syncthreads();
    const uint8_t* ev = evals + (size_t)vb.x * KZG_EVAL_BYTES;
    const bool aligned = (reinterpret_cast<uintptr_t>(evals) & 3) == 0;  // (a caller's device pointer may be odd)
#pragma unroll 1
    for (u32 i = t; i < 4096; i += KZG_NTT_THREADS) {
        const bls::Fr f = kzg_get_be32(ev + 32 * (size_t)i, aligned);
        if (!bls::below_modulus<bls::FrT>(f.w)) atomicMin(&s_bad, i);
        kzg_lds_put(x, i, f);
    }
    if (points && t == 0) status[n_blobs + vb.x] = bls::below_modulus<bls::FrT>(kzg_get_be32(points + 32 * (size_t)vb.x, false).w) ? 0u : 1u;
    __syncthreads();
    const u32 bad = s_bad;  // (the same for every lane: all leave, or none)
    if (t == 0) status[vb.x] = bad + 1u;
    if (bad != ~0u) return;
    kzg_fr_intt4096(x, t, tw);
    // 1 / 4096 in Montgomery form is 2^256 / 2^12 = 2^244, which is below r (a number of 255 bits) as it stands
    bls::Fr inv_width = bls::zero<bls::FrT>();
    inv_width.w[7] = 1u << 20;
    uint4* out = reinterpret_cast<uint4*>(coeffs + (size_t)vb.x * KZG_EVAL_BYTES);
#pragma unroll 1
    for (u32 k = t; k < 4096; k += KZG_NTT_THREADS) kzg_lds_put(out, k, bls::mul<bls::FrT>(kzg_lds_get(x, k), inv_width));
}

// word `wi` (big-endian, as SHA-256 reads it) of the padded preimage of compute_challenge: 8 words of domain and degree, 32 768 of the
// evaluation form, 12 of the commitment, the padding bit, zeros, the bit length in the last word
static __device__ __forceinline__ u32 kzg_fs_word(const uint8_t* evals, bool aligned, const uint8_t* commitment, u32 wi) {
    constexpr u32 EV = 8, CM = EV + KZG_EVAL_BYTES / 4, PAD = CM + 12, LAST = KZG_FS_BLOCKS * 16 - 1;
    if (wi >= EV && wi < CM) {
        if (aligned) return __builtin_bswap32(*reinterpret_cast<const u32*>(evals + 4 * (size_t)(wi - EV)));
        const uint8_t* b = evals + 4 * (size_t)(wi - EV);
        return ((u32)b[0] << 24) | ((u32)b[1] << 16) | ((u32)b[2] << 8) | (u32)b[3];
    }
    if (wi >= CM && wi < PAD) {
        const uint8_t* b = commitment + 4 * (wi - CM);
        return ((u32)b[0] << 24) | ((u32)b[1] << 16) | ((u32)b[2] << 8) | (u32)b[3];
    }
    switch (wi) {
        case 0: return 0x4653424Cu;  // "FSBL"
        case 1: return 0x4F425645u;  // "OBVE"
        case 2: return 0x52494659u;  // "RIFY"
        case 3: return 0x5F56315Fu;  // "_V1_"
        case 7: return 4096u;        // the degree as 16 big-endian bytes
        case PAD: return 0x80000000u;
        case LAST: return (32 + KZG_EVAL_BYTES + 48) * 8;
        default: return 0;
    }
}

// grid n_blobs, 64 lanes. The chain of the 2 050 compressions is serial and runs on lane 0; the message schedules are not: the 64 lanes
// load and expand the schedules of 64 blocks (round constant added) into LDS, word i of lane l at [i][l], then lane 0 runs those blocks'
// rounds. (The plain form, lane 0 alone through sha256_compress with its own loads, took 16.7 ms a blob against 4.9: profiles/r16.) The
// digest, a big-endian integer below 2^256 < 3 r, is reduced by at most two subtractions and written as 32 big-endian bytes at
// out + blob * out_stride
static __device__ __forceinline__ void k_kzg_blob_challenge(const VB& vb, const uint8_t* __restrict__ evals, const uint8_t* __restrict__ commitments,
                                                            u32 commitment_stride, uint8_t* __restrict__ out, u32 out_stride) {
    __shared__ u32 sched[64 * 64];
    const u32 lane = threadIdx.x;
    const uint8_t* ev = evals + (size_t)vb.x * KZG_EVAL_BYTES;
    const uint8_t* cm = commitments + (size_t)vb.x * commitment_stride;
    const bool aligned = (reinterpret_cast<uintptr_t>(evals) & 3) == 0;
    u32 st[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
#pragma unroll 1
    for (u32 base = 0; base < KZG_FS_BLOCKS; base += 64) {
        const u32 blk = base + lane;
        if (blk < KZG_FS_BLOCKS) {
            u32 w[16];
#pragma unroll
            for (int i = 0; i < 16; i++) w[i] = kzg_fs_word(ev, aligned, cm, 16 * blk + i);
#pragma unroll
            for (int i = 0; i < 64; i++) {
                if (i >= 16) {
                    const u32 w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
                    const u32 s0 = rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3), s1 = rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10);
                    w[i & 15] = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
                }
                sched[i * 64 + lane] = w[i & 15] + c_sha_k[i];
            }
        }
        __syncthreads();
        if (lane == 0) {
            const u32 count = KZG_FS_BLOCKS - base < 64 ? KZG_FS_BLOCKS - base : 64;
#pragma unroll 1
            for (u32 k = 0; k < count; k++) {
                u32 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
                for (int i = 0; i < 64; i++) {
                    const u32 S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25), ch = (e & f) ^ (~e & g);
                    const u32 t1 = h + S1 + ch + sched[i * 64 + k];
                    const u32 S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22), mj = (a & b) ^ (a & c) ^ (b & c);
                    const u32 t2 = S0 + mj;
                    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
                }
                st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
            }
        }
        __syncthreads();
    }
    if (lane != 0) return;
    u32 v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = st[7 - j];
    bls::Fr c = bls::cond_sub<bls::FrT>(v, 0);
    c = bls::cond_sub<bls::FrT>(c.w, 0);
    kzg_put_be32(out + (size_t)vb.x * out_stride, c);
}

// a lane per byte: proofs [n_blobs][2][48] (opening, blob) -> the first 96 bytes of each of the n_blobs records
static __device__ __forceinline__ void k_kzg_proofs_out(const VB& vb, const uint8_t* __restrict__ proofs, u32 n_blobs, uint8_t* __restrict__ recs) {
    const u32 i = vb.x * blockDim.x + threadIdx.x;
    if (i >= n_blobs * 96u) return;
    recs[(size_t)(i / 96u) * KZG_PRF_BYTES + i % 96u] = proofs[i];
}

}  // namespace zkw
