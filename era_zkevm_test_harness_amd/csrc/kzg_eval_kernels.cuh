// kzg_eval_kernels.cuh — a blob in EVALUATION form evaluated at a point (eval_poly, kzg/src/lib.rs:327-358 of the reference) on gfx950, on
// top of kzg_open_kernels.cuh: the step between compute_challenge and the pairing check in verify_proof_poly (lib.rs:292-301).
//
// A blob is 4 096 elements of 32 big-endian bytes, element i = p(w_i) with w_i = w^brp12(i) (what zkw_eip4844_prove writes and
// k_kzg_blob_challenge hashes). The barycentric formula over the 4 096th roots of unity:
//     y = (z^4096 - 1) / 4096 * sum_i f_i w_i / (z - w_i)            (y = f_i if z = w_i)
//   k_kzg_blob_eval   a workgroup per blob, 256 lanes. Lane t owns the elements i = t + 256 j, j < 16 (a wave's loads are contiguous), and
//                     brp12(t + 256 j) = 16 brp8(t) + brp4(j): the sixteen roots of a lane are tw[e] for e < 2048 and -tw[e - 2048] otherwise,
//                     from the table of k_kzg_twiddles. The sixteen denominators of a lane are inverted by Montgomery's trick (prefix
//                     products up, ONE bls::fr_inv, back down); the 256 lane sums are added by a tree through LDS; z^4096 is twelve squarings.
//                     A zero denominator (z on the domain: at most one lane, the roots are distinct) is replaced by one inside the trick, the
//                     lane publishes its f_i through LDS and the workgroup returns that instead of the sum.
// An element or a point that is not below r is data: the status word of the blob says which, and the value written is 32 zero bytes.
// As in k_kzg_quotient the running values are PLAIN and the point, the roots, the denominators and the constants in Montgomery form:
// mul(plain, Montgomery) is plain, so nothing is converted on the way in or out. A body for both launch forms (zkw_launch.h).
#pragma once
#include "kzg_open_kernels.cuh"

namespace zkw {

enum : int { KZG_EVAL_THREADS = 256, KZG_EVAL_PER_LANE = KZG_EVAL_BYTES / 32 / KZG_EVAL_THREADS };
// a blob's status: 0, 1 + e for the LOWEST element index e that is not below r, or KZG_EVAL_BAD_POINT
enum : u32 { KZG_EVAL_OK = 0, KZG_EVAL_BAD_POINT = 4097 };
static_assert(KZG_EVAL_PER_LANE == 16, "brp12(t + 256 j) = 16 brp8(t) + brp4(j)");

// 32 big-endian bytes as plain words; two 16-byte loads when the address allows (a caller's device pointer may be odd)
static __device__ __forceinline__ bls::Fr kzg_eval_be32(const uint8_t* b, bool aligned) {
    bls::Fr e;
    if (aligned) {
        const uint4 hi = reinterpret_cast<const uint4*>(b)[0], lo = reinterpret_cast<const uint4*>(b)[1];
        e.w[7] = __builtin_bswap32(hi.x); e.w[6] = __builtin_bswap32(hi.y); e.w[5] = __builtin_bswap32(hi.z); e.w[4] = __builtin_bswap32(hi.w);
        e.w[3] = __builtin_bswap32(lo.x); e.w[2] = __builtin_bswap32(lo.y); e.w[1] = __builtin_bswap32(lo.z); e.w[0] = __builtin_bswap32(lo.w);
    } else {
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const uint8_t* p = b + 4 * (7 - m);
            e.w[m] = ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | (u32)p[3];
        }
    }
    return e;
}

// w_(t + 256 j) in Montgomery form; base = 16 brp8(t), so the exponent is below 4096 and the index below 2048
static __device__ __forceinline__ bls::Fr kzg_eval_root(const bls::Fr* __restrict__ tw, u32 base, u32 j) {
    const u32 e = base + (__brev(j) >> 28);
    const bls::Fr w = tw[e & 2047u];
    return e < 2048u ? w : bls::neg(w);  // w^2048 = -1 (no root is zero)
}

// grid n_blobs, 256 lanes. Blob b: its 4 096 elements at evals + b * KZG_EVAL_BYTES, its point (32 big-endian bytes) at
// points + b * point_stride, its value (the same form) at values + b * value_stride, its status at status[b]. tw: k_kzg_twiddles' table
static __device__ __forceinline__ void k_kzg_blob_eval(const VB& vb, const uint8_t* __restrict__ evals, const uint8_t* __restrict__ points, u32 point_stride,
                                                       const bls::Fr* __restrict__ tw, uint8_t* __restrict__ values, u32 value_stride, u32* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint4 sums[2 * KZG_EVAL_THREADS];  // the add tree: 256 Fr
    __shared__ u32 s_bad, s_on_domain, s_element[8];
    const u32 t = threadIdx.x;
    if (t == 0) {
        s_bad = ~0u;
        s_on_domain = 0;
    }
    __syncthreads();
    const uint8_t* ev = evals + (size_t)vb.x * KZG_EVAL_BYTES;
    const bool aligned = (reinterpret_cast<uintptr_t>(evals) & 15) == 0;  // (a blob is a multiple of 16 bytes)
    const bls::Fr z = kzg_eval_be32(points + (size_t)vb.x * point_stride, false);
    if (t == 0 && !bls::below_modulus<bls::FrT>(z.w)) atomicMin(&s_bad, (u32)KZG_EVAL_BAD_POINT);
    const bls::Fr zm = bls::to_mont(z), one = bls::one<bls::FrT>();
    const u32 base = (__brev(t) >> 24) << 4;
    // up: prefix[j] = d_0 .. d_j with d_j = z - w_(t + 256 j), a zero d_j taken as one
    bls::Fr prefix[KZG_EVAL_PER_LANE];
    u32 hit = KZG_EVAL_PER_LANE;
#pragma unroll
    for (u32 j = 0; j < KZG_EVAL_PER_LANE; j++) {
        bls::Fr d = bls::sub(zm, kzg_eval_root(tw, base, j));
        const bool on = bls::is_zero(d);
        hit = on ? j : hit;
        d = bls::select(on, one, d);
        prefix[j] = j ? bls::mul<bls::FrT>(prefix[j - 1], d) : d;
    }
    bls::Fr inv = bls::fr_inv(prefix[KZG_EVAL_PER_LANE - 1]);  // 1 / (d_0 .. d_j) on the way down
    bls::Fr acc = bls::zero<bls::FrT>();
#pragma unroll
    for (int j = KZG_EVAL_PER_LANE - 1; j >= 0; j--) {
        const u32 i = t + (u32)KZG_EVAL_THREADS * (u32)j;  // < 4096
        const bls::Fr f = kzg_eval_be32(ev + 32 * (size_t)i, aligned);
        if (!bls::below_modulus<bls::FrT>(f.w)) atomicMin(&s_bad, 1u + i);
        const bls::Fr w = kzg_eval_root(tw, base, (u32)j);
        const bool on = hit == (u32)j;
        const bls::Fr dinv = j ? bls::mul<bls::FrT>(inv, prefix[j - 1]) : inv;
        if (j) inv = bls::mul<bls::FrT>(inv, bls::select(on, one, bls::sub(zm, w)));
        acc = bls::add(acc, bls::mul<bls::FrT>(bls::mul<bls::FrT>(f, w), dinv));
        if (on) {  // z = w_i: the value is f_i
            s_on_domain = 1;
#pragma unroll
            for (int m = 0; m < 8; m++) s_element[m] = f.w[m];
        }
    }
    kzg_lds_put(sums, t, acc);
    __syncthreads();
#pragma unroll 1
    for (u32 d = KZG_EVAL_THREADS / 2; d; d >>= 1) {
        if (t < d) kzg_lds_put(sums, t, bls::add(kzg_lds_get(sums, t), kzg_lds_get(sums, t + d)));
        __syncthreads();
    }
    if (t != 0) return;
    bls::Fr zp = zm;  // z^4096
#pragma unroll 1
    for (int s = 0; s < 12; s++) zp = bls::sqr(zp);
    // 1 / 4096 in Montgomery form is 2^256 / 2^12 = 2^244, which is below r (a number of 255 bits) as it stands
    bls::Fr inv_width = bls::zero<bls::FrT>();
    inv_width.w[7] = 1u << 20;
    bls::Fr y = bls::mul<bls::FrT>(bls::mul<bls::FrT>(kzg_lds_get(sums, 0), bls::sub(zp, one)), inv_width);
    if (s_on_domain) {
#pragma unroll
        for (int m = 0; m < 8; m++) y.w[m] = s_element[m];
    }
    const u32 bad = s_bad;
    if (bad != ~0u) y = bls::zero<bls::FrT>();
    kzg_put_be32(values + (size_t)vb.x * value_stride, y);
    status[vb.x] = bad != ~0u ? bad : (u32)KZG_EVAL_OK;
}

}  // namespace zkw
