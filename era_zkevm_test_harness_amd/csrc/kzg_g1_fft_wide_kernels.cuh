// kzg_g1_fft_wide_kernels.cuh — the Fourier transform of G1 points beyond one wave, n = 2^m for 128 < n <= 4 096, on top of
// kzg_cell_kernels.cuh: the trusted setup between the monomial basis S[k] = [tau^k] G1 and the Lagrange basis L[u] = [l_u(tau)] G1
// (KzgSettings::new, kzg/src/lib.rs:91-141 of the reference, keeps L in bit-reversed order).
//
// Decimation in frequency as in k_kzg_g1_fft: stage s pairs i0 with i1 = i0 + half, half = n / 2 >> s, j = i0 mod half,
// (u, v) -> (u + v, [w_n^(j 2^s)] (u - v)). The first m - 7 stages run over Jacobian points in HBM, a launch a stage and a lane a butterfly
// (a butterfly reads and writes its own two slots only: in place). After them the transform is n / 128 contiguous blocks, each the input of
// a 128-point transform with root w128 — k_kzg_g1_fft as it is, which leaves a block in natural order: element t of block b is output
// u = (t << (m - 7)) | brp_(m-7)(b). k_kzg_g1_fft_order takes that to natural or to bit-reversed order, and does the inverse's 1 / n.
//   k_kzg_g1_fft_stage   a lane per butterfly, n_ffts n / 2 lanes in workgroups of 64, no LDS; the product is kzg_g1_mul_split with the
//                        lane's window table in global memory, the twiddle a row of d_kzg_g1_twiddle_wide (global memory as well)
//   k_kzg_g1_fft_order   a lane per point (at most `lanes` of them, each walking its points): the tail's order to the caller's, with the
//                        product by 2^-m for the inverse
//   k_kzg_g1_fft_load    affine points (a settings table's row 0) to Jacobian, in their order or un-bit-reversed
//   k_kzg_g1_affine      Jacobian to affine, a lane per point (a settings table's row 0)
// Every addition is the complete jadd: the point at infinity, equal and opposite points are ordinary data of a transform.
#pragma once
#include "kzg_cell_kernels.cuh"

namespace zkw {

enum : u32 { KZG_G1_FFT_WIDE_MAX = 4096, KZG_G1_FFT_WIDE_LOG = 12, KZG_G1_FFT_WIDE_HALF = 2048, KZG_G1_FFT_WIDE_POINTS = 65536 };

// grid n_ffts n / 128, one wave. x: [n_ffts][n] Jacobian points, n = 2^log_n, 8 <= log_n <= 12; stage s < log_n - 7 (so half >= 128 and the 64
// lanes of a wave are 64 consecutive j of one run). tab: KZG_G1_TAB_WORDS words a workgroup. The twiddle w_n^(j 2^s) = w4096^e, e =
// (j << s) (4096 / n) < 2048; the inverse's w4096^-e = -w4096^(2048 - e) is that row on the negated point, and e = 0 is no product
static __device__ __forceinline__ void k_kzg_g1_fft_stage(const VB& vb, bls::G1Jac* __restrict__ x, u32* tab, u32 log_n, u32 s, u32 inverse, u32 n_butterflies) {
    const u32 g = vb.x * KZG_G1_FFT_THREADS + threadIdx.x;
    if (g >= n_butterflies) return;
    u32* mine = tab + (size_t)vb.x * KZG_G1_TAB_WORDS + threadIdx.x;
    const u32 half_n = 1u << (log_n - 1), t = g & (half_n - 1), half = half_n >> s;
    const u32 j = t & (half - 1), i0 = ((t >> (log_n - 1 - s)) << (log_n - s)) | j, i1 = i0 + half;  // i1 <= n - 1
    bls::G1Jac* base = x + ((size_t)(g >> (log_n - 1)) << log_n);
    const bls::G1Jac u = base[i0], v = base[i1];
    base[i0] = bls::jadd(u, v);
    bls::G1Jac d = bls::jadd(u, bls::G1Jac{v.X, bls::neg(v.Y), v.Z});
    const u32 e = (j << s) << (KZG_G1_FFT_WIDE_LOG - log_n);  // < 2048
    if (e) {
        if (inverse) d.Y = bls::neg(d.Y);
        d = kzg_g1_mul_split(d, d_kzg_g1_twiddle_wide[inverse ? KZG_G1_FFT_WIDE_HALF - e : e], mine);
    }
    base[i1] = d;
}

// grid lanes / 64 (lanes a multiple of 64, at most n_points). in: [n_ffts][n] as the 128-point tail leaves them (log_n > 7: block b of a
// transform holds outputs (t << (log_n - 7)) | brp(b) at t; log_n <= 7: natural order); out: output u of a transform at u, or with `brp`
// at brp_(log_n)(u) (for log_n > 7 that is (b << 7) | brp7(t)). scale_row != 0: the product by that row of d_kzg_g1_twiddle_wide (2^-log_n)
// on the way. tab: KZG_G1_TAB_WORDS words a workgroup, read only with scale_row. in != out
static __device__ __forceinline__ void k_kzg_g1_fft_order(const VB& vb, const bls::G1Jac* __restrict__ in, bls::G1Jac* __restrict__ out, u32* tab, u32 log_n,
                                                          u32 n_points, u32 lanes, u32 scale_row, u32 brp) {
    u32* mine = tab + (size_t)vb.x * KZG_G1_TAB_WORDS + threadIdx.x;
    const u32 mask = (1u << log_n) - 1;
#pragma unroll 1
    for (u32 p = vb.x * KZG_G1_FFT_THREADS + threadIdx.x; p < n_points; p += lanes) {
        const u32 k = p & mask;
        u32 u = k;
        if (log_n > 7) u = ((k & 127u) << (log_n - 7)) | kzg_brp(k >> 7, log_n - 7);
        if (brp) u = kzg_brp(u, log_n);
        bls::G1Jac v = in[p];
        if (scale_row) v = kzg_g1_mul_split(v, d_kzg_g1_twiddle_wide[scale_row], mine);
        out[(p & ~mask) | u] = v;  // u < n
    }
}

// a lane per point: out[k] = in[k], or with `brp` in[brp_(log_n)(k)], as a Jacobian point (infinity is (0, 0) in a table)
static __device__ __forceinline__ void k_kzg_g1_fft_load(const VB& vb, const bls::G1Aff* __restrict__ in, u32 log_n, u32 brp, bls::G1Jac* __restrict__ out) {
    const u32 k = vb.x * blockDim.x + threadIdx.x;
    if (k >> log_n) return;
    const u32 from = brp ? kzg_brp(k, log_n) : k;
    const bls::Fq ax = in[from].x, ay = in[from].y;  // (as k_kzg_g1_lift: field by field, nothing on the stack)
    out[k].X = ax;
    out[k].Y = ay;
    out[k].Z = bls::is_zero(ax) && bls::is_zero(ay) ? bls::zero<bls::FqT>() : bls::one<bls::FqT>();
}

// a lane per point: to affine (infinity becomes (0, 0) and contributes nothing to a sum)
static __device__ __forceinline__ void k_kzg_g1_affine(const VB& vb, const bls::G1Jac* __restrict__ in, u32 n, bls::G1Aff* __restrict__ out) {
    const u32 k = vb.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    out[k] = bls::to_affine(in[k]);
}

}  // namespace zkw
