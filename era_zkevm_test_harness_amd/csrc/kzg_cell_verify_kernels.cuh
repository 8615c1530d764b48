// kzg_cell_verify_kernels.cuh — the verification of EIP-7594 cell proofs (verify_cell_kzg_proof_batch of the consensus specs, a verdict per
// claim) on gfx950, on top of kzg_cell_kernels.cuh and kzg_verify_kernels.cuh.
//
// With W = 7^((r - 1) / 8192), c_k = w128^brp7(k) and h_k = W^brp7(k) (h_k^64 = c_k): cell k holds p at the 64 roots of X^64 - c_k, in the
// order h_k w64^brp6(t), w64 = W^128, and I_k is the polynomial of degree below 64 through them. Then p = q_k (X^64 - c_k) + I_k and
// pi_k = [q_k(tau)] G1, so the claim "(C, k, cell, pi)" holds exactly when
//     e(C - [I_k(tau)] G1 + [c_k] pi, -G2) e(pi, [tau^64] G2) = 1
// — kzg_verify_kernels.cuh's equation with [y] G1 replaced by the commitment of I_k, z by c_k and the second G2 point by [tau^64] G2. Both
// G2 points are still fixed: a zkw_kzg_verifier made from [tau^64] G2 is the line table, and k_kzg_verify_pairing runs as it is.
//   k_kzg_cell_interpolate    a wave per claim: the 64 elements range-checked while they are loaded; b_i = I_k[i] h_k^i is the inverse
//                             transform of the cell over w64, and the cell's order is the order a decimation-in-frequency transform
//                             leaves, so its six stages undone last first (kzg_fr_intt4096's form) take the cell as it is and leave b in
//                             natural order: no permutation pass. Then I_k[i] = b_i / (64 h_k^i), h_k^-i = W^(8192 - brp7(k) i) from
//                             k_kzg_cell_wpow's table (W^(4096 + m) = -W^m): no inversion and no power chain. Out as the 2 048 digit
//                             bytes k_kzg_cell_msm reads, and a status word per claim
//   k_kzg_cell_commit_msm     k_kzg_cell_msm's body (kzg_cell_kernels.cuh) over columns 0..63 of the SETTINGS' table, table[w n_points + i]:
//                             a workgroup per claim, the eight bit sums of [I_k(tau)] G1; k_kzg_cell_horner follows as it is
//   k_kzg_verify_cell_points  a lane per claim, the sibling of k_kzg_verify_points: C and pi decompressed and checked, the statuses merged,
//                             P1 = [c_k] pi + C - I_k by one double-and-add walk over the one scalar c_k, to affine by one inversion
// As in kzg_open_kernels.cuh the Fr twiddles are in Montgomery form and the running values PLAIN. Every kernel is a body for both launch forms.
#pragma once
#include "kzg_cell_kernels.cuh"
#include "kzg_verify_kernels.cuh"

namespace zkw {

enum : int { KZG_CELL_INTERP_THREADS = 256, KZG_CELL_INTERP_CLAIMS = KZG_CELL_INTERP_THREADS / 64 };
// k_kzg_cell_interpolate's status word: 0, or KZG_CELL_ST_BAD_INDEX (the index is not below 128; every element is below r), or
// KZG_CELL_ST_BAD_ELEMENT + e for the LOWEST element e that is not below r (whatever the index is: the lower verdict code wins)
enum : u32 { KZG_CELL_ST_OK = 0, KZG_CELL_ST_BAD_INDEX = 1, KZG_CELL_ST_BAD_ELEMENT = 2 };

// the cell index of claim i: 8 little-endian bytes at any address, both words read. *k: the index when it is below 128, else its low 7 bits
// (so that what follows stays inside its tables)
static __device__ __forceinline__ bool kzg_cell_index(const uint8_t* __restrict__ indices, size_t i, u32* k) {
    const uint8_t* b = indices + 8 * i;
    const u32 lo = (u32)b[0] | ((u32)b[1] << 8) | ((u32)b[2] << 16) | ((u32)b[3] << 24);
    const u32 hi = (u32)b[4] | ((u32)b[5] << 8) | ((u32)b[6] << 16) | ((u32)b[7] << 24);
    *k = lo & (KZG_CELLS - 1);
    return hi == 0 && lo < KZG_CELLS;
}

// grid ceil(n / 4), 256 lanes: wave v of workgroup g takes claim 4 g + v (a wave past the end repeats the last claim and stores nothing).
// indices: [n] of 8 bytes; cells: [n][2048], element t of a cell as 32 big-endian bytes, any address; tw: k_kzg_twiddles' table (w64^e =
// tw[64 e]); wpow: k_kzg_cell_wpow's. c: [n][64][32], I_k[i] as 32 little-endian bytes (16-byte aligned); status: [n]. A claim whose status
// is not 0 gets digits all the same (of no meaning, and nothing downstream may use them)
static __device__ __forceinline__ void k_kzg_cell_interpolate(const VB& vb, const uint8_t* __restrict__ indices, const uint8_t* __restrict__ cells, u32 n,
                                                              const bls::Fr* __restrict__ tw, const bls::Fr* __restrict__ wpow, uint8_t* __restrict__ c,
                                                              u32* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint4 lds[KZG_CELL_INTERP_CLAIMS * 2 * KZG_CELL_ELEMENTS];
    const u32 wave = threadIdx.x >> 6, l = threadIdx.x & 63u, claim = vb.x * KZG_CELL_INTERP_CLAIMS + wave;
    const u32 at = claim < n ? claim : n - 1;  // (n >= 1)
    uint4* x = lds + wave * 2 * KZG_CELL_ELEMENTS;
    u32 k;
    const bool index_ok = kzg_cell_index(indices, at, &k);
    const bool aligned = (reinterpret_cast<uintptr_t>(cells) & 3) == 0;  // (a caller's device pointer may be odd)
    const bls::Fr e = kzg_get_be32(cells + (size_t)at * KZG_CELL_BYTES + 32 * l, aligned);
    const unsigned long long bad = __ballot(!bls::below_modulus<bls::FrT>(e.w));
    if (l == 0 && claim < n) status[claim] = bad ? KZG_CELL_ST_BAD_ELEMENT + (u32)(__ffsll(bad) - 1) : index_ok ? KZG_CELL_ST_OK : KZG_CELL_ST_BAD_INDEX;
    kzg_lds_put(x, l, e);
    __syncthreads();
    // the six stages of the 64-point transform undone, last first: butterfly b < 32 of stage s (half-width h = 32 >> s) has j = b mod h and
    // pairs i0 = (b div h) 2 h + j with i1 = i0 + h; forward it sent (u, v) to (a, d) = (u + v, (u - v) w64^e), e = j 2^s, so
    // (2 u, 2 v) = (a + d w64^-e, a - d w64^-e) and w64^-e = -w64^(32 - e): the same table with add and sub exchanged, for e = 0 as they are
#pragma unroll 1
    for (u32 s = 6; s-- > 0;) {
        if (l < 32) {
            const u32 half = 32u >> s;
            const u32 j = l & (half - 1), i0 = ((l >> (5 - s)) << (6 - s)) | j, i1 = i0 + half;  // i1 <= 63
            const bls::Fr u = kzg_lds_get(x, i0);
            bls::Fr m = kzg_lds_get(x, i1);
            if (s < 5) m = bls::mul<bls::FrT>(m, tw[((32u - (j << s)) & 31u) * 64u]);  // index <= 31 * 64 (the first stage undone has no twiddle but 1)
            const bls::Fr with = bls::add(u, m), without = bls::sub(u, m);
            kzg_lds_put(x, i0, bls::select(j == 0, with, without));
            kzg_lds_put(x, i1, bls::select(j == 0, without, with));
        }
        __syncthreads();
    }
    // x[l] = 64 b_l. 1 / 64 in Montgomery form is 2^256 / 2^6 = 2^250, which is below r as it stands; h_k^-l = W^ex, ex = 8192 - brp7(k) l
    // (brp7(k) l <= 127 * 63 < 8192) or 0, and W^(4096 + m) = -W^m
    bls::Fr inv_width = bls::zero<bls::FrT>();
    inv_width.w[7] = 1u << 26;
    const u32 down = kzg_brp(k, 7) * l, ex = down ? 8192u - down : 0u;  // < 8192
    bls::Fr a = bls::mul<bls::FrT>(bls::mul<bls::FrT>(kzg_lds_get(x, l), inv_width), wpow[ex & 4095u]);
    a = bls::select(ex >= 4096u, bls::neg(a), a);
    if (claim < n) kzg_lds_put(reinterpret_cast<uint4*>(c), (size_t)claim * KZG_CELL_ELEMENTS + l, a);
}

// grid n claims, 256 lanes: the eight bit sums of sum_i I_k[i] S[i] for claim vb.x. c: k_kzg_cell_interpolate's rows; table: the settings'
// byte-window table [32][n_points], n_points >= 64, of which columns 0..63 are read; sums: [n][8]
struct KzgSettingsColumns {
    u32 n_points;
    __device__ __forceinline__ size_t operator()(u32 w, u32 i) const { return (size_t)w * n_points + i; }  // w < 32, i < 64 <= n_points
};
static __device__ __forceinline__ void k_kzg_cell_commit_msm(const VB& vb, const uint8_t* __restrict__ c, const bls::G1Aff* __restrict__ table, u32 n_points,
                                                             bls::G1Jac* __restrict__ sums) {
    kzg_cell_msm_sum(vb.x, KzgSettingsColumns{n_points}, c, table, sums);
}

// a lane per claim. hs: [n] Jacobian, [I_k(tau)] G1 of k_kzg_cell_horner; interp: k_kzg_cell_interpolate's status words. pts and status:
// what k_kzg_verify_pairing reads — pts [n][2] = (P1, pi), affine in Montgomery form, zeros when the claim's status is not 0; status [n], 0
// or the verdict code of the first rule the claim breaks (2 commitment, 3 proof, 4 a cell element not below r, 5 the index)
static __device__ __forceinline__ void k_kzg_verify_cell_points(const VB& vb, const uint8_t* __restrict__ commitments, const uint8_t* __restrict__ indices,
                                                                const uint8_t* __restrict__ proofs, const u32* __restrict__ interp,
                                                                const bls::G1Jac* __restrict__ hs, const bls::Fr* __restrict__ tw, u32 n,
                                                                bls::G1Aff* __restrict__ pts, u32* __restrict__ status) {
    const u32 i = vb.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 k;
    (void)kzg_cell_index(indices, i, &k);
    bls::G1Aff c, pi;
    u32 st = 0;
    const u32 ist = interp[i];
    if (!kzg_point_in(commitments + 48 * (size_t)i, &c)) st = KZG_VERDICT_BAD_COMMITMENT;
    else if (!kzg_point_in(proofs + 48 * (size_t)i, &pi)) st = KZG_VERDICT_BAD_PROOF;
    else if (ist >= KZG_CELL_ST_BAD_ELEMENT) st = KZG_VERDICT_BAD_SCALAR;
    else if (ist == KZG_CELL_ST_BAD_INDEX) st = KZG_VERDICT_BAD_INDEX;
    status[i] = st;
    if (st) {
        const bls::G1Aff none{bls::zero<bls::FqT>(), bls::zero<bls::FqT>()};
        pts[2 * (size_t)i] = none;
        pts[2 * (size_t)i + 1] = none;
        return;
    }
    // c_k = w128^brp7(k) as a plain scalar: w128^m = w^(32 m) for m < 64 (index <= 32 * 63), and w128^(64 + m) = -w128^m
    const u32 m = kzg_brp(k, 7);
    bls::Fr ck = bls::from_mont(tw[(m & 63u) * 32u]);
    ck = bls::select(m >= 64u, bls::neg(ck), ck);
    bls::G1Jac acc = bls::jac_inf();
#pragma unroll 1
    for (int wi = 7; wi >= 0; wi--) {
        const u32 zw = kzg_pop_word(ck);
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            acc = bls::jdbl(acc);
            if ((zw >> bit) & 1) acc = bls::jmadd(acc, pi);
        }
    }
    acc = bls::jmadd(acc, c);
    {
        const bls::G1Jac h = hs[i];
        acc = bls::jadd(acc, bls::G1Jac{h.X, bls::neg(h.Y), h.Z});  // (complete: I_k = O for an all-zero cell, P1 = O for a constant)
    }
    pts[2 * (size_t)i] = bls::to_affine(acc);
    pts[2 * (size_t)i + 1] = pi;
}

}  // namespace zkw
