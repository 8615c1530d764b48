// kzg_recover_kernels.cuh — EIP-7594 recovery on gfx950, on top of kzg_cell_kernels.cuh: the polynomial of a blob (and with it all 128 cells
// and, by the FK20 path as it is, all 128 cell proofs) from any 64 or more of its cells (recover_cells_and_kzg_proofs of the consensus specs).
//
// Notation of kzg_cell_kernels.cuh: W = 7^((r - 1) / 8192), w = W^2, w128 = w^32, position j of the extended blob holds p(W^brp13(j)), cell k
// = positions 64 k .. 64 k + 63, the roots of X^64 - c_k, c_k = w128^brp7(k). Position 4096 h + i is the point W^h w^brp12(i): each half of
// the extended blob is a coset of the blob's own domain, in the blob's order. With M the missing cells, z(Y) = prod_(k in M) (Y - c_k)
// (degree <= 64) and Z(X) = z(X^64): Z vanishes on the missing cells, E Z is known at all 8 192 points (zero where a cell is absent), and its
// interpolant D = P Z has degree below 8 192. P = D / Z is taken on the coset s w^i, s = 7, where Z has no zero (s^8192 != 1) and takes only
// 64 different values, z(s^64 w128^(2 u)), u = brp12(i') mod 64. No transform of 8 192 points is formed (it would not fit the LDS):
//   k_kzg_recover_vanish    a wave per call: the <= 65 coefficients of z, then two transforms of 128 points (kzg_fr_ntt128,
//                           kzg_open_kernels.cuh): z(w128^brp7(k)) = z(c_k) comes out at position k, the factor of cell k; on the coefficients
//                           scaled by s^(64 m), z(s^64 w128^(2 u)) comes out at position brp6(u) < 64, inverted a lane each (Fermat)
//   k_kzg_recover_halves    a workgroup per (blob, half h): positions 4096 h .. 4096 h + 4095 of E Z (range-checked while they are loaded),
//                           the twelve stages undone (kzg_fr_intt4096); half 0 is a = D mod (X^4096 - 1), half 1 after the unscaling by W^-i
//                           (= -W^(4096 - i): k_kzg_cell_wpow's table backwards, the sign changed) is b = D mod (X^4096 + 1)
//   k_kzg_recover_quotient  a workgroup per blob: F = D mod (X^4096 - s^4096) = a (1 + s^4096) / 2 + b (1 - s^4096) / 2, scaled by s^i, kzg_fr_ntt4096
//                           (position i' then holds F(s w^brp12(i'))), times 1 / Z there — inverse number brp6(i' >> 6), 64
//                           neighbours share one —, the twelve stages undone, unscaled by s^-i: the coefficients of P as rows of 32
//                           little-endian bytes (KzgSrc form 0). No permutation pass anywhere.
//   k_kzg_recover_check     after k_kzg_cells on those coefficients: every supplied cell against the recomputed one, byte for byte. Equal
//                           means the polynomial of degree below 4 096 passes through all supplied cells, and through 64 or more it is unique.
// The running values are PLAIN and the factors (z(c_k), 1 / Z, the powers of s and W, the fold constants) in Montgomery form, as in
// kzg_open_kernels.cuh; inside k_kzg_recover_vanish everything is in Montgomery form. Every kernel is a body for both launch forms.
#pragma once
#include "kzg_cell_kernels.cuh"

namespace zkw {

enum : u32 { KZG_RECOVER_ABSENT = 0xff };
enum : int { KZG_RECOVER_VANISH_THREADS = 64, KZG_RECOVER_CHECK_THREADS = 256 };

// slot[k]: the position of cell k in the call's list, KZG_RECOVER_ABSENT for a missing cell. It travels as a kernel argument (a body takes
// it by reference: zkw_launch.h)
struct KzgSlots {
    uint8_t slot[KZG_CELLS];
};

// the shift s = 7 (the generator the roots of unity are powers of: s^8192 != 1), in Montgomery form
static __device__ __forceinline__ bls::Fr kzg_recover_s() {
    const bls::Fr one = bls::one<bls::FrT>(), two = bls::add(one, one), four = bls::add(two, two);
    return bls::add(bls::add(four, two), one);
}
// 1 / s, and the fold constants (1 + s^4096) / (2 * 4096^2) and (1 - s^4096) / (2 * 4096^2): the 1 / 2 of the two residues and the 1 / 4096
// of both inverse transforms (Montgomery form; tests/test_kzg_recover_model.py checks the words against these definitions)
static __device__ __forceinline__ bls::Fr kzg_recover_s_inv() {
    return bls::Fr{{0xdb6db6dcu, 0xdb6db6dau, 0xdb6cc6dau, 0xe6b5824au, 0x05810db9u, 0xf8b356e0u, 0x60ec4796u, 0x66d0f1e6u}};
}
static __device__ __forceinline__ bls::Fr kzg_recover_fold_a() {
    return bls::Fr{{0xc513d2f4u, 0xe650a823u, 0xaed0835au, 0x8752af84u, 0xb955de69u, 0x6c809273u, 0x07c3c617u, 0x12417736u}};
}
static __device__ __forceinline__ bls::Fr kzg_recover_fold_b() {
    return bls::Fr{{0x3aec2d0du, 0x19af57dbu, 0x512dd8a4u, 0xcc6af47eu, 0x504bf99bu, 0xc6b94594u, 0x21d9b730u, 0x61ac311du}};
}

static __device__ __forceinline__ bls::Fr kzg_recover_sqr_n(bls::Fr v, int n) {  // v^(2^n)
#pragma unroll 1
    for (int k = 0; k < n; k++) v = bls::sqr(v);
    return v;
}

// grid 1, 64 lanes. zc: [128], zc[k] = z(c_k) — zero exactly on the missing cells; zinv: [64], zinv[u] = 1 / z(s^64 w128^(2 u)) (both in
// Montgomery form). tw: k_kzg_twiddles' table. At most 64 cells are missing (the caller's count check), so z has at most 65 coefficients;
// lane l keeps z[l]
static __device__ __forceinline__ void k_kzg_recover_vanish(const VB& vb, const KzgSlots& slots, const bls::Fr* __restrict__ tw, bls::Fr* __restrict__ zc,
                                                            bls::Fr* __restrict__ zinv) {
    __shared__ __attribute__((aligned(16))) uint4 x[2 * KZG_CELLS];
    const u32 l = threadIdx.x;  // < 64
    bls::Fr lo = l ? bls::zero<bls::FrT>() : bls::one<bls::FrT>();
    kzg_lds_put(x, l, lo);
    kzg_lds_put(x, 64 + l, bls::zero<bls::FrT>());
    __syncthreads();
    u32 missing = 0;
#pragma unroll 1
    for (u32 k = 0; k < KZG_CELLS; k++) {  // z <- z (Y - c_k): z[m] <- z[m - 1] - c_k z[m], m < 64
        if (slots.slot[k] != KZG_RECOVER_ABSENT) continue;  // (the same for every lane)
        missing++;
        const u32 u = kzg_brp(k, 7);
        bls::Fr c = tw[32u * (u & 63u)];  // w128^u = w^(32 u), and w128^64 = -1
        if (u >= 64) c = bls::neg(c);
        const bls::Fr below = l ? kzg_lds_get(x, l - 1) : bls::zero<bls::FrT>();
        __syncthreads();
        lo = bls::sub(below, bls::mul<bls::FrT>(lo, c));
        kzg_lds_put(x, l, lo);
        __syncthreads();
    }
    // z is monic of degree `missing` <= 64: of the upper half only z[64] can be other than zero, and it is 1 when 64 cells are missing
    const bls::Fr hi = l == 0 && missing == 64 ? bls::one<bls::FrT>() : bls::zero<bls::FrT>();
    kzg_lds_put(x, 64 + l, hi);
    __syncthreads();
    kzg_fr_ntt128(x, l, tw);
    zc[l] = kzg_lds_get(x, l);  // position k: z(w128^brp7(k)) = z(c_k)
    zc[64 + l] = kzg_lds_get(x, 64 + l);
    __syncthreads();
    const bls::Fr s64 = kzg_recover_sqr_n(kzg_recover_s(), 6);
    const bls::Fr pl = kzg_fr_pow(s64, l, 6);  // s^(64 l)
    kzg_lds_put(x, l, bls::mul<bls::FrT>(lo, pl));
    kzg_lds_put(x, 64 + l, bls::mul<bls::FrT>(hi, bls::mul<bls::FrT>(pl, kzg_recover_sqr_n(s64, 6))));  // s^(64 (64 + l))
    __syncthreads();
    kzg_fr_ntt128(x, l, tw);
    // position q < 64: z(s^64 w128^brp7(q)) and brp7(q) = 2 brp6(q). Never zero: s^64 w128^e is no 128th root of unity
    zinv[kzg_brp(l, 6)] = bls::fr_inv(kzg_lds_get(x, l));
}

// grid (n_blobs, 2), 512 lanes, KZG_NTT_LDS bytes of dynamic LDS. cells: [n_blobs][n_cells][2048] big-endian, any address, the cells of the
// list in its order (slots.slot[k] < n_cells wherever it is not absent). Half h = vb.y: x[i] = E[4096 h + i] z(c_k), k = 64 h + (i >> 6), zero
// for an absent cell; then kzg_fr_intt4096. ab: [n_blobs][2][4096] plain elements (32-byte aligned): 4096 a and 4096 b.
// status[2 blob + h]: 0, or 1 + the LOWEST 64 (position in the list) + element of a supplied element that is not below r (the values
// written are then meaningless; the caller refuses the call)
static __device__ __forceinline__ void k_kzg_recover_halves(const VB& vb, const KzgSlots& slots, const uint8_t* __restrict__ cells, u32 n_cells,
                                                            const bls::Fr* __restrict__ zc, const bls::Fr* __restrict__ tw, const bls::Fr* __restrict__ wpow,
                                                            uint8_t* __restrict__ ab, u32* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint4 kzg_recover_lds[];
    __shared__ u32 s_bad;
    uint4* x = kzg_recover_lds;
    const u32 t = threadIdx.x, h = vb.y;
    if (t == 0) s_bad = ~0u;
    __syncthreads();
    const uint8_t* mine = cells + (size_t)vb.x * n_cells * KZG_CELL_BYTES;
    const bool aligned = (reinterpret_cast<uintptr_t>(cells) & 3) == 0;  // (a caller's device pointer may be odd; a blob's cells are a multiple of 4 bytes)
#pragma unroll 1
    for (u32 i = t; i < 4096; i += KZG_NTT_THREADS) {
        const u32 k = 64u * h + (i >> 6), slot = slots.slot[k];  // k < 128
        bls::Fr f = bls::zero<bls::FrT>();
        if (slot != KZG_RECOVER_ABSENT) {
            const u32 e = 64u * slot + (i & 63u);  // < 64 n_cells
            f = kzg_get_be32(mine + 32 * (size_t)e, aligned);
            if (!bls::below_modulus<bls::FrT>(f.w)) atomicMin(&s_bad, e);
            f = bls::mul<bls::FrT>(f, zc[k]);
        }
        kzg_lds_put(x, i, f);
    }
    __syncthreads();
    if (t == 0) status[2 * vb.x + h] = s_bad + 1u;
    kzg_fr_intt4096(x, t, tw);
    // half 1 holds the coefficients of D(W X) mod (X^4096 - 1), b_i W^i: W^-i = W^(8192 - i) = -W^(4096 - i) for i >= 1 (W^4096 = -1)
    uint4* out = reinterpret_cast<uint4*>(ab + ((size_t)vb.x * 2 + h) * KZG_EVAL_BYTES);
#pragma unroll 1
    for (u32 k = t; k < 4096; k += KZG_NTT_THREADS) {
        bls::Fr v = kzg_lds_get(x, k);
        if (h && k) v = bls::neg(bls::mul<bls::FrT>(v, wpow[4096u - k]));  // index 1 .. 4095
        kzg_lds_put(out, k, v);
    }
}

// grid n_blobs, 512 lanes, KZG_NTT_LDS bytes of dynamic LDS. ab: k_kzg_recover_halves' rows; zinv: k_kzg_recover_vanish's; coeffs:
// [n_blobs][4096][32] little-endian, row k = the coefficient of X^k (KzgSrc{.., 4096, 0}), 16-byte aligned. Lane t owns the elements
// t + 512 m, so its powers of s are s^t (s^512)^m. inconsistent[blob] is cleared for k_kzg_recover_check
static __device__ __forceinline__ void k_kzg_recover_quotient(const VB& vb, const uint8_t* __restrict__ ab, const bls::Fr* __restrict__ zinv,
                                                              const bls::Fr* __restrict__ tw, uint8_t* __restrict__ coeffs, u32* __restrict__ inconsistent) {
    extern __shared__ __attribute__((aligned(16))) uint4 kzg_recover_lds[];
    uint4* x = kzg_recover_lds;
    const u32 t = threadIdx.x;
    if (t == 0) inconsistent[vb.x] = 0;
    const uint4* a = reinterpret_cast<const uint4*>(ab + (size_t)vb.x * 2 * KZG_EVAL_BYTES);
    const uint4* b = reinterpret_cast<const uint4*>(ab + ((size_t)vb.x * 2 + 1) * KZG_EVAL_BYTES);
    {
        const bls::Fr fa = kzg_recover_fold_a(), fb = kzg_recover_fold_b(), s = kzg_recover_s(), step = kzg_recover_sqr_n(s, 9);
        bls::Fr sp = kzg_fr_pow(s, t, 9);
#pragma unroll 1
        for (u32 i = t; i < 4096; i += KZG_NTT_THREADS) {  // F_i s^i
            const bls::Fr f = bls::add(bls::mul<bls::FrT>(kzg_lds_get(a, i), fa), bls::mul<bls::FrT>(kzg_lds_get(b, i), fb));
            kzg_lds_put(x, i, bls::mul<bls::FrT>(f, sp));
            sp = bls::mul<bls::FrT>(sp, step);
        }
    }
    __syncthreads();
    kzg_fr_ntt4096(x, t, tw);  // position i' <- F(s w^brp12(i'))
#pragma unroll 1
    for (u32 i = t; i < 4096; i += KZG_NTT_THREADS)  // Z(s w^e) = z(s^64 w128^(2 (e mod 64))), and brp12(i') mod 64 = brp6(i' >> 6)
        kzg_lds_put(x, i, bls::mul<bls::FrT>(kzg_lds_get(x, i), zinv[kzg_brp(i >> 6, 6)]));
    __syncthreads();
    kzg_fr_intt4096(x, t, tw);
    uint4* out = reinterpret_cast<uint4*>(coeffs + (size_t)vb.x * KZG_EVAL_BYTES);
    const bls::Fr s_inv = kzg_recover_s_inv(), step = kzg_recover_sqr_n(s_inv, 9);
    bls::Fr sp = kzg_fr_pow(s_inv, t, 9);
#pragma unroll 1
    for (u32 i = t; i < 4096; i += KZG_NTT_THREADS) {  // P_i s^i -> P_i
        kzg_lds_put(out, i, bls::mul<bls::FrT>(kzg_lds_get(x, i), sp));
        sp = bls::mul<bls::FrT>(sp, step);
    }
}

// grid (128, n_blobs), 256 lanes of 8 bytes: cell k = vb.x of blob vb.y as supplied against the same cell of `full` ([n_blobs][128][2048],
// k_kzg_cells on the recovered coefficients; any address). inconsistent[blob] (cleared by k_kzg_recover_quotient) is set on a difference
static __device__ __forceinline__ void k_kzg_recover_check(const VB& vb, const KzgSlots& slots, const uint8_t* __restrict__ cells, u32 n_cells,
                                                           const uint8_t* __restrict__ full, u32* __restrict__ inconsistent) {
    const u32 slot = slots.slot[vb.x];  // vb.x < 128
    if (slot == KZG_RECOVER_ABSENT) return;
    const uint8_t* a = cells + ((size_t)vb.y * n_cells + slot) * KZG_CELL_BYTES + 8 * threadIdx.x;  // 256 lanes x 8 bytes = 2048
    const uint8_t* b = full + ((size_t)vb.y * KZG_CELLS + vb.x) * KZG_CELL_BYTES + 8 * threadIdx.x;
    bool differ = false;
    if (((reinterpret_cast<uintptr_t>(cells) | reinterpret_cast<uintptr_t>(full)) & 3) == 0) {
        const u32 *wa = reinterpret_cast<const u32*>(a), *wb = reinterpret_cast<const u32*>(b);
        differ = wa[0] != wb[0] || wa[1] != wb[1];
    } else {
#pragma unroll
        for (int m = 0; m < 8; m++) differ = differ || a[m] != b[m];
    }
    if (differ) inconsistent[vb.y] = 1u;
}

}  // namespace zkw
