// kzg_verify_kernels.cuh — the verification of KZG proofs (verify_kzg_proof, kzg/src/lib.rs:259-282 of the reference) on gfx950, on top
// of kzg_open_kernels.cuh and bls12_381_pairing.cuh.
//
// The claim "p(z) = y for the polynomial behind C, by the proof pi" holds exactly when
//     e(C - [y] G1 + [z] pi, -G2) e(pi, [tau] G2) = 1
// (the reference subtracts [z] G2 from [tau] G2 instead; moving [z] to the other side keeps BOTH G2 points fixed, so every run-time
// scalar multiplication is in G1 and the G2 work happens once per verifier handle):
//   k_kzg_g2_prepare      once per handle, a lane per point (-G2 from constant memory, [tau] G2 from the caller): decompression, the
//                         twist and subgroup checks, the 68 lines of the Miller loop as (lam, lam xT - yT), 26 KB in HBM for the two
//   k_kzg_verify_points   a lane per claim: C and pi decompressed and checked (curve, subgroup), z and y below r, then
//                         P1 = C - [y] G1 + [z] pi by one double-and-add walk over both scalars, to affine; a status per claim
//   k_kzg_verify_pairing  8 lanes per claim, 8 claims a wave (the layout of bls12_381_pairing.cuh): the Miller functions of the two
//                         pairs on one accumulator, one final exponentiation, the comparison with one, the verdict byte. A pair whose
//                         G1 point is infinity contributes the factor 1 (a constant polynomial has pi = O and P1 = O)
// Every kernel is a body for both launch forms (zkw_launch.h).
#pragma once
#include "bls12_381_pairing.cuh"
#include "kzg_open_kernels.cuh"

namespace zkw {

enum : int { KZG_VFY_THREADS = 64, KZG_VFY_CLAIMS_PER_BLOCK = KZG_VFY_THREADS / bls::F12_LANES };
// a verdict byte; the lowest applicable code above 1 wins (5: zkw_kzg_verify_cells alone, a cell index that is not below 128)
enum : u32 { KZG_VERDICT_FAILS = 0, KZG_VERDICT_HOLDS = 1, KZG_VERDICT_BAD_COMMITMENT = 2, KZG_VERDICT_BAD_PROOF = 3, KZG_VERDICT_BAD_SCALAR = 4,
             KZG_VERDICT_BAD_INDEX = 5 };
enum : int { KZG_G2_INFINITY = 6 };  // k_kzg_g2_prepare's status beside bls::G1_OK .. G1_NOT_IN_SUBGROUP

// -G2 for the standard generator G2 (G2Affine::one() of the reference), compressed
static __constant__ uint8_t c_kzg_neg_g2[96] = {
    0xb3, 0xe0, 0x2b, 0x60, 0x52, 0x71, 0x9f, 0x60, 0x7d, 0xac, 0xd3, 0xa0, 0x88, 0x27, 0x4f, 0x65, 0x59, 0x6b, 0xd0, 0xd0, 0x99, 0x20, 0xb6, 0x1a,
    0xb5, 0xda, 0x61, 0xbb, 0xdc, 0x7f, 0x50, 0x49, 0x33, 0x4c, 0xf1, 0x12, 0x13, 0x94, 0x5d, 0x57, 0xe5, 0xac, 0x7d, 0x05, 0x5d, 0x04, 0x2b, 0x7e,
    0x02, 0x4a, 0xa2, 0xb2, 0xf0, 0x8f, 0x0a, 0x91, 0x26, 0x08, 0x05, 0x27, 0x2d, 0xc5, 0x10, 0x51, 0xc6, 0xe4, 0x7a, 0xd4, 0xfa, 0x40, 0x3b, 0x02,
    0xb4, 0x51, 0x0b, 0x64, 0x7a, 0xe3, 0xd1, 0x77, 0x0b, 0xac, 0x03, 0x26, 0xa8, 0x05, 0xbb, 0xef, 0xd4, 0x80, 0x56, 0xc8, 0xc1, 0x21, 0xbd, 0xb8};

// the standard generator G1 (G1Affine::one() of the reference), Montgomery form
static __device__ __forceinline__ bls::G1Aff kzg_g1_generator() {
    return bls::G1Aff{
        bls::Fq{{0xfd530c16u, 0x5cb38790u, 0x9976fff5u, 0x7817fc67u, 0x143ba1c1u, 0x154f95c7u, 0xf3d0e747u, 0xf0ae6acdu, 0x21dbf440u, 0xedce6eccu, 0x9e0bfb75u, 0x12017741u}},
        bls::Fq{{0x0ce72271u, 0xbaac93d5u, 0x7918fd8eu, 0x8c22631au, 0x570725ceu, 0xdd595f13u, 0x50405194u, 0x51ac5829u, 0xad0059c0u, 0x0e1c8c3fu, 0x5008a26au, 0x0bbc3efcu}}};
}

// grid 1, 64 lanes (two at work). lines: [2][G2_LINES], point 0 = -G2, point 1 = the caller's 96 bytes; status: [2]
static __device__ __forceinline__ void k_kzg_g2_prepare(const VB& vb, const uint8_t* __restrict__ tau_g2, bls::G2Line* __restrict__ lines, u32* __restrict__ status) {
    const u32 p = vb.x * blockDim.x + threadIdx.x;
    if (p >= 2) return;
    const uint8_t* in = p ? tau_g2 : c_kzg_neg_g2;
    bls::G2Aff q;
    int st = bls::g2_decompress(in, &q);
    if (st == bls::G1_OK && bls::is_inf(q)) st = KZG_G2_INFINITY;
    if (st == bls::G1_OK && !bls::g2_prepare(q, lines + p * bls::G2_LINES)) st = bls::G1_NOT_IN_SUBGROUP;
    status[p] = (u32)st;
}

// where the claims of a call are. records == 0: four arrays, claim i at commitments + 48 i, points + 32 i and values + 32 i (32
// little-endian bytes), proofs + 48 i. records == 1: `commitments` is n / 2 zkw_eip4844_record and `proofs` n / 2
// zkw_eip4844_proof_record; claim 2 j is blob j's opening at the record's evaluation_point and opening_value, claim 2 j + 1 its blob
// proof at blob_challenge and blob_value, both against the record's commitment. records == 2 (zkw_eip4844_verify_blobs): commitments and
// proofs as in form 0, `points` and `values` inside rows of 64 bytes (the openings: challenge, value; 32 big-endian bytes each), and
// pre[i] != 0 (k_kzg_blob_eval's status: an element of blob i is not below r) makes claim i KZG_VERDICT_BAD_SCALAR when neither of its
// points is malformed
struct KzgClaims {
    const uint8_t *commitments, *points, *values, *proofs;
    u32 records;
    const u32* pre;
};

static __device__ __forceinline__ bls::Fr kzg_scalar(const uint8_t* b, u32 form) {  // KZG_Z_LE32, KZG_Z_BE16 or KZG_Z_BE32
    bls::Fr v = bls::zero<bls::FrT>();
    if (form == KZG_Z_LE32) {
#pragma unroll
        for (int j = 0; j < 8; j++) v.w[j] = (u32)b[4 * j] | ((u32)b[4 * j + 1] << 8) | ((u32)b[4 * j + 2] << 16) | ((u32)b[4 * j + 3] << 24);
    } else {
        const u32 words = form == KZG_Z_BE16 ? 4u : 8u;
#pragma unroll
        for (u32 j = 0; j < 8; j++)
            if (j < words) {
                const uint8_t* p = b + 4 * (words - 1 - j);
                v.w[j] = ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | (u32)p[3];
            }
    }
    return v;
}
static __device__ __forceinline__ u32 kzg_pop_word(bls::Fr& v) {  // the top word; the others move up (no dynamic register index)
    const u32 top = v.w[7];
#pragma unroll
    for (int j = 7; j > 0; j--) v.w[j] = v.w[j - 1];
    return top;
}
// decompression with the subgroup check: is the point acceptable?
static __device__ __forceinline__ bool kzg_point_in(const uint8_t* in, bls::G1Aff* out) {
    if (bls::decompress(in, out) != bls::G1_OK) return false;
    return bls::is_inf(*out) || bls::in_subgroup(*out);
}

// a lane per claim. pts: [n][2] = (P1, pi), affine in Montgomery form, zeros when the claim's status is not 0; status: [n], 0 or the
// verdict code of the first rule the claim breaks
static __device__ __forceinline__ void k_kzg_verify_points(const VB& vb, KzgClaims cl, u32 n, bls::G1Aff* __restrict__ pts, u32* __restrict__ status) {
    const u32 i = vb.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *cb, *pb, *zb, *yb;
    u32 z_form = KZG_Z_LE32, y_form = KZG_Z_LE32;
    if (cl.records != 1) {
        const u32 row = cl.records ? 64u : 32u;
        cb = cl.commitments + 48 * (size_t)i;
        pb = cl.proofs + 48 * (size_t)i;
        zb = cl.points + row * (size_t)i;
        yb = cl.values + row * (size_t)i;
        if (cl.records) z_form = y_form = KZG_Z_BE32;
    } else {
        const uint8_t* rec = cl.commitments + (size_t)(i >> 1) * KZG_REC_BYTES;
        const uint8_t* prf = cl.proofs + (size_t)(i >> 1) * KZG_PRF_BYTES;
        cb = rec + KZG_REC_COMMITMENT;
        pb = prf + (i & 1 ? KZG_PRF_BLOB : KZG_PRF_OPENING);
        zb = i & 1 ? prf + KZG_PRF_CHALLENGE : rec + KZG_REC_Z;
        yb = i & 1 ? prf + KZG_PRF_VALUE : rec + KZG_REC_Y;
        z_form = i & 1 ? KZG_Z_BE32 : KZG_Z_BE16;
        y_form = KZG_Z_BE32;
    }
    bls::Fr z = kzg_scalar(zb, z_form), y = kzg_scalar(yb, y_form);
    bls::G1Aff c, pi;
    u32 st = 0;
    if (!kzg_point_in(cb, &c)) st = KZG_VERDICT_BAD_COMMITMENT;
    else if (!kzg_point_in(pb, &pi)) st = KZG_VERDICT_BAD_PROOF;
    else if (!bls::below_modulus<bls::FrT>(z.w) || !bls::below_modulus<bls::FrT>(y.w)) st = KZG_VERDICT_BAD_SCALAR;
    else if (cl.records == 2 && cl.pre[i]) st = KZG_VERDICT_BAD_SCALAR;
    status[i] = st;
    const bls::G1Aff none{bls::zero<bls::FqT>(), bls::zero<bls::FqT>()};
    if (st) {
        pts[2 * (size_t)i] = none;
        pts[2 * (size_t)i + 1] = none;
        return;
    }
    // [z] pi - [y] G1 by one walk over both scalars (below r: 255 bits), then + C
    bls::G1Aff mg = kzg_g1_generator();
    mg.y = bls::neg(mg.y);
    bls::G1Jac acc = bls::jac_inf();
#pragma unroll 1
    for (int wi = 7; wi >= 0; wi--) {
        const u32 zw = kzg_pop_word(z), yw = kzg_pop_word(y);
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            acc = bls::jdbl(acc);
            if ((zw >> bit) & 1) acc = bls::jmadd(acc, pi);
            if ((yw >> bit) & 1) acc = bls::jmadd(acc, mg);
        }
    }
    acc = bls::jmadd(acc, c);
    pts[2 * (size_t)i] = bls::to_affine(acc);
    pts[2 * (size_t)i + 1] = pi;
}

// grid ceil(n / 8), 64 lanes, f12_lds_bytes(64) of dynamic LDS. lines: [2][G2_LINES] of k_kzg_g2_prepare. verdicts: [n] bytes
static __device__ __forceinline__ void k_kzg_verify_pairing(const VB& vb, const bls::G1Aff* __restrict__ pts, const u32* __restrict__ status,
                                                            const bls::G2Line* __restrict__ lines, u32 n, uint8_t* __restrict__ verdicts) {
    const bls::F12G g = bls::f12_group();
    const u32 claim = vb.x * KZG_VFY_CLAIMS_PER_BLOCK + threadIdx.x / bls::F12_LANES;
    const u32 at = claim < n ? claim : n - 1;  // (n >= 1) a group past the end repeats the last claim and stores nothing
    bls::f12_miller2(g, 0, 1, lines, lines + bls::G2_LINES, pts + 2 * (size_t)at);  // (P1, -G2), (pi, [tau] G2)
    bls::f12_final_exp(g);
    const bool holds = bls::f12_is_one(g, 0);
    if (claim < n && threadIdx.x % bls::F12_LANES == 0) {
        const u32 st = status[claim];
        verdicts[claim] = (uint8_t)(st ? st : holds ? KZG_VERDICT_HOLDS : KZG_VERDICT_FAILS);
    }
}

}  // namespace zkw
