// bls12_381_pairing.cuh — the tower Fq2, Fq12, the group G2 and the optimal-ate pairing of BLS12-381 on top of bls12_381.cuh, for the
// verification of KZG proofs (kzg_verify_kernels.cuh). Depends on nothing else in the tree, so that
// tests/csrc_gpu/bls_pairing_test.hip can run it alone against Python integers (tests/kzg_pairing_model.py).
//
// Tower and basis. Fq2 = Fq[u] / (u^2 + 1), two Fq in one lane. Fq12 = six Fq2 coefficients of w^k, w^6 = xi = 1 + u. An Fq12 is 144
// words and a lane that held two of them would spill, so ONE Fq12 IS SPREAD OVER A GROUP OF 8 LANES: lane k < 6 of the group owns the
// coefficient of w^k (lanes 6 and 7 shadow lanes 0 and 1 and never store), eight elements share a wave. The values themselves live in
// LDS, in numbered slots of 6 x 24 words per group (F12_SLOTS of them, in dynamic LDS: f12_lds_bytes), and every operation names its
// slots: a product reads a_i and b_((k - i) mod 6) straight from the slots, six Fq2 products a lane, with the xi wrap where i > k; a
// product by a line (coefficients 0, 2, 3 only) is three. mul_fq stays the one outlined product; the product of Fq12 is a loop of six
// steps around it, inlined at FIVE sites in all (f12_run's step, two in f12_pow_x, two in f12_miller2). In this basis conjugation (w -> -w), the Frobenius maps and the
// wrap are lane-local. The inversion goes through the norms: a conj(a) lies in Fq6, s s^(p^2) s^(p^4) in Fq2: one Fq inversion.
//
// G2 is the order-r subgroup of the twist y^2 = x^3 + 4 xi over Fq2, affine, a point per lane ((0, 0) is infinity). The verifier's two
// G2 points are fixed, so G2 arithmetic happens once per point: g2_prepare walks |x| = 0xd201000000010000 by AFFINE steps (one Fq2
// inversion each: a Jacobian point of G2 in a lane would spill) and leaves the 68 lines as (lam, lam xT - yT). The line through T with
// slope lam at P = (xP, yP) of G1, scaled by w^3 (in Fq4: the final exponentiation sends it to 1), is
//     (lam xT - yT)  -  lam xP w^2  +  yP w^3.
// The walk ends at [|x|] Q, and psi(Q) = [x] Q (psi: untwist, Frobenius, twist) holds exactly on the subgroup, so the membership test
// costs two products more.
//
// Final exponentiation: f12_final_exp raises to c = 3 times (p^12 - 1) / r, by
//     3 (p^4 - p^2 + 1) / r = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3,
// five powers by |x| (plain square-and-multiply in the slots), written as a program of 31 steps (c_f12_final_exp). p^4 - p^2 + 1 = 1 mod 3, so the result is one exactly when the pairing
// is. Every function that touches slots must be called by ALL lanes of the workgroup in uniform control flow (they synchronise).
#pragma once
#include "bls12_381.cuh"

namespace zkw {
namespace bls {

// ---- Fq2 ----------------------------------------------------------------------------------------------------------------------------
struct Fq2 {
    Fq c0, c1;
};
// (p - 3) / 4 and (p - 1) / 2 (the square root of Fq2), walked bit by bit
static __constant__ u32 c_fq_p34_e[12] = {0xffffeaaau, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                                          0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};
static __constant__ u32 c_fq_p12_e[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u,
                                          0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};
// w^(k (p - 1)) in Fq2 and w^(k (p^2 - 1)) in Fq, k < 6 (Montgomery form; `python -m tests.kzg_pairing_model` prints them)
static __constant__ Fq2 c_f12_gamma1[6] = {
    {{{0x0002fffdu, 0x76090000u, 0xc40c0002u, 0xebf4000bu, 0x53c758bau, 0x5f489857u, 0x70525745u, 0x77ce5853u, 0xa256ec6du, 0x5c071a97u, 0xfa80e493u, 0x15f65ec3u}}, {{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}}},
    {{{0xb319d465u, 0x07089552u, 0xb50a8313u, 0xc6695f92u, 0xd117228fu, 0x97e83cccu, 0xb2dc29eeu, 0xa35baecau, 0x5daace4du, 0x1ce393eau, 0xb0fb66ebu, 0x08f2220fu}}, {{0x4ce5d646u, 0xb2f66aadu, 0xfc497cecu, 0x5842a06bu, 0x2599d394u, 0xcf4895d4u, 0x40a8e8d0u, 0xc11b9cbau, 0xe5a0de89u, 0x2e3813cbu, 0x88847fafu, 0x110eefdau}}},
    {{{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}}, {{0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu, 0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u}}},
    {{{0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u, 0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u, 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu}}, {{0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u, 0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u, 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu}}},
    {{{0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u, 0x309b7e2cu, 0x50880866u, 0x7e881024u, 0xa20d1b8cu, 0xe2db9068u, 0x14e4f04fu, 0x1564853au, 0x14e56d3fu}}, {{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}}},
    {{{0x0dbce43fu, 0x82d83cf5u, 0xdf9d018fu, 0xa2813e53u, 0x3c65e181u, 0xc6f0caa5u, 0x8d50fe95u, 0x7525cf52u, 0xf4798a6bu, 0x4a85ed50u, 0x6cf8eebdu, 0x171da0fdu}}, {{0xf242c66cu, 0x3726c30au, 0xd1b6fe70u, 0x7c2ac1aau, 0xba4b14a2u, 0xa04007fbu, 0x66341429u, 0xef517c32u, 0x4ed2226bu, 0x0095ba65u, 0xcc86f7ddu, 0x02e370ecu}}},
};
static __constant__ Fq c_f12_gamma2[6] = {
    {{0x0002fffdu, 0x76090000u, 0xc40c0002u, 0xebf4000bu, 0x53c758bau, 0x5f489857u, 0x70525745u, 0x77ce5853u, 0xa256ec6du, 0x5c071a97u, 0xfa80e493u, 0x15f65ec3u}},
    {{0x798dba3au, 0xecfb361bu, 0x91865a2cu, 0xc100ddb8u, 0x232bda8eu, 0x0ec08ff1u, 0xf1ca4721u, 0xd5c13cc6u, 0xbf7b5c04u, 0x47222a47u, 0xe51c5f59u, 0x0110f184u}},
    {{0x798a64e8u, 0x30f1361bu, 0x7ece5a2au, 0xf3b8ddabu, 0xc61577f7u, 0x16a8ca3au, 0x74fd029bu, 0xc26a2ff8u, 0x60701c6eu, 0x3636b766u, 0x241b6160u, 0x051ba4abu}},
    {{0xfffcaaaeu, 0x43f5ffffu, 0xed47fffdu, 0x32b7fff2u, 0xa2e99d69u, 0x07e83a49u, 0x8332bb7au, 0xeca8f331u, 0xa0f4c069u, 0xef148d1eu, 0x3eff0206u, 0x040ab326u}},
    {{0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu, 0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u}},
    {{0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u, 0x309b7e2cu, 0x50880866u, 0x7e881024u, 0xa20d1b8cu, 0xe2db9068u, 0x14e4f04fu, 0x1564853au, 0x14e56d3fu}},
};
// psi(x, y) = (conj(x) / xi^((p - 1) / 3), conj(y) / xi^((p - 1) / 2)): the two factors
static __constant__ Fq2 c_g2_psi[2] = {
    {{{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}}, {{0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u, 0x309b7e2cu, 0x50880866u, 0x7e881024u, 0xa20d1b8cu, 0xe2db9068u, 0x14e4f04fu, 0x1564853au, 0x14e56d3fu}}},
    {{{0xa55c9ad1u, 0x3e2f585du, 0x86c18183u, 0x4294213du, 0x8b623732u, 0x382844c8u, 0x19103e18u, 0x92ad2afdu, 0xac7cf0b9u, 0x1d794e4fu, 0x7d825ec8u, 0x0bd592fcu}}, {{0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u, 0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u, 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu}}},
};

__device__ __forceinline__ Fq2 fq2_zero() { return Fq2{zero<FqT>(), zero<FqT>()}; }
__device__ __forceinline__ Fq2 fq2_one() { return Fq2{one<FqT>(), zero<FqT>()}; }
__device__ __forceinline__ bool is_zero(const Fq2& a) { return is_zero(a.c0) && is_zero(a.c1); }
__device__ __forceinline__ bool eq(const Fq2& a, const Fq2& b) { return eq(a.c0, b.c0) && eq(a.c1, b.c1); }
__device__ __forceinline__ Fq2 select(bool c, const Fq2& a, const Fq2& b) { return Fq2{select(c, a.c0, b.c0), select(c, a.c1, b.c1)}; }
__device__ __forceinline__ Fq2 add(const Fq2& a, const Fq2& b) { return Fq2{add(a.c0, b.c0), add(a.c1, b.c1)}; }
__device__ __forceinline__ Fq2 sub(const Fq2& a, const Fq2& b) { return Fq2{sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
__device__ __forceinline__ Fq2 neg(const Fq2& a) { return Fq2{neg(a.c0), neg(a.c1)}; }
__device__ __forceinline__ Fq2 dbl(const Fq2& a) { return Fq2{dbl(a.c0), dbl(a.c1)}; }
__device__ __forceinline__ Fq2 conj(const Fq2& a) { return Fq2{a.c0, neg(a.c1)}; }
__device__ __forceinline__ Fq2 mul_xi(const Fq2& a) { return Fq2{sub(a.c0, a.c1), add(a.c0, a.c1)}; }  // (1 + u)(c0 + c1 u)
__device__ __forceinline__ Fq2 mul_u(const Fq2& a) { return Fq2{neg(a.c1), a.c0}; }
// three products of Fq (Karatsuba)
__device__ __forceinline__ Fq2 mul(const Fq2& a, const Fq2& b) {
    const Fq v0 = mul<FqT>(a.c0, b.c0), v1 = mul<FqT>(a.c1, b.c1);
    const Fq m = mul<FqT>(add(a.c0, a.c1), add(b.c0, b.c1));
    return Fq2{sub(v0, v1), sub(sub(m, v0), v1)};
}
__device__ __forceinline__ Fq2 sqr(const Fq2& a) {  // (c0 + c1)(c0 - c1), 2 c0 c1
    const Fq m = mul<FqT>(a.c0, a.c1);
    return Fq2{mul<FqT>(add(a.c0, a.c1), sub(a.c0, a.c1)), dbl(m)};
}
__device__ __forceinline__ Fq2 scale(const Fq2& a, const Fq& s) { return Fq2{mul<FqT>(a.c0, s), mul<FqT>(a.c1, s)}; }
// conj(a) / (c0^2 + c1^2): one Fermat inversion of Fq; 0 -> 0
__device__ __forceinline__ Fq2 fq2_inv(const Fq2& a) {
    const Fq n = fq_inv(add(sqr(a.c0), sqr(a.c1)));
    return Fq2{mul<FqT>(a.c0, n), neg(mul<FqT>(a.c1, n))};
}
__device__ __forceinline__ Fq2 fq2_pow_const(const Fq2& a, const u32* e, int n_words) {
    Fq2 r = fq2_one();
#pragma unroll 1
    for (int wi = n_words - 1; wi >= 0; wi--) {
        const u32 word = e[wi];
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            r = sqr(r);
            if ((word >> bit) & 1) r = mul(r, a);
        }
    }
    return r;
}
// a square root of a when it has one (p = 3 mod 4: Adj and Rodriguez-Henriquez, algorithm 9), the same root as the host model's;
// false when a is no square
__device__ __forceinline__ bool fq2_sqrt(const Fq2& a, Fq2* out) {
    const Fq2 a1 = fq2_pow_const(a, c_fq_p34_e, 12);
    const Fq2 x0 = mul(a1, a), alpha = mul(a1, x0);
    const Fq2 minus_one = neg(fq2_one());
    const bool no_root = eq(mul(conj(alpha), alpha), minus_one);
    const Fq2 b = fq2_pow_const(add(fq2_one(), alpha), c_fq_p12_e, 12);
    const Fq2 x = select(eq(alpha, minus_one), mul_u(x0), mul(b, x0));
    *out = x;
    return !no_root && eq(sqr(x), a);
}
// the compressed form's sign of y (Montgomery form in): y above -y, comparing c1 first and c0 when c1 is zero
__device__ __forceinline__ bool fq2_is_larger(const Fq2& y) {
    const bool by_c0 = is_zero(y.c1);
    return fq_is_larger_root(from_mont(select(by_c0, y.c0, y.c1)));
}

// ---- G2, a point per lane -------------------------------------------------------------------------------------------------------------
struct G2Aff {
    Fq2 x, y;
};
struct G2Line {  // the line of one Miller step: its slope and lam xT - yT
    Fq2 lam, c;
};
enum : int { G2_LINES = 68 };                      // 63 doublings and 5 additions
enum : u64 { BLS_X_ABS = 0xd201000000010000ull };  // the curve's parameter is -BLS_X_ABS
__device__ __forceinline__ bool is_inf(const G2Aff& a) { return is_zero(a.x) && is_zero(a.y); }

__device__ __forceinline__ Fq fq_from_be48(const uint8_t* in, u32 top_mask) {
    Fq x;
#pragma unroll
    for (int i = 0; i < 12; i++)
        x.w[11 - i] = ((u32)in[4 * i] << 24) | ((u32)in[4 * i + 1] << 16) | ((u32)in[4 * i + 2] << 8) | (u32)in[4 * i + 3];
    x.w[11] &= top_mask;
    return x;
}
// the 96-byte compressed form: x.c1 then x.c0, big-endian, the flags of G1's form in byte 0. Returns G1_OK and the point, or the first
// rule the bytes break, in G1's codes (the subgroup check is g2_prepare's)
__device__ __forceinline__ int g2_decompress(const uint8_t* in, G2Aff* out) {
    out->x = fq2_zero();
    out->y = fq2_zero();
    const u32 b0 = in[0];
    if (!(b0 & 0x80)) return G1_NOT_COMPRESSED;
    if (b0 & 0x40) {
        u32 rest = b0 & 0x3F;
        for (int i = 1; i < 96; i++) rest |= in[i];
        return rest ? G1_BAD_INFINITY : G1_OK;
    }
    const Fq c1 = fq_from_be48(in, 0x1FFFFFFFu), c0 = fq_from_be48(in + 48, 0xFFFFFFFFu);
    if (!below_modulus<FqT>(c1.w) || !below_modulus<FqT>(c0.w)) return G1_X_TOO_LARGE;
    const Fq2 x{to_mont(c0), to_mont(c1)};
    Fq four = dbl(one<FqT>());
    four = dbl(four);
    const Fq2 y2 = add(mul(sqr(x), x), Fq2{four, four});  // x^3 + 4 (1 + u)
    Fq2 y;
    if (!fq2_sqrt(y2, &y)) return G1_NOT_ON_CURVE;
    if (fq2_is_larger(y) != ((b0 & 0x20) != 0)) y = neg(y);
    out->x = x;
    out->y = y;
    return G1_OK;
}
// the lines of the Miller loop of an affine point Q != O on the twist, in the order the loop uses them, and the membership test.
// Returns whether Q lies in the order-r subgroup. A zero denominator (T = +-Q, or 2 T = O) cannot occur on the subgroup, r being a prime
// above every multiple the walk passes through: it is a refusal (the lines written are then meaningless)
__device__ __forceinline__ bool g2_prepare(const G2Aff& q, G2Line* __restrict__ lines) {
    G2Aff t = q;
    bool bad = false;
    int n = 0;
#pragma unroll 1
    for (int bit = 62; bit >= 0; bit--) {
        const bool with_add = (BLS_X_ABS >> bit) & 1;
#pragma unroll 1
        for (int step = 0; step <= (with_add ? 1 : 0); step++) {
            // doubling: lam = 3 xT^2 / 2 yT; addition: lam = (yT - yQ) / (xT - xQ)
            const Fq2 xx = sqr(t.x);
            const Fq2 num = step ? sub(t.y, q.y) : add(dbl(xx), xx), den = step ? sub(t.x, q.x) : dbl(t.y);
            bad = bad || is_zero(den);
            const Fq2 lam = mul(num, fq2_inv(den));
            const Fq2 x3 = sub(sub(sqr(lam), t.x), step ? q.x : t.x);
            lines[n++] = G2Line{lam, sub(mul(lam, t.x), t.y)};
            t.y = sub(mul(lam, sub(t.x, x3)), t.y);
            t.x = x3;
        }
    }
    // psi(Q) = [x] Q = -[|x|] Q
    const Fq2 px = mul(conj(q.x), c_g2_psi[0]), py = mul(conj(q.y), c_g2_psi[1]);
    return !bad && eq(px, t.x) && eq(py, neg(t.y));
}

// ---- Fq12 over a group of 8 lanes, in LDS slots ---------------------------------------------------------------------------------------
enum : int { F12_LANES = 8, F12_SLOTS = 6, F12_SLOT_VEC = 6 * 6 /* uint4 per slot */, F12_GROUP_VEC = F12_SLOTS * F12_SLOT_VEC };
// dynamic LDS of a workgroup of `threads` lanes
__host__ __device__ constexpr size_t f12_lds_bytes(int threads) { return (size_t)(threads / F12_LANES) * F12_GROUP_VEC * 16; }

struct F12G {       // a lane's place
    u32 base;       // of its group's slot 0, in uint4
    u32 k;          // the coefficient it computes: lane-in-group mod 6
    u32 writer;     // lane-in-group < 6
};
__device__ __forceinline__ F12G f12_group() {
    const u32 l = threadIdx.x % F12_LANES;
    return F12G{(threadIdx.x / F12_LANES) * (u32)F12_GROUP_VEC, l < 6 ? l : l - 6, l < 6 ? 1u : 0u};
}
__device__ __forceinline__ uint4* f12_lds() {
    extern __shared__ __attribute__((aligned(16))) uint4 f12_lds_mem[];
    return f12_lds_mem;
}
__device__ __forceinline__ Fq2 f12_get(u32 base, u32 slot, u32 coef) {
    const uint4* p = f12_lds() + base + slot * F12_SLOT_VEC + coef * 6;
    const uint4 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4], f = p[5];
    return Fq2{Fq{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w}}, Fq{{d.x, d.y, d.z, d.w, e.x, e.y, e.z, e.w, f.x, f.y, f.z, f.w}}};
}
// this lane's coefficient of a slot
__device__ __forceinline__ void f12_put(const F12G& g, u32 slot, const Fq2& v) {
    if (!g.writer) return;
    uint4* p = f12_lds() + g.base + slot * F12_SLOT_VEC + g.k * 6;
    p[0] = uint4{v.c0.w[0], v.c0.w[1], v.c0.w[2], v.c0.w[3]};
    p[1] = uint4{v.c0.w[4], v.c0.w[5], v.c0.w[6], v.c0.w[7]};
    p[2] = uint4{v.c0.w[8], v.c0.w[9], v.c0.w[10], v.c0.w[11]};
    p[3] = uint4{v.c1.w[0], v.c1.w[1], v.c1.w[2], v.c1.w[3]};
    p[4] = uint4{v.c1.w[4], v.c1.w[5], v.c1.w[6], v.c1.w[7]};
    p[5] = uint4{v.c1.w[8], v.c1.w[9], v.c1.w[10], v.c1.w[11]};
}
__device__ __forceinline__ Fq2 f12_mine(const F12G& g, u32 slot) { return f12_get(g.base, slot, g.k); }
__device__ __forceinline__ void f12_set_one(const F12G& g, u32 slot) { f12_put(g, slot, select(g.k == 0, fq2_one(), fq2_zero())); }

// dst = a b; dst may be a or b. Six products of Fq2 a lane, the loop NOT unrolled: a site is one product of Fq2 around mul_fq
__device__ __forceinline__ void f12_mul(const F12G& g, u32 dst, u32 a, u32 b) {
    __syncthreads();  // the operands are written
    Fq2 lo = fq2_zero(), hi = fq2_zero();
#pragma unroll 1
    for (u32 i = 0; i < 6; i++) {
        const bool wrap = i > g.k;  // i + j = k + 6: w^6 = xi
        const Fq2 t = mul(f12_get(g.base, a, i), f12_get(g.base, b, wrap ? g.k + 6 - i : g.k - i));
        const Fq2 s = add(select(wrap, hi, lo), t);
        hi = select(wrap, s, hi);
        lo = select(wrap, lo, s);
    }
    __syncthreads();  // and read by every lane
    f12_put(g, dst, add(lo, mul_xi(hi)));
}
// dst = a l for an l whose coefficients 1, 4 and 5 are zero (a line): three products of Fq2 a lane
__device__ __forceinline__ void f12_mul_line(const F12G& g, u32 dst, u32 a, u32 l) {
    __syncthreads();
    Fq2 lo = fq2_zero(), hi = fq2_zero();
#pragma unroll 1
    for (u32 n = 0; n < 3; n++) {
        const u32 j = n ? n + 1 : 0;  // 0, 2, 3
        const bool wrap = j > g.k;
        const Fq2 t = mul(f12_get(g.base, a, wrap ? g.k + 6 - j : g.k - j), f12_get(g.base, l, j));
        const Fq2 s = add(select(wrap, hi, lo), t);
        hi = select(wrap, s, hi);
        lo = select(wrap, lo, s);
    }
    __syncthreads();
    f12_put(g, dst, add(lo, mul_xi(hi)));
}
// the lane-local maps (dst may be a): a lane reads and writes its own coefficient only
__device__ __forceinline__ void f12_conj(const F12G& g, u32 dst, u32 a) {  // the p^6 map: w -> -w
    const Fq2 v = f12_mine(g, a);
    f12_put(g, dst, select(g.k & 1, neg(v), v));
}
__device__ __forceinline__ void f12_frob1(const F12G& g, u32 dst, u32 a) { f12_put(g, dst, mul(conj(f12_mine(g, a)), c_f12_gamma1[g.k])); }
__device__ __forceinline__ void f12_frob2(const F12G& g, u32 dst, u32 a) { f12_put(g, dst, scale(f12_mine(g, a), c_f12_gamma2[g.k])); }
// dst = a^x for a in the cyclotomic subgroup, where the inverse is the conjugate. dst != a
__device__ __forceinline__ void f12_pow_x(const F12G& g, u32 dst, u32 a) {
    f12_put(g, dst, f12_mine(g, a));
#pragma unroll 1
    for (int bit = 62; bit >= 0; bit--) {
        f12_mul(g, dst, dst, dst);
        if ((BLS_X_ABS >> bit) & 1) f12_mul(g, dst, dst, a);
    }
    f12_conj(g, dst, dst);
}

// Longer computations are PROGRAMS over the slots, run by one loop, so that the product above is inlined at three sites here (a step
// here, two in f12_pow_x) instead of at every line of a formula: the instruction cache is 64 KB.
enum : u32 { F12_MUL, F12_CONJ, F12_FROB1, F12_FROB2, F12_POW_X, F12_INV0, F12_SCALE };
struct F12Step {
    u32 op, d, a, b;  // MUL d = a b; CONJ, FROB1, FROB2, POW_X: d = op(a); INV0: n = 1 / (coefficient 0 of a), in registers; SCALE d = a n
};
// slot 0 = its (3 (p^12 - 1) / r)-th power, slot 0 != 0; slots 1 .. 5 are overwritten. The first F12_INV_STEPS steps alone are the
// inversion: slot 5 = 1 / slot 0 (0 -> 0), slots 2, 3, 4 overwritten
enum : int { F12_INV_STEPS = 9, F12_FINAL_EXP_STEPS = 31 };
static __constant__ F12Step c_f12_final_exp[F12_FINAL_EXP_STEPS] = {
    {F12_CONJ, 2, 0, 0},   // conj(f)
    {F12_MUL, 3, 0, 2},    // s = f conj(f), in Fq6
    {F12_FROB2, 4, 3, 0},  // s^(p^2)
    {F12_FROB2, 5, 4, 0},  // s^(p^4)
    {F12_MUL, 4, 4, 5},
    {F12_MUL, 5, 3, 4},    // the norm of s, in Fq2: coefficient 0
    {F12_INV0, 0, 5, 0},
    {F12_MUL, 3, 2, 4},    // conj(f) s^(p^2) s^(p^4)
    {F12_SCALE, 5, 3, 0},  // 5: 1 / f
    {F12_CONJ, 1, 0, 0},
    {F12_MUL, 1, 1, 5},    // p^6 - 1
    {F12_FROB2, 2, 1, 0},
    {F12_MUL, 1, 2, 1},    // p^2 + 1. 1: t, in the cyclotomic subgroup
    {F12_POW_X, 2, 1, 0},
    {F12_CONJ, 5, 1, 0},
    {F12_MUL, 2, 2, 5},    // t^(x - 1)
    {F12_POW_X, 3, 2, 0},
    {F12_CONJ, 5, 2, 0},
    {F12_MUL, 2, 3, 5},    // t^((x - 1)^2)
    {F12_POW_X, 3, 2, 0},
    {F12_FROB1, 5, 2, 0},
    {F12_MUL, 3, 3, 5},    // 3: ^(x + p)
    {F12_POW_X, 4, 3, 0},
    {F12_POW_X, 5, 4, 0},
    {F12_FROB2, 4, 3, 0},
    {F12_MUL, 5, 5, 4},
    {F12_CONJ, 4, 3, 0},
    {F12_MUL, 5, 5, 4},    // 5: ^(x^2 + p^2 - 1)
    {F12_MUL, 4, 1, 1},
    {F12_MUL, 4, 4, 1},    // t^3
    {F12_MUL, 0, 5, 4},
};
__device__ __forceinline__ void f12_run(const F12G& g, const F12Step* prog, int n_steps) {
    Fq2 n = fq2_zero();
#pragma unroll 1
    for (int pc = 0; pc < n_steps; pc++) {
        const F12Step s = prog[pc];
        switch (s.op) {
            case F12_MUL: f12_mul(g, s.d, s.a, s.b); break;
            case F12_CONJ: f12_conj(g, s.d, s.a); break;
            case F12_FROB1: f12_frob1(g, s.d, s.a); break;
            case F12_FROB2: f12_frob2(g, s.d, s.a); break;
            case F12_POW_X: f12_pow_x(g, s.d, s.a); break;
            case F12_INV0:
                __syncthreads();  // lane 0's coefficient is written
                n = fq2_inv(f12_get(g.base, s.a, 0));
                break;
            default: f12_put(g, s.d, mul(f12_mine(g, s.a), n)); break;  // F12_SCALE
        }
    }
}
__device__ __forceinline__ void f12_inv(const F12G& g) { f12_run(g, c_f12_final_exp, F12_INV_STEPS); }
__device__ __forceinline__ void f12_final_exp(const F12G& g) { f12_run(g, c_f12_final_exp, F12_FINAL_EXP_STEPS); }
// is the slot one? (the same answer in every lane of the group; a workgroup of whole waves of 64 lanes)
__device__ __forceinline__ bool f12_is_one(const F12G& g, u32 slot) {
    __syncthreads();
    const bool mine = eq(f12_mine(g, slot), select(g.k == 0, fq2_one(), fq2_zero()));
    const u64 all = __ballot(mine);
    return ((all >> ((threadIdx.x & 63u) & ~7u)) & 0xFFu) == 0xFFu;
}
// slot l = the line (lam, c) at the affine point P of G1, or one when P is infinity (the pair then contributes the factor 1)
__device__ __forceinline__ void f12_put_line(const F12G& g, u32 l, const G2Line& line, const G1Aff& p) {
    const bool inf = is_inf(p);
    Fq2 v = fq2_zero();
    v = select(g.k == 0, select(inf, fq2_one(), line.c), v);
    v = select(g.k == 2 && !inf, neg(scale(line.lam, p.x)), v);
    v = select(g.k == 3 && !inf, Fq2{p.y, zero<FqT>()}, v);
    f12_put(g, l, v);
}
// slot f = the product of the Miller functions of (P[0], Q0) and (P[1], Q1), the Q by their prepared lines (lines0, lines1), on one
// accumulator; slot l is overwritten. The pointers may differ from group to group, not within one
__device__ __forceinline__ void f12_miller2(const F12G& g, u32 f, u32 l, const G2Line* __restrict__ lines0, const G2Line* __restrict__ lines1,
                                            const G1Aff* __restrict__ p) {
    f12_set_one(g, f);
    int n = 0;
#pragma unroll 1
    for (int bit = 62; bit >= 0; bit--) {
        f12_mul(g, f, f, f);
        const int steps = ((BLS_X_ABS >> bit) & 1) ? 2 : 1;  // the doubling's line, then the addition's
#pragma unroll 1
        for (int s = 0; s < 2 * steps; s++) {
            const int pair = s & 1;
            f12_put_line(g, l, (pair ? lines1 : lines0)[n + (s >> 1)], p[pair]);
            f12_mul_line(g, f, f, l);
        }
        n += steps;
    }
    f12_conj(g, f, f);  // x is negative
}
}  // namespace bls
}  // namespace zkw
