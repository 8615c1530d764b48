// bls12_381.cuh — the base field Fq (381 bits, 12 words), the scalar field Fr (255 bits, 8 words) and the group G1 (y^2 = x^3 + 4) of
// BLS12-381 for the KZG commitment of an EIP-4844 blob (kzg_kernels.cuh). A value is N 32-bit words in N registers of one lane.
// Field elements travel in MONTGOMERY form (a R mod p, R = 2^(32 N)) between to_mont and from_mont; every function takes canonical words
// (< p) and returns canonical words. The multiplication is ONE outlined function per field that every call site calls, operands and
// result by value (ec_field.cuh, ecf::mul, is the precedent: inlined, a point addition would be sixteen copies of ~450 instructions).
// Depends on nothing else in the tree, so that tests/csrc_gpu/bls_field_test.hip can run it alone against Python integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zkw {
namespace bls {
typedef uint32_t u32;
typedef uint64_t u64;

// p, -p^-1 mod 2^32, R mod p, R^2 mod p. (constexpr tables inside device functions: after unrolling every index is a literal)
struct FqT {
    static constexpr int N = 12;
    static constexpr u32 NINV = 0xfffcfffdu;
    static __device__ __forceinline__ constexpr u32 p(int i) {
        constexpr u32 t[12] = {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                               0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
        return t[i];
    }
    static __device__ __forceinline__ constexpr u32 one(int i) {
        constexpr u32 t[12] = {0x0002fffdu, 0x76090000u, 0xc40c0002u, 0xebf4000bu, 0x53c758bau, 0x5f489857u,
                               0x70525745u, 0x77ce5853u, 0xa256ec6du, 0x5c071a97u, 0xfa80e493u, 0x15f65ec3u};
        return t[i];
    }
    static __device__ __forceinline__ constexpr u32 r2(int i) {
        constexpr u32 t[12] = {0x1c341746u, 0xf4df1f34u, 0x09d104f1u, 0x0a76e6a6u, 0x4c95b6d5u, 0x8de5476cu,
                               0x939d83c0u, 0x67eb88a9u, 0xb519952du, 0x9a793e85u, 0x92cae3aau, 0x11988fe5u};
        return t[i];
    }
};
struct FrT {
    static constexpr int N = 8;
    static constexpr u32 NINV = 0xffffffffu;
    static __device__ __forceinline__ constexpr u32 p(int i) {
        constexpr u32 t[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
        return t[i];
    }
    static __device__ __forceinline__ constexpr u32 one(int i) {
        constexpr u32 t[8] = {0xfffffffeu, 0x00000001u, 0x00034802u, 0x5884b7fau, 0xecbc4ff5u, 0x998c4fefu, 0xacc5056fu, 0x1824b159u};
        return t[i];
    }
    static __device__ __forceinline__ constexpr u32 r2(int i) {
        constexpr u32 t[8] = {0xf3f29c6du, 0xc999e990u, 0x87925c23u, 0x2b6cedcbu, 0x7254398fu, 0x05d31496u, 0x9f59ff11u, 0x0748d9d9u};
        return t[i];
    }
};
// exponents and moduli that are walked bit by bit (dynamic index: constant memory). p - 2 and (p + 1) / 4 of Fq; r - 2 and r of Fr
static __constant__ u32 c_fq_inv_e[12] = {0xffffaaa9u, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                                          0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
static __constant__ u32 c_fq_sqrt_e[12] = {0xffffeaabu, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                                           0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};
static __constant__ u32 c_fr_inv_e[8] = {0xffffffffu, 0xfffffffeu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
static __constant__ u32 c_fr_mod[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};

template <class T> struct Fe {
    u32 w[T::N];
};
typedef Fe<FqT> Fq;
typedef Fe<FrT> Fr;

__device__ __forceinline__ u64 mad32(u32 a, u32 b, u64 acc) {  // a * b + acc (no overflow by construction)
    u64 r, dead;
    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(dead) : "v"(a), "v"(b), "v"(acc));
    return r;
}

template <class T> __device__ __forceinline__ Fe<T> zero() {
    Fe<T> o;
#pragma unroll
    for (int i = 0; i < T::N; i++) o.w[i] = 0;
    return o;
}
template <class T> __device__ __forceinline__ Fe<T> one() {  // 1 in Montgomery form
    Fe<T> o;
#pragma unroll
    for (int i = 0; i < T::N; i++) o.w[i] = T::one(i);
    return o;
}
template <class T> __device__ __forceinline__ bool is_zero(const Fe<T>& a) {
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < T::N; i++) o |= a.w[i];
    return o == 0;
}
template <class T> __device__ __forceinline__ bool eq(const Fe<T>& a, const Fe<T>& b) {
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < T::N; i++) o |= a.w[i] ^ b.w[i];
    return o == 0;
}
template <class T> __device__ __forceinline__ Fe<T> select(bool c, const Fe<T>& a, const Fe<T>& b) {  // c ? a : b
    Fe<T> o;
#pragma unroll
    for (int i = 0; i < T::N; i++) o.w[i] = c ? a.w[i] : b.w[i];
    return o;
}
// words (any value below 2^(32 N)) below the modulus?
template <class T> __device__ __forceinline__ bool below_modulus(const u32* w) {
    long long c = 0;
#pragma unroll
    for (int i = 0; i < T::N; i++) { c += (long long)w[i] - (long long)T::p(i); c >>= 32; }
    return c != 0;  // w - p borrows
}
// t + carry * 2^(32 N) < 2 p  ->  mod p
template <class T> __device__ __forceinline__ Fe<T> cond_sub(const u32* t, u32 carry) {
    u32 d[T::N];
    long long c = 0;
#pragma unroll
    for (int i = 0; i < T::N; i++) { c += (long long)t[i] - (long long)T::p(i); d[i] = (u32)c; c >>= 32; }
    const bool ge = carry != 0 || c == 0;  // no borrow: t >= p
    Fe<T> o;
#pragma unroll
    for (int i = 0; i < T::N; i++) o.w[i] = ge ? d[i] : t[i];
    return o;
}
template <class T> __device__ __forceinline__ Fe<T> add(const Fe<T>& a, const Fe<T>& b) {
    u32 t[T::N];
    u64 c = 0;
#pragma unroll
    for (int i = 0; i < T::N; i++) { c += (u64)a.w[i] + b.w[i]; t[i] = (u32)c; c >>= 32; }
    return cond_sub<T>(t, (u32)c);
}
template <class T> __device__ __forceinline__ Fe<T> sub(const Fe<T>& a, const Fe<T>& b) {
    u32 t[T::N];
    long long c = 0;
#pragma unroll
    for (int i = 0; i < T::N; i++) { c += (long long)a.w[i] - (long long)b.w[i]; t[i] = (u32)c; c >>= 32; }
    const bool borrowed = c != 0;
    Fe<T> o;
    u64 d = 0;
#pragma unroll
    for (int i = 0; i < T::N; i++) { d += (u64)t[i] + (borrowed ? T::p(i) : 0u); o.w[i] = (u32)d; d >>= 32; }
    return o;
}
template <class T> __device__ __forceinline__ Fe<T> neg(const Fe<T>& a) { return sub(zero<T>(), a); }
template <class T> __device__ __forceinline__ Fe<T> dbl(const Fe<T>& a) { return add(a, a); }

// Montgomery product a b R^-1 mod p, word by word (CIOS): row i adds a * b_i onto the N + 1 running words, then m * p with
// m = t_0 * (-p^-1) clears the lowest word and the rest moves down a word. Both moduli leave the top bit of their top word free
// (p < 2^(32 N - 1)), so the running value stays below 2 p < 2^(32 N) after every row and N + 1 words hold every intermediate sum.
// 2 N^2 multiply-adds (v_mad_u64_u32) and N low multiplications, one conditional subtraction.
template <class T> __device__ __forceinline__ Fe<T> mul_body(const Fe<T>& a, const Fe<T>& b) {
    constexpr int N = T::N;
    u32 t[N];
#pragma unroll
    for (int i = 0; i < N; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        u64 v = 0;
        u32 c = 0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            v = mad32(a.w[j], b.w[i], (u64)t[j]) + c;
            t[j] = (u32)v;
            c = (u32)(v >> 32);
        }
        const u32 top = c;  // word N of the running value
        const u32 m = t[0] * T::NINV;
        v = mad32(m, T::p(0), (u64)t[0]);
        c = (u32)(v >> 32);
#pragma unroll
        for (int j = 1; j < N; j++) {
            v = mad32(m, T::p(j), (u64)t[j]) + c;
            t[j - 1] = (u32)v;
            c = (u32)(v >> 32);
        }
        t[N - 1] = top + c;  // (< 2^32: the value is below 2 p)
    }
    return cond_sub<T>(t, 0);
}
// The outlined functions. Aggregate arguments travel in at most 16 registers in all (the rest would go through the stack, i.e. scratch):
// Fr's two operands are exactly that; Fq's 24 words travel as six 4-word vectors, which are not aggregates.
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
__device__ __attribute__((noinline)) Fr mul_fr(Fr a, Fr b) { return mul_body<FrT>(a, b); }
__device__ __attribute__((noinline)) Fq mul_fq(u32x4 a0, u32x4 a1, u32x4 a2, u32x4 b0, u32x4 b1, u32x4 b2) {
    const Fq a{{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w}};
    const Fq b{{b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w}};
    return mul_body<FqT>(a, b);
}
template <class T> __device__ __forceinline__ Fe<T> mul(const Fe<T>& a, const Fe<T>& b);
template <> __device__ __forceinline__ Fr mul<FrT>(const Fr& a, const Fr& b) { return mul_fr(a, b); }
template <> __device__ __forceinline__ Fq mul<FqT>(const Fq& a, const Fq& b) {
    return mul_fq(u32x4{a.w[0], a.w[1], a.w[2], a.w[3]}, u32x4{a.w[4], a.w[5], a.w[6], a.w[7]}, u32x4{a.w[8], a.w[9], a.w[10], a.w[11]},
                  u32x4{b.w[0], b.w[1], b.w[2], b.w[3]}, u32x4{b.w[4], b.w[5], b.w[6], b.w[7]}, u32x4{b.w[8], b.w[9], b.w[10], b.w[11]});
}
template <class T> __device__ __forceinline__ Fe<T> sqr(const Fe<T>& a) { return mul<T>(a, a); }
template <class T> __device__ __forceinline__ Fe<T> to_mont(const Fe<T>& a) {
    Fe<T> r2;
#pragma unroll
    for (int i = 0; i < T::N; i++) r2.w[i] = T::r2(i);
    return mul<T>(a, r2);
}
template <class T> __device__ __forceinline__ Fe<T> from_mont(const Fe<T>& a) {
    Fe<T> o = zero<T>();
    o.w[0] = 1;
    return mul<T>(a, o);
}
// a^e for an exponent in constant memory (n_words words, most significant bit first; uniform control flow). a in Montgomery form
template <class T> __device__ __forceinline__ Fe<T> pow_const(const Fe<T>& a, const u32* e, int n_words) {
    Fe<T> r = one<T>();
#pragma unroll 1
    for (int wi = n_words - 1; wi >= 0; wi--) {
        const u32 word = e[wi];
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            r = mul<T>(r, r);
            if ((word >> bit) & 1) r = mul<T>(r, a);
        }
    }
    return r;
}
__device__ __forceinline__ Fq fq_inv(const Fq& a) { return pow_const<FqT>(a, c_fq_inv_e, 12); }  // 0 -> 0
__device__ __forceinline__ Fr fr_inv(const Fr& a) { return pow_const<FrT>(a, c_fr_inv_e, 8); }
// a^((p + 1) / 4): the square root of a when it has one (p = 3 mod 4); the caller squares the result to find out
__device__ __forceinline__ Fq fq_sqrt(const Fq& a) { return pow_const<FqT>(a, c_fq_sqrt_e, 12); }
// plain (not Montgomery) y above (p - 1) / 2: the "lexicographically larger" root
__device__ __forceinline__ bool fq_is_larger_root(const Fq& y_plain) {
    const Fq n = neg(y_plain);  // p - y
    long long c = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) { c += (long long)n.w[i] - (long long)y_plain.w[i]; c >>= 32; }
    return c != 0;  // (p - y) - y borrows: y > p - y
}

// ---- G1 -----------------------------------------------------------------------------------------------------------------------------
// Coordinates in Montgomery form. Affine: (0, 0) is the point at infinity (not on the curve: 0 != 4). Jacobian: Z = 0 is infinity.
struct G1Aff {
    Fq x, y;
};
struct G1Jac {
    Fq X, Y, Z;
};
__device__ __forceinline__ bool is_inf(const G1Aff& a) { return is_zero(a.x) && is_zero(a.y); }
__device__ __forceinline__ bool is_inf(const G1Jac& a) { return is_zero(a.Z); }
__device__ __forceinline__ G1Jac jac_inf() { return G1Jac{zero<FqT>(), zero<FqT>(), zero<FqT>()}; }
__device__ __forceinline__ G1Jac to_jac(const G1Aff& a) { return G1Jac{a.x, a.y, is_inf(a) ? zero<FqT>() : one<FqT>()}; }
__device__ __forceinline__ G1Jac select(bool c, const G1Jac& a, const G1Jac& b) {
    return G1Jac{select(c, a.X, b.X), select(c, a.Y, b.Y), select(c, a.Z, b.Z)};
}
// doubling (a = 0): 2 multiplications + 5 squarings. Complete: Z = 0 gives Z = 0, and so does Y = 0 (a point of order two)
__device__ __forceinline__ G1Jac jdbl(const G1Jac& p) {
    const Fq a = sqr(p.X), b = sqr(p.Y), c = sqr(b);
    Fq t = add(p.X, b);
    t = sub(sub(sqr(t), a), c);
    const Fq d = dbl(t), e = add(dbl(a), a), f = sqr(e);
    G1Jac o;
    o.X = sub(f, dbl(d));
    o.Y = sub(mul<FqT>(e, sub(d, o.X)), dbl(dbl(dbl(c))));
    o.Z = dbl(mul<FqT>(p.Y, p.Z));
    return o;
}
// Jacobian + affine (11 multiplications). Complete: either operand at infinity, equal operands (doubling), opposite operands (infinity)
__device__ __forceinline__ G1Jac jmadd(const G1Jac& p, const G1Aff& q) {
    const Fq zz = sqr(p.Z), u2 = mul<FqT>(q.x, zz), s2 = mul<FqT>(q.y, mul<FqT>(zz, p.Z));
    const Fq h = sub(u2, p.X), r = sub(s2, p.Y);
    const Fq h2 = sqr(h), h3 = mul<FqT>(h2, h), v = mul<FqT>(p.X, h2);
    G1Jac o;
    o.X = sub(sub(sub(sqr(r), h3), v), v);
    o.Y = sub(mul<FqT>(r, sub(v, o.X)), mul<FqT>(p.Y, h3));
    o.Z = mul<FqT>(p.Z, h);
    const bool p_inf = is_inf(p), q_inf = is_inf(q);
    if (!p_inf && !q_inf && is_zero(h)) o = is_zero(r) ? jdbl(p) : jac_inf();
    o = select(q_inf, p, o);
    o = select(p_inf, to_jac(q), o);  // (q at infinity too: to_jac gives Z = 0)
    return o;
}
// Jacobian + Jacobian (16 multiplications), complete in the same cases
__device__ __forceinline__ G1Jac jadd(const G1Jac& p, const G1Jac& q) {
    const Fq z1z1 = sqr(p.Z), z2z2 = sqr(q.Z);
    const Fq u1 = mul<FqT>(p.X, z2z2), u2 = mul<FqT>(q.X, z1z1);
    const Fq s1 = mul<FqT>(p.Y, mul<FqT>(z2z2, q.Z)), s2 = mul<FqT>(q.Y, mul<FqT>(z1z1, p.Z));
    const Fq h = sub(u2, u1), r = sub(s2, s1);
    const Fq h2 = sqr(h), h3 = mul<FqT>(h2, h), v = mul<FqT>(u1, h2);
    G1Jac o;
    o.X = sub(sub(sub(sqr(r), h3), v), v);
    o.Y = sub(mul<FqT>(r, sub(v, o.X)), mul<FqT>(s1, h3));
    o.Z = mul<FqT>(mul<FqT>(p.Z, q.Z), h);
    const bool p_inf = is_inf(p), q_inf = is_inf(q);
    if (!p_inf && !q_inf && is_zero(h)) o = is_zero(r) ? jdbl(p) : jac_inf();
    o = select(q_inf, p, o);
    o = select(p_inf, q, o);
    return o;
}
// to affine by one Fermat inversion; infinity (Z = 0) comes out as (0, 0) by itself: 0^(p - 2) = 0
__device__ __forceinline__ G1Aff to_affine(const G1Jac& p) {
    const Fq zi = fq_inv(p.Z), zi2 = sqr(zi);
    return G1Aff{mul<FqT>(p.X, zi2), mul<FqT>(p.Y, mul<FqT>(zi2, zi))};
}
// [r] P = O for an affine point on the curve: membership of the order-r subgroup (double-and-add over the 255 bits of r)
__device__ __forceinline__ bool in_subgroup(const G1Aff& p) {
    G1Jac acc = jac_inf();
#pragma unroll 1
    for (int bit = 254; bit >= 0; bit--) {
        acc = jdbl(acc);
        if ((c_fr_mod[bit >> 5] >> (bit & 31)) & 1) acc = jmadd(acc, p);
    }
    return is_inf(acc);
}

// the 48-byte compressed form: big-endian x, bit 7 of byte 0 always set, bit 6 infinity (every other bit then 0), bit 5 the larger root
enum { G1_OK = 0, G1_NOT_COMPRESSED = 1, G1_BAD_INFINITY = 2, G1_X_TOO_LARGE = 3, G1_NOT_ON_CURVE = 4, G1_NOT_IN_SUBGROUP = 5 };
__device__ __forceinline__ void compress(const G1Aff& a, uint8_t* out) {
    if (is_inf(a)) {
        out[0] = 0xC0;
        for (int i = 1; i < 48; i++) out[i] = 0;
        return;
    }
    const Fq x = from_mont(a.x), y = from_mont(a.y);
    const bool larger = fq_is_larger_root(y);
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const u32 w = x.w[11 - i];
        out[4 * i] = (uint8_t)(w >> 24);
        out[4 * i + 1] = (uint8_t)(w >> 16);
        out[4 * i + 2] = (uint8_t)(w >> 8);
        out[4 * i + 3] = (uint8_t)w;
    }
    out[0] |= 0x80 | (larger ? 0x20 : 0);
}
// returns G1_OK and the point, or the first rule of the encoding the 48 bytes break (the subgroup check is the caller's: in_subgroup)
__device__ __forceinline__ int decompress(const uint8_t* in, G1Aff* out) {
    out->x = zero<FqT>();
    out->y = zero<FqT>();
    const u32 b0 = in[0];
    if (!(b0 & 0x80)) return G1_NOT_COMPRESSED;
    if (b0 & 0x40) {
        u32 rest = b0 & 0x3F;
        for (int i = 1; i < 48; i++) rest |= in[i];
        return rest ? G1_BAD_INFINITY : G1_OK;
    }
    Fq x;
#pragma unroll
    for (int i = 0; i < 12; i++)
        x.w[11 - i] = ((u32)in[4 * i] << 24) | ((u32)in[4 * i + 1] << 16) | ((u32)in[4 * i + 2] << 8) | (u32)in[4 * i + 3];
    x.w[11] &= 0x1FFFFFFFu;
    if (!below_modulus<FqT>(x.w)) return G1_X_TOO_LARGE;
    const Fq xm = to_mont(x);
    Fq four = dbl(one<FqT>());
    four = dbl(four);
    const Fq y2 = add(mul<FqT>(sqr(xm), xm), four);
    Fq y = fq_sqrt(y2);
    if (!eq(sqr(y), y2)) return G1_NOT_ON_CURVE;
    if (fq_is_larger_root(from_mont(y)) != ((b0 & 0x20) != 0)) y = neg(y);
    out->x = xm;
    out->y = y;
    return G1_OK;
}
}  // namespace bls
}  // namespace zkw
