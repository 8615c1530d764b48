// gl_field_test.hip — every function of csrc/gl64.cuh in its device form (and, on the same inputs, in its host form) against plain
// `unsigned __int128` arithmetic with `% p` written in this file, compared after gl::canon. One launch per operation, one lane per
// operand tuple, weak results canonicalised on the host.
//   Inputs per operation: the cross product of 18 edge words (the lists of gl_mul_vcc_test.hip and p2_quad_test.hip, p - 2 and
//   0xFFFFFFFE00000002); 2^16 seeded tuples, a third of them with a word >= p on one side or both; and sets built so that every carry
//   of every form fires and does not fire. The carries are classified by a host word model of the device steps (the flags below) and
//   counted; the counts are conditions on the inputs, printed as "cover <op> n <tuples> <key> <hex mask> ..." lines:
//     mul, mul_cyc   flags: bit f set when a pair with cm * 4 + c1 * 2 + b1 == f is present (gl_mul_flags.h) — all eight
//     mul_sched, mul_lat   bc: bit (borrow of lo - hh) * 2 + (carry of + hl * EPS) — all four; cm: bit cm — both;
//                    borrow with carry comes from b = t / a mod 2^64 (a odd, 1 <= t < 2^16: the product's low half is t), borrow
//                    without carry from (2^48, 2^48)
//     reduce128      bc as above, fed (lo, hi) directly, hi over the edge words (2^64 - 1 and 0xFFFFFFFF00000000 among them)
//     add            cc: bit c + 2 * c2 — (0,0), (1,0), (1,1); c2 without c cannot be   sub   bb: the same for the two borrows
//     add_canon      w: bit (wrap) — both, (2^64 - 1) + (p - 1) among them
//     mul_small      c / c3: bit (carry of l + (hl << 32)) / bit (carry of + hh * EPS) — both each
//     mul_pow2       s0 / s1: bit s set when some x does not / does carry at shift s — every s / every s >= 1 (s = 0 has no high part)
// `--host-only` builds and classifies the inputs, checks the host forms and prints the cover lines without touching HIP.
// Prints "ok <tuples>" last and exits 0, or the first mismatch (operation, operands, got, want, flags) and exits 1.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../era_zkevm_test_harness_amd/csrc/gl64.cuh"
#include "gl_mul_flags.h"
using gl::u32;
using gl::u64;
typedef unsigned __int128 u128;

#define CHECK(x)                                                                            \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) { printf("hip error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } \
    } while (0)

enum Op { ADD, SUB, NEG, ADD_CANON, REDUCE128, MUL, MUL_CYC, MUL_SCHED, MUL_LAT, SQR, MUL_ADD, POW7, POW7_LAT, MUL_SMALL, MUL_POW2, POW, INV, CANON, N_OPS };
static const char* const OP_NAME[N_OPS] = {"add", "sub", "neg", "add_canon", "reduce128", "mul", "mul_cyc", "mul_sched", "mul_lat", "sqr", "mul_add",
                                           "pow7", "pow7_lat", "mul_small", "mul_pow2", "pow", "inv", "canon"};

// one lane, one tuple; the grid is padded to whole blocks and the tail lanes do nothing
__global__ __launch_bounds__(256) void k_op(int op, const u64* a, const u64* b, const u64* c, u64* r, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 x = a[i], y = b[i], z = c[i];
    u64 v = 0;
    switch (op) {
        case ADD: v = gl::add(x, y); break;
        case SUB: v = gl::sub(x, y); break;
        case NEG: v = gl::neg(x); break;
        case ADD_CANON: v = gl::add_canon(x, y); break;
        case REDUCE128: v = gl::reduce128(x, y); break;
        case MUL: v = gl::mul(x, y); break;
        case MUL_CYC: v = gl::mul_cyc(x, y); break;
        case MUL_SCHED: v = gl::mul_sched(x, y); break;
        case MUL_LAT: v = gl::mul_lat(x, y); break;
        case SQR: v = gl::sqr(x); break;
        case MUL_ADD: v = gl::mul_add(x, y, z); break;
        case POW7: v = gl::pow7(x); break;
        case POW7_LAT: v = gl::pow7_lat(x); break;
        case MUL_SMALL: v = gl::mul_small(x, (u32)y); break;
        case MUL_POW2: v = gl::mul_pow2(x, (u32)y); break;
        case POW: v = gl::pow(x, y); break;
        case INV: v = gl::inv(x); break;
        case CANON: v = gl::canon(x); break;
    }
    r[i] = v;
}

static u64 sm(u64& s) {
    u64 z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// ---- the reference: plain 128-bit arithmetic, no gl:: function
static const u64 RP = 0xFFFFFFFF00000001ULL;
static u64 r_mul(u64 a, u64 b) { return (u64)((u128)a * b % RP); }
static u64 r_add(u64 a, u64 b) { return (u64)(((u128)a + b) % RP); }
static u64 r_pow(u64 a, u64 e) {
    u64 r = 1;
    for (a %= RP; e; e >>= 1, a = r_mul(a, a))
        if (e & 1) r = r_mul(r, a);
    return r;
}
static u64 reference(int op, u64 a, u64 b, u64 c) {
    switch (op) {
        case ADD: case ADD_CANON: return r_add(a, b);
        case SUB: return (u64)(((u128)(a % RP) + RP - b % RP) % RP);
        case NEG: return (RP - a % RP) % RP;
        case REDUCE128: return (u64)((((u128)b << 64) | a) % RP);
        case MUL: case MUL_CYC: case MUL_SCHED: case MUL_LAT: return r_mul(a, b);
        case SQR: return r_mul(a, a);
        case MUL_ADD: return r_add(r_mul(a, b), c % RP);
        case POW7: case POW7_LAT: return r_pow(a, 7);
        case MUL_SMALL: return (u64)((u128)a * (u32)b % RP);
        case MUL_POW2: return (u64)(((u128)a << (u32)b) % RP);
        case POW: return r_pow(a, b);
        case INV: return r_pow(a, RP - 2);
        default: return a % RP;
    }
}
// the host forms of gl64.cuh: the second subject under test (mul_cyc and mul_sched have none)
static bool host_form(int op, u64 a, u64 b, u64 c, u64* v) {
    switch (op) {
        case ADD: *v = gl::add(a, b); return true;
        case SUB: *v = gl::sub(a, b); return true;
        case NEG: *v = gl::neg(a); return true;
        case ADD_CANON: *v = gl::add_canon(a, b); return true;
        case REDUCE128: *v = gl::reduce128(a, b); return true;
        case MUL: *v = gl::mul(a, b); return true;
        case MUL_LAT: *v = gl::mul_lat(a, b); return true;
        case SQR: *v = gl::sqr(a); return true;
        case MUL_ADD: *v = gl::mul_add(a, b, c); return true;
        case POW7: *v = gl::pow7(a); return true;
        case POW7_LAT: *v = gl::pow7_lat(a); return true;
        case MUL_SMALL: *v = gl::mul_small(a, (u32)b); return true;
        case MUL_POW2: *v = gl::mul_pow2(a, (u32)b); return true;
        case POW: *v = gl::pow(a, b); return true;
        case INV: *v = gl::inv(a); return true;
        case CANON: *v = gl::canon(a); return true;
        default: return false;
    }
}

// ---- host word models of the device steps
static int f_add(u64 a, u64 b) {  // c + 2 * c2
    const u64 s = a + b;
    const int c = s < a;
    const u64 t = s + (c ? gl::EPS : 0);
    return c + 2 * (t < s);
}
static int f_sub(u64 a, u64 b) {  // br + 2 * br2
    const u64 d = a - b;
    const int br = a < b;
    return br + 2 * (d < (br ? gl::EPS : 0));
}
static int f_reduce(u64 lo, u64 hi) {  // borrow * 2 + carry
    const u64 hh = hi >> 32, hl = hi & gl::EPS;
    const int borrow = lo < hh;
    const u64 t0 = lo - hh - (borrow ? gl::EPS : 0), t1 = (hl << 32) - hl;
    return borrow * 2 + ((u64)(t0 + t1) < t0);
}
static int f_sched(u64 a, u64 b) {  // cm * 4 + borrow * 2 + carry
    const u128 pr = (u128)a * b;
    return (gl_mul_flags(a, b) & 4) | f_reduce((u64)pr, (u64)(pr >> 64));
}
static int f_small(u64 x, u32 k) {  // c + 2 * c3
    const u64 l = (x & gl::EPS) * k, h = (x >> 32) * k, hh = h >> 32, hl = h & gl::EPS;
    const u64 r = l + (hl << 32);
    const int c = r < l;
    const u64 t = hh * gl::EPS, r2 = r + (c ? gl::EPS : 0);
    return c + 2 * ((u64)(r2 + t) < t);
}
static int f_pow2(u64 x, u32 s) {
    const u64 lo = x << s, hi = s ? x >> (64 - s) : 0, t1 = (hi << 32) - hi;
    return (u64)(lo + t1) < t1;
}

struct Set {
    std::vector<u64> a, b, c;
    void push(u64 x, u64 y = 0, u64 z = 0) { a.push_back(x); b.push_back(y); c.push_back(z); }
    size_t n() const { return a.size(); }
};

static const std::vector<u64> EDGE = {0, 1, 2, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, 0x00000001FFFFFFFFull, 0x7FFFFFFFFFFFFFFFull,
                                      0x8000000000000000ull, 0xFFFFFFFE00000002ull, 0xFFFFFFFEFFFFFFFFull, RP - 2, RP - 1, RP, RP + 1,
                                      0xFFFFFFFF00000000ull, 0xFFFFFFFFFFFFFFFEull, 0xFFFFFFFFFFFFFFFFull};

// 2^16 seeded tuples; a third of them with a word >= p: on the first side, on the second, on both. canon2: the second stays canonical.
static void seeded(Set& s, u64 seed, bool canon2) {
    for (int i = 0; i < (1 << 16); i++) {
        u64 x = sm(seed), y = sm(seed), z = sm(seed);
        const u64 wx = RP + (u32)sm(seed) % 0xFFFFFFFFu, wy = RP + (u32)sm(seed) % 0xFFFFFFFFu;
        if (i % 9 == 1 || i % 9 == 7) x = wx;
        if (i % 9 == 4 || i % 9 == 7) y = wy;
        if (i % 9 == 4) z |= 0xFFFFFFFF00000000ull;
        if (canon2) y %= RP;
        s.push(x, y, z);
    }
}

static void build(int op, Set& s) {
    switch (op) {
        case ADD: case SUB: case REDUCE128:
            for (u64 x : EDGE)
                for (u64 y : EDGE) s.push(x, y);
            seeded(s, 100 + op, false);
            if (op == REDUCE128) {  // random words never borrow: low halves below the high half's high word, with hl on both sides
                u64 sd = 31;
                for (int i = 0; i < 4096; i++) {
                    const u64 hi = sm(sd) | (i & 1 ? 0 : 0xFFFFFFFF00000000ull), lo = sm(sd) % ((hi >> 32) + 1);
                    s.push(lo, i & 2 ? hi : hi & 0xFFFFFFFF00000003ull);
                }
            }
            break;
        case ADD_CANON:
            for (u64 x : EDGE)
                for (u64 y : EDGE) s.push(x, y % RP);
            s.push(0xFFFFFFFFFFFFFFFFull, RP - 1);
            seeded(s, 100 + op, true);
            break;
        case MUL: case MUL_CYC: case MUL_SCHED: case MUL_LAT: {
            for (u64 x : EDGE)
                for (u64 y : EDGE) s.push(x, y);
            // every combination of (cm, c1, b1): seeded candidates of a few shapes, up to 32 kept each, and the built pairs both ways round
            int kept[8] = {0};
            auto keep = [&](u64 x, u64 y) {
                const int f = gl_mul_flags(x, y);
                if (kept[f] < 32) { kept[f]++; s.push(x, y); }
            };
            u64 sd = 7;
            for (int i = 0; i < 100000; i++) {
                u64 w[2];
                for (u64& v : w) {
                    v = sm(sd);
                    const u64 k = sm(sd);
                    if (k % 4 == 1) v = (v << 32) | (k >> 8 & 1 ? 0xFFFFFFFFull : 1);
                    else if (k % 4 == 2) v = ~(v >> (24 + (k >> 8) % 40));
                    else if (k % 4 == 3) v >>= 31;
                }
                keep(w[0], w[1]);
            }
            for (auto& p : GL_MUL_BUILT_PAIRS) { keep(p[0], p[1]); keep(p[1], p[0]); }
            // the reduction of mul_sched / mul_lat: the low half t of a * b below the top word of the high half
            s.push(1ull << 48, 1ull << 48);
            for (int i = 0; i < 1024; i++) {
                const u64 x = sm(sd) | 1, t = 1 + sm(sd) % 0xFFFF;
                u64 inv = x;  // Newton: x^-1 mod 2^64
                for (int k = 0; k < 6; k++) inv *= 2 - x * inv;
                s.push(x, t * inv);
            }
            seeded(s, 200, false);  // the four products see the same pairs
            break;
        }
        case MUL_ADD:
            for (u64 x : EDGE)
                for (u64 y : EDGE)
                    for (u64 z : EDGE) s.push(x, y, z);
            for (auto& p : GL_MUL_BUILT_PAIRS) { s.push(p[0], p[1], 0xFFFFFFFFFFFFFFFFull); s.push(p[1], p[0], RP - 1); }
            seeded(s, 100 + op, false);
            break;
        case MUL_SMALL: {
            const u64 ks[] = {0, 1, 2, 3, 7, 0xFFFF, 0x10000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF};
            for (u64 x : EDGE)
                for (u64 k : ks) s.push(x, k);
            seeded(s, 100 + op, false);
            for (size_t i = EDGE.size() * 11; i < s.n(); i++) s.b[i] = (u32)s.b[i] >> (i % 4 == 3 ? 20 : 0);
            break;
        }
        case MUL_POW2: {
            for (u64 x : EDGE)
                for (u64 sh = 0; sh < 32; sh++) s.push(x, sh);
            seeded(s, 100 + op, false);
            for (size_t i = EDGE.size() * 32; i < s.n(); i++) s.b[i] = i % 32;
            break;
        }
        case POW: {
            const u64 es[] = {0, 1, 2, RP - 2, RP - 1, 0xFFFFFFFFFFFFFFFFull};
            u64 sd = 5;
            for (u64 e : es) {
                for (u64 x : EDGE) s.push(x, e);
                for (int i = 0; i < 1024; i++) s.push(i % 3 == 1 ? RP + (u32)sm(sd) % 0xFFFFFFFFu : sm(sd), e);
            }
            break;
        }
        default:  // one operand: neg, sqr, pow7, pow7_lat, inv, canon
            for (u64 x : EDGE) s.push(x);
            if (op == SQR)
                for (auto& p : GL_MUL_BUILT_PAIRS) { s.push(p[0]); s.push(p[1]); }
            seeded(s, 100 + op, false);
    }
}

static std::string hex(unsigned long long v) {
    char buf[32];
    snprintf(buf, sizeof buf, "%llx", v);
    return buf;
}

// the cover line of one operation; returns false when a condition on the inputs does not hold
static bool cover(int op, const Set& s, std::string& line) {
    line = std::string("cover ") + OP_NAME[op] + " n " + std::to_string(s.n());
    unsigned m = 0, m2 = 0;
    switch (op) {
        case ADD: for (size_t i = 0; i < s.n(); i++) m |= 1u << f_add(s.a[i], s.b[i]);
            line += " cc " + hex(m); return m == 0xB;
        case SUB: for (size_t i = 0; i < s.n(); i++) m |= 1u << f_sub(s.a[i], s.b[i]);
            line += " bb " + hex(m); return m == 0xB;
        case ADD_CANON: for (size_t i = 0; i < s.n(); i++) { m |= 1u << ((u64)(s.a[i] + s.b[i]) < s.a[i]); if (s.b[i] >= RP) return false; }
            line += " w " + hex(m); return m == 3;
        case REDUCE128: for (size_t i = 0; i < s.n(); i++) m |= 1u << f_reduce(s.a[i], s.b[i]);
            line += " bc " + hex(m); return m == 0xF;
        case MUL: case MUL_CYC: case SQR: case MUL_ADD:
            for (size_t i = 0; i < s.n(); i++) m |= 1u << gl_mul_flags(s.a[i], op == SQR ? s.a[i] : s.b[i]);
            line += " flags " + hex(m); return op == SQR || op == MUL_ADD || m == 0xFF;
        case MUL_SCHED: case MUL_LAT:
            for (size_t i = 0; i < s.n(); i++) { const int f = f_sched(s.a[i], s.b[i]); m |= 1u << (f & 3); m2 |= 1u << (f >> 2); }
            line += " bc " + hex(m) + " cm " + hex(m2); return m == 0xF && m2 == 3;
        case MUL_SMALL:
            for (size_t i = 0; i < s.n(); i++) { const int f = f_small(s.a[i], (u32)s.b[i]); m |= 1u << (f & 1); m2 |= 1u << (f >> 1); }
            line += " c " + hex(m) + " c3 " + hex(m2); return m == 3 && m2 == 3;
        case MUL_POW2:
            for (size_t i = 0; i < s.n(); i++) (f_pow2(s.a[i], (u32)s.b[i]) ? m2 : m) |= 1u << s.b[i];
            line += " s0 " + hex(m) + " s1 " + hex(m2); return m == 0xFFFFFFFFu && m2 == 0xFFFFFFFEu;
        default: return true;
    }
}

static std::string flag_text(int op, u64 a, u64 b) {
    switch (op) {
        case ADD: return "c + 2 c2 = " + std::to_string(f_add(a, b));
        case SUB: return "br + 2 br2 = " + std::to_string(f_sub(a, b));
        case REDUCE128: return "2 borrow + carry = " + std::to_string(f_reduce(a, b));
        case MUL: case MUL_CYC: case MUL_ADD: return "4 cm + 2 c1 + b1 = " + std::to_string(gl_mul_flags(a, b));
        case SQR: return "4 cm + 2 c1 + b1 = " + std::to_string(gl_mul_flags(a, a));
        case MUL_SCHED: case MUL_LAT: return "4 cm + 2 borrow + carry = " + std::to_string(f_sched(a, b));
        case MUL_SMALL: return "c + 2 c3 = " + std::to_string(f_small(a, (u32)b));
        case MUL_POW2: return "carry = " + std::to_string(f_pow2(a, (u32)b));
        default: return "-";
    }
}
static int mismatch(const char* side, int op, const Set& s, size_t i, u64 got, u64 want) {
    printf("mismatch %s %s tuple %zu: %016llx %016llx %016llx got %016llx want %016llx (%s)\n", side, OP_NAME[op], i, (unsigned long long)s.a[i],
           (unsigned long long)s.b[i], (unsigned long long)s.c[i], (unsigned long long)got, (unsigned long long)want, flag_text(op, s.a[i], s.b[i]).c_str());
    return 1;
}

int main(int argc, char** argv) {
    const bool host_only = argc > 1 && !strcmp(argv[1], "--host-only");
    std::vector<Set> sets(N_OPS);
    std::vector<std::vector<u64>> want(N_OPS);
    size_t total = 0, widest = 0;
    bool covered = true;
    for (int op = 0; op < N_OPS; op++) {
        Set& s = sets[op];
        build(op, s);
        total += s.n();
        if (s.n() > widest) widest = s.n();
        std::string line;
        if (!cover(op, s, line)) { covered = false; line += " MISSING"; }
        printf("%s\n", line.c_str());
        want[op].resize(s.n());
        for (size_t i = 0; i < s.n(); i++) {
            const u64 w = want[op][i] = reference(op, s.a[i], s.b[i], s.c[i]);
            u64 v;
            if (host_form(op, s.a[i], s.b[i], s.c[i], &v) && gl::canon(v) != w) return mismatch("host", op, s, i, v, w);
            if (op == INV && (s.a[i] % RP ? r_mul(s.a[i] % RP, w) != 1 : w != 0)) return mismatch("reference", op, s, i, w, 1);
        }
    }
    if (!covered) { printf("a carry is not covered by the inputs\n"); return 1; }
    if (host_only) { printf("ok %zu host-only\n", total); return 0; }

    u64 *da = nullptr, *db = nullptr, *dc = nullptr, *dr = nullptr;
    CHECK(hipMalloc(&da, widest * sizeof(u64)));
    CHECK(hipMalloc(&db, widest * sizeof(u64)));
    CHECK(hipMalloc(&dc, widest * sizeof(u64)));
    CHECK(hipMalloc(&dr, widest * sizeof(u64)));
    std::vector<std::vector<u64>> got(N_OPS);
    for (int op = 0; op < N_OPS; op++) {
        const Set& s = sets[op];
        const size_t n = s.n();
        CHECK(hipMemcpy(da, s.a.data(), n * sizeof(u64), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(db, s.b.data(), n * sizeof(u64), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(dc, s.c.data(), n * sizeof(u64), hipMemcpyHostToDevice));
        CHECK(hipMemset(dr, 0xA5, n * sizeof(u64)));
        hipLaunchKernelGGL(k_op, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, da, db, dc, dr, n);
        CHECK(hipGetLastError());
        got[op].resize(n);
        CHECK(hipMemcpy(got[op].data(), dr, n * sizeof(u64), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) {
            if (gl::canon(got[op][i]) != want[op][i]) return mismatch("device", op, s, i, got[op][i], want[op][i]);
            // a * inv(a) = 1 with the device's own inverse
            if (op == INV && s.a[i] % RP && r_mul(s.a[i] % RP, got[op][i] % RP) != 1) return mismatch("device a * inv(a)", op, s, i, got[op][i], want[op][i]);
        }
    }
    CHECK(hipFree(da)); CHECK(hipFree(db)); CHECK(hipFree(dc)); CHECK(hipFree(dr));
    // gl::mul on the device is mul_cyc: the same weak word, not only the same element
    for (size_t i = 0; i < sets[MUL].n(); i++)
        if (got[MUL][i] != got[MUL_CYC][i]) return mismatch("device mul against mul_cyc", MUL, sets[MUL], i, got[MUL][i], got[MUL_CYC][i]);
    printf("ok %zu\n", total);
    return 0;
}
