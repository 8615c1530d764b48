// p2_forms_test.hip — the device forms of csrc/poseidon2.cuh piece by piece and as whole permutations, and on the same inputs the host forms,
// against the permutation's definition written in this file with `unsigned __int128 % p`: the layers as matrices (M4,
// circ(2 M4, M4, M4), all-ones + diag(2^shift)) built from include/zkw_poseidon2_params.h, the S-box as x^7, no gl:: or p2:: call.
// Every comparison is made after gl::canon. Every kernel runs full 64-lane waves (the forms move words by DPP): the inputs are padded to
// whole blocks. In the row form lanes 12..15 hold 0 and must come back 0.
//   mode "layers":
//     wp_reduce(L, H) over L, H < 2^63 against (L + 2^32 H) % p: edge words, seeded words, the callers' range < 2^47 and pairs built so
//       that (c, c2) takes (0,0), (1,0) and (0,1). (1,1) cannot occur below 2^63: with c the high word of L took a carry, so x < 2^63 - 2^32,
//       and (Hhi + 1) * EPS <= 2^63 - 2^31: the sum stays at or below 2^64 - 2^32 - 2^31 - 1.
//     add_rc_sched, Coop4::add_rc<false>, Coop4::add_rc<true> (the constant a kernel argument: an SGPR) against (x + c) % p for weak x and
//       every round constant, 0 and p - 1; wrap and no wrap.
//     one external and one internal layer of the lane form, Coop, Coop2 and Coop4, and of the host Wide forms, on the two edge families of
//       p2_quad_test.hip and 2^12 seeded states. A host word model of Coop::external / Coop::internal counts the states in which a lane
//       takes the final v_cndmask wrap (and is itself checked against the definition); another counts the second wrap of wp_reduce
//       inside the lane form's layers.
//     Coop::pow7_pair, lane 0 of each row, against x^7.
//   mode "perms": p2::permute, p2::permute_lat, Coop::permute, Coop2::permute and coop_flattened (all 130 stored values per state, in the
//     order of orc_poseidon2_flattened) on 2^14 states by the recipe of p2_quad_test.hip, against the definition's round-by-round trace,
//     and the host p2::permute / permute_lat against the same.
//   "--host-only": builds and classifies every input, checks the host forms and the word models, prints the cover lines, no HIP call.
// Prints "cover <what> key=value ..." lines and "ok <compared values> <mode>" last, exit 0; or the first mismatch and exit 1.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../era_zkevm_test_harness_amd/csrc/poseidon2.cuh"
using gl::u32;
using gl::u64;
typedef unsigned __int128 u128;

#define CHECK(x)                                                                            \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) { printf("hip error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } \
    } while (0)

enum { EXT, INT, PERM, PERM_LAT, POW7_PAIR };

// ---------------------------------------------------------------- kernels: every lane of every wave is live
__global__ __launch_bounds__(256) void k_wp_reduce(const u64* L, const u64* H, u64* r) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    r[i] = p2::wp_reduce(L[i], H[i]);
#endif
}
__global__ __launch_bounds__(256) void k_add_rc(const u64* x, const u64* c, u64* r_sched, u64* r_q4) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    r_sched[i] = p2::add_rc_sched(x[i], c[i]);
    r_q4[i] = p2::Coop4::add_rc<false>(x[i], (u32)c[i], (u32)(c[i] >> 32));
#endif
}
__global__ __launch_bounds__(256) void k_add_rc_sgpr(const u64* x, u64* r, u32 c0, u32 c1) {  // c0 wave-uniform: a scalar register
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    r[i] = p2::Coop4::add_rc<true>(x[i], c0, c1);
#endif
}
template <int MODE>
__global__ __launch_bounds__(256) void k_lane(u64* st) {  // one state per lane
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    u64 s[12];
    for (int k = 0; k < 12; k++) s[k] = st[12 * i + k];
    if constexpr (MODE == EXT) p2::external(s);
    else if constexpr (MODE == INT) p2::internal(s);
    else if constexpr (MODE == PERM) p2::permute(s);
    else p2::permute_lat(s);
    for (int k = 0; k < 12; k++) st[12 * i + k] = s[k];
}
template <int MODE>
__global__ __launch_bounds__(256) void k_row(const u64* in16, u64* out16) {  // one state per 16-lane row; lanes 12..15 are given 0
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    p2::Coop co;
    co.init((int)(t & 15));
    const u64 x = in16[t];
    u64 y;
    if constexpr (MODE == EXT) y = co.external(x);
    else if constexpr (MODE == INT) y = co.internal(x);
    else if constexpr (MODE == PERM) y = co.permute(x);
    else y = co.pow7_pair(x);
    out16[t] = y;
}
__global__ __launch_bounds__(256) void k_row_flat(const u64* in16, u64* out16, u64* slots) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const u32 g = (u32)(t & 15);
    p2::Coop co;
    co.init((int)g);
    u64* mine = slots + 130 * (t / 16);
    out16[t] = p2::coop_flattened(co, in16[t], g, [&](u32 idx, u64 v) { mine[idx] = v; });
}
template <int MODE>
__global__ __launch_bounds__(256) void k_pair(u64* st) {  // one state per pair of lanes
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x, i = t / 2;
    const int j = (int)(t & 1);
    p2::Coop2 co;
    co.init(j);
    u64 x[6];
    for (int c = 0; c < 3; c++) { x[2 * c] = st[12 * i + 4 * c + 2 * j]; x[2 * c + 1] = st[12 * i + 4 * c + 2 * j + 1]; }
    if constexpr (MODE == EXT) co.external(x);
    else if constexpr (MODE == INT) co.internal(x);
    else co.permute(x);
    for (int c = 0; c < 3; c++) { st[12 * i + 4 * c + 2 * j] = x[2 * c]; st[12 * i + 4 * c + 2 * j + 1] = x[2 * c + 1]; }
}
template <int MODE>
__global__ __launch_bounds__(256) void k_quad(u64* st) {  // one state per quad (Coop4::permute: p2_quad_test.hip)
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x, i = t / 4;
    const int j = (int)(t & 3);
    p2::Coop4 co;
    co.init(j);
    u64 x[3];
    for (int c = 0; c < 3; c++) x[c] = st[12 * i + 4 * c + j];
    if constexpr (MODE == EXT) co.external(x);
    else co.internal(x);
    for (int c = 0; c < 3; c++) st[12 * i + 4 * c + j] = x[c];
}

static u64 sm(u64& s) {
    u64 z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// ---------------------------------------------------------------- the definition
static const u64 RP = 0xFFFFFFFF00000001ULL;
static u64 ME[12][12], MI[12][12];  // circ(2 M4, M4, M4); all-ones + diag(2^shift)
static void build_matrices() {
    for (int b = 0; b < 3; b++)
        for (int i = 0; i < 4; i++)
            for (int c = 0; c < 3; c++)
                for (int j = 0; j < 4; j++) ME[4 * b + i][4 * c + j] = P2_M4[i][j] * (b == c ? 2 : 1);
    for (int i = 0; i < 12; i++)
        for (int j = 0; j < 12; j++) MI[i][j] = 1 + (i == j ? 1ull << P2_INTERNAL_DIAG_SHIFTS[i] : 0);
}
static void r_matrix(const u64 M[12][12], u64 s[12]) {
    u64 y[12];
    for (int i = 0; i < 12; i++) {
        u128 acc = 0;
        for (int j = 0; j < 12; j++) acc += (u128)M[i][j] * (s[j] % RP);
        y[i] = (u64)(acc % RP);
    }
    memcpy(s, y, sizeof y);
}
static u64 r_mul(u64 a, u64 b) { return (u64)((u128)a * b % RP); }
static u64 r_pow7(u64 x) {
    x %= RP;
    const u64 x2 = r_mul(x, x), x4 = r_mul(x2, x2);
    return r_mul(r_mul(x4, x2), x);
}
static u64 r_addc(u64 x, u64 c) { return (u64)(((u128)x + c) % RP); }
// the permutation with the 130 values of the flattened gate: the input, the state after each of the first four full rounds, the S-box
// output of each partial round, the state after each of the last four full rounds (the last is the output)
static void r_permute(const u64 in[12], u64 slots[130]) {
    u64 s[12];
    for (int i = 0; i < 12; i++) slots[i] = s[i] = in[i] % RP;
    int pos = 12, r = 0;
    r_matrix(ME, s);
    for (int half = 0; half < 2; half++) {
        for (int k = 0; k < P2_HALF_FULL_ROUNDS; k++, r++) {
            for (int i = 0; i < 12; i++) s[i] = r_pow7(r_addc(s[i], P2_ROUND_CONSTANTS[12 * r + i]));
            r_matrix(ME, s);
            for (int i = 0; i < 12; i++) slots[pos++] = s[i];
        }
        for (int k = 0; half == 0 && k < P2_PARTIAL_ROUNDS; k++, r++) {
            slots[pos++] = s[0] = r_pow7(r_addc(s[0], P2_ROUND_CONSTANTS[12 * r + P2_PARTIAL_CONSTANT_INDEX]));
            r_matrix(MI, s);
        }
    }
}

// ---------------------------------------------------------------- host word models of the device steps
static int f_wp(u64 L, u64 H) {  // c + 2 * c2 of wp_reduce
    const u32 l1 = (u32)(L >> 32), h0 = (u32)H, h1 = (u32)(H >> 32);
    const u64 n = (u64)l1 + h0;
    const u32 c = (u32)(n >> 32), k = h1 + c;
    const u64 x = (n << 32) | (u32)L;
    return (int)c + 2 * (int)(((u128)x + (u128)k * gl::EPS) >> 64);
}
// the last steps of Coop::external / internal: y (96 bits) -> ylo + y2 * EPS, and EPS once more when that wraps (the v_cndmask)
static u64 row_tail(u128 y, bool* wrap) {
    const u128 r = (u128)(u64)y + (u128)(u64)(y >> 64) * gl::EPS;
    *wrap = (r >> 64) != 0;
    return (u64)r + (*wrap ? gl::EPS : 0);
}
static u128 row_m4(const u64 s[12], int g) {  // the M4 row of lane g on the two word planes: L + 2^32 H
    const int b = g & ~3, j = g & 3;
    const u64 a = s[g], bb = s[b + ((j + 1) & 3)], c = s[b + ((j + 2) & 3)], d = s[b + ((j + 3) & 3)];
    const u64 ka = j & 1 ? 6 : 5, kb = j & 1 ? 1 : 7, kd = j & 1 ? 4 : 3;
    const u64 L = (a & gl::EPS) * ka + (bb & gl::EPS) * kb + (c & gl::EPS) + (d & gl::EPS) * kd;
    const u64 H = (a >> 32) * ka + (bb >> 32) * kb + (c >> 32) + (d >> 32) * kd;
    return (u128)L + ((u128)H << 32);
}
static bool model_row_external(const u64 s[12], u64 y[12]) {  // true: some lane wrapped
    bool any = false, w;
    for (int g = 0; g < 12; g++) {
        const int j = g & 3;
        y[g] = row_tail(row_m4(s, g) + row_m4(s, j) + row_m4(s, 4 + j) + row_m4(s, 8 + j), &w);
        any |= w;
    }
    return any;
}
static bool model_row_internal(const u64 s[12], u64 y[12]) {
    u128 sum = 0;
    for (int g = 0; g < 12; g++) sum += s[g];
    bool any = false, w;
    for (int g = 0; g < 12; g++) {
        y[g] = row_tail(((u128)s[g] << P2_INTERNAL_DIAG_SHIFTS[g]) + sum, &w);
        any |= w;
    }
    return any;
}
// the (L, H) pairs that the lane form's layers hand to wp_reduce: true when one of them takes the second wrap
static bool model_lane_c2(const u64 s[12], bool internal) {
    bool any = false;
    for (int g = 0; g < 12; g++) {
        u64 L = 0, H = 0;
        for (int j = 0; j < 12; j++) {
            const u64 k = internal ? MI[g][j] : ME[g][j];
            L += (s[j] & gl::EPS) * k;
            H += (s[j] >> 32) * k;
        }
        any |= (f_wp(L, H) & 2) != 0;
    }
    return any;
}

// ---------------------------------------------------------------- inputs
static const std::vector<u64> EDGE = {0, 1, 2, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, gl::P - 1, gl::P, gl::P + 1,
                                      0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFF00000000ull, 0xFFFFFFFEFFFFFFFFull, 0x8000000000000000ull,
                                      0x7FFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFEull, 0x00000001FFFFFFFFull};
// the recipe of p2_quad_test.hip: uniform edge states, one edge word in one position with the rest 0 or all ones, then seeded states with
// the same mix of weak words, n states in all
static std::vector<u64> states(size_t n, u64 seed) {
    std::vector<u64> st;
    for (u64 e : EDGE)
        for (int k = 0; k < 12; k++) st.push_back(e);
    for (u64 e : EDGE)
        for (int pos = 0; pos < 12; pos++)
            for (u64 rest : {0ull, 0xFFFFFFFFFFFFFFFFull})
                for (int k = 0; k < 12; k++) st.push_back(k == pos ? e : rest);
    u64 s = seed;
    while (st.size() < 12 * n) {
        const size_t i = st.size() / 12;
        for (int k = 0; k < 12; k++) {
            u64 w = sm(s);
            if (i % 3 == 0) w = EDGE[sm(s) % EDGE.size()];   // states of edge words only
            else if (i % 5 == 0) w |= 0xFFFFFFFF00000000ull; // high words of all ones
            else if (i % 7 == 0) w &= 0xFFFFFFFFull;         // low words only
            st.push_back(w);
        }
    }
    return st;
}
static void pad(std::vector<u64>& v, size_t multiple) {
    while (v.size() % multiple) v.push_back(0);
}
// 12 words per state -> 16 lanes per state, lanes 12..15 zero; and back
static std::vector<u64> to16(const std::vector<u64>& st) {
    std::vector<u64> r(st.size() / 12 * 16, 0);
    for (size_t i = 0; i < st.size() / 12; i++)
        for (int k = 0; k < 12; k++) r[16 * i + k] = st[12 * i + k];
    return r;
}

static int bad(const char* what, size_t i, int k, u64 in, u64 got, u64 want, const char* note = "") {
    printf("mismatch %s: item %zu element %d: in %016llx got %016llx want %016llx %s\n", what, i, k, (unsigned long long)in, (unsigned long long)got,
           (unsigned long long)want, note);
    return 1;
}
// got (12 words per state, weak) against want (canonical) on the first n states
static int compare(const char* what, const std::vector<u64>& in, const std::vector<u64>& got, const std::vector<u64>& want, size_t n, size_t& total) {
    for (size_t i = 0; i < 12 * n; i++)
        if (gl::canon(got[i]) != want[i]) return bad(what, i / 12, (int)(i % 12), in[i], got[i], want[i]);
    total += 12 * n;
    return 0;
}
// the row form's 16 lanes per state: lanes 0..11 against want, lanes 12..15 zero
static int compare16(const char* what, const std::vector<u64>& in, const std::vector<u64>& got16, const std::vector<u64>& want, size_t n, size_t& total) {
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 16; k++) {
            const u64 g = got16[16 * i + k];
            if (k >= 12 ? g != 0 : gl::canon(g) != want[12 * i + k]) return bad(what, i, k, k < 12 ? in[12 * i + k] : 0, g, k < 12 ? want[12 * i + k] : 0, k >= 12 ? "(idle lane)" : "");
        }
    total += 16 * n;
    return 0;
}

static int up(const std::vector<u64>& v, u64** d) {
    CHECK(hipMalloc(d, v.size() * sizeof(u64)));
    CHECK(hipMemcpy(*d, v.data(), v.size() * sizeof(u64), hipMemcpyHostToDevice));
    return 0;
}
static int down(u64* d, std::vector<u64>& v, size_t n) {
    CHECK(hipGetLastError());
    v.resize(n);
    CHECK(hipMemcpy(v.data(), d, n * sizeof(u64), hipMemcpyDeviceToHost));
    CHECK(hipFree(d));
    return 0;
}
// runs one in-place state kernel (threads_per_state lanes per state) on a copy of st
#define RUN_STATES(KERNEL, TPS, ST, GOT)                                              \
    do {                                                                              \
        u64* d_ = nullptr;                                                            \
        if (up(ST, &d_)) return 1;                                                    \
        KERNEL<<<dim3((unsigned)((ST).size() / 12 * (TPS) / 256)), dim3(256)>>>(d_);  \
        if (down(d_, GOT, (ST).size())) return 1;                                     \
    } while (0)
#define RUN_ROWS(KERNEL, IN16, GOT16)                                                 \
    do {                                                                              \
        u64 *di_ = nullptr, *do_ = nullptr;                                           \
        if (up(IN16, &di_) || up(IN16, &do_)) return 1;                               \
        KERNEL<<<dim3((unsigned)((IN16).size() / 256)), dim3(256)>>>(di_, do_);       \
        if (down(do_, GOT16, (IN16).size())) return 1;                                \
        CHECK(hipFree(di_));                                                          \
    } while (0)

// ---------------------------------------------------------------- mode "layers"
static int layers(bool device, size_t& total) {
    // ---- wp_reduce
    std::vector<u64> L, H;
    {
        const u64 e63[] = {0, 1, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, 0x7FFFFFFFFFFFull, 0x800000000000ull, 0x7FFFFFFF00000000ull,
                           0x7FFFFFFF00000001ull, 0x7FFFFFFEFFFFFFFFull, 0x00000000FFFFFFFEull, 0x7FFFFFFFFFFFFFFEull, 0x7FFFFFFFFFFFFFFFull};
        for (u64 l : e63)
            for (u64 h : e63) { L.push_back(l); H.push_back(h); }
        u64 s = 17;
        for (int i = 0; i < (1 << 14); i++) {
            const int sh = i % 4 == 0 ? 17 : 1;  // a quarter in the callers' range, below 2^47
            L.push_back(sm(s) >> sh); H.push_back(sm(s) >> sh);
        }
        for (int i = 0; i < 1024; i++) {  // built: the high word of L and the low word of H sum to 2^32 - 1 (no c), then any Hhi >= 1 wraps (c2)
            const int bits = i & 1 ? 15 : 31;
            const u64 l1 = sm(s) & ((1ull << bits) - 1), k = 1 + (sm(s) & ((1ull << bits) - 1)) % ((1ull << bits) - 1);
            L.push_back((l1 << 32) | (u32)sm(s)); H.push_back((k << 32) | (0xFFFFFFFFull - l1));
        }
        pad(L, 256); pad(H, 256);
    }
    unsigned cc = 0, cc47 = 0;
    size_t lt47 = 0;
    std::vector<u64> want_wp(L.size());
    for (size_t i = 0; i < L.size(); i++) {
        if ((L[i] | H[i]) >> 63) { printf("wp_reduce input %zu out of range\n", i); return 1; }
        const int f = f_wp(L[i], H[i]);
        cc |= 1u << f;
        if (!((L[i] | H[i]) >> 47)) { lt47++; cc47 |= 1u << f; }
        want_wp[i] = (u64)(((u128)L[i] + ((u128)H[i] << 32)) % RP);
    }
    printf("cover wp_reduce n=%zu cc=0x%x lt47=%zu cc47=0x%x\n", L.size(), cc, lt47, cc47);

    // ---- round-constant additions: every weak x against every constant
    std::vector<u64> consts(P2_ROUND_CONSTANTS, P2_ROUND_CONSTANTS + P2_TOTAL_ROUNDS * P2_WIDTH), xs(EDGE);
    consts.push_back(0); consts.push_back(RP - 1);
    {
        u64 s = 19;
        while (xs.size() < 256) xs.push_back(xs.size() % 3 ? sm(s) : sm(s) | 0xFFFFFFFF00000000ull);
    }
    std::vector<u64> ax, ac, want_rc;
    unsigned w = 0;
    for (u64 c : consts) {
        if (c >= RP) { printf("round constant %016llx is not canonical\n", (unsigned long long)c); return 1; }
        for (u64 x : xs) { ax.push_back(x); ac.push_back(c); want_rc.push_back(r_addc(x, c)); w |= 1u << ((u64)(x + c) < x); }
    }
    printf("cover add_rc n=%zu consts=%zu w=0x%x\n", ax.size(), consts.size(), w);

    // ---- layers
    const size_t n = 16 + 16 * 12 * 2 + (1 << 12);
    std::vector<u64> st = states(n, 23);
    pad(st, 12 * 256);
    const size_t np = st.size() / 12;
    std::vector<u64> want_e(st), want_i(st), tmp(12);
    size_t row_ext_wrap = 0, row_int_wrap = 0, lane_ext_c2 = 0, lane_int_c2 = 0;
    for (size_t i = 0; i < np; i++) {
        const u64* s = &st[12 * i];
        r_matrix(ME, &want_e[12 * i]);
        r_matrix(MI, &want_i[12 * i]);
        // the host forms (Wide: m4w, wadd, wshl, wreduce)
        u64 h[12];
        memcpy(h, s, sizeof h); p2::external(h);
        for (int k = 0; k < 12; k++) if (gl::canon(h[k]) != want_e[12 * i + k]) return bad("host external", i, k, s[k], h[k], want_e[12 * i + k]);
        memcpy(h, s, sizeof h); p2::internal(h);
        for (int k = 0; k < 12; k++) if (gl::canon(h[k]) != want_i[12 * i + k]) return bad("host internal", i, k, s[k], h[k], want_i[12 * i + k]);
        for (int b = 0; b < 3; b++) {
            p2::Wide t[4];
            p2::m4w(s + 4 * b, t);
            for (int r = 0; r < 4; r++) {
                u128 acc = 0;
                for (int j = 0; j < 4; j++) acc += (u128)P2_M4[r][j] * s[4 * b + j];
                const u64 g = p2::wreduce(t[r]);
                if (gl::canon(g) != (u64)(acc % RP)) return bad("host m4w", i, 4 * b + r, s[4 * b + r], g, (u64)(acc % RP));
            }
        }
        for (u32 sh = 1; sh < 32; sh++) {
            const u64 add = sh < 31 ? s[(sh + 1) % 12] : 0;  // wreduce takes a high part below 2^31
            const u64 g = p2::wreduce(p2::wadd(p2::wshl(p2::wide(s[sh % 12]), sh), p2::wide(add)));
            const u64 wnt = (u64)((((u128)s[sh % 12] << sh) + add) % RP);
            if (gl::canon(g) != wnt) return bad("host wshl + wadd", i, (int)sh, s[sh % 12], g, wnt);
        }
        // the word models count the wraps, and must themselves compute the layers
        u64 m[12];
        if (model_row_external(s, m)) row_ext_wrap++;
        for (int k = 0; k < 12; k++) if (gl::canon(m[k]) != want_e[12 * i + k]) return bad("word model of Coop::external", i, k, s[k], m[k], want_e[12 * i + k]);
        if (model_row_internal(s, m)) row_int_wrap++;
        for (int k = 0; k < 12; k++) if (gl::canon(m[k]) != want_i[12 * i + k]) return bad("word model of Coop::internal", i, k, s[k], m[k], want_i[12 * i + k]);
        if (model_lane_c2(s, false)) lane_ext_c2++;
        if (model_lane_c2(s, true)) lane_int_c2++;
    }
    printf("cover layers n=%zu row_ext_wrap=%zu row_int_wrap=%zu lane_ext_c2=%zu lane_int_c2=%zu\n", n, row_ext_wrap, row_int_wrap, lane_ext_c2, lane_int_c2);

    // ---- pow7_pair: lane 0 of a row holds x, the other lanes hold words that must not matter
    std::vector<u64> px;
    {
        u64 s = 29;
        for (u64 e : EDGE) px.push_back(e);
        while (px.size() < 4096) px.push_back(px.size() % 3 ? sm(s) : gl::P + (u32)sm(s) % 0xFFFFFFFFu);
    }
    std::vector<u64> p16(16 * px.size());
    {
        u64 s = 31;
        for (size_t t = 0; t < p16.size(); t++) p16[t] = t % 16 ? sm(s) : px[t / 16];
    }
    printf("cover pow7_pair n=%zu\n", px.size());
    if (!device) return 0;

    std::vector<u64> got, got2;
    {
        u64 *dl = nullptr, *dh = nullptr, *dr = nullptr;
        if (up(L, &dl) || up(H, &dh) || up(L, &dr)) return 1;
        k_wp_reduce<<<dim3((unsigned)(L.size() / 256)), dim3(256)>>>(dl, dh, dr);
        if (down(dr, got, L.size())) return 1;
        CHECK(hipFree(dl)); CHECK(hipFree(dh));
        for (size_t i = 0; i < L.size(); i++)
            if (gl::canon(got[i]) != want_wp[i]) {
                printf("mismatch wp_reduce: pair %zu: L %016llx H %016llx got %016llx want %016llx (c + 2 c2 = %d)\n", i, (unsigned long long)L[i],
                       (unsigned long long)H[i], (unsigned long long)got[i], (unsigned long long)want_wp[i], f_wp(L[i], H[i]));
                return 1;
            }
        total += L.size();
    }
    {
        u64 *dx = nullptr, *dc = nullptr, *d1 = nullptr, *d2 = nullptr, *d3 = nullptr, *dxs = nullptr;
        if (up(ax, &dx) || up(ac, &dc) || up(ax, &d1) || up(ax, &d2) || up(ax, &d3) || up(xs, &dxs)) return 1;
        k_add_rc<<<dim3((unsigned)(ax.size() / 256)), dim3(256)>>>(dx, dc, d1, d2);
        for (size_t ci = 0; ci < consts.size(); ci++)
            k_add_rc_sgpr<<<dim3((unsigned)(xs.size() / 256)), dim3(256)>>>(dxs, d3 + ci * xs.size(), (u32)consts[ci], (u32)(consts[ci] >> 32));
        std::vector<u64> got3;
        if (down(d1, got, ax.size()) || down(d2, got2, ax.size()) || down(d3, got3, ax.size())) return 1;
        CHECK(hipFree(dx)); CHECK(hipFree(dc)); CHECK(hipFree(dxs));
        for (size_t i = 0; i < ax.size(); i++) {
            const char* note = (u64)(ax[i] + ac[i]) < ax[i] ? "(wrap)" : "(no wrap)";
            if (gl::canon(got[i]) != want_rc[i]) return bad("add_rc_sched", i, 0, ax[i], got[i], want_rc[i], note);
            if (gl::canon(got2[i]) != want_rc[i]) return bad("Coop4::add_rc<false>", i, 0, ax[i], got2[i], want_rc[i], note);
            if (gl::canon(got3[i]) != want_rc[i]) return bad("Coop4::add_rc<true>", i, 0, ax[i], got3[i], want_rc[i], note);
        }
        total += 3 * ax.size();
    }
    const std::vector<u64> st16 = to16(st);
    RUN_STATES(k_lane<EXT>, 1, st, got);
    if (compare("lane form external", st, got, want_e, np, total)) return 1;
    RUN_STATES(k_lane<INT>, 1, st, got);
    if (compare("lane form internal", st, got, want_i, np, total)) return 1;
    RUN_ROWS(k_row<EXT>, st16, got);
    if (compare16("Coop::external", st, got, want_e, np, total)) return 1;
    RUN_ROWS(k_row<INT>, st16, got);
    if (compare16("Coop::internal", st, got, want_i, np, total)) return 1;
    RUN_STATES(k_pair<EXT>, 2, st, got);
    if (compare("Coop2::external", st, got, want_e, np, total)) return 1;
    RUN_STATES(k_pair<INT>, 2, st, got);
    if (compare("Coop2::internal", st, got, want_i, np, total)) return 1;
    RUN_STATES(k_quad<EXT>, 4, st, got);
    if (compare("Coop4::external", st, got, want_e, np, total)) return 1;
    RUN_STATES(k_quad<INT>, 4, st, got);
    if (compare("Coop4::internal", st, got, want_i, np, total)) return 1;
    RUN_ROWS(k_row<POW7_PAIR>, p16, got);
    for (size_t i = 0; i < px.size(); i++)
        if (gl::canon(got[16 * i]) != r_pow7(px[i])) return bad("Coop::pow7_pair", i, 0, px[i], got[16 * i], r_pow7(px[i]));
    total += px.size();
    return 0;
}

// ---------------------------------------------------------------- mode "perms"
static int perms(bool device, size_t& total) {
    const size_t n = 1 << 14;  // a multiple of 256
    const std::vector<u64> st = states(n, 11);
    std::vector<u64> slots(130 * n), want(12 * n);
    for (size_t i = 0; i < n; i++) {
        r_permute(&st[12 * i], &slots[130 * i]);
        memcpy(&want[12 * i], &slots[130 * i + 118], 96);
        u64 h[12];
        memcpy(h, &st[12 * i], sizeof h); p2::permute(h);
        for (int k = 0; k < 12; k++) if (gl::canon(h[k]) != want[12 * i + k]) return bad("host permute", i, k, st[12 * i + k], h[k], want[12 * i + k]);
        memcpy(h, &st[12 * i], sizeof h); p2::permute_lat(h);
        for (int k = 0; k < 12; k++) if (gl::canon(h[k]) != want[12 * i + k]) return bad("host permute_lat", i, k, st[12 * i + k], h[k], want[12 * i + k]);
    }
    printf("cover perms n=%zu\n", n);
    if (!device) return 0;

    std::vector<u64> got, got2;
    const std::vector<u64> st16 = to16(st);
    RUN_STATES(k_lane<PERM>, 1, st, got);
    if (compare("lane form permute", st, got, want, n, total)) return 1;
    RUN_STATES(k_lane<PERM_LAT>, 1, st, got);
    if (compare("lane form permute_lat", st, got, want, n, total)) return 1;
    RUN_ROWS(k_row<PERM>, st16, got);
    if (compare16("Coop::permute", st, got, want, n, total)) return 1;
    RUN_STATES(k_pair<PERM>, 2, st, got);
    if (compare("Coop2::permute", st, got, want, n, total)) return 1;
    {
        u64 *di = nullptr, *d16 = nullptr, *ds = nullptr;
        const std::vector<u64> poison(130 * n, 0xA5A5A5A5A5A5A5A5ull);
        if (up(st16, &di) || up(st16, &d16) || up(poison, &ds)) return 1;
        k_row_flat<<<dim3((unsigned)(st16.size() / 256)), dim3(256)>>>(di, d16, ds);
        if (down(d16, got, st16.size()) || down(ds, got2, 130 * n)) return 1;
        CHECK(hipFree(di));
        for (size_t i = 0; i < n; i++) {
            for (int k = 0; k < 130; k++)  // stored canonical
                if (got2[130 * i + k] != slots[130 * i + k]) return bad("coop_flattened slot", i, k, st[12 * i + k % 12], got2[130 * i + k], slots[130 * i + k]);
            for (int k = 0; k < 12; k++)
                if (got[16 * i + k] != want[12 * i + k]) return bad("coop_flattened result", i, k, st[12 * i + k], got[16 * i + k], want[12 * i + k]);
        }
        total += 142 * n;
    }
    return 0;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "all";
    const bool host_only = !strcmp(mode, "--host-only"), all = host_only || !strcmp(mode, "all");
    if (!all && strcmp(mode, "layers") && strcmp(mode, "perms")) { printf("usage: p2_forms_test [--host-only | layers | perms]\n"); return 2; }
    build_matrices();
    size_t total = 0;
    if ((all || !strcmp(mode, "layers")) && layers(!host_only, total)) return 1;
    if ((all || !strcmp(mode, "perms")) && perms(!host_only, total)) return 1;
    printf("ok %zu %s\n", total, host_only ? "host-only" : mode);
    return 0;
}
