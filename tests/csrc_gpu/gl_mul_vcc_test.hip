// gl_mul_vcc_test.hip — gl::mul_vcc (the 15-instruction product of the chain forms, its carries in VCC) against the host gl::mul_lat,
// compared after canonicalisation, on: the full cross product of eleven edge words; pairs kept from a seeded enumeration so that every
// combination of the product's three flags occurs (cm: the cross terms carry out of 64 bits; c1: w2 * EPS + (w1:w0) wraps; b1: the
// subtraction of w3 borrows — classified on the host by flags() below); and 2^16 seeded random pairs, non-canonical words among them.
// Two of the eight combinations (cm with b1, with and without c1) need a product whose words 1 and 2 cancel in x, about one pair in
// 2^32 and one in 2^64: the enumeration is seeded with pairs built for them (b = w0 / a mod 2^96 by lattice reduction, and a search).
// Prints "ok <pairs> combos <mask>" and exits 0, or the first mismatch / the missing combinations and exits 1.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "../../era_zkevm_test_harness_amd/csrc/gl64.cuh"
using gl::u32;
using gl::u64;

#define CHECK(x)                                                                            \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) { printf("hip error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } \
    } while (0)

__global__ __launch_bounds__(256) void k_mul_vcc(const u64* a, const u64* b, u64* r, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) r[i] = gl::mul_vcc(a[i], b[i]);  // weak out: the host canonicalises
}

static u64 sm(u64& s) {
    u64 z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// cm * 4 + c1 * 2 + b1 of mul_vcc(a, b)
static int flags(u64 a, u64 b) {
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    const unsigned __int128 q = (unsigned __int128)((u64)a0 * b1) + (u64)a1 * b0, pr = (unsigned __int128)a * b;
    const u32 w0 = (u32)pr, w1 = (u32)(pr >> 32), w2 = (u32)(pr >> 64), w3 = (u32)(pr >> 96);
    const unsigned __int128 x = (unsigned __int128)w2 * 0xFFFFFFFFu + (((u64)w1 << 32) | w0);
    return (int)(q >> 64) * 4 + (int)(x >> 64) * 2 + ((u64)x < w3 ? 1 : 0);
}

int main() {
    const std::vector<u64> edge = {0, 1, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, 0x8000000000000000ull, gl::P - 1, gl::P, gl::P + 1,
                                   0xFFFFFFFF00000000ull, 0xFFFFFFFFFFFFFFFFull};
    std::vector<u64> a, b;
    for (u64 x : edge)
        for (u64 y : edge) { a.push_back(x); b.push_back(y); }

    // flag combinations: seeded candidates of a few shapes, then the built pairs; up to 32 kept per combination
    static const u64 built[][2] = {
        {0xe6eb8c9efd69fe29ull, 0xe7bd541e6870ff79ull}, {0xcd464138e6233255ull, 0xcbda28c7fd7a54caull}, {0xde527100f814e8a3ull, 0xe074284f872cabbdull},
        {0xe87c966cf77b9aa3ull, 0xd8a27c493fb105baull}, {0xe1da8978e06f5c67ull, 0xf426792c4ee52fccull}, {0xd8921396c0ddb74dull, 0xe1082b5b6fc7281eull},
        {0xc021c246e148b905ull, 0xc0ac1741fe4b8282ull}, {0xd65ca199c1c5f494ull, 0xed5dd83dd7ec64a2ull}, {0xe76c9686cff99085ull, 0xc5494e5ac62cdf56ull},
        {0xf1fefe17c04e698dull, 0xe3e33286e39402bbull}, {0xe0d3707dde9dbc8full, 0xdf6aec11ce98637full}, {0xfc0f574ccdb8abc9ull, 0xc41a5667f81c1196ull}};
    int kept[8] = {0};
    auto keep = [&](u64 x, u64 y) {
        const int f = flags(x, y);
        if (kept[f] < 32) { kept[f]++; a.push_back(x); b.push_back(y); }
    };
    u64 s = 7;
    auto cand = [&]() -> u64 {
        const u64 w = sm(s);
        switch (sm(s) % 6) {
            case 0: return w;
            case 1: return (w << 32) | (u64[]){0, 1, 0xFFFFFFFFull, 0xFFFFFFFEull}[sm(s) & 3];
            case 2: return ((u64[]){0xFFFFFFFFull, 0xFFFFFFFEull, 0x80000000ull, 1}[sm(s) & 3] << 32) | (u32)w;
            case 3: return edge[sm(s) % edge.size()];
            case 4: return w >> 31;
            default: return ~(w >> (24 + sm(s) % 40));
        }
    };
    for (int i = 0; i < 200000; i++) { const u64 x = cand(), y = cand(); keep(x, y); }
    for (auto& p : built) { keep(p[0], p[1]); keep(p[1], p[0]); }
    int mask = 0;
    for (int f = 0; f < 8; f++) mask |= (kept[f] ? 1 : 0) << f;
    if (mask != 0xFF) { printf("flag combinations missing: mask %02x\n", mask); return 1; }

    // 2^16 seeded random pairs; a third of them with a non-canonical word (>= p) on one side or both
    s = 13;
    for (int i = 0; i < (1 << 16); i++) {
        u64 x = sm(s), y = sm(s);
        if (i % 3 == 1) x |= 0xFFFFFFFF00000000ull;
        if (i % 6 == 1 || i % 3 == 2) y = gl::P + (u32)y % 0xFFFFFFFFu;
        a.push_back(x); b.push_back(y);
    }

    const size_t n = a.size();
    u64 *da = nullptr, *db = nullptr, *dr = nullptr;
    CHECK(hipMalloc(&da, n * sizeof(u64)));
    CHECK(hipMalloc(&db, n * sizeof(u64)));
    CHECK(hipMalloc(&dr, n * sizeof(u64)));
    CHECK(hipMemcpy(da, a.data(), n * sizeof(u64), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(db, b.data(), n * sizeof(u64), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_mul_vcc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, da, db, dr, n);
    CHECK(hipGetLastError());
    std::vector<u64> got(n);
    CHECK(hipMemcpy(got.data(), dr, n * sizeof(u64), hipMemcpyDeviceToHost));
    CHECK(hipFree(da)); CHECK(hipFree(db)); CHECK(hipFree(dr));
    for (size_t i = 0; i < n; i++) {
        const u64 want = gl::canon(gl::mul_lat(a[i], b[i]));
        if (gl::canon(got[i]) != want) {
            printf("mismatch pair %zu: %016llx * %016llx got %016llx want %016llx (flags %d)\n", i, (unsigned long long)a[i], (unsigned long long)b[i],
                   (unsigned long long)got[i], (unsigned long long)want, flags(a[i], b[i]));
            return 1;
        }
    }
    printf("ok %zu combos %02x\n", n, mask);
    return 0;
}
