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
#include "gl_mul_flags.h"
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

// cm * 4 + c1 * 2 + b1 of mul_vcc(a, b): the host word model shared with gl_field_test.hip
static int flags(u64 a, u64 b) { return gl_mul_flags(a, b); }

int main() {
    const std::vector<u64> edge = {0, 1, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, 0x8000000000000000ull, gl::P - 1, gl::P, gl::P + 1,
                                   0xFFFFFFFF00000000ull, 0xFFFFFFFFFFFFFFFFull};
    std::vector<u64> a, b;
    for (u64 x : edge)
        for (u64 y : edge) { a.push_back(x); b.push_back(y); }

    // flag combinations: seeded candidates of a few shapes, then the built pairs; up to 32 kept per combination
    const auto& built = GL_MUL_BUILT_PAIRS;
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
