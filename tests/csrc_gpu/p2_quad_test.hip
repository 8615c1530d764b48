// p2_quad_test.hip — the quad form of the Poseidon2 permutation (p2::Coop4: lane j of a quad holds elements j, 4 + j, 8 + j; the form of
// the queue-chain kernels k_chain_full_q4 / q4x4) against the host p2::permute, on 2^16 seeded states and on states built from weak,
// non-canonical words (P, P + 1, 2^64 - 1, 0xFFFFFFFF00000000, ...) that exercise every carry of the word-plane linear layers.
// Canonical results must be equal. Prints "ok <states>" and exits 0, or the first mismatch and exits 1.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../era_zkevm_test_harness_amd/csrc/poseidon2.cuh"
using gl::u64;

#define CHECK(x)                                                                            \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) { printf("hip error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } \
    } while (0)

// Every wave is full (the grid is padded to whole blocks): Coop4 moves words across the lanes of a quad with DPP.
__global__ __launch_bounds__(256) void k_perm_q4(u64* st, size_t n) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t i = t / 4;
    const int j = (int)(t & 3);
    p2::Coop4 co;
    co.init(j);
    u64 x[3];
    const bool live = i < n;
    for (int c = 0; c < 3; c++) x[c] = live ? st[12 * i + 4 * c + j] : 0;
    co.permute(x);
    if (live)
        for (int c = 0; c < 3; c++) st[12 * i + 4 * c + j] = gl::canon(x[c]);
}

static u64 sm(u64& s) {
    u64 z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

int main() {
    const std::vector<u64> edge = {0, 1, 2, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, gl::P - 1, gl::P, gl::P + 1,
                                   0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFF00000000ull, 0xFFFFFFFEFFFFFFFFull, 0x8000000000000000ull,
                                   0x7FFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFEull, 0x00000001FFFFFFFFull};
    std::vector<u64> st;
    // uniform states: every element the same edge word
    for (u64 e : edge)
        for (int k = 0; k < 12; k++) st.push_back(e);
    // one edge word in one position, the rest zero or all ones
    for (u64 e : edge)
        for (int pos = 0; pos < 12; pos++)
            for (u64 rest : {0ull, 0xFFFFFFFFFFFFFFFFull})
                for (int k = 0; k < 12; k++) st.push_back(k == pos ? e : rest);
    u64 s = 11;
    while (st.size() < 12 * (size_t)(1 << 16)) {
        const size_t i = st.size() / 12;
        for (int k = 0; k < 12; k++) {
            u64 w = sm(s);
            if (i % 3 == 0) w = edge[sm(s) % edge.size()];   // states of edge words only
            else if (i % 5 == 0) w |= 0xFFFFFFFF00000000ull; // high words of all ones
            else if (i % 7 == 0) w &= 0xFFFFFFFFull;         // low words only
            st.push_back(w);
        }
    }
    const size_t n = st.size() / 12;
    std::vector<u64> want(st);
    for (size_t i = 0; i < n; i++) {
        p2::permute(&want[12 * i]);
        for (int k = 0; k < 12; k++) want[12 * i + k] = gl::canon(want[12 * i + k]);
    }
    u64* d = nullptr;
    CHECK(hipMalloc(&d, st.size() * sizeof(u64)));
    CHECK(hipMemcpy(d, st.data(), st.size() * sizeof(u64), hipMemcpyHostToDevice));
    const size_t threads = 4 * n, blocks = (threads + 255) / 256;
    hipLaunchKernelGGL(k_perm_q4, dim3((unsigned)blocks), dim3(256), 0, 0, d, n);
    CHECK(hipGetLastError());
    std::vector<u64> got(st.size());
    CHECK(hipMemcpy(got.data(), d, got.size() * sizeof(u64), hipMemcpyDeviceToHost));
    CHECK(hipFree(d));
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 12; k++)
            if (got[12 * i + k] != want[12 * i + k]) {
                printf("mismatch state %zu element %d: in %016llx got %016llx want %016llx\n", i, k, (unsigned long long)st[12 * i + k],
                       (unsigned long long)got[12 * i + k], (unsigned long long)want[12 * i + k]);
                return 1;
            }
    printf("ok %zu\n", n);
    return 0;
}
