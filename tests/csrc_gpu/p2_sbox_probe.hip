// p2_sbox_probe.hip — a straight-line probe of the quad-form Poseidon2 permutation (p2::Coop4) for tests/test_chain_sbox_isa.py, which
// only compiles it, once as it stands (S-boxes through gl::mul_vcc) and once with -DGL_CHAIN_MUL_COMPILER_FORM (through gl::mul_lat).
// k_sbox_one runs one permutation per quad; k_sbox_none is the same kernel without it, so the difference of their instruction counts
// is the permutation's.
#include <hip/hip_runtime.h>
#include "../../era_zkevm_test_harness_amd/csrc/poseidon2.cuh"

template <bool PERMUTE>
__device__ __forceinline__ void sbox_probe(gl::u64* io) {
    p2::Coop4 co;
    co.init(threadIdx.x & 3);
    gl::u64 x[3];
    for (int c = 0; c < 3; c++) x[c] = io[64 * c + threadIdx.x];
    if (PERMUTE) {
        co.permute(x);
    } else {  // what the permutation would read, kept live at no instruction
        for (int k = 0; k < 2 * P2_HALF_FULL_ROUNDS; k++)
            for (int c = 0; c < 3; c++) asm volatile("" ::"v"(co.rc_full[k][c]));
        for (int c = 0; c < 3; c++) asm volatile("" : "+v"(x[c]) : "v"(co.pw[c]));
        asm volatile("" ::"v"(co.ka), "v"(co.kb), "v"(co.kd), "v"((int)co.first), "v"((int)co.second));
    }
    for (int c = 0; c < 3; c++) io[64 * c + threadIdx.x] = x[c];
}
extern "C" __global__ __launch_bounds__(64) void k_sbox_one(gl::u64* io) { sbox_probe<true>(io); }
extern "C" __global__ __launch_bounds__(64) void k_sbox_none(gl::u64* io) { sbox_probe<false>(io); }
