// era_zkevm_test_harness_amd/csrc/bls12_381.cuh alone (it includes nothing else of the tree): the fields Fq and Fr and the group G1 of
// BLS12-381, a case per lane. `bls_field_test CASES RESULTS`: CASES is a file of records {u32 op; u32 in[72]} written by
// tests/test_gpu_bls_field.py, RESULTS receives {u32 flag; u32 out[24]} per case; the expected values are Python integers there.
// Operands and results are PLAIN integers (little-endian 32-bit words); the kernel converts to and from Montgomery form except for the
// "raw" operations, which hand their operands to the Montgomery product as they are. Test infrastructure (built on the GPU box).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../era_zkevm_test_harness_amd/csrc/bls12_381.cuh"

using namespace zkw::bls;

struct Case { u32 op; u32 in[72]; };
struct Result { u32 flag; u32 out[24]; };

enum { FQ_MUL = 0, FQ_ADD = 1, FQ_SUB = 2, FQ_INV = 3, FQ_SQRT = 4, FQ_RAW_MUL = 5, FQ_NEG = 6,
       FR_MUL = 10, FR_ADD = 11, FR_SUB = 12, FR_INV = 13, FR_RAW_MUL = 15,
       G1_DBL = 20, G1_MADD = 21, G1_ADD = 22, G1_IN_SUBGROUP = 23, G1_COMPRESS = 24, G1_DECOMPRESS = 25 };

template <class T> __device__ Fe<T> load(const u32* w) {
    Fe<T> o;
    for (int i = 0; i < T::N; i++) o.w[i] = w[i];
    return o;
}
template <class T> __device__ void store(u32* w, const Fe<T>& a) {
    for (int i = 0; i < T::N; i++) w[i] = a.w[i];
}
__device__ G1Aff load_aff(const u32* w) { return G1Aff{to_mont(load<FqT>(w)), to_mont(load<FqT>(w + 12))}; }
// (x l^2, y l^3, l): the same point with a Z that is not 1
__device__ G1Jac load_jac(const u32* w, const u32* lambda) {
    const G1Aff a = load_aff(w);
    if (is_inf(a)) return jac_inf();
    const Fq l = to_mont(load<FqT>(lambda)), l2 = sqr(l);
    return G1Jac{mul<FqT>(a.x, l2), mul<FqT>(a.y, mul<FqT>(l2, l)), l};
}
__device__ void store_point(Result* r, const G1Jac& p) {
    const G1Aff a = to_affine(p);
    store(r->out, from_mont(a.x));
    store(r->out + 12, from_mont(a.y));
}

__global__ void k_cases(const Case* cases, Result* results, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Case& c = cases[i];
    Result* r = results + i;
    r->flag = 0;
    for (int j = 0; j < 24; j++) r->out[j] = 0;
    const u32 *a = c.in, *b = c.in + 12;
    switch (c.op) {
        case FQ_MUL: store(r->out, from_mont(mul<FqT>(to_mont(load<FqT>(a)), to_mont(load<FqT>(b))))); break;
        case FQ_ADD: store(r->out, add(load<FqT>(a), load<FqT>(b))); break;
        case FQ_SUB: store(r->out, sub(load<FqT>(a), load<FqT>(b))); break;
        case FQ_NEG: store(r->out, neg(load<FqT>(a))); break;
        case FQ_INV: store(r->out, from_mont(fq_inv(to_mont(load<FqT>(a))))); break;
        case FQ_SQRT: {
            const Fq am = to_mont(load<FqT>(a)), s = fq_sqrt(am);
            r->flag = eq(sqr(s), am);
            store(r->out, from_mont(s));
            break;
        }
        case FQ_RAW_MUL: store(r->out, mul<FqT>(load<FqT>(a), load<FqT>(b))); break;
        case FR_MUL: store(r->out, from_mont(mul<FrT>(to_mont(load<FrT>(a)), to_mont(load<FrT>(b))))); break;
        case FR_ADD: store(r->out, add(load<FrT>(a), load<FrT>(b))); break;
        case FR_SUB: store(r->out, sub(load<FrT>(a), load<FrT>(b))); break;
        case FR_INV: store(r->out, from_mont(fr_inv(to_mont(load<FrT>(a))))); break;
        case FR_RAW_MUL: store(r->out, mul<FrT>(load<FrT>(a), load<FrT>(b))); break;
        case G1_DBL: store_point(r, jdbl(load_jac(c.in, c.in + 48))); break;
        case G1_MADD: store_point(r, jmadd(load_jac(c.in, c.in + 48), load_aff(c.in + 24))); break;
        case G1_ADD: store_point(r, jadd(load_jac(c.in, c.in + 48), load_jac(c.in + 24, c.in + 60))); break;
        case G1_IN_SUBGROUP: r->flag = in_subgroup(load_aff(c.in)); break;
        case G1_COMPRESS: compress(load_aff(c.in), reinterpret_cast<uint8_t*>(r->out)); break;
        case G1_DECOMPRESS: {
            G1Aff p;
            r->flag = (u32)decompress(reinterpret_cast<const uint8_t*>(c.in), &p);
            store(r->out, from_mont(p.x));
            store(r->out + 12, from_mont(p.y));
            break;
        }
        default: r->flag = 0xBADu;
    }
}

#define CHECK(e)                                                                                    \
    do {                                                                                            \
        hipError_t _e = (e);                                                                        \
        if (_e != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(_e)); return 2; }          \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: bls_field_test CASES RESULTS\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
    std::vector<Case> cases;
    Case c;
    while (fread(&c, sizeof c, 1, f) == 1) cases.push_back(c);
    fclose(f);
    const int n = (int)cases.size();
    if (n == 0) { printf("no cases\n"); return 2; }
    Case* d_cases = nullptr;
    Result* d_results = nullptr;
    CHECK(hipMalloc(&d_cases, n * sizeof(Case)));
    CHECK(hipMalloc(&d_results, n * sizeof(Result)));
    CHECK(hipMemcpy(d_cases, cases.data(), n * sizeof(Case), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_cases, dim3((n + 63) / 64), dim3(64), 0, 0, d_cases, d_results, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<Result> results(n);
    CHECK(hipMemcpy(results.data(), d_results, n * sizeof(Result), hipMemcpyDeviceToHost));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(results.data(), sizeof(Result), n, f) != (size_t)n) { printf("cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    printf("ok %d\n", n);
    return 0;
}
