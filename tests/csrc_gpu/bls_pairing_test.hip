// era_zkevm_test_harness_amd/csrc/bls12_381_pairing.cuh alone (with bls12_381.cuh, which it builds on): the tower Fq2 / Fq12, the group
// G2 and the pairing of BLS12-381. `bls_pairing_test CASES RESULTS`: CASES is a file of records {u32 op; u32 in[288]} written by
// tests/test_gpu_bls_pairing.py, RESULTS receives {u32 flag; u32 out[144]} per case; the expected values are Python integers there
// (tests/kzg_pairing_model.py). Operands and results are PLAIN integers (little-endian 32-bit words); the kernels convert to and from
// Montgomery form. Operations below 100 take a lane per case; the others work on elements of Fq12 spread over 8 lanes and synchronise,
// so every workgroup of such a launch runs ONE operation: the host launches each run of equal operations on its own. Test
// infrastructure (built on the GPU box).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../era_zkevm_test_harness_amd/csrc/bls12_381_pairing.cuh"

using namespace zkw::bls;

struct Case { u32 op; u32 in[288]; };
struct Result { u32 flag; u32 out[144]; };

enum { FQ2_MUL = 0, FQ2_SQR = 1, FQ2_INV = 2, FQ2_SQRT = 3, G2_DECOMPRESS = 10, G2_PREPARE = 11,
       F12_OP_MUL = 100, F12_OP_SQR = 101, F12_OP_INV = 102, F12_OP_MUL_LINE = 103, F12_OP_CONJ = 104, F12_OP_FROB1 = 105, F12_OP_FROB2 = 106,
       F12_OP_FINAL_EXP = 107, F12_OP_PAIRING = 108 };

__device__ Fq load_fq(const u32* w) {
    Fq o;
    for (int i = 0; i < 12; i++) o.w[i] = w[i];
    return to_mont(o);
}
__device__ void store_fq(u32* w, const Fq& a) {
    const Fq p = from_mont(a);
    for (int i = 0; i < 12; i++) w[i] = p.w[i];
}
__device__ Fq2 load_fq2(const u32* w) { return Fq2{load_fq(w), load_fq(w + 12)}; }
__device__ void store_fq2(u32* w, const Fq2& a) {
    store_fq(w, a.c0);
    store_fq(w + 12, a.c1);
}

// a lane per case
__global__ void k_lane_cases(const Case* cases, Result* results, G2Line* lines, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Case& c = cases[i];
    Result* r = results + i;
    r->flag = 0;
    for (int j = 0; j < 144; j++) r->out[j] = 0;
    const Fq2 a = load_fq2(c.in), b = load_fq2(c.in + 24);
    switch (c.op) {
        case FQ2_MUL: store_fq2(r->out, mul(a, b)); break;
        case FQ2_SQR: store_fq2(r->out, sqr(a)); break;
        case FQ2_INV: store_fq2(r->out, fq2_inv(a)); break;
        case FQ2_SQRT: {
            Fq2 s;
            r->flag = fq2_sqrt(a, &s);
            store_fq2(r->out, s);
            break;
        }
        case G2_DECOMPRESS: {  // in: the 96 bytes; flag: g2_decompress's code; out: x, y
            G2Aff q;
            r->flag = (u32)g2_decompress(reinterpret_cast<const uint8_t*>(c.in), &q);
            store_fq2(r->out, q.x);
            store_fq2(r->out + 24, q.y);
            break;
        }
        case G2_PREPARE: {  // in: x, y of a point of the twist; flag: in the subgroup?; out: the first and the last line
            const G2Aff q{a, b};
            G2Line* mine = lines + (size_t)i * G2_LINES;
            r->flag = g2_prepare(q, mine);
            store_fq2(r->out, mine[0].lam);
            store_fq2(r->out + 24, mine[0].c);
            store_fq2(r->out + 48, mine[G2_LINES - 1].lam);
            store_fq2(r->out + 72, mine[G2_LINES - 1].c);
            break;
        }
    }
}

// 8 lanes per case, 64 lanes a workgroup, f12_lds_bytes(64) of dynamic LDS; every case of the launch has the operation `op`.
// in: the Fq12 operand a (6 x 24 words), then b. F12_OP_PAIRING: in = P0 (x, y: 24 words; zeros for infinity), P1, Q0 (x, y of the
// twist: 48 words), Q1; out = the final exponentiation of the two pairs' Miller product, flag = is it one
__global__ void k_group_cases(u32 op, const Case* cases, Result* results, G2Line* lines, G1Aff* points, int n) {
    const F12G g = f12_group();
    const int group = blockIdx.x * (blockDim.x / F12_LANES) + threadIdx.x / F12_LANES;
    const int i = group < n ? group : n - 1;  // a group past the end repeats the last case and stores nothing
    const bool store = group < n && g.writer;
    const Case& c = cases[i];
    f12_put(g, 0, load_fq2(c.in + 24 * g.k));
    f12_put(g, 1, load_fq2(c.in + 144 + 24 * g.k));
    u32 out = 0;
    switch (op) {
        case F12_OP_MUL: f12_mul(g, 2, 0, 1); out = 2; break;
        case F12_OP_SQR: f12_mul(g, 0, 0, 0); break;
        case F12_OP_INV: f12_inv(g); out = 5; break;
        case F12_OP_MUL_LINE: f12_mul_line(g, 0, 0, 1); break;
        case F12_OP_CONJ: f12_conj(g, 0, 0); break;
        case F12_OP_FROB1: f12_frob1(g, 2, 0); out = 2; break;
        case F12_OP_FROB2: f12_frob2(g, 0, 0); break;
        case F12_OP_FINAL_EXP: f12_final_exp(g); break;
        case F12_OP_PAIRING: {
            const u32 l = threadIdx.x % F12_LANES;
            G2Line* mine = lines + (size_t)group * 2 * G2_LINES;
            G1Aff* pts = points + (size_t)group * 2;
            if (l < 2) {
                pts[l] = G1Aff{load_fq(c.in + 24 * l), load_fq(c.in + 24 * l + 12)};
                g2_prepare(G2Aff{load_fq2(c.in + 48 + 48 * l), load_fq2(c.in + 48 + 48 * l + 24)}, mine + l * G2_LINES);
            }
            __syncthreads();
            f12_miller2(g, 0, 1, mine, mine + G2_LINES, pts);
            f12_final_exp(g);
            break;
        }
    }
    const bool one = f12_is_one(g, out);
    if (store) store_fq2(results[i].out + 24 * g.k, f12_mine(g, out));
    if (group < n && threadIdx.x % F12_LANES == 0) results[i].flag = one;
}

#define CHECK(e)                                                                                    \
    do {                                                                                            \
        hipError_t _e = (e);                                                                        \
        if (_e != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(_e)); return 2; }          \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: bls_pairing_test CASES RESULTS\n"); return 2; }
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
    G2Line* d_lines = nullptr;
    G1Aff* d_points = nullptr;
    const size_t groups = ((size_t)n + 7) / 8 * 8 + 8;  // (a launch's groups are counted from its own first case)
    CHECK(hipMalloc(&d_cases, n * sizeof(Case)));
    CHECK(hipMalloc(&d_results, n * sizeof(Result)));
    CHECK(hipMalloc(&d_lines, groups * 2 * G2_LINES * sizeof(G2Line)));
    CHECK(hipMalloc(&d_points, groups * 2 * sizeof(G1Aff)));
    CHECK(hipMemcpy(d_cases, cases.data(), n * sizeof(Case), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_results, 0, n * sizeof(Result)));
    for (int lo = 0; lo < n;) {  // runs of equal operations (all the lane operations count as one)
        int hi = lo + 1;
        const bool lanes = cases[lo].op < 100;
        while (hi < n && (lanes ? cases[hi].op < 100 : cases[hi].op == cases[lo].op)) hi++;
        const int m = hi - lo;
        if (lanes) hipLaunchKernelGGL(k_lane_cases, dim3((m + 63) / 64), dim3(64), 0, 0, d_cases + lo, d_results + lo, d_lines, m);
        else hipLaunchKernelGGL(k_group_cases, dim3((m + 7) / 8), dim3(64), f12_lds_bytes(64), 0, cases[lo].op, d_cases + lo, d_results + lo, d_lines, d_points, m);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        lo = hi;
    }
    std::vector<Result> results(n);
    CHECK(hipMemcpy(results.data(), d_results, n * sizeof(Result), hipMemcpyDeviceToHost));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(results.data(), sizeof(Result), n, f) != (size_t)n) { printf("cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    printf("ok %d\n", n);
    return 0;
}
