// rs_seg_sort_test.hip — the segmented form of the library's radix sort (radix_sort_pairs_segmented of
// era_zkevm_test_harness_amd/csrc/radix_sort.cuh) against std::stable_sort of every segment on the host, bit for bit. As rs_sort_test.hip
// the program includes the library's header and calls its driver on a context from zkw_create(0) of the built libzkw.so. Under test: the
// map from a workgroup to (segment, tile in segment), the histogram indexed [segment][digit][tile], whose flat scan has to place every
// pair inside its own segment, and the size of the temporary.
//   segments  sizes 1, 2 047, 2 048, 2 049 and 4 097 (around a tile of 2 048: a segment's last tile is partial, whole, one pair), mixed in
//             one call; 1 segment (each size), 2 and 3 segments (every rotation of the sizes), 300 segments (about 770 tiles = 12 scan chunks
//             of 16 384 histogram entries: chunk borders fall inside segments), and 3 segments of which the middle one is empty
//   end_bit   1, 8, 9, 33 (u64) and 1, 8, 9 (u32); the key bits above end_bit are random and must be ignored
//   keys      uniform, and few distinct keys (long runs of equal digits: stability inside a segment shows in the values)
//   values    the pair's position in the array, so a pair that left its segment or two equal keys that swapped are both visible
//   checks    kout / vout equal the reference; kin / vin unchanged; the temporary is radix_temp_bytes(n, n_segs) bytes exactly; 256 canary
//             bytes behind kout, vout and the temporary intact; ZKW_OK; a temporary one byte short returns ZKW_ERR_INVALID and writes nothing
// Prints "ok <cases> ..." and exits 0, or the first mismatch and exits 1. tests/test_gpu_radix_segmented.py builds and runs it.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../era_zkevm_test_harness_amd/csrc/radix_sort.cuh"

#define HIPCHK(x)                                                                                             \
    do {                                                                                                      \
        hipError_t e_ = (x);                                                                                  \
        if (e_ != hipSuccess) { printf("hip error: %s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); exit(2); } \
    } while (0)

static const size_t SIZES[5] = {1, 2047, 2048, 2049, 4097};
static const size_t MAXN = 300 * 4097, MAXSEGS = 300, CANARY = 256;
static const int PAT = 0xA5;
static int g_cases = 0;

struct Rng {
    u64 s;
    u64 next() {
        u64 z = (s += 0x9E3779B97F4A7C15ULL);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    }
};

struct Bufs {
    char *kin, *vin, *kout, *vout, *tmp;
    std::vector<unsigned char> h_k, h_v, h_t, h_in;
};

static bool all_pattern(const unsigned char* p, size_t bytes, size_t* at) {
    for (size_t i = 0; i < bytes; i++)
        if (p[i] != PAT) { *at = i; return false; }
    return true;
}

struct Ref { u64 k; u32 i; };

template <class K>
static void seg_case(zkw_ctx* ctx, Bufs& b, const std::vector<uint64_t>& offs, bool few, unsigned end_bit, const char* what) {
    const char* kt = sizeof(K) == 4 ? "u32" : "u64";
    const size_t n_segs = offs.size() - 1, n = offs[n_segs];
    g_cases++;
    Rng r{0x5E65EED0ull + (u64)n * 7919ull + n_segs * 1000003ull + end_bit * 131ull + sizeof(K) + (few ? 17 : 0)};
    const u64 mask = end_bit >= 64 ? ~0ull : (1ull << end_bit) - 1;
    u64 distinct[3] = {r.next() & mask, r.next() & mask, r.next() & mask};
    std::vector<K> keys(n);
    std::vector<u32> vals(n);
    for (size_t i = 0; i < n; i++) {
        const u64 low = few ? distinct[r.next() % 3] : r.next() & mask;
        keys[i] = (K)(low | (r.next() & ~mask));
        vals[i] = (u32)i;
    }
    const size_t kb = n * sizeof(K), vb = n * 4, tb = radix_temp_bytes(n, n_segs);
    hipStream_t st = ctx->stream;
    HIPCHK(hipMemcpyAsync(b.kin, keys.data(), kb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b.vin, vals.data(), vb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b.kout, PAT, kb + CANARY, st));
    HIPCHK(hipMemsetAsync(b.vout, PAT, vb + CANARY, st));
    HIPCHK(hipMemsetAsync(b.tmp, PAT, tb + CANARY, st));
    size_t at = 0;
#define CASE_FMT "FAIL rs_seg_sort %s %s keys=%s n=%zu segments=%zu end_bit=%u: "
#define CASE_ARGS kt, what, few ? "few_distinct" : "uniform", n, n_segs, end_bit
    {  // one byte short: refused, and nothing launched
        const int rc = radix_sort_pairs_segmented<K>(ctx, b.tmp, tb - 1, (const K*)b.kin, (K*)b.kout, (const u32*)b.vin, (u32*)b.vout, offs.data(), n_segs, end_bit);
        if (rc != ZKW_ERR_INVALID) { printf(CASE_FMT "a temporary one byte short returned %d, expected ZKW_ERR_INVALID\n", CASE_ARGS, rc); exit(1); }
        HIPCHK(hipMemcpyAsync(b.h_k.data(), b.kout, kb + CANARY, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(b.h_v.data(), b.vout, vb + CANARY, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(b.h_t.data(), b.tmp, tb + CANARY, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!all_pattern(b.h_k.data(), kb + CANARY, &at)) { printf(CASE_FMT "the refused call wrote kout, byte %zu\n", CASE_ARGS, at); exit(1); }
        if (!all_pattern(b.h_v.data(), vb + CANARY, &at)) { printf(CASE_FMT "the refused call wrote vout, byte %zu\n", CASE_ARGS, at); exit(1); }
        if (!all_pattern(b.h_t.data(), tb + CANARY, &at)) { printf(CASE_FMT "the refused call wrote the temporary, byte %zu\n", CASE_ARGS, at); exit(1); }
    }
    const int rc = radix_sort_pairs_segmented<K>(ctx, b.tmp, tb, (const K*)b.kin, (K*)b.kout, (const u32*)b.vin, (u32*)b.vout, offs.data(), n_segs, end_bit);
    if (rc != ZKW_OK) { printf(CASE_FMT "returned %d (%s)\n", CASE_ARGS, rc, zkw_last_error()); exit(1); }
    HIPCHK(hipMemcpyAsync(b.h_k.data(), b.kout, kb + CANARY, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b.h_v.data(), b.vout, vb + CANARY, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b.h_t.data(), b.tmp + tb, CANARY, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b.h_in.data(), b.kin, kb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b.h_in.data() + MAXN * 8, b.vin, vb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    // the reference: a stable sort of every segment's positions by the masked key
    std::vector<Ref> ord(n);
    for (size_t i = 0; i < n; i++) ord[i] = Ref{(u64)keys[i] & mask, (u32)i};
    for (size_t s = 0; s < n_segs; s++)
        std::stable_sort(ord.begin() + offs[s], ord.begin() + offs[s + 1], [](const Ref& x, const Ref& y) { return x.k < y.k; });
    const K* gk = reinterpret_cast<const K*>(b.h_k.data());
    const u32* gv = reinterpret_cast<const u32*>(b.h_v.data());
    for (size_t i = 0; i < n; i++) {
        const K ek = keys[ord[i].i];
        const u32 ev = vals[ord[i].i];
        if (gk[i] != ek) { printf(CASE_FMT "kout[%zu] got %llx expected %llx\n", CASE_ARGS, i, (unsigned long long)gk[i], (unsigned long long)ek); exit(1); }
        if (gv[i] != ev) { printf(CASE_FMT "vout[%zu] got %x expected %x (key %llx)\n", CASE_ARGS, i, gv[i], ev, (unsigned long long)ek); exit(1); }
    }
    if (!all_pattern(b.h_k.data() + kb, CANARY, &at)) { printf(CASE_FMT "canary behind kout, byte %zu\n", CASE_ARGS, at); exit(1); }
    if (!all_pattern(b.h_v.data() + vb, CANARY, &at)) { printf(CASE_FMT "canary behind vout, byte %zu\n", CASE_ARGS, at); exit(1); }
    if (!all_pattern(b.h_t.data(), CANARY, &at)) { printf(CASE_FMT "canary behind the temporary (%zu bytes), byte %zu\n", CASE_ARGS, tb, at); exit(1); }
    if (memcmp(b.h_in.data(), keys.data(), kb) != 0) { printf(CASE_FMT "kin was changed\n", CASE_ARGS); exit(1); }
    if (memcmp(b.h_in.data() + MAXN * 8, vals.data(), vb) != 0) { printf(CASE_FMT "vin was changed\n", CASE_ARGS); exit(1); }
#undef CASE_FMT
#undef CASE_ARGS
}

static std::vector<uint64_t> offsets_of(const std::vector<size_t>& sizes) {
    std::vector<uint64_t> o(sizes.size() + 1, 0);
    for (size_t s = 0; s < sizes.size(); s++) o[s + 1] = o[s] + sizes[s];
    return o;
}

static void all_cases(zkw_ctx* ctx, Bufs& b) {
    struct Shape { std::vector<size_t> sizes; const char* what; };
    std::vector<Shape> shapes;
    for (int k = 0; k < 5; k++) shapes.push_back({{SIZES[k]}, "one segment"});
    for (int k = 0; k < 5; k++) shapes.push_back({{SIZES[k], SIZES[(k + 2) % 5]}, "two segments"});
    for (int k = 0; k < 5; k++) shapes.push_back({{SIZES[(k + 3) % 5], SIZES[k], SIZES[(k + 1) % 5]}, "three segments"});
    shapes.push_back({{2049, 0, 1}, "three segments, the middle one empty"});
    {
        Rng r{300};
        std::vector<size_t> many(MAXSEGS);
        for (size_t s = 0; s < MAXSEGS; s++) many[s] = SIZES[r.next() % 5];
        shapes.push_back({many, "300 segments"});
    }
    static const unsigned END_BITS[] = {1, 8, 9, 33};
    for (const Shape& sh : shapes) {
        const std::vector<uint64_t> offs = offsets_of(sh.sizes);
        for (unsigned e : END_BITS)
            for (int few = 0; few < 2; few++) {
                seg_case<u64>(ctx, b, offs, few != 0, e, sh.what);
                if (e <= 32) seg_case<u32>(ctx, b, offs, few != 0, e, sh.what);
            }
    }
}

int main() {
    const auto t0 = std::chrono::steady_clock::now();
    zkw_ctx* ctx = zkw_create(0);
    if (!ctx) { printf("zkw_create failed: %s\n", zkw_last_error()); return 2; }
    Bufs b;
    const size_t tmp_max = radix_temp_bytes(MAXN, MAXSEGS);
    HIPCHK(hipMalloc(&b.kin, MAXN * 8));
    HIPCHK(hipMalloc(&b.vin, MAXN * 4));
    HIPCHK(hipMalloc(&b.kout, MAXN * 8 + CANARY));
    HIPCHK(hipMalloc(&b.vout, MAXN * 4 + CANARY));
    HIPCHK(hipMalloc(&b.tmp, tmp_max + CANARY));
    b.h_k.resize(MAXN * 8 + CANARY);
    b.h_v.resize(MAXN * 4 + CANARY);
    b.h_t.resize(tmp_max + CANARY);
    b.h_in.resize(MAXN * 12);
    all_cases(ctx, b);
    HIPCHK(hipFree(b.kin));
    HIPCHK(hipFree(b.vin));
    HIPCHK(hipFree(b.kout));
    HIPCHK(hipFree(b.vout));
    HIPCHK(hipFree(b.tmp));
    zkw_destroy(ctx);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("ok %d (%.1f s)\n", g_cases, secs);
    return 0;
}
