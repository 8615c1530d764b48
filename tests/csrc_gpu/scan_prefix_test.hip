// scan_prefix_test.hip — the tiled prefix counts and sums of era_zkevm_test_harness_amd/csrc/scan_kernels.cuh against sequential loops on the
// host, bit for bit. The program includes the library's header and calls its drivers (flag_prefix, route_prefix<6>, sum_prefix<1 / 2 / 3>: the
// widths of the log demuxer, the storage sorter, the callstack simulator and the precompiles) on a context from zkw_create(0) of the built
// libzkw.so, with functors that read device arrays.
//   sizes        0, 1, 63, 64, 65, 1 023, 1 024, 1 025, 2 049 (one tile, two, three), 1 048 576 (1 024 tiles: one full round of the loop over
//                the tile totals), 1 048 577 and 1 049 601 (1 025 and 1 026 tiles: the round that starts from `carry`)
//   flag_prefix  flags all 0 / all non-zero / alternating / one in three, seeded / only the last item of every tile; prefix[0..n] and the
//                256 bytes behind prefix[n]; prefix[0] = 0 at n = 0
//   route_prefix routes in [-1, 6): uniform, and long stretches of -1 with one route that never occurs; the six inclusive count rows
//   sum_prefix   values with 2^64 - 1 (-1 as a signed delta) and 2^63 among them, and deltas of +1 / -1 / 0: out[c][0..n] and totals[c] equal the
//                sums modulo 2^64, out[c][n] == totals[c], zeros at n = 0
// and k_flag_prefix_offsets / k_sum_prefix_offsets on 1, 1 024, 1 025 and 2 500 tile totals made for the purpose, through the library's own
// launch (Launcher -> k_single). Prints "ok <cases> ..." and exits 0, or the first mismatch (case, n, index, got, expected) and exits 1; with
// --all it goes on and prints the first mismatch of every failing case. tests/test_gpu_radix_scan_units.py builds and runs it.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../era_zkevm_test_harness_amd/csrc/scan_kernels.cuh"

#define HIPCHK(x)                                                                                             \
    do {                                                                                                      \
        hipError_t e_ = (x);                                                                                  \
        if (e_ != hipSuccess) { printf("hip error: %s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); exit(2); } \
    } while (0)

static const size_t MAXN = 1049601, CANARY = 256;
static const int PAT = 0xA5;
static bool g_all = false;
static int g_cases = 0, g_failed = 0;

static void failed() {
    g_failed++;
    if (!g_all) exit(1);
}

struct Rng {
    u64 s;
    u64 next() {
        u64 z = (s += 0x9E3779B97F4A7C15ULL);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    }
};

struct ArrayFlag {
    const uint8_t* f;
    __device__ u32 operator()(size_t i) const { return f[i]; }
};
struct ArrayRoute {
    const int8_t* r;
    __device__ int operator()(size_t i) const { return r[i]; }
};
template <int K>
struct ArrayVal {
    const u64* v;  // [n][K]
    __device__ void operator()(size_t i, u64 o[K]) const {
#pragma unroll
        for (int c = 0; c < K; c++) o[c] = v[i * K + c];
    }
};

struct Bufs {
    char *in, *out, *totals;           // device: the functor's array, the result (+ canary), sum_prefix's totals (+ canary)
    std::vector<unsigned char> h_out;  // host copy of `out`
};

static bool all_pattern(const unsigned char* p, size_t bytes, size_t* at) {
    for (size_t i = 0; i < bytes; i++)
        if (p[i] != PAT) { *at = i; return false; }
    return true;
}

static const char* const FLAGS[] = {"all_0", "all_nonzero", "alternating", "one_in_three", "last_of_tile"};
static void flag_case(zkw_ctx* ctx, Bufs& b, int kind, size_t n) {
    g_cases++;
    Rng r{0xF1A6ull + n * 31 + kind};
    std::vector<uint8_t> f(n);
    for (size_t i = 0; i < n; i++) {
        switch (kind) {
        case 0: f[i] = 0; break;
        case 1: f[i] = (uint8_t)(1 + i % 255); break;
        case 2: f[i] = i & 1; break;
        case 3: f[i] = r.next() % 3 == 0; break;
        default: f[i] = i % FLAG_PREFIX_TILE == FLAG_PREFIX_TILE - 1 ? 0x80 : 0;
        }
    }
    const size_t ob = (n + 1) * 4;
    hipStream_t st = ctx->stream;
    if (n) HIPCHK(hipMemcpyAsync(b.in, f.data(), n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b.out, PAT, ob + CANARY, st));
    const int rc = flag_prefix(ctx, "flag_prefix_test", ArrayFlag{(const uint8_t*)b.in}, n, (u32*)b.out);
    if (rc != ZKW_OK) { printf("FAIL flag_prefix flags=%s n=%zu: returned %d (%s)\n", FLAGS[kind], n, rc, zkw_last_error()); return failed(); }
    HIPCHK(hipMemcpyAsync(b.h_out.data(), b.out, ob + CANARY, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    const u32* got = reinterpret_cast<const u32*>(b.h_out.data());
    u32 run = 0;
    for (size_t k = 0; k <= n; k++) {
        if (got[k] != run) { printf("FAIL flag_prefix flags=%s n=%zu: prefix[%zu] got %u expected %u\n", FLAGS[kind], n, k, got[k], run); return failed(); }
        if (k < n) run += f[k] != 0;
    }
    size_t at = 0;
    if (!all_pattern(b.h_out.data() + ob, CANARY, &at)) { printf("FAIL flag_prefix flags=%s n=%zu: canary byte %zu behind prefix[n] got %02x expected %02x\n", FLAGS[kind], n, at, b.h_out[ob + at], PAT); return failed(); }
}

static const char* const ROUTES[] = {"uniform", "stretches_without_route_4"};
static void route_case(zkw_ctx* ctx, Bufs& b, int kind, size_t n) {
    constexpr int K = 6;
    g_cases++;
    Rng r{0x2007Eull + n * 31 + kind};
    std::vector<int8_t> route(n);
    for (size_t i = 0; i < n;) {
        if (kind == 0) { route[i++] = (int8_t)((int)(r.next() % (K + 1)) - 1); continue; }
        // a stretch of -1 (up to three tiles long), then a few routed items; route 4 never occurs
        const size_t gap = (size_t)(r.next() % (3 * FLAG_PREFIX_TILE + 1)), some = 1 + (size_t)(r.next() % 200);
        for (size_t j = 0; j < gap && i < n; j++) route[i++] = -1;
        for (size_t j = 0; j < some && i < n; j++) {
            const int c = (int)(r.next() % (K - 1));
            route[i++] = (int8_t)(c >= 4 ? c + 1 : c);
        }
    }
    const size_t ob = (size_t)K * n * 4;
    hipStream_t st = ctx->stream;
    if (n) HIPCHK(hipMemcpyAsync(b.in, route.data(), n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b.out, PAT, ob + CANARY, st));
    const int rc = route_prefix<K>(ctx, "route_prefix_test", ArrayRoute{(const int8_t*)b.in}, n, (u32*)b.out);
    if (rc != ZKW_OK) { printf("FAIL route_prefix<6> routes=%s n=%zu: returned %d (%s)\n", ROUTES[kind], n, rc, zkw_last_error()); return failed(); }
    HIPCHK(hipMemcpyAsync(b.h_out.data(), b.out, ob + CANARY, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    const u32* got = reinterpret_cast<const u32*>(b.h_out.data());
    for (int c = 0; c < K; c++) {
        u32 run = 0;
        for (size_t i = 0; i < n; i++) {
            run += route[i] == c;
            if (got[(size_t)c * n + i] != run) { printf("FAIL route_prefix<6> routes=%s n=%zu: count[%d][%zu] got %u expected %u\n", ROUTES[kind], n, c, i, got[(size_t)c * n + i], run); return failed(); }
        }
    }
    size_t at = 0;
    if (!all_pattern(b.h_out.data() + ob, CANARY, &at)) { printf("FAIL route_prefix<6> routes=%s n=%zu: canary byte %zu behind count[6][n)\n", ROUTES[kind], n, at); return failed(); }
}

static const char* const VALS[] = {"wrapping", "signed_deltas"};
static u64 sum_value(int kind, Rng& r) {
    const u64 x = r.next();
    if (kind == 1) return x % 3 == 0 ? 1ull : x % 3 == 1 ? ~0ull : 0ull;
    switch (x % 5) {
    case 0: return ~0ull;
    case 1: return 1ull << 63;
    case 2: return (x >> 8) % 1000;
    case 3: return r.next();
    default: return 0;
    }
}
template <int K>
static void sum_case(zkw_ctx* ctx, Bufs& b, int kind, size_t n) {
    g_cases++;
    Rng r{0x50Full + n * 31 + kind * 7 + K};
    std::vector<u64> v(n * K);
    for (auto& x : v) x = sum_value(kind, r);
    const size_t ob = (size_t)K * (n + 1) * 8, tb = K * 8;
    hipStream_t st = ctx->stream;
    if (n) HIPCHK(hipMemcpyAsync(b.in, v.data(), n * K * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b.out, PAT, ob + CANARY, st));
    HIPCHK(hipMemsetAsync(b.totals, PAT, tb + CANARY, st));
    const int rc = sum_prefix<K>(ctx, "sum_prefix_test", ArrayVal<K>{(const u64*)b.in}, n, (u64*)b.out, (u64*)b.totals);
    if (rc != ZKW_OK) { printf("FAIL sum_prefix<%d> values=%s n=%zu: returned %d (%s)\n", K, VALS[kind], n, rc, zkw_last_error()); return failed(); }
    unsigned char h_tot[K * 8 + CANARY];
    HIPCHK(hipMemcpyAsync(b.h_out.data(), b.out, ob + CANARY, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_tot, b.totals, tb + CANARY, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    const u64* got = reinterpret_cast<const u64*>(b.h_out.data());
    const u64* tot = reinterpret_cast<const u64*>(h_tot);
    for (int c = 0; c < K; c++) {
        u64 run = 0;
        for (size_t i = 0; i <= n; i++) {
            const u64 g = got[(size_t)c * (n + 1) + i];
            if (g != run) { printf("FAIL sum_prefix<%d> values=%s n=%zu: out[%d][%zu] got %llx expected %llx\n", K, VALS[kind], n, c, i, (unsigned long long)g, (unsigned long long)run); return failed(); }
            if (i < n) run += v[i * K + c];
        }
        if (tot[c] != run) { printf("FAIL sum_prefix<%d> values=%s n=%zu: totals[%d] got %llx expected %llx\n", K, VALS[kind], n, c, (unsigned long long)tot[c], (unsigned long long)run); return failed(); }
        if (tot[c] != got[(size_t)c * (n + 1) + n]) { printf("FAIL sum_prefix<%d> values=%s n=%zu: out[%d][n] differs from totals[%d]\n", K, VALS[kind], n, c, c); return failed(); }
    }
    size_t at = 0;
    if (!all_pattern(b.h_out.data() + ob, CANARY, &at)) { printf("FAIL sum_prefix<%d> values=%s n=%zu: canary byte %zu behind out[%d][n]\n", K, VALS[kind], n, at, K - 1); return failed(); }
    if (!all_pattern(h_tot + tb, CANARY, &at)) { printf("FAIL sum_prefix<%d> values=%s n=%zu: canary byte %zu behind totals\n", K, VALS[kind], n, at); return failed(); }
}

// the bodies through the library's launch of a body on a context of its own (Launcher::go -> k_single)
static int launch_flag_offsets(zkw_ctx* ctx, u32* tile_sums, u32 n_tiles) {
    ZKW_LAUNCH(ctx, k_flag_prefix_offsets, 1, 1024, tile_sums, n_tiles);
    return ZKW_OK;
}
static int launch_sum_offsets(zkw_ctx* ctx, u64* tile_sums, u32 n_tiles, u64* total, u64* out_last) {
    ZKW_LAUNCH(ctx, k_sum_prefix_offsets, 1, 1024, tile_sums, n_tiles, total, out_last);
    return ZKW_OK;
}

static void flag_offsets_case(zkw_ctx* ctx, Bufs& b, u32 n) {
    g_cases++;
    Rng r{0x0FF5E7ull + n};
    std::vector<u32> h(n), got(n + CANARY / 4);
    for (auto& x : h) x = (u32)(r.next() % (FLAG_PREFIX_TILE + 1));  // a tile's count
    u32* d = reinterpret_cast<u32*>(b.out);
    HIPCHK(hipMemsetAsync(d, PAT, n * 4 + CANARY, ctx->stream));
    HIPCHK(hipMemcpyAsync(d, h.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    const int rc = launch_flag_offsets(ctx, d, n);
    if (rc != ZKW_OK) { printf("FAIL k_flag_prefix_offsets n_tiles=%u: launch returned %d (%s)\n", n, rc, zkw_last_error()); return failed(); }
    HIPCHK(hipMemcpyAsync(got.data(), d, n * 4 + CANARY, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    u32 run = 0;
    for (u32 i = 0; i < n; i++) {
        if (got[i] != run) { printf("FAIL k_flag_prefix_offsets n_tiles=%u: tile_sums[%u] got %u expected %u\n", n, i, got[i], run); return failed(); }
        run += h[i];
    }
    size_t at = 0;
    if (!all_pattern(reinterpret_cast<unsigned char*>(got.data() + n), CANARY, &at)) { printf("FAIL k_flag_prefix_offsets n_tiles=%u: canary byte %zu behind tile_sums\n", n, at); return failed(); }
}

static void sum_offsets_case(zkw_ctx* ctx, Bufs& b, u32 n) {
    g_cases++;
    Rng r{0x50FF5E7ull + n};
    std::vector<u64> h(n), got(n + CANARY / 8), two(2 + CANARY / 8);
    for (auto& x : h) x = sum_value(0, r);
    u64* d = reinterpret_cast<u64*>(b.out);
    u64* dt = reinterpret_cast<u64*>(b.totals);  // total, out_last
    HIPCHK(hipMemsetAsync(d, PAT, n * 8 + CANARY, ctx->stream));
    HIPCHK(hipMemsetAsync(dt, PAT, 16 + CANARY, ctx->stream));
    HIPCHK(hipMemcpyAsync(d, h.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
    const int rc = launch_sum_offsets(ctx, d, n, dt, dt + 1);
    if (rc != ZKW_OK) { printf("FAIL k_sum_prefix_offsets n_tiles=%u: launch returned %d (%s)\n", n, rc, zkw_last_error()); return failed(); }
    HIPCHK(hipMemcpyAsync(got.data(), d, n * 8 + CANARY, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(two.data(), dt, 16 + CANARY, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    u64 run = 0;
    for (u32 i = 0; i < n; i++) {
        if (got[i] != run) { printf("FAIL k_sum_prefix_offsets n_tiles=%u: tile_sums[%u] got %llx expected %llx\n", n, i, (unsigned long long)got[i], (unsigned long long)run); return failed(); }
        run += h[i];
    }
    if (two[0] != run || two[1] != run) { printf("FAIL k_sum_prefix_offsets n_tiles=%u: total %llx, out_last %llx, expected %llx\n", n, (unsigned long long)two[0], (unsigned long long)two[1], (unsigned long long)run); return failed(); }
    size_t at = 0;
    if (!all_pattern(reinterpret_cast<unsigned char*>(got.data() + n), CANARY, &at)) { printf("FAIL k_sum_prefix_offsets n_tiles=%u: canary byte %zu behind tile_sums\n", n, at); return failed(); }
    if (!all_pattern(reinterpret_cast<unsigned char*>(two.data() + 2), CANARY, &at)) { printf("FAIL k_sum_prefix_offsets n_tiles=%u: canary byte %zu behind the totals\n", n, at); return failed(); }
}

int main(int argc, char** argv) {
    g_all = argc > 1 && strcmp(argv[1], "--all") == 0;
    const auto t0 = std::chrono::steady_clock::now();
    zkw_ctx* ctx = zkw_create(0);
    if (!ctx) { printf("zkw_create failed: %s\n", zkw_last_error()); return 2; }
    Bufs b;
    const size_t out_max = 6 * MAXN * 4 > 3 * (MAXN + 1) * 8 ? 6 * MAXN * 4 : 3 * (MAXN + 1) * 8;
    HIPCHK(hipMalloc(&b.in, MAXN * 3 * 8));
    HIPCHK(hipMalloc(&b.out, out_max + CANARY));
    HIPCHK(hipMalloc(&b.totals, 3 * 8 + CANARY));
    b.h_out.resize(out_max + CANARY);
    static const size_t SIZES[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 1048576, 1048577, 1049601};
    for (size_t n : SIZES) {
        for (int kind = 0; kind < 5; kind++) flag_case(ctx, b, kind, n);
        for (int kind = 0; kind < 2; kind++) route_case(ctx, b, kind, n);
        for (int kind = 0; kind < 2; kind++) {
            sum_case<1>(ctx, b, kind, n);
            sum_case<2>(ctx, b, kind, n);
            sum_case<3>(ctx, b, kind, n);
        }
    }
    const int drivers = g_cases;
    for (u32 n : {1u, 1024u, 1025u, 2500u}) {
        flag_offsets_case(ctx, b, n);
        sum_offsets_case(ctx, b, n);
    }
    HIPCHK(hipFree(b.in));
    HIPCHK(hipFree(b.out));
    HIPCHK(hipFree(b.totals));
    zkw_destroy(ctx);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (g_failed) { printf("%d of %d cases failed\n", g_failed, g_cases); return 1; }
    printf("ok %d (%d driver cases, %d scan bodies, %.1f s)\n", g_cases, drivers, g_cases - drivers, secs);
    return 0;
}
