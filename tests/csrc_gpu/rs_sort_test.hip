// rs_sort_test.hip — the library's radix sort (era_zkevm_test_harness_amd/csrc/radix_sort.cuh) against std::stable_sort on the host, bit for
// bit. The program includes the library's header and calls its driver, radix_sort_pairs<u32> / <u64>, on a context from zkw_create(0) of
// the built libzkw.so (Launcher, zkw_fail and the caches are the library's): the ping-pong between kout and the temporary, the masks and
// the chunked scan of the histogram are what is under test.
//   sizes     0, 1, 63 .. 4 097 (around a wave of 64, a wave's share of 512 and a tile of 2 048), 131 072 (64 tiles: exactly one chunk of
//             16 384 histogram entries), 131 073 (two chunks, a last tile of one pair), 133 849 (66 tiles: a chunk border inside a digit's run
//             of tiles), 262 145 (129 tiles, three chunks)
//   end_bit   1, 7, 8, 9, 16, 32, 33 and, for u64, 40 and 64: one pass, even and odd numbers of passes, 1-bit last masks, the sorters' 33;
//             the key bits above end_bit are random and must be ignored
//   keys      uniform / all equal / only digits 0 and 255 / descending / sorted / constant per aligned 64 (a whole wave matches in one
//             ballot) / constant per aligned 512 / at most five distinct keys in long runs / {0, 1, 2^8 - 1, 2^8, 2^32 - 1, 2^32, 2^64 - 1};
//             every family at 2 049, 133 849 and 262 145, uniform and two more at the other sizes
//   values    seeded u32 with 0 and 0xFFFFFFFF among them; an iota as well where equal keys make stability visible
//   checks    kout / vout equal the reference; kin / vin unchanged; the temporary is radix_temp_bytes(n) bytes exactly; 256 canary bytes
//             behind kout, vout and the temporary intact; ZKW_OK; a temporary one byte short returns ZKW_ERR_INVALID and writes nothing
// and the two scan bodies on arrays made for the purpose, through the library's own launch (Launcher -> k_single): k_rs_scan_b on 1 .. 2 500
// chunk totals (above 1 024 its loop carries a sum into a second and third round: the driver gets there above 134 217 728 pairs), k_rs_scan_a
// on 1 .. 40 000 entries. Prints "ok <cases> ..." and exits 0, or the first mismatch (case, n, end_bit, index, got, expected) and exits 1;
// with --all it goes on and prints the first mismatch of every failing case. tests/test_gpu_radix_scan_units.py builds and runs it.
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

static const size_t MAXN = 262145, CANARY = 256;
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

enum { F_UNIFORM, F_EQUAL, F_DIGITS_0_255, F_DESCENDING, F_SORTED, F_GROUP64, F_GROUP512, F_FEW, F_SPECIAL, N_FAMILIES };
static const char* const FAMILY[N_FAMILIES] = {"uniform", "all_equal", "digits_0_255", "descending", "sorted", "group64", "group512", "few_distinct", "special"};
static bool shows_stability(int f) { return f == F_EQUAL || f == F_GROUP64 || f == F_GROUP512 || f == F_FEW || f == F_SPECIAL; }
static u64 low_mask(unsigned bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }

// the low end_bit bits of the keys of a family
static void family_keys(int fam, size_t n, u64 mask, Rng& r, std::vector<u64>& k) {
    static const u64 SPECIAL[7] = {0, 1, 255, 256, 0xFFFFFFFFull, 1ull << 32, ~0ull};
    k.resize(n);
    u64 c = r.next() & mask, prev = 0;
    switch (fam) {
    case F_UNIFORM: case F_DESCENDING: case F_SORTED:
        for (size_t i = 0; i < n; i++) k[i] = r.next() & mask;
        if (fam != F_UNIFORM) std::sort(k.begin(), k.end());
        if (fam == F_DESCENDING) std::reverse(k.begin(), k.end());
        break;
    case F_EQUAL:
        for (size_t i = 0; i < n; i++) k[i] = c;
        break;
    case F_DIGITS_0_255:
        for (size_t i = 0; i < n; i++) {
            const u64 x = r.next();
            u64 v = 0;
            for (int b = 0; b < 8; b++) if ((x >> b) & 1) v |= 0xFFull << (8 * b);
            k[i] = v & mask;
        }
        break;
    case F_GROUP64:
        for (size_t i = 0; i < n; i++) {
            if (i % 64 == 0) c = r.next() & mask;
            k[i] = c;
        }
        break;
    case F_GROUP512:
        for (size_t i = 0; i < n; i++) {
            if (i % 512 == 0) {
                c = r.next() & mask;
                if (i && c == prev) c = (c + 1) & mask;
                prev = c;
            }
            k[i] = c;
        }
        break;
    case F_FEW: {
        u64 d[5];
        const int nd = 2 + (int)(r.next() % 4);
        for (int j = 0; j < nd; j++) d[j] = r.next() & mask;
        for (size_t i = 0; i < n;) {
            const size_t len = 1 + (size_t)(r.next() % (n / 3 + 1));
            const u64 v = d[r.next() % nd];
            for (size_t j = 0; j < len && i < n; j++) k[i++] = v;
        }
        break;
    }
    default:
        for (size_t i = 0; i < n; i++) k[i] = SPECIAL[r.next() % 7] & mask;
    }
}

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
static void sort_case(zkw_ctx* ctx, Bufs& b, int fam, bool iota, size_t n, unsigned end_bit) {
    const char* kt = sizeof(K) == 4 ? "u32" : "u64";
    const char* vk = iota ? "iota" : "random";
    g_cases++;
    Rng r{0x5EED0000ull + (u64)fam * 1000003ull + (u64)n * 7919ull + end_bit * 131ull + sizeof(K) + (iota ? 17 : 0)};
    const u64 mask = low_mask(end_bit);
    std::vector<u64> low;
    family_keys(fam, n, mask, r, low);
    std::vector<K> keys(n);
    std::vector<u32> vals(n);
    for (size_t i = 0; i < n; i++) {
        keys[i] = (K)(low[i] | (r.next() & ~mask));  // random bits above end_bit (none when end_bit is the key's width)
        u32 v = (u32)r.next();
        if (i % 13 == 0) v = 0;
        if (i % 13 == 1) v = 0xFFFFFFFFu;
        vals[i] = iota ? (u32)i : v;
    }
    const size_t kb = n * sizeof(K), vb = n * 4, tb = radix_temp_bytes(n);
    hipStream_t st = ctx->stream;
    if (n) {
        HIPCHK(hipMemcpyAsync(b.kin, keys.data(), kb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b.vin, vals.data(), vb, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemsetAsync(b.kout, PAT, kb + CANARY, st));
    HIPCHK(hipMemsetAsync(b.vout, PAT, vb + CANARY, st));
    HIPCHK(hipMemsetAsync(b.tmp, PAT, tb + CANARY, st));
    size_t at = 0;
#define CASE_FMT "FAIL rs_sort %s family=%s values=%s n=%zu end_bit=%u: "
#define CASE_ARGS kt, FAMILY[fam], vk, n, end_bit
    if (n) {  // one byte short: refused, and nothing launched
        const int rc = radix_sort_pairs<K>(ctx, b.tmp, tb - 1, (const K*)b.kin, (K*)b.kout, (const u32*)b.vin, (u32*)b.vout, n, end_bit);
        if (rc != ZKW_ERR_INVALID) { printf(CASE_FMT "a temporary of radix_temp_bytes(n) - 1 bytes returned %d, expected ZKW_ERR_INVALID\n", CASE_ARGS, rc); return failed(); }
        HIPCHK(hipMemcpyAsync(b.h_k.data(), b.kout, kb + CANARY, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(b.h_v.data(), b.vout, vb + CANARY, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(b.h_t.data(), b.tmp, tb + CANARY, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!all_pattern(b.h_k.data(), kb + CANARY, &at)) { printf(CASE_FMT "the refused call wrote kout, byte %zu\n", CASE_ARGS, at); return failed(); }
        if (!all_pattern(b.h_v.data(), vb + CANARY, &at)) { printf(CASE_FMT "the refused call wrote vout, byte %zu\n", CASE_ARGS, at); return failed(); }
        if (!all_pattern(b.h_t.data(), tb + CANARY, &at)) { printf(CASE_FMT "the refused call wrote the temporary, byte %zu\n", CASE_ARGS, at); return failed(); }
    }
    const int rc = radix_sort_pairs<K>(ctx, b.tmp, tb, (const K*)b.kin, (K*)b.kout, (const u32*)b.vin, (u32*)b.vout, n, end_bit);
    if (rc != ZKW_OK) { printf(CASE_FMT "returned %d (%s)\n", CASE_ARGS, rc, zkw_last_error()); return failed(); }
    HIPCHK(hipMemcpyAsync(b.h_k.data(), b.kout, kb + CANARY, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b.h_v.data(), b.vout, vb + CANARY, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b.h_t.data(), b.tmp + tb, CANARY, hipMemcpyDeviceToHost, st));
    if (n) {
        HIPCHK(hipMemcpyAsync(b.h_in.data(), b.kin, kb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(b.h_in.data() + MAXN * 8, b.vin, vb, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    // the reference: a stable sort of the positions by the masked key
    std::vector<Ref> ord(n);
    for (size_t i = 0; i < n; i++) ord[i] = Ref{(u64)keys[i] & mask, (u32)i};
    std::stable_sort(ord.begin(), ord.end(), [](const Ref& x, const Ref& y) { return x.k < y.k; });
    const K* gk = reinterpret_cast<const K*>(b.h_k.data());
    const u32* gv = reinterpret_cast<const u32*>(b.h_v.data());
    for (size_t i = 0; i < n; i++) {
        const K ek = keys[ord[i].i];
        const u32 ev = vals[ord[i].i];
        if (gk[i] != ek) { printf(CASE_FMT "kout[%zu] got %llx expected %llx\n", CASE_ARGS, i, (unsigned long long)gk[i], (unsigned long long)ek); return failed(); }
        if (gv[i] != ev) { printf(CASE_FMT "vout[%zu] got %x expected %x (key %llx)\n", CASE_ARGS, i, gv[i], ev, (unsigned long long)ek); return failed(); }
    }
    if (!all_pattern(b.h_k.data() + kb, CANARY, &at)) { printf(CASE_FMT "canary behind kout, byte %zu got %02x expected %02x\n", CASE_ARGS, at, b.h_k[kb + at], PAT); return failed(); }
    if (!all_pattern(b.h_v.data() + vb, CANARY, &at)) { printf(CASE_FMT "canary behind vout, byte %zu got %02x expected %02x\n", CASE_ARGS, at, b.h_v[vb + at], PAT); return failed(); }
    if (!all_pattern(b.h_t.data(), CANARY, &at)) { printf(CASE_FMT "canary behind the temporary (%zu bytes), byte %zu got %02x expected %02x\n", CASE_ARGS, tb, at, b.h_t[at], PAT); return failed(); }
    if (n && memcmp(b.h_in.data(), keys.data(), kb) != 0) { printf(CASE_FMT "kin was changed\n", CASE_ARGS); return failed(); }
    if (n && memcmp(b.h_in.data() + MAXN * 8, vals.data(), vb) != 0) { printf(CASE_FMT "vin was changed\n", CASE_ARGS); return failed(); }
#undef CASE_FMT
#undef CASE_ARGS
}

// the bodies through the library's launch of a body on a context of its own (Launcher::go -> k_single)
static int launch_scan_a(zkw_ctx* ctx, u32* hist, size_t n_entries, u32* chunk_tot) {
    ZKW_LAUNCH(ctx, k_rs_scan_a, (n_entries + RS_CHUNK - 1) / RS_CHUNK, 1024, hist, n_entries, chunk_tot);
    return ZKW_OK;
}
static int launch_scan_b(zkw_ctx* ctx, u32* chunk_tot, u32 n_chunks) {
    ZKW_LAUNCH(ctx, k_rs_scan_b, 1, 1024, chunk_tot, n_chunks);
    return ZKW_OK;
}

static void scan_b_case(zkw_ctx* ctx, Bufs& b, u32 n) {
    g_cases++;
    Rng r{0xB0D1E5ull + n};
    std::vector<u32> h(n), got(n + CANARY / 4);
    for (u32 i = 0; i < n; i++) h[i] = (u32)(r.next() % (RS_TILE * 64 + 1));  // at most a chunk of full tiles of one digit
    u32* d = reinterpret_cast<u32*>(b.tmp);
    HIPCHK(hipMemsetAsync(d, PAT, n * 4 + CANARY, ctx->stream));
    HIPCHK(hipMemcpyAsync(d, h.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    const int rc = launch_scan_b(ctx, d, n);
    if (rc != ZKW_OK) { printf("FAIL k_rs_scan_b n_chunks=%u: launch returned %d (%s)\n", n, rc, zkw_last_error()); return failed(); }
    HIPCHK(hipMemcpyAsync(got.data(), d, n * 4 + CANARY, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    u32 run = 0;
    for (u32 i = 0; i < n; i++) {
        if (got[i] != run) { printf("FAIL k_rs_scan_b n_chunks=%u: chunk_tot[%u] got %u expected %u\n", n, i, got[i], run); return failed(); }
        run += h[i];
    }
    size_t at = 0;
    if (!all_pattern(reinterpret_cast<unsigned char*>(got.data() + n), CANARY, &at)) { printf("FAIL k_rs_scan_b n_chunks=%u: canary byte %zu behind chunk_tot\n", n, at); return failed(); }
}

static void scan_a_case(zkw_ctx* ctx, Bufs& b, size_t n) {
    g_cases++;
    Rng r{0xA0D1E5ull + n};
    const size_t chunks = (n + RS_CHUNK - 1) / RS_CHUNK;
    std::vector<u32> h(n), got(n + CANARY / 4), tot(chunks + CANARY / 4);
    for (size_t i = 0; i < n; i++) h[i] = (u32)(r.next() % (RS_TILE + 1));  // a tile's count of one digit
    u32* d = reinterpret_cast<u32*>(b.tmp);
    u32* dt = reinterpret_cast<u32*>(b.kout);
    HIPCHK(hipMemsetAsync(d, PAT, n * 4 + CANARY, ctx->stream));
    HIPCHK(hipMemsetAsync(dt, PAT, chunks * 4 + CANARY, ctx->stream));
    HIPCHK(hipMemcpyAsync(d, h.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    const int rc = launch_scan_a(ctx, d, n, dt);
    if (rc != ZKW_OK) { printf("FAIL k_rs_scan_a n_entries=%zu: launch returned %d (%s)\n", n, rc, zkw_last_error()); return failed(); }
    HIPCHK(hipMemcpyAsync(got.data(), d, n * 4 + CANARY, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(tot.data(), dt, chunks * 4 + CANARY, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    u32 run = 0;
    for (size_t i = 0; i < n; i++) {
        if (i % RS_CHUNK == 0) run = 0;
        if (got[i] != run) { printf("FAIL k_rs_scan_a n_entries=%zu: hist[%zu] got %u expected %u\n", n, i, got[i], run); return failed(); }
        run += h[i];
        if (i % RS_CHUNK == RS_CHUNK - 1 || i == n - 1) {
            const size_t c = i / RS_CHUNK;
            if (tot[c] != run) { printf("FAIL k_rs_scan_a n_entries=%zu: chunk_tot[%zu] got %u expected %u\n", n, c, tot[c], run); return failed(); }
        }
    }
    size_t at = 0;
    if (!all_pattern(reinterpret_cast<unsigned char*>(got.data() + n), CANARY, &at)) { printf("FAIL k_rs_scan_a n_entries=%zu: canary byte %zu behind hist[n_entries)\n", n, at); return failed(); }
    if (!all_pattern(reinterpret_cast<unsigned char*>(tot.data() + chunks), CANARY, &at)) { printf("FAIL k_rs_scan_a n_entries=%zu: canary byte %zu behind chunk_tot\n", n, at); return failed(); }
}

template <class K>
static void sort_cases(zkw_ctx* ctx, Bufs& b) {
    static const size_t SIZES[] = {0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, 131072, 131073, 133849, 262145};
    static const unsigned END_BITS[] = {1, 7, 8, 9, 16, 32, 33, 40, 64};
    int rot = 1;
    for (size_t n : SIZES) {
        const bool every = n == 2049 || n == 133849 || n == 262145;
        bool use[N_FAMILIES];
        for (int f = 0; f < N_FAMILIES; f++) use[f] = every || f == F_UNIFORM;
        if (!every) {  // two more families, by rotation
            use[1 + rot % (N_FAMILIES - 1)] = true;
            use[1 + (rot + 1) % (N_FAMILIES - 1)] = true;
            rot += 2;
        }
        for (int f = 0; f < N_FAMILIES; f++) {
            if (!use[f]) continue;
            for (unsigned e : END_BITS) {
                if (e > 8 * sizeof(K)) continue;
                sort_case<K>(ctx, b, f, false, n, e);
                if (shows_stability(f)) sort_case<K>(ctx, b, f, true, n, e);
            }
        }
    }
}

int main(int argc, char** argv) {
    g_all = argc > 1 && strcmp(argv[1], "--all") == 0;
    const auto t0 = std::chrono::steady_clock::now();
    zkw_ctx* ctx = zkw_create(0);
    if (!ctx) { printf("zkw_create failed: %s\n", zkw_last_error()); return 2; }
    Bufs b;
    const size_t tmp_max = radix_temp_bytes(MAXN);
    HIPCHK(hipMalloc(&b.kin, MAXN * 8));
    HIPCHK(hipMalloc(&b.vin, MAXN * 4));
    HIPCHK(hipMalloc(&b.kout, MAXN * 8 + CANARY));
    HIPCHK(hipMalloc(&b.vout, MAXN * 4 + CANARY));
    HIPCHK(hipMalloc(&b.tmp, tmp_max + CANARY));
    b.h_k.resize(MAXN * 8 + CANARY);
    b.h_v.resize(MAXN * 4 + CANARY);
    b.h_t.resize(tmp_max + CANARY);
    b.h_in.resize(MAXN * 12);
    sort_cases<u32>(ctx, b);
    sort_cases<u64>(ctx, b);
    const int sorts = g_cases;
    for (u32 n : {1u, 1023u, 1024u, 1025u, 2048u, 2500u}) scan_b_case(ctx, b, n);
    for (size_t n : {(size_t)1, (size_t)16383, (size_t)16384, (size_t)16385, (size_t)40000}) scan_a_case(ctx, b, n);
    HIPCHK(hipFree(b.kin));
    HIPCHK(hipFree(b.vin));
    HIPCHK(hipFree(b.kout));
    HIPCHK(hipFree(b.vout));
    HIPCHK(hipFree(b.tmp));
    zkw_destroy(ctx);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (g_failed) { printf("%d of %d cases failed\n", g_failed, g_cases); return 1; }
    printf("ok %d (%d sorts, %d scan bodies, %.1f s)\n", g_cases, sorts, g_cases - sorts, secs);
    return 0;
}
