// zkw_kzg.hip — the EIP-4844 blob witness behind include/zkw.h: zkw_kzg_settings (the monomial trusted setup as a fixed-base table in
// HBM), zkw_kzg_commit and zkw_eip4844_witness (generate_eip4844_witness, src/utils.rs:119-231 of the reference). Kernels and the
// decomposition: kzg_kernels.cuh; field and group arithmetic: bls12_381.cuh.
#include "zkw_ctx.h"
#include "kzg_kernels.cuh"

#include <cstddef>

static_assert(sizeof(zkw_eip4844_record) == KZG_REC_BYTES && offsetof(zkw_eip4844_record, linear_hash) == KZG_REC_LINEAR &&
                  offsetof(zkw_eip4844_record, versioned_hash) == KZG_REC_VERSIONED && offsetof(zkw_eip4844_record, output_hash) == KZG_REC_OUTPUT &&
                  offsetof(zkw_eip4844_record, evaluation_point) == KZG_REC_Z && offsetof(zkw_eip4844_record, opening_value) == KZG_REC_Y &&
                  offsetof(zkw_eip4844_record, commitment) == KZG_REC_COMMITMENT,
              "kzg_kernels.cuh writes zkw_eip4844_record by byte offset");
static_assert(sizeof(bls::G1Aff) == 96 && sizeof(bls::G1Jac) == 144, "table entries are 96 bytes, bucket sums 144");

struct zkw_kzg_settings {
    zkw_ctx* ctx = nullptr;
    size_t n = 0, bytes = 0;
    bls::G1Aff* table = nullptr;  // [32][n]: table[w * n + k] = 2^(8 w) S[k]
};

static const char* kzg_reason(u32 status) {
    switch (status) {
        case bls::G1_NOT_COMPRESSED: return "bit 7 of its first byte is clear (not a compressed point)";
        case bls::G1_BAD_INFINITY: return "the infinity flag is set with other bits";
        case bls::G1_X_TOO_LARGE: return "x is not below p";
        case bls::G1_NOT_ON_CURVE: return "x has no y on y^2 = x^3 + 4";
        default: return "the point is outside the order-r subgroup";
    }
}

extern "C" int zkw_kzg_settings_create(zkw_ctx* ctx, const uint8_t* g1_monomial, size_t n_points, zkw_kzg_settings** out) {
    if (!ctx || !out || !g1_monomial) return fail(ZKW_ERR_INVALID, "zkw_kzg_settings_create: null argument");
    if (n_points == 0 || n_points > KZG_MAX_POINTS) return fail(ZKW_ERR_INVALID, "zkw_kzg_settings_create: 1 to %u points, not %zu", (unsigned)KZG_MAX_POINTS, n_points);
    if (ctx->batch) return fail(ZKW_ERR_INVALID, "zkw_kzg_settings_create: the context belongs to a batch of blocks");
    HIP_TRY(hipSetDevice(ctx->device));
    *out = nullptr;
    const uint8_t* d_in = nullptr;
    ZKW_TRY(ctx->in("kzg_in_points", g1_monomial, n_points * 48, &d_in));
    u32* d_status = nullptr;
    ZKW_TRY(ctx->scratch_t<u32>("kzg_status", n_points, &d_status));
    zkw_kzg_settings* s = new zkw_kzg_settings();
    s->ctx = ctx;
    s->n = n_points;
    s->bytes = (size_t)KZG_WINDOWS * n_points * sizeof(bls::G1Aff);
    auto drop = [&](int rc) {
        (void)ctx->sync_stream();  // nothing queued may still write the table
        if (s->table) dev_free(s->table);
        delete s;
        return rc;
    };
    const hipError_t e = dev_malloc(&s->table, s->bytes + 64);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return drop(fail(ZKW_ERR_OOM, "zkw_kzg_settings_create: %zu points need %zu bytes of device memory: %s", n_points, s->bytes, hipGetErrorString(e)));
    }
    std::vector<u32> status(n_points);
    int rc = [&]() -> int {
        { Prof _p(ctx, "k_kzg_decompress"); ZKW_LAUNCH(ctx, k_kzg_decompress, blocks_for(n_points, 64), 64, d_in, (u32)n_points, s->table, d_status); }
        return ctx->read_small(status.data(), d_status, n_points * sizeof(u32));
    }();
    if (rc != ZKW_OK) return drop(rc);
    for (size_t k = 0; k < n_points; k++)
        if (status[k] != bls::G1_OK) return drop(fail(ZKW_ERR_INVALID, "zkw_kzg_settings_create: point %zu is refused: %s", k, kzg_reason(status[k])));
    rc = [&]() -> int {
        { Prof _p(ctx, "k_kzg_table"); ZKW_LAUNCH_2D(ctx, k_kzg_table, blocks_for(n_points, 64), KZG_WINDOWS - 1, 64, s->table, (u32)n_points); }
        HIP_TRY(ctx->sync_stream());  // other contexts read the table without any ordering with this stream
        return ZKW_OK;
    }();
    if (rc != ZKW_OK) return drop(rc);
    ctx_retain(ctx);
    *out = s;
    return ZKW_OK;
}

extern "C" void zkw_kzg_settings_free(zkw_kzg_settings* s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)s->ctx->sync_stream();
    dev_free(s->table);
    zkw_ctx* owner = s->ctx;
    delete s;
    ctx_release(owner);
}
extern "C" size_t zkw_kzg_settings_num_points(const zkw_kzg_settings* s) { return s ? s->n : 0; }
extern "C" size_t zkw_kzg_settings_bytes(const zkw_kzg_settings* s) { return s ? s->bytes : 0; }

// buckets of n_polys polynomials, their eight bit sums, then their commitments at d_out + j * out_stride
static int kzg_commit_device(const zkw_kzg_settings* s, zkw_ctx* ctx, KzgSrc src, u32 poly_stride, size_t n_polys, uint8_t* d_out, u32 out_stride) {
    bls::G1Jac* buckets = nullptr;
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_buckets", n_polys * (KZG_BUCKETS + 8), &buckets));
    { Prof _p(ctx, "k_kzg_accumulate"); ZKW_LAUNCH_2D(ctx, k_kzg_accumulate, KZG_BUCKETS - 1, n_polys, KZG_ACC_THREADS, src, poly_stride, (const bls::G1Aff*)s->table, (u32)s->n, buckets); }
    bls::G1Jac* sums = buckets + n_polys * KZG_BUCKETS;
    { Prof _p(ctx, "k_kzg_finish"); ZKW_LAUNCH_2D(ctx, k_kzg_finish, n_polys, 2, KZG_FIN_THREADS, (const bls::G1Jac*)buckets, sums); }
    { Prof _p(ctx, "k_kzg_compress"); ZKW_LAUNCH(ctx, k_kzg_compress, blocks_for(n_polys, 64), 64, (const bls::G1Jac*)sums, (u32)n_polys, d_out, out_stride); }
    return ZKW_OK;
}

static int kzg_check_call(const char* who, const zkw_kzg_settings* s, zkw_ctx* ctx, size_t n) {
    if (ctx->device != s->ctx->device) return fail(ZKW_ERR_INVALID, "%s: the settings live on device %d, the context on device %d", who, s->ctx->device, ctx->device);
    if (n > 65535) return fail(ZKW_ERR_INVALID, "%s: at most 65535 polynomials per call, not %zu", who, n);
    return ZKW_OK;
}

extern "C" int zkw_kzg_commit(const zkw_kzg_settings* s, zkw_ctx* ctx, const uint8_t* coeffs, size_t n_coeffs, size_t n_polys, uint8_t* out) {
    if (!s || !ctx || (n_polys && (!out || (n_coeffs && !coeffs)))) return fail(ZKW_ERR_INVALID, "zkw_kzg_commit: null argument");
    if (n_coeffs > s->n) return fail(ZKW_ERR_INVALID, "zkw_kzg_commit: %zu coefficients, the settings hold %zu points", n_coeffs, s->n);
    ZKW_TRY(kzg_check_call("zkw_kzg_commit", s, ctx, n_polys));
    if (n_polys == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t total = n_coeffs * n_polys;
    const uint8_t* d_c = nullptr;
    ZKW_TRY(ctx->in("kzg_in_coeffs", coeffs, total * 32, &d_c));
    if (total) {
        u32 *d_flag = nullptr, h_flag = ~0u;
        ZKW_TRY(ctx->scratch_t<u32>("kzg_flag", 1, &d_flag));
        HIP_TRY(ctx->memset_async(d_flag, 0xFF, sizeof(u32)));
        { Prof _p(ctx, "k_kzg_check"); ZKW_LAUNCH(ctx, k_kzg_check, blocks_for(total, 256), 256, d_c, (u32)total, d_flag); }
        ZKW_TRY(ctx->read_small(&h_flag, d_flag, sizeof h_flag));
        if (h_flag != ~0u)
            return fail(ZKW_ERR_INVALID, "zkw_kzg_commit: coefficient %zu of polynomial %zu is not below r", (size_t)h_flag % n_coeffs, (size_t)h_flag / n_coeffs);
    }
    uint8_t* d_out = nullptr;
    ZKW_TRY(ctx->out("kzg_out", out, n_polys * 48, &d_out));
    ZKW_TRY(kzg_commit_device(s, ctx, KzgSrc{d_c, (u32)n_coeffs, 0}, (u32)(n_coeffs * 32), n_polys, d_out, 48));
    ZKW_TRY(ctx->finish_out(out, d_out, n_polys * 48));
    return ctx->sync_if_host();
}

extern "C" int zkw_eip4844_witness(const zkw_kzg_settings* s, zkw_ctx* ctx, const uint8_t* blobs, size_t n_blobs, zkw_eip4844_record* out) {
    if (!s || !ctx || (n_blobs && (!blobs || !out))) return fail(ZKW_ERR_INVALID, "zkw_eip4844_witness: null argument");
    if (s->n != KZG_BLOB_ELEMENTS) return fail(ZKW_ERR_INVALID, "zkw_eip4844_witness: a blob has 4096 elements, the settings hold %zu points", s->n);
    ZKW_TRY(kzg_check_call("zkw_eip4844_witness", s, ctx, n_blobs));
    if (n_blobs == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t* d_b = nullptr;
    ZKW_TRY(ctx->in("kzg_in_blobs", blobs, n_blobs * KZG_BLOB_BYTES, &d_b));
    zkw_eip4844_record* d_rec = nullptr;
    ZKW_TRY(ctx->out("kzg_records", out, n_blobs, &d_rec));
    uint8_t* rec = reinterpret_cast<uint8_t*>(d_rec);
    // the blob's sponge depends on nothing the commitment writes: beside it on a stream of the pool, joined ahead of z. (A context of a
    // batch has one stream; under zkw_profile the kernels run one after another so that every span times its own kernel.)
    const bool beside = !ctx->batched() && !ctx->profiling;
    if (beside) {
        hipStream_t side = nullptr;
        ZKW_TRY(ctx->side_fork(&side));
        Launcher<&k_kzg_linear_hash, 64>::S::template single<&k_kzg_linear_hash, 64>(side, dim3((unsigned)n_blobs), 0, d_b, rec + KZG_REC_LINEAR, (u32)KZG_REC_BYTES);
        ZKW_TRY(launch_check("k_kzg_linear_hash"));
    } else {
        Prof _p(ctx, "k_kzg_linear_hash");
        ZKW_LAUNCH(ctx, k_kzg_linear_hash, n_blobs, 64, d_b, rec + KZG_REC_LINEAR, (u32)KZG_REC_BYTES);
    }
    ZKW_TRY(kzg_commit_device(s, ctx, KzgSrc{d_b, (u32)KZG_BLOB_ELEMENTS, 1}, (u32)KZG_BLOB_BYTES, n_blobs, rec + KZG_REC_COMMITMENT, (u32)KZG_REC_BYTES));
    if (beside) ZKW_TRY(ctx->side_join());
    { Prof _p(ctx, "k_kzg_tail"); ZKW_LAUNCH(ctx, k_kzg_tail, n_blobs, KZG_TAIL_THREADS, d_b, rec); }
    ZKW_TRY(ctx->finish_out(out, d_rec, n_blobs));
    return ctx->sync_if_host();
}
