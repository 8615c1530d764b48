// zkw_kzg.hip — the EIP-4844 blob witness behind include/zkw.h: zkw_kzg_settings (the monomial trusted setup as a fixed-base table in
// HBM), zkw_kzg_commit and zkw_eip4844_witness (generate_eip4844_witness, src/utils.rs:119-231 of the reference), and the KZG proofs
// zkw_kzg_open and zkw_eip4844_prove (compute_proof, compute_proof_poly, kzg/src/lib.rs), and their check, zkw_kzg_verifier with
// zkw_kzg_verify and zkw_eip4844_verify (verify_kzg_proof), zkw_kzg_evaluate_blobs (eval_poly) and zkw_eip4844_verify_blobs
// (verify_proof_poly), and the producers from a blob in evaluation form, zkw_kzg_blob_coefficients, zkw_kzg_commit_blobs,
// zkw_kzg_open_blobs and zkw_eip4844_prove_blobs (compute_commitment, compute_proof, compute_proof_poly as the reference calls them), and
// the EIP-7594 cells and cell proofs, zkw_kzg_cell_settings with zkw_kzg_g1_fft, zkw_kzg_cells_blobs, zkw_kzg_cell_proofs_blobs and
// zkw_eip4844_cell_proofs, and the way back from any half of the cells, zkw_kzg_recover_cells_blobs, and the check of cell proofs,
// zkw_kzg_verify_cells with zkw_kzg_commit_cells (the reference has no counterpart of the three), and the setup in the Lagrange basis
// (KzgSettings::new, kzg/src/lib.rs:36-156): zkw_kzg_g1_fft_wide, zkw_kzg_settings_to_lagrange, _to_monomial, _points and _basis.
// Kernels and the decomposition: kzg_kernels.cuh, kzg_open_kernels.cuh, kzg_eval_kernels.cuh, kzg_verify_kernels.cuh, kzg_cell_kernels.cuh,
// kzg_recover_kernels.cuh, kzg_cell_verify_kernels.cuh, kzg_g1_fft_wide_kernels.cuh; field and group arithmetic: bls12_381.cuh, the tower and the pairing: bls12_381_pairing.cuh.
// What the calls share is written once, ahead of them: the handles' owner logic (KzgHandle), the blob limit, the 128 KiB of dynamic LDS of
// the five transform kernels, and the twiddles.
#include "zkw_ctx.h"
#include "kzg_kernels.cuh"
#include "kzg_open_kernels.cuh"
#include "kzg_eval_kernels.cuh"
#include "kzg_verify_kernels.cuh"
#include "kzg_cell_kernels.cuh"
#include "kzg_recover_kernels.cuh"
#include "kzg_cell_verify_kernels.cuh"
#include "kzg_g1_fft_wide_kernels.cuh"

#include <cstddef>

static_assert(sizeof(zkw_eip4844_record) == KZG_REC_BYTES && offsetof(zkw_eip4844_record, linear_hash) == KZG_REC_LINEAR &&
                  offsetof(zkw_eip4844_record, versioned_hash) == KZG_REC_VERSIONED && offsetof(zkw_eip4844_record, output_hash) == KZG_REC_OUTPUT &&
                  offsetof(zkw_eip4844_record, evaluation_point) == KZG_REC_Z && offsetof(zkw_eip4844_record, opening_value) == KZG_REC_Y &&
                  offsetof(zkw_eip4844_record, commitment) == KZG_REC_COMMITMENT,
              "kzg_kernels.cuh writes zkw_eip4844_record by byte offset");
static_assert(sizeof(zkw_eip4844_proof_record) == KZG_PRF_BYTES && offsetof(zkw_eip4844_proof_record, opening_proof) == KZG_PRF_OPENING &&
                  offsetof(zkw_eip4844_proof_record, blob_proof) == KZG_PRF_BLOB && offsetof(zkw_eip4844_proof_record, blob_challenge) == KZG_PRF_CHALLENGE &&
                  offsetof(zkw_eip4844_proof_record, blob_value) == KZG_PRF_VALUE,
              "kzg_open_kernels.cuh writes zkw_eip4844_proof_record by byte offset");
static_assert(sizeof(bls::G1Aff) == 96 && sizeof(bls::G1Jac) == 144, "table entries are 96 bytes, bucket sums 144");

// What the three handles (zkw_kzg_settings, zkw_kzg_verifier, zkw_kzg_cell_settings) share: one table in device memory, read by any context of
// the device, and the context it was built on, which the handle keeps alive. *_create validates, makes the handle (kzg_handle_new), runs its
// own kernels and on a failure drops it (kzg_handle_drop); *_free is witness_free (zkw_ctx.h: set device, sync, release, release the context).
template <class T> struct KzgHandle {
    zkw_ctx* ctx = nullptr;
    size_t bytes = 0;
    T* table = nullptr;
    void release() { dev_free(table); }
};
template <class H> static int kzg_handle_drop(H* h, int rc) {
    (void)h->ctx->sync_stream();  // nothing queued may still write the table
    if (h->table) dev_free(h->table);
    delete h;
    return rc;
}
// a handle of ctx with `bytes` of table (and `slack` bytes behind it); on an error nothing is left, and the caller words the refusal
template <class H> static hipError_t kzg_handle_new(zkw_ctx* ctx, size_t bytes, size_t slack, H** out) {
    H* h = new H();
    h->ctx = ctx;
    h->bytes = bytes;
    const hipError_t e = dev_malloc(&h->table, bytes + slack);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)kzg_handle_drop(h, 0);
        h = nullptr;
    }
    *out = h;
    return e;
}

struct zkw_kzg_settings : KzgHandle<bls::G1Aff> {  // table: [32][n], table[w * n + k] = 2^(8 w) S[k]
    size_t n = 0;
    int basis = 0;  // 1: zkw_kzg_settings_to_lagrange made it, S[k] = L[brp(k)]; 0: as created (taken as [tau^k] G1)
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
    zkw_kzg_settings* s = nullptr;
    const size_t bytes = (size_t)KZG_WINDOWS * n_points * sizeof(bls::G1Aff);
    const hipError_t e = kzg_handle_new(ctx, bytes, 64, &s);
    if (e != hipSuccess) return fail(ZKW_ERR_OOM, "zkw_kzg_settings_create: %zu points need %zu bytes of device memory: %s", n_points, bytes, hipGetErrorString(e));
    s->n = n_points;
    auto drop = [&](int rc) { return kzg_handle_drop(s, rc); };
    std::vector<u32> status(n_points);
    int rc = [&]() -> int {
        ZKW_LAUNCH(ctx, k_kzg_decompress, blocks_for(n_points, 64), 64, d_in, (u32)n_points, s->table, d_status);
        return ctx->read_small(status.data(), d_status, n_points * sizeof(u32));
    }();
    if (rc != ZKW_OK) return drop(rc);
    for (size_t k = 0; k < n_points; k++)
        if (status[k] != bls::G1_OK) return drop(fail(ZKW_ERR_INVALID, "zkw_kzg_settings_create: point %zu is refused: %s", k, kzg_reason(status[k])));
    rc = [&]() -> int {
        ZKW_LAUNCH_2D(ctx, k_kzg_table, blocks_for(n_points, 64), KZG_WINDOWS - 1, 64, s->table, (u32)n_points);
        HIP_TRY(ctx->sync_stream());  // other contexts read the table without any ordering with this stream
        return ZKW_OK;
    }();
    if (rc != ZKW_OK) return drop(rc);
    ctx_retain(ctx);
    *out = s;
    return ZKW_OK;
}

extern "C" void zkw_kzg_settings_free(zkw_kzg_settings* s) { witness_free(s); }
extern "C" size_t zkw_kzg_settings_num_points(const zkw_kzg_settings* s) { return s ? s->n : 0; }
extern "C" size_t zkw_kzg_settings_bytes(const zkw_kzg_settings* s) { return s ? s->bytes : 0; }

// buckets of n_polys polynomials, their eight bit sums, then their commitments at d_out + j * out_stride
static int kzg_commit_device(const zkw_kzg_settings* s, zkw_ctx* ctx, KzgSrc src, u32 poly_stride, size_t n_polys, uint8_t* d_out, u32 out_stride) {
    bls::G1Jac* buckets = nullptr;
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_buckets", n_polys * (KZG_BUCKETS + 8), &buckets));
    ZKW_LAUNCH_2D(ctx, k_kzg_accumulate, KZG_BUCKETS - 1, n_polys, KZG_ACC_THREADS, src, poly_stride, (const bls::G1Aff*)s->table, (u32)s->n, buckets);
    bls::G1Jac* sums = buckets + n_polys * KZG_BUCKETS;
    ZKW_LAUNCH_2D(ctx, k_kzg_finish, n_polys, 2, KZG_FIN_THREADS, (const bls::G1Jac*)buckets, sums);
    ZKW_LAUNCH(ctx, k_kzg_compress, blocks_for(n_polys, 64), 64, (const bls::G1Jac*)sums, (u32)n_polys, d_out, out_stride);
    return ZKW_OK;
}

// every call that reads S[k] as [tau^k] G1 refuses a handle in the Lagrange basis, ahead of its first launch
static int kzg_monomial_only(const char* who, const zkw_kzg_settings* s) {
    if (s->basis != 0) return fail(ZKW_ERR_INVALID, "%s: the settings are in the Lagrange basis (zkw_kzg_settings_to_lagrange made them), the call needs [tau^k] G1", who);
    return ZKW_OK;
}

enum KzgBasis { KZG_MONOMIAL, KZG_ANY_BASIS };
static int kzg_check_call(const char* who, const zkw_kzg_settings* s, zkw_ctx* ctx, size_t n, KzgBasis basis = KZG_MONOMIAL) {
    if (basis == KZG_MONOMIAL) ZKW_TRY(kzg_monomial_only(who, s));
    if (ctx->device != s->ctx->device) return fail(ZKW_ERR_INVALID, "%s: the settings live on device %d, the context on device %d", who, s->ctx->device, ctx->device);
    if (n > 65535) return fail(ZKW_ERR_INVALID, "%s: at most 65535 polynomials per call, not %zu", who, n);
    return ZKW_OK;
}

// a call takes at most 32 767 blobs: zkw_eip4844_prove makes two polynomials of each, and 65 535 are a grid's rows
enum : size_t { KZG_MAX_BLOBS = 32767 };
static int kzg_blob_limit(const char* who, size_t n) {
    if (n > KZG_MAX_BLOBS) return fail(ZKW_ERR_INVALID, "%s: at most 32767 blobs per call, not %zu", who, n);
    return ZKW_OK;
}

// 128 KiB of dynamic LDS, more than the default 64, for the five kernels that keep 4 096 elements of Fr there: once per device, and the
// first call that needs one of them pays for all five
static int kzg_allow_ntt_lds(zkw_ctx* ctx) {
    static bool attr_set[16] = {};
    if (attr_set[ctx->device & 15]) return ZKW_OK;
    ZKW_TRY((Launcher<&k_kzg_blob_ntt, KZG_NTT_THREADS>::allow_dynamic_lds(KZG_NTT_LDS)));
    ZKW_TRY((Launcher<&k_kzg_blob_intt, KZG_NTT_THREADS>::allow_dynamic_lds(KZG_NTT_LDS)));
    ZKW_TRY((Launcher<&k_kzg_cells, KZG_NTT_THREADS>::allow_dynamic_lds(KZG_NTT_LDS)));
    ZKW_TRY((Launcher<&k_kzg_recover_halves, KZG_NTT_THREADS>::allow_dynamic_lds(KZG_NTT_LDS)));
    ZKW_TRY((Launcher<&k_kzg_recover_quotient, KZG_NTT_THREADS>::allow_dynamic_lds(KZG_NTT_LDS)));
    attr_set[ctx->device & 15] = true;
    return ZKW_OK;
}

// w^j (j < 2048) and, with d_wpow, W^k (k < 4096) into context scratch, launched at `at` (the context's stream or beside it)
static int kzg_twiddles_device(const LaunchAt& at, const bls::Fr** d_tw, const bls::Fr** d_wpow = nullptr) {
    bls::Fr *tw = nullptr, *wpow = nullptr;
    ZKW_TRY(at.ctx->scratch_t<bls::Fr>("kzg_twiddles", 2048, &tw));
    ZKW_LAUNCH(at, k_kzg_twiddles, 8, 256, tw);
    *d_tw = tw;
    if (d_wpow) {
        ZKW_TRY(at.ctx->scratch_t<bls::Fr>("kzg_cell_wpow", 4096, &wpow));
        ZKW_LAUNCH(at, k_kzg_cell_wpow, 16, 256, wpow);
        *d_wpow = wpow;
    }
    return ZKW_OK;
}

extern "C" int zkw_kzg_commit(const zkw_kzg_settings* s, zkw_ctx* ctx, const uint8_t* coeffs, size_t n_coeffs, size_t n_polys, uint8_t* out) {
    if (!s || !ctx || (n_polys && (!out || (n_coeffs && !coeffs)))) return fail(ZKW_ERR_INVALID, "zkw_kzg_commit: null argument");
    if (n_coeffs > s->n) return fail(ZKW_ERR_INVALID, "zkw_kzg_commit: %zu coefficients, the settings hold %zu points", n_coeffs, s->n);
    ZKW_TRY(kzg_check_call("zkw_kzg_commit", s, ctx, n_polys, KZG_ANY_BASIS));  // a sum over the points, whatever they are
    if (n_polys == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t total = n_coeffs * n_polys;
    const uint8_t* d_c = nullptr;
    ZKW_TRY(ctx->in("kzg_in_coeffs", coeffs, total * 32, &d_c));
    if (total) {
        u32 *d_flag = nullptr, h_flag = ~0u;
        ZKW_TRY(ctx->scratch_t<u32>("kzg_flag", 1, &d_flag));
        HIP_TRY(ctx->memset_async(d_flag, 0xFF, sizeof(u32)));
        ZKW_LAUNCH(ctx, k_kzg_check, blocks_for(total, 256), 256, d_c, (u32)total, d_flag);
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
    LaunchAt at = ctx;
    if (beside) ZKW_TRY(side_fork_at(ctx, &at));
    ZKW_LAUNCH(at, k_kzg_linear_hash, n_blobs, 64, d_b, rec + KZG_REC_LINEAR, (u32)KZG_REC_BYTES);
    ZKW_TRY(kzg_commit_device(s, ctx, KzgSrc{d_b, (u32)KZG_BLOB_ELEMENTS, 1}, (u32)KZG_BLOB_BYTES, n_blobs, rec + KZG_REC_COMMITMENT, (u32)KZG_REC_BYTES));
    if (beside) ZKW_TRY(ctx->side_join());
    ZKW_LAUNCH(ctx, k_kzg_tail, n_blobs, KZG_TAIL_THREADS, d_b, rec);
    ZKW_TRY(ctx->finish_out(out, d_rec, n_blobs));
    return ctx->sync_if_host();
}

// ---- the proofs: an opening is the commitment of the quotient, whose rows k_kzg_quotient leaves in context scratch ----------------------
extern "C" int zkw_kzg_open(const zkw_kzg_settings* s, zkw_ctx* ctx, const uint8_t* coeffs, size_t n_coeffs, size_t n_polys, const uint8_t* points,
                            uint8_t* proofs, uint8_t* values) {
    if (!s || !ctx || (n_polys && (!points || !proofs || !values || (n_coeffs && !coeffs)))) return fail(ZKW_ERR_INVALID, "zkw_kzg_open: null argument");
    if (n_coeffs > s->n) return fail(ZKW_ERR_INVALID, "zkw_kzg_open: %zu coefficients, the settings hold %zu points", n_coeffs, s->n);
    ZKW_TRY(kzg_check_call("zkw_kzg_open", s, ctx, n_polys));
    if (n_polys == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t total = n_coeffs * n_polys, n_rows = n_coeffs ? n_coeffs - 1 : 0;
    const uint8_t *d_c = nullptr, *d_z = nullptr;
    ZKW_TRY(ctx->in("kzg_in_coeffs", coeffs, total * 32, &d_c));
    ZKW_TRY(ctx->in("kzg_in_points", points, n_polys * 32, &d_z));
    {
        u32 *d_flag = nullptr, h_flag[2] = {~0u, ~0u};  // the first bad coefficient, the first bad point
        ZKW_TRY(ctx->scratch_t<u32>("kzg_flag", 2, &d_flag));
        HIP_TRY(ctx->memset_async(d_flag, 0xFF, sizeof h_flag));
        if (total) ZKW_LAUNCH(ctx, k_kzg_check, blocks_for(total, 256), 256, d_c, (u32)total, d_flag);
        ZKW_LAUNCH(span_as(ctx, "k_kzg_check_points"), k_kzg_check, blocks_for(n_polys, 256), 256, d_z, (u32)n_polys, d_flag + 1);
        ZKW_TRY(ctx->read_small(h_flag, d_flag, sizeof h_flag));
        if (h_flag[0] != ~0u)
            return fail(ZKW_ERR_INVALID, "zkw_kzg_open: coefficient %zu of polynomial %zu is not below r", (size_t)h_flag[0] % n_coeffs, (size_t)h_flag[0] / n_coeffs);
        if (h_flag[1] != ~0u) return fail(ZKW_ERR_INVALID, "zkw_kzg_open: the point of polynomial %zu is not below r", (size_t)h_flag[1]);
    }
    uint8_t *d_proofs = nullptr, *d_values = nullptr, *d_rows = nullptr;
    ZKW_TRY(ctx->out("kzg_out", proofs, n_polys * 48, &d_proofs));
    ZKW_TRY(ctx->out("kzg_out_values", values, n_polys * 32, &d_values));
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_quotient_rows", n_polys * n_rows * 32, &d_rows));
    ZKW_LAUNCH(ctx, k_kzg_quotient, n_polys, KZG_QUO_THREADS, KzgSrc{d_c, (u32)n_coeffs, 0}, (u32)(n_coeffs * 32), d_z, 32u, (u32)KZG_Z_LE32, d_rows, (u32)(n_rows * 32), d_values, 32u, 0u);
    ZKW_TRY(kzg_commit_device(s, ctx, KzgSrc{d_rows, (u32)n_rows, 0}, (u32)(n_rows * 32), n_polys, d_proofs, 48));
    ZKW_TRY(ctx->finish_out(proofs, d_proofs, n_polys * 48));
    ZKW_TRY(ctx->finish_out(values, d_values, n_polys * 32));
    return ctx->sync_if_host();
}

extern "C" int zkw_eip4844_prove(const zkw_kzg_settings* s, zkw_ctx* ctx, const uint8_t* blobs, size_t n_blobs, const zkw_eip4844_record* records,
                                 zkw_eip4844_proof_record* out, uint8_t* blob_evaluations) {
    if (!s || !ctx || (n_blobs && (!blobs || !records || !out))) return fail(ZKW_ERR_INVALID, "zkw_eip4844_prove: null argument");
    if (s->n != KZG_BLOB_ELEMENTS) return fail(ZKW_ERR_INVALID, "zkw_eip4844_prove: a blob has 4096 elements, the settings hold %zu points", s->n);
    if (n_blobs > KZG_MAX_BLOBS) return fail(ZKW_ERR_INVALID, "zkw_eip4844_prove: at most 32767 blobs per call (two polynomials each), not %zu", n_blobs);
    ZKW_TRY(kzg_check_call("zkw_eip4844_prove", s, ctx, 2 * n_blobs));
    if (n_blobs == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    ZKW_TRY(kzg_allow_ntt_lds(ctx));
    const uint8_t* d_b = nullptr;
    ZKW_TRY(ctx->in("kzg_in_blobs", blobs, n_blobs * KZG_BLOB_BYTES, &d_b));
    const zkw_eip4844_record* d_rec = nullptr;
    ZKW_TRY(ctx->in("kzg_in_records", records, n_blobs, &d_rec));
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(d_rec);
    zkw_eip4844_proof_record* d_out = nullptr;
    ZKW_TRY(ctx->out("kzg_proof_records", out, n_blobs, &d_out));
    uint8_t *prf = reinterpret_cast<uint8_t*>(d_out), *d_ev = nullptr, *d_rows = nullptr, *d_proofs = nullptr;
    if (blob_evaluations) ZKW_TRY(ctx->out("kzg_evals", blob_evaluations, n_blobs * KZG_EVAL_BYTES, &d_ev));
    else ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_evals", n_blobs * KZG_EVAL_BYTES, &d_ev));  // the challenge hashes it either way
    const bls::Fr* d_tw = nullptr;
    // blob j's two quotients side by side: rows 2 j (at the record's z) and 2 j + 1 (at the challenge), so are their proofs
    constexpr u32 ROWS = (KZG_BLOB_ELEMENTS - 1) * 32;
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_quotient_rows", 2 * n_blobs * ROWS, &d_rows));
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_proofs", 2 * n_blobs * 48, &d_proofs));
    const KzgSrc blob_src{d_b, (u32)KZG_BLOB_ELEMENTS, 1};
    const unsigned nb = (unsigned)n_blobs;
    // the evaluation form and its sponge depend on nothing the opening at z writes: beside it on a stream of the pool, joined ahead of the
    // opening at the challenge. (A context of a batch has one stream; under zkw_profile every span times its own kernel.)
    const bool beside = !ctx->batched() && !ctx->profiling;
    LaunchAt at = ctx;
    if (beside) ZKW_TRY(side_fork_at(ctx, &at));
    ZKW_TRY(kzg_twiddles_device(at, &d_tw));
    ZKW_LAUNCH_D(at, k_kzg_blob_ntt, "k_kzg_blob_ntt", dim3(nb), KZG_NTT_THREADS, KZG_NTT_LDS, d_b, d_tw, d_ev);
    ZKW_LAUNCH(at, k_kzg_blob_challenge, nb, 64, (const uint8_t*)d_ev, rec + KZG_REC_COMMITMENT, (u32)KZG_REC_BYTES, prf + KZG_PRF_CHALLENGE, (u32)KZG_PRF_BYTES);
    ZKW_LAUNCH(ctx, k_kzg_quotient, nb, KZG_QUO_THREADS, blob_src, (u32)KZG_BLOB_BYTES, rec + KZG_REC_Z, (u32)KZG_REC_BYTES, (u32)KZG_Z_BE16, d_rows, 2 * ROWS, (uint8_t*)nullptr, 0u, 0u);
    if (beside) ZKW_TRY(ctx->side_join());
    ZKW_LAUNCH(ctx, k_kzg_quotient, nb, KZG_QUO_THREADS, blob_src, (u32)KZG_BLOB_BYTES, (const uint8_t*)prf + KZG_PRF_CHALLENGE, (u32)KZG_PRF_BYTES, (u32)KZG_Z_BE32, d_rows + ROWS, 2 * ROWS, prf + KZG_PRF_VALUE, (u32)KZG_PRF_BYTES, 1u);
    ZKW_TRY(kzg_commit_device(s, ctx, KzgSrc{d_rows, (u32)KZG_BLOB_ELEMENTS - 1, 0}, ROWS, 2 * n_blobs, d_proofs, 48));
    ZKW_LAUNCH(ctx, k_kzg_proofs_out, blocks_for(n_blobs * 96, 256), 256, (const uint8_t*)d_proofs, (u32)nb, prf);
    ZKW_TRY(ctx->finish_out(out, d_out, n_blobs));
    if (blob_evaluations) ZKW_TRY(ctx->finish_out(blob_evaluations, d_ev, n_blobs * KZG_EVAL_BYTES));
    return ctx->sync_if_host();
}

// ---- the producers from a blob in evaluation form: back to the coefficients in Fr, then the kernels above as they are ------------------
static int kzg_blobs_check_call(const char* who, const zkw_kzg_settings* s, zkw_ctx* ctx, size_t n) {
    if (s->n != KZG_BLOB_ELEMENTS) return fail(ZKW_ERR_INVALID, "%s: a blob has 4096 elements, the settings hold %zu points", who, s->n);
    ZKW_TRY(kzg_blob_limit(who, n));
    return kzg_check_call(who, s, ctx, n);
}

// the twiddles and k_kzg_blob_intt over n >= 1 blobs on the context's stream, then the call's ONE readback: the n status words and, with
// d_points, the n flags of the points. The coefficients ([n][4096][32], zkw_kzg_commit's form) are left in context scratch, so that a
// refused call has written nothing of the caller's
static int kzg_blob_coefficients_device(const char* who, zkw_ctx* ctx, const uint8_t* d_ev, const uint8_t* d_points, size_t n, const uint8_t** d_coeffs) {
    ZKW_TRY(kzg_allow_ntt_lds(ctx));
    const bls::Fr* d_tw = nullptr;
    uint8_t* d_c = nullptr;
    u32* d_st = nullptr;
    const size_t words = d_points ? 2 * n : n;
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_blob_coeffs", n * KZG_EVAL_BYTES, &d_c));
    ZKW_TRY(ctx->scratch_t<u32>("kzg_intt_status", words, &d_st));
    ZKW_TRY(kzg_twiddles_device(ctx, &d_tw));
    ZKW_LAUNCH_D(ctx, k_kzg_blob_intt, "k_kzg_blob_intt", dim3((unsigned)n), KZG_NTT_THREADS, KZG_NTT_LDS, d_ev, d_tw, d_c, d_points, (u32)n, d_st);
    std::vector<u32> st(words);
    ZKW_TRY(ctx->read_small(st.data(), d_st, words * sizeof(u32)));
    for (size_t j = 0; j < n; j++)
        if (st[j]) return fail(ZKW_ERR_INVALID, "%s: element %u of blob %zu is not below r", who, (unsigned)(st[j] - 1), j);
    for (size_t j = n; j < words; j++)
        if (st[j]) return fail(ZKW_ERR_INVALID, "%s: the point of blob %zu is not below r", who, j - n);
    *d_coeffs = d_c;
    return ZKW_OK;
}

extern "C" int zkw_kzg_blob_coefficients(zkw_ctx* ctx, const uint8_t* blob_evaluations, size_t n, uint8_t* coeffs) {
    if (!ctx || (n && (!blob_evaluations || !coeffs))) return fail(ZKW_ERR_INVALID, "zkw_kzg_blob_coefficients: null argument");
    ZKW_TRY(kzg_blob_limit("zkw_kzg_blob_coefficients", n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *d_ev = nullptr, *d_c = nullptr;
    ZKW_TRY(ctx->in("kzg_in_evals", blob_evaluations, n * KZG_EVAL_BYTES, &d_ev));
    ZKW_TRY(kzg_blob_coefficients_device("zkw_kzg_blob_coefficients", ctx, d_ev, nullptr, n, &d_c));
    ZKW_TRY(ctx->copy_out(coeffs, d_c, n * KZG_EVAL_BYTES));
    return ctx->sync_if_host();
}

extern "C" int zkw_kzg_commit_blobs(const zkw_kzg_settings* s, zkw_ctx* ctx, const uint8_t* blob_evaluations, size_t n, uint8_t* commitments) {
    if (!s || !ctx || (n && (!blob_evaluations || !commitments))) return fail(ZKW_ERR_INVALID, "zkw_kzg_commit_blobs: null argument");
    ZKW_TRY(kzg_blobs_check_call("zkw_kzg_commit_blobs", s, ctx, n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *d_ev = nullptr, *d_c = nullptr;
    ZKW_TRY(ctx->in("kzg_in_evals", blob_evaluations, n * KZG_EVAL_BYTES, &d_ev));
    ZKW_TRY(kzg_blob_coefficients_device("zkw_kzg_commit_blobs", ctx, d_ev, nullptr, n, &d_c));
    uint8_t* d_out = nullptr;
    ZKW_TRY(ctx->out("kzg_out", commitments, n * 48, &d_out));
    ZKW_TRY(kzg_commit_device(s, ctx, KzgSrc{d_c, (u32)KZG_BLOB_ELEMENTS, 0}, (u32)KZG_EVAL_BYTES, n, d_out, 48));
    ZKW_TRY(ctx->finish_out(commitments, d_out, n * 48));
    return ctx->sync_if_host();
}

// the quotients of n polynomials of 4 096 coefficients (scratch rows) at points of 32 big-endian bytes, the values in the same form, and
// the commitments of the quotients at d_proofs
static int kzg_open_coefficients_device(const zkw_kzg_settings* s, zkw_ctx* ctx, const uint8_t* d_c, const uint8_t* d_z, u32 z_stride, size_t n, uint8_t* d_proofs,
                                        uint8_t* d_values, u32 value_stride) {
    constexpr u32 ROWS = (KZG_BLOB_ELEMENTS - 1) * 32;
    uint8_t* d_rows = nullptr;
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_quotient_rows", n * ROWS, &d_rows));
    ZKW_LAUNCH(ctx, k_kzg_quotient, n, KZG_QUO_THREADS, KzgSrc{d_c, (u32)KZG_BLOB_ELEMENTS, 0}, (u32)KZG_EVAL_BYTES, d_z, z_stride, (u32)KZG_Z_BE32, d_rows, ROWS, d_values, value_stride, 1u);
    return kzg_commit_device(s, ctx, KzgSrc{d_rows, (u32)KZG_BLOB_ELEMENTS - 1, 0}, ROWS, n, d_proofs, 48);
}

extern "C" int zkw_kzg_open_blobs(const zkw_kzg_settings* s, zkw_ctx* ctx, const uint8_t* blob_evaluations, const uint8_t* points, size_t n, uint8_t* proofs,
                                  uint8_t* values) {
    if (!s || !ctx || (n && (!blob_evaluations || !points || !proofs || !values))) return fail(ZKW_ERR_INVALID, "zkw_kzg_open_blobs: null argument");
    ZKW_TRY(kzg_blobs_check_call("zkw_kzg_open_blobs", s, ctx, n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *d_ev = nullptr, *d_z = nullptr, *d_c = nullptr;
    ZKW_TRY(ctx->in("kzg_in_evals", blob_evaluations, n * KZG_EVAL_BYTES, &d_ev));
    ZKW_TRY(ctx->in("kzg_in_points", points, n * 32, &d_z));
    ZKW_TRY(kzg_blob_coefficients_device("zkw_kzg_open_blobs", ctx, d_ev, d_z, n, &d_c));
    uint8_t *d_proofs = nullptr, *d_values = nullptr;
    ZKW_TRY(ctx->out("kzg_out", proofs, n * 48, &d_proofs));
    ZKW_TRY(ctx->out("kzg_out_values", values, n * 32, &d_values));
    ZKW_TRY(kzg_open_coefficients_device(s, ctx, d_c, d_z, 32u, n, d_proofs, d_values, 32u));
    ZKW_TRY(ctx->finish_out(proofs, d_proofs, n * 48));
    ZKW_TRY(ctx->finish_out(values, d_values, n * 32));
    return ctx->sync_if_host();
}

extern "C" int zkw_eip4844_prove_blobs(const zkw_kzg_settings* s, zkw_ctx* ctx, const uint8_t* blob_evaluations, const uint8_t* commitments, size_t n,
                                       uint8_t* proofs, uint8_t* openings) {
    if (!s || !ctx || (n && (!blob_evaluations || !commitments || !proofs))) return fail(ZKW_ERR_INVALID, "zkw_eip4844_prove_blobs: null argument");
    ZKW_TRY(kzg_blobs_check_call("zkw_eip4844_prove_blobs", s, ctx, n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *d_ev = nullptr, *d_cm = nullptr, *d_c = nullptr;
    ZKW_TRY(ctx->in("kzg_in_evals", blob_evaluations, n * KZG_EVAL_BYTES, &d_ev));
    ZKW_TRY(ctx->in("kzg_in_commitments", commitments, n * 48, &d_cm));
    uint8_t* d_open = nullptr;  // a row: the blob's challenge, then its value there (scratch in both pointer modes: a refused call leaves `openings` untouched)
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_openings", n * 64, &d_open));
    // the sponge depends on nothing the transform writes: beside it on a stream of the pool, joined ahead of the quotient. (A context of a
    // batch has one stream; under zkw_profile every span times its own kernel.)
    const bool beside = !ctx->batched() && !ctx->profiling;
    LaunchAt at = ctx;
    if (beside) ZKW_TRY(side_fork_at(ctx, &at));
    ZKW_LAUNCH(at, k_kzg_blob_challenge, n, 64, d_ev, d_cm, 48u, d_open, 64u);
    const int rc = kzg_blob_coefficients_device("zkw_eip4844_prove_blobs", ctx, d_ev, nullptr, n, &d_c);
    if (beside) ZKW_TRY(ctx->side_join());  // (after a refusal too: the sponge of this call is not left to run into the next one's scratch)
    if (rc != ZKW_OK) return rc;
    uint8_t* d_proofs = nullptr;
    ZKW_TRY(ctx->out("kzg_out", proofs, n * 48, &d_proofs));
    ZKW_TRY(kzg_open_coefficients_device(s, ctx, d_c, d_open, 64u, n, d_proofs, d_open + 32, 64u));
    ZKW_TRY(ctx->finish_out(proofs, d_proofs, n * 48));
    if (openings) ZKW_TRY(ctx->copy_out(openings, d_open, n * 64));
    return ctx->sync_if_host();
}

// ---- the check: a verifier is the prepared lines of -G2 and [tau] G2; a call is two kernels and reads nothing back ----------------------
static_assert(sizeof(bls::G2Line) == 192, "a line is two elements of Fq2");

struct zkw_kzg_verifier : KzgHandle<bls::G2Line> {};  // table: the lines [2][68] of -G2 and [tau] G2

static const char* kzg_g2_reason(u32 status) {
    switch (status) {
        case bls::G1_X_TOO_LARGE: return "a coordinate of x is not below p";
        case bls::G1_NOT_ON_CURVE: return "x has no y on y^2 = x^3 + 4 (1 + u)";
        case KZG_G2_INFINITY: return "it is the point at infinity";
        default: return kzg_reason(status);  // the flags and the subgroup: G1's words
    }
}

extern "C" int zkw_kzg_verifier_create(zkw_ctx* ctx, const uint8_t* tau_g2, zkw_kzg_verifier** out) {
    if (!ctx || !out || !tau_g2) return fail(ZKW_ERR_INVALID, "zkw_kzg_verifier_create: null argument");
    if (ctx->batch) return fail(ZKW_ERR_INVALID, "zkw_kzg_verifier_create: the context belongs to a batch of blocks");
    HIP_TRY(hipSetDevice(ctx->device));
    *out = nullptr;
    const uint8_t* d_in = nullptr;
    ZKW_TRY(ctx->in("kzg_in_points", tau_g2, 96, &d_in));
    u32* d_status = nullptr;
    ZKW_TRY(ctx->scratch_t<u32>("kzg_status", 2, &d_status));
    zkw_kzg_verifier* v = nullptr;
    const size_t bytes = 2 * (size_t)bls::G2_LINES * sizeof(bls::G2Line);
    const hipError_t e = kzg_handle_new(ctx, bytes, 0, &v);
    if (e != hipSuccess) return fail(ZKW_ERR_OOM, "zkw_kzg_verifier_create: %zu bytes of device memory: %s", bytes, hipGetErrorString(e));
    auto drop = [&](int rc) { return kzg_handle_drop(v, rc); };
    u32 status[2] = {0, 0};
    const int rc = [&]() -> int {
        ZKW_LAUNCH(ctx, k_kzg_g2_prepare, 1, 64, d_in, v->table, d_status);
        return ctx->read_small(status, d_status, sizeof status);  // (synchronises: other contexts read the lines without any ordering with this stream)
    }();
    if (rc != ZKW_OK) return drop(rc);
    if (status[0] != bls::G1_OK) return drop(fail(ZKW_ERR_CHECK_FAILED, "zkw_kzg_verifier_create: the generator of G2 is refused: %s", kzg_g2_reason(status[0])));
    if (status[1] != bls::G1_OK) return drop(fail(ZKW_ERR_INVALID, "zkw_kzg_verifier_create: the point is refused: %s", kzg_g2_reason(status[1])));
    ctx_retain(ctx);
    *out = v;
    return ZKW_OK;
}

extern "C" void zkw_kzg_verifier_free(zkw_kzg_verifier* v) { witness_free(v); }
extern "C" size_t zkw_kzg_verifier_bytes(const zkw_kzg_verifier* v) { return v ? v->bytes : 0; }

// the two kernels over n >= 1 claims; d_verdicts: n bytes on the device
static int kzg_verify_device(const zkw_kzg_verifier* v, zkw_ctx* ctx, const KzgClaims& claims, size_t n, uint8_t* d_verdicts) {
    bls::G1Aff* d_pts = nullptr;
    u32* d_status = nullptr;
    ZKW_TRY(ctx->scratch_t<bls::G1Aff>("kzg_verify_points", 2 * n, &d_pts));
    ZKW_TRY(ctx->scratch_t<u32>("kzg_verify_status", n, &d_status));
    ZKW_LAUNCH(ctx, k_kzg_verify_points, blocks_for(n, 64), 64, claims, (u32)n, d_pts, d_status);
    ZKW_LAUNCH_D(ctx, k_kzg_verify_pairing, "k_kzg_verify_pairing", dim3(blocks_for(n, KZG_VFY_CLAIMS_PER_BLOCK)), KZG_VFY_THREADS, bls::f12_lds_bytes(KZG_VFY_THREADS), (const bls::G1Aff*)d_pts, (const u32*)d_status, (const bls::G2Line*)v->table, (u32)n, d_verdicts);
    return ZKW_OK;
}

static int kzg_verify_check_call(const char* who, const zkw_kzg_verifier* v, zkw_ctx* ctx, size_t n_claims) {
    if (ctx->device != v->ctx->device) return fail(ZKW_ERR_INVALID, "%s: the verifier lives on device %d, the context on device %d", who, v->ctx->device, ctx->device);
    if (n_claims > (1u << 24)) return fail(ZKW_ERR_INVALID, "%s: at most %u claims per call, not %zu", who, 1u << 24, n_claims);
    return ZKW_OK;
}

extern "C" int zkw_kzg_verify(const zkw_kzg_verifier* v, zkw_ctx* ctx, const uint8_t* commitments, const uint8_t* points, const uint8_t* values,
                              const uint8_t* proofs, size_t n, uint8_t* verdicts) {
    if (!v || !ctx || (n && (!commitments || !points || !values || !proofs || !verdicts))) return fail(ZKW_ERR_INVALID, "zkw_kzg_verify: null argument");
    ZKW_TRY(kzg_verify_check_call("zkw_kzg_verify", v, ctx, n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    KzgClaims cl{nullptr, nullptr, nullptr, nullptr, 0, nullptr};
    ZKW_TRY(ctx->in("kzg_in_commitments", commitments, n * 48, &cl.commitments));
    ZKW_TRY(ctx->in("kzg_in_points", points, n * 32, &cl.points));
    ZKW_TRY(ctx->in("kzg_in_values", values, n * 32, &cl.values));
    ZKW_TRY(ctx->in("kzg_in_proofs", proofs, n * 48, &cl.proofs));
    uint8_t* d_verdicts = nullptr;
    ZKW_TRY(ctx->out("kzg_verdicts", verdicts, n, &d_verdicts));
    ZKW_TRY(kzg_verify_device(v, ctx, cl, n, d_verdicts));
    ZKW_TRY(ctx->finish_out(verdicts, d_verdicts, n));
    return ctx->sync_if_host();
}

extern "C" int zkw_eip4844_verify(const zkw_kzg_verifier* v, zkw_ctx* ctx, const zkw_eip4844_record* records, const zkw_eip4844_proof_record* proofs,
                                  size_t n, uint8_t* verdicts) {
    if (!v || !ctx || (n && (!records || !proofs || !verdicts))) return fail(ZKW_ERR_INVALID, "zkw_eip4844_verify: null argument");
    ZKW_TRY(kzg_verify_check_call("zkw_eip4844_verify", v, ctx, 2 * n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const zkw_eip4844_record* d_rec = nullptr;
    const zkw_eip4844_proof_record* d_prf = nullptr;
    ZKW_TRY(ctx->in("kzg_in_records", records, n, &d_rec));
    ZKW_TRY(ctx->in("kzg_in_proof_records", proofs, n, &d_prf));
    uint8_t* d_verdicts = nullptr;
    ZKW_TRY(ctx->out("kzg_verdicts", verdicts, 2 * n, &d_verdicts));
    const KzgClaims cl{reinterpret_cast<const uint8_t*>(d_rec), nullptr, nullptr, reinterpret_cast<const uint8_t*>(d_prf), 1, nullptr};
    ZKW_TRY(kzg_verify_device(v, ctx, cl, 2 * n, d_verdicts));
    ZKW_TRY(ctx->finish_out(verdicts, d_verdicts, 2 * n));
    return ctx->sync_if_host();
}

// ---- the check from the blob itself: challenge and value are recomputed, nothing the prover wrote down is taken on trust ----------------
extern "C" int zkw_kzg_evaluate_blobs(zkw_ctx* ctx, const uint8_t* blob_evaluations, const uint8_t* points, size_t n, uint8_t* values) {
    if (!ctx || (n && (!blob_evaluations || !points || !values))) return fail(ZKW_ERR_INVALID, "zkw_kzg_evaluate_blobs: null argument");
    ZKW_TRY(kzg_blob_limit("zkw_kzg_evaluate_blobs", n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *d_ev = nullptr, *d_z = nullptr;
    ZKW_TRY(ctx->in("kzg_in_evals", blob_evaluations, n * KZG_EVAL_BYTES, &d_ev));
    ZKW_TRY(ctx->in("kzg_in_points", points, n * 32, &d_z));
    const bls::Fr* d_tw = nullptr;
    uint8_t* d_y = nullptr;  // (scratch in both pointer modes: a refused call leaves `values` untouched)
    u32* d_st = nullptr;
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_eval_values", n * 32, &d_y));
    ZKW_TRY(ctx->scratch_t<u32>("kzg_eval_status", n, &d_st));
    ZKW_TRY(kzg_twiddles_device(ctx, &d_tw));
    ZKW_LAUNCH(ctx, k_kzg_blob_eval, n, KZG_EVAL_THREADS, d_ev, d_z, 32u, d_tw, d_y, 32u, d_st);
    std::vector<u32> st(n);
    ZKW_TRY(ctx->read_small(st.data(), d_st, n * sizeof(u32)));
    for (size_t j = 0; j < n; j++) {
        if (st[j] == KZG_EVAL_BAD_POINT) return fail(ZKW_ERR_INVALID, "zkw_kzg_evaluate_blobs: the point of blob %zu is not below r", j);
        if (st[j] != KZG_EVAL_OK) return fail(ZKW_ERR_INVALID, "zkw_kzg_evaluate_blobs: element %u of blob %zu is not below r", (unsigned)(st[j] - 1), j);
    }
    ZKW_TRY(ctx->copy_out(values, d_y, n * 32));
    return ctx->sync_if_host();
}

extern "C" int zkw_eip4844_verify_blobs(const zkw_kzg_verifier* v, zkw_ctx* ctx, const uint8_t* blob_evaluations, const uint8_t* commitments,
                                        const uint8_t* proofs, size_t n, uint8_t* verdicts, uint8_t* openings) {
    if (!v || !ctx || (n && (!blob_evaluations || !commitments || !proofs || !verdicts))) return fail(ZKW_ERR_INVALID, "zkw_eip4844_verify_blobs: null argument");
    ZKW_TRY(kzg_blob_limit("zkw_eip4844_verify_blobs", n));
    ZKW_TRY(kzg_verify_check_call("zkw_eip4844_verify_blobs", v, ctx, n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t* d_ev = nullptr;
    KzgClaims cl{nullptr, nullptr, nullptr, nullptr, 2, nullptr};
    ZKW_TRY(ctx->in("kzg_in_evals", blob_evaluations, n * KZG_EVAL_BYTES, &d_ev));
    ZKW_TRY(ctx->in("kzg_in_commitments", commitments, n * 48, &cl.commitments));
    ZKW_TRY(ctx->in("kzg_in_proofs", proofs, n * 48, &cl.proofs));
    uint8_t *d_verdicts = nullptr, *d_open = nullptr;  // a row of d_open: the blob's challenge, then its value there
    ZKW_TRY(ctx->out("kzg_verdicts", verdicts, n, &d_verdicts));
    if (openings) ZKW_TRY(ctx->out("kzg_openings", openings, n * 64, &d_open));
    else ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_openings", n * 64, &d_open));  // the check reads them either way
    const bls::Fr* d_tw = nullptr;
    u32* d_st = nullptr;
    ZKW_TRY(ctx->scratch_t<u32>("kzg_eval_status", n, &d_st));
    // one after another on the context's stream: the evaluation needs the challenge, the points kernel needs both
    ZKW_TRY(kzg_twiddles_device(ctx, &d_tw));
    ZKW_LAUNCH(ctx, k_kzg_blob_challenge, n, 64, d_ev, cl.commitments, 48u, d_open, 64u);
    ZKW_LAUNCH(ctx, k_kzg_blob_eval, n, KZG_EVAL_THREADS, d_ev, (const uint8_t*)d_open, 64u, d_tw, d_open + 32, 64u, d_st);
    cl.points = d_open;
    cl.values = d_open + 32;
    cl.pre = d_st;
    ZKW_TRY(kzg_verify_device(v, ctx, cl, n, d_verdicts));
    ZKW_TRY(ctx->finish_out(verdicts, d_verdicts, n));
    if (openings) ZKW_TRY(ctx->finish_out(openings, d_open, n * 64));
    return ctx->sync_if_host();
}

// ---- EIP-7594: the 128 cells of a blob and their proofs (kzg_cell_kernels.cuh) ----------------------------------------------------------
static_assert(KZG_CELL_POINTS == 64 * KZG_CELLS && KZG_CELLS_BYTES == 2 * KZG_EVAL_BYTES, "64 offsets of 128 points; the extended blob is two blobs long");

struct zkw_kzg_cell_settings : KzgHandle<bls::G1Aff> {};  // table: [32][8192], table[w * 8192 + j * 64 + i] = 2^(8 w) X_i[j], X_i = G1_FFT_128(x_i)

// n_ffts transforms of 2^log_n Jacobian points each on the context's stream (d_in == d_out is fine)
static int kzg_g1_fft_device(zkw_ctx* ctx, const bls::G1Jac* d_in, bls::G1Jac* d_out, u32 log_n, size_t n_ffts, bool inverse, bool scale, bool upper_inf) {
    u32* d_tab = nullptr;  // the lanes' window tables
    ZKW_TRY(ctx->scratch_t<u32>("kzg_g1_fft_tables", n_ffts * KZG_G1_TAB_WORDS, &d_tab));
    ZKW_LAUNCH(ctx, k_kzg_g1_fft, n_ffts, KZG_G1_FFT_THREADS, d_in, d_out, d_tab, log_n, inverse ? 1u : 0u, scale ? 1u : 0u, upper_inf ? 1u : 0u);
    return ZKW_OK;
}

extern "C" int zkw_kzg_cell_settings_create(const zkw_kzg_settings* s, zkw_ctx* ctx, zkw_kzg_cell_settings** out) {
    if (!s || !ctx || !out) return fail(ZKW_ERR_INVALID, "zkw_kzg_cell_settings_create: null argument");
    ZKW_TRY(kzg_monomial_only("zkw_kzg_cell_settings_create", s));
    if (s->n != KZG_BLOB_ELEMENTS) return fail(ZKW_ERR_INVALID, "zkw_kzg_cell_settings_create: a blob has 4096 elements, the settings hold %zu points", s->n);
    if (ctx->device != s->ctx->device)
        return fail(ZKW_ERR_INVALID, "zkw_kzg_cell_settings_create: the settings live on device %d, the context on device %d", s->ctx->device, ctx->device);
    if (ctx->batch) return fail(ZKW_ERR_INVALID, "zkw_kzg_cell_settings_create: the context belongs to a batch of blocks");
    HIP_TRY(hipSetDevice(ctx->device));
    *out = nullptr;
    bls::G1Jac* d_x = nullptr;
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_cell_setup", KZG_CELL_POINTS, &d_x));
    zkw_kzg_cell_settings* cs = nullptr;
    const size_t bytes = (size_t)KZG_WINDOWS * KZG_CELL_POINTS * sizeof(bls::G1Aff);
    const hipError_t e = kzg_handle_new(ctx, bytes, 64, &cs);
    if (e != hipSuccess) return fail(ZKW_ERR_OOM, "zkw_kzg_cell_settings_create: %zu bytes of device memory: %s", bytes, hipGetErrorString(e));
    const int rc = [&]() -> int {
        ZKW_LAUNCH(ctx, k_kzg_cell_setup_x, blocks_for(KZG_CELL_POINTS, 64), 64, (const bls::G1Aff*)s->table, d_x);
        ZKW_TRY(kzg_g1_fft_device(ctx, d_x, d_x, 7, 64, false, false, false));
        ZKW_LAUNCH(ctx, k_kzg_cell_setup_affine, blocks_for(KZG_CELL_POINTS, 64), 64, (const bls::G1Jac*)d_x, cs->table);
        ZKW_LAUNCH_2D(ctx, k_kzg_table, blocks_for(KZG_CELL_POINTS, 64), KZG_WINDOWS - 1, 64, cs->table, (u32)KZG_CELL_POINTS);
        HIP_TRY(ctx->sync_stream());  // other contexts read the table without any ordering with this stream
        return ZKW_OK;
    }();
    if (rc != ZKW_OK) return kzg_handle_drop(cs, rc);
    ctx_retain(ctx);
    *out = cs;
    return ZKW_OK;
}

extern "C" void zkw_kzg_cell_settings_free(zkw_kzg_cell_settings* cs) { witness_free(cs); }
extern "C" size_t zkw_kzg_cell_settings_bytes(const zkw_kzg_cell_settings* cs) { return cs ? cs->bytes : 0; }

extern "C" int zkw_kzg_g1_fft(zkw_ctx* ctx, const uint8_t* points, size_t n, size_t n_ffts, int inverse, uint8_t* out) {
    if (!ctx || (n_ffts && (!points || !out))) return fail(ZKW_ERR_INVALID, "zkw_kzg_g1_fft: null argument");
    if (n == 0 || n > KZG_G1_FFT_MAX || (n & (n - 1))) return fail(ZKW_ERR_INVALID, "zkw_kzg_g1_fft: a power of two from 1 to %u points, not %zu", (unsigned)KZG_G1_FFT_MAX, n);
    if (n_ffts > 65535) return fail(ZKW_ERR_INVALID, "zkw_kzg_g1_fft: at most 65535 transforms per call, not %zu", n_ffts);
    if (n_ffts == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t total = n * n_ffts;
    u32 log_n = 0;
    while ((size_t)1 << log_n < n) log_n++;
    const uint8_t* d_in = nullptr;
    ZKW_TRY(ctx->in("kzg_in_points", points, total * 48, &d_in));
    bls::G1Aff* d_aff = nullptr;
    bls::G1Jac* d_jac = nullptr;
    u32* d_status = nullptr;
    ZKW_TRY(ctx->scratch_t<bls::G1Aff>("kzg_g1_fft_affine", total, &d_aff));
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_g1_fft_points", total, &d_jac));
    ZKW_TRY(ctx->scratch_t<u32>("kzg_status", total, &d_status));
    ZKW_LAUNCH(ctx, k_kzg_decompress, blocks_for(total, 64), 64, d_in, (u32)total, d_aff, d_status);
    std::vector<u32> status(total);
    ZKW_TRY(ctx->read_small(status.data(), d_status, total * sizeof(u32)));
    for (size_t k = 0; k < total; k++)
        if (status[k] != bls::G1_OK) return fail(ZKW_ERR_INVALID, "zkw_kzg_g1_fft: point %zu of transform %zu is refused: %s", k % n, k / n, kzg_reason(status[k]));
    uint8_t* d_out = nullptr;
    ZKW_TRY(ctx->out("kzg_out", out, total * 48, &d_out));
    ZKW_LAUNCH(ctx, k_kzg_g1_lift, blocks_for(total, 64), 64, (const bls::G1Aff*)d_aff, (u32)total, d_jac);
    ZKW_TRY(kzg_g1_fft_device(ctx, d_jac, d_jac, log_n, n_ffts, inverse != 0, inverse != 0, false));
    ZKW_LAUNCH(ctx, k_kzg_g1_compress, blocks_for(total, 64), 64, (const bls::G1Jac*)d_jac, (u32)total, 0u, d_out);
    ZKW_TRY(ctx->finish_out(out, d_out, total * 48));
    return ctx->sync_if_host();
}

// ---- the wide G1 transform and the setup's two bases (kzg_g1_fft_wide_kernels.cuh) -------------------------------------------------------
static_assert(KZG_G1_FFT_WIDE_MAX == KZG_MAX_POINTS && KZG_G1_FFT_WIDE_POINTS % KZG_G1_FFT_MAX == 0, "a setup is one wide transform");

// n_ffts transforms of 2^log_n <= 4 096 Jacobian points each (n_ffts 2^log_n <= 65 536), in place at d_x up to the order of the result:
// *d_res is d_x when the result is there in natural order (n <= 128 without `brp`), else d_y (as many points, another buffer), in natural
// order or with `brp` output u at brp(u). The inverse carries its 1 / n
static int kzg_g1_fft_wide_device(zkw_ctx* ctx, bls::G1Jac* d_x, bls::G1Jac* d_y, u32 log_n, size_t n_ffts, bool inverse, bool brp, const bls::G1Jac** d_res) {
    const size_t total = n_ffts << log_n;
    const u32 inv = inverse ? 1u : 0u;
    if (log_n <= 7) {
        ZKW_TRY(kzg_g1_fft_device(ctx, d_x, d_x, log_n, n_ffts, inverse, inverse, false));
        *d_res = d_x;
        if (!brp) return ZKW_OK;
    }
    const unsigned order_blocks = blocks_for(total < KZG_G1_FFT_WIDE_POINTS / 2 ? total : KZG_G1_FFT_WIDE_POINTS / 2, KZG_G1_FFT_THREADS);
    const size_t waves = log_n > 7 ? total / KZG_G1_FFT_MAX : 0;  // of a stage and of the tail; the order kernel has at most as many with a table
    u32* d_tab = nullptr;                                          // the lanes' window tables (kzg_g1_fft_device asks for the same ones)
    ZKW_TRY(ctx->scratch_t<u32>("kzg_g1_fft_tables", (waves > order_blocks ? waves : order_blocks) * KZG_G1_TAB_WORDS, &d_tab));
    if (log_n > 7) {
        for (u32 s = 0; s + 7 < log_n; s++)
            ZKW_LAUNCH(ctx, k_kzg_g1_fft_stage, waves, KZG_G1_FFT_THREADS, d_x, d_tab, log_n, s, inv, (u32)(total / 2));
        ZKW_TRY(kzg_g1_fft_device(ctx, d_x, d_x, 7, waves, inverse, false, false));
    }
    const u32 scale_row = inverse && log_n > 7 ? KZG_G1_FFT_WIDE_HALF + log_n - 8 : 0u;
    ZKW_LAUNCH(ctx, k_kzg_g1_fft_order, order_blocks, KZG_G1_FFT_THREADS, (const bls::G1Jac*)d_x, d_y, d_tab, log_n, (u32)total, order_blocks * (u32)KZG_G1_FFT_THREADS,
               scale_row, brp ? 1u : 0u);
    *d_res = d_y;
    return ZKW_OK;
}

extern "C" int zkw_kzg_g1_fft_wide(zkw_ctx* ctx, const uint8_t* points, size_t n, size_t n_ffts, int inverse, uint8_t* out) {
    const char* who = "zkw_kzg_g1_fft_wide";
    if (!ctx || (n_ffts && (!points || !out))) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    if (n == 0 || n > KZG_G1_FFT_WIDE_MAX || (n & (n - 1))) return fail(ZKW_ERR_INVALID, "%s: a power of two from 1 to %u points, not %zu", who, (unsigned)KZG_G1_FFT_WIDE_MAX, n);
    if (n_ffts > 65535) return fail(ZKW_ERR_INVALID, "%s: at most 65535 transforms per call, not %zu", who, n_ffts);
    if (n * n_ffts > KZG_G1_FFT_WIDE_POINTS) return fail(ZKW_ERR_INVALID, "%s: at most %u points per call, not %zu transforms of %zu", who, (unsigned)KZG_G1_FFT_WIDE_POINTS, n_ffts, n);
    if (n_ffts == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t total = n * n_ffts;
    u32 log_n = 0;
    while ((size_t)1 << log_n < n) log_n++;
    const uint8_t* d_in = nullptr;
    ZKW_TRY(ctx->in("kzg_in_points", points, total * 48, &d_in));
    bls::G1Aff* d_aff = nullptr;
    bls::G1Jac *d_jac = nullptr, *d_ord = nullptr;
    u32* d_status = nullptr;
    ZKW_TRY(ctx->scratch_t<bls::G1Aff>("kzg_g1_fft_affine", total, &d_aff));
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_g1_fft_points", total, &d_jac));
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_g1_fft_ordered", total, &d_ord));
    ZKW_TRY(ctx->scratch_t<u32>("kzg_status", total, &d_status));
    ZKW_LAUNCH(ctx, k_kzg_decompress, blocks_for(total, 64), 64, d_in, (u32)total, d_aff, d_status);
    std::vector<u32> status(total);
    ZKW_TRY(ctx->read_small(status.data(), d_status, total * sizeof(u32)));
    for (size_t k = 0; k < total; k++)
        if (status[k] != bls::G1_OK) return fail(ZKW_ERR_INVALID, "%s: point %zu of transform %zu is refused: %s", who, k % n, k / n, kzg_reason(status[k]));
    uint8_t* d_out = nullptr;
    ZKW_TRY(ctx->out("kzg_out", out, total * 48, &d_out));
    ZKW_LAUNCH(ctx, k_kzg_g1_lift, blocks_for(total, 64), 64, (const bls::G1Aff*)d_aff, (u32)total, d_jac);
    const bls::G1Jac* d_res = nullptr;
    ZKW_TRY(kzg_g1_fft_wide_device(ctx, d_jac, d_ord, log_n, n_ffts, inverse != 0, false, &d_res));
    ZKW_LAUNCH(ctx, k_kzg_g1_compress, blocks_for(total, 64), 64, d_res, (u32)total, 0u, d_out);
    ZKW_TRY(ctx->finish_out(out, d_out, total * 48));
    return ctx->sync_if_host();
}

// a new handle from row 0 of s's table, device to device: to the Lagrange basis S'[i] = L[brp(i)], L the inverse transform of S, or back,
// S = the forward transform of L[u] = S'[brp(u)]. Sums of checked points stay in the subgroup: nothing is decompressed or checked again
static int kzg_settings_transform(const char* who, const zkw_kzg_settings* s, zkw_ctx* ctx, bool to_lagrange, zkw_kzg_settings** out) {
    if (!s || !ctx || !out) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    if (s->n & (s->n - 1)) return fail(ZKW_ERR_INVALID, "%s: a transform has a power of two of points, the settings hold %zu", who, s->n);
    if (to_lagrange && s->basis != 0) return fail(ZKW_ERR_INVALID, "%s: the settings are in the Lagrange basis already", who);
    if (ctx->device != s->ctx->device) return fail(ZKW_ERR_INVALID, "%s: the settings live on device %d, the context on device %d", who, s->ctx->device, ctx->device);
    if (ctx->batch) return fail(ZKW_ERR_INVALID, "%s: the context belongs to a batch of blocks", who);
    HIP_TRY(hipSetDevice(ctx->device));
    *out = nullptr;
    const size_t n = s->n;
    u32 log_n = 0;
    while ((size_t)1 << log_n < n) log_n++;
    bls::G1Jac *d_x = nullptr, *d_y = nullptr;
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_g1_fft_points", n, &d_x));
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_g1_fft_ordered", n, &d_y));
    zkw_kzg_settings* h = nullptr;
    const hipError_t e = kzg_handle_new(ctx, s->bytes, 64, &h);
    if (e != hipSuccess) return fail(ZKW_ERR_OOM, "%s: %zu points need %zu bytes of device memory: %s", who, n, s->bytes, hipGetErrorString(e));
    h->n = n;
    h->basis = to_lagrange ? 1 : 0;
    const int rc = [&]() -> int {
        ZKW_LAUNCH(ctx, k_kzg_g1_fft_load, blocks_for(n, 64), 64, (const bls::G1Aff*)s->table, log_n, to_lagrange ? 0u : 1u, d_x);
        const bls::G1Jac* d_res = nullptr;
        ZKW_TRY(kzg_g1_fft_wide_device(ctx, d_x, d_y, log_n, 1, to_lagrange, to_lagrange, &d_res));
        ZKW_LAUNCH(ctx, k_kzg_g1_affine, blocks_for(n, 64), 64, d_res, (u32)n, h->table);
        ZKW_LAUNCH_2D(ctx, k_kzg_table, blocks_for(n, 64), KZG_WINDOWS - 1, 64, h->table, (u32)n);
        HIP_TRY(ctx->sync_stream());  // other contexts read the table without any ordering with this stream
        return ZKW_OK;
    }();
    if (rc != ZKW_OK) return kzg_handle_drop(h, rc);
    ctx_retain(ctx);
    *out = h;
    return ZKW_OK;
}

extern "C" int zkw_kzg_settings_to_lagrange(const zkw_kzg_settings* s, zkw_ctx* ctx, zkw_kzg_settings** out) {
    return kzg_settings_transform("zkw_kzg_settings_to_lagrange", s, ctx, true, out);
}
extern "C" int zkw_kzg_settings_to_monomial(const zkw_kzg_settings* s, zkw_ctx* ctx, zkw_kzg_settings** out) {
    return kzg_settings_transform("zkw_kzg_settings_to_monomial", s, ctx, false, out);
}
extern "C" int zkw_kzg_settings_basis(const zkw_kzg_settings* s) { return s ? s->basis : 0; }

extern "C" int zkw_kzg_settings_points(const zkw_kzg_settings* s, zkw_ctx* ctx, uint8_t* out) {
    const char* who = "zkw_kzg_settings_points";
    if (!s || !ctx || !out) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    if (ctx->device != s->ctx->device) return fail(ZKW_ERR_INVALID, "%s: the settings live on device %d, the context on device %d", who, s->ctx->device, ctx->device);
    HIP_TRY(hipSetDevice(ctx->device));
    bls::G1Jac* d_x = nullptr;
    uint8_t* d_out = nullptr;
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_g1_fft_points", s->n, &d_x));
    ZKW_TRY(ctx->out("kzg_out", out, s->n * 48, &d_out));
    ZKW_LAUNCH(ctx, k_kzg_g1_lift, blocks_for(s->n, 64), 64, (const bls::G1Aff*)s->table, (u32)s->n, d_x);
    ZKW_LAUNCH(ctx, k_kzg_g1_compress, blocks_for(s->n, 64), 64, (const bls::G1Jac*)d_x, (u32)s->n, 0u, d_out);
    ZKW_TRY(ctx->finish_out(out, d_out, s->n * 48));
    return ctx->sync_if_host();
}

// the cells of n >= 1 polynomials read through src; d_evals: their evaluation forms, when the caller has them (cells 0..63 are a copy)
static int kzg_cells_device(zkw_ctx* ctx, KzgSrc src, u32 poly_stride, const uint8_t* d_evals, const bls::Fr* d_tw, const bls::Fr* d_wpow, size_t n, uint8_t* d_cells) {
    ZKW_TRY(kzg_allow_ntt_lds(ctx));
    ZKW_LAUNCH_D(ctx, k_kzg_cells, "k_kzg_cells", dim3((unsigned)n, 2), KZG_NTT_THREADS, KZG_NTT_LDS, src, poly_stride, d_evals, d_tw, d_wpow, d_cells);
    return ZKW_OK;
}

// FK20 from the coefficients of n >= 1 polynomials read through src: the 128 proofs of each at d_proofs ([n][128][48])
static int kzg_cell_proofs_device(const zkw_kzg_cell_settings* cs, zkw_ctx* ctx, KzgSrc src, u32 poly_stride, const bls::Fr* d_tw, size_t n, uint8_t* d_proofs) {
    const size_t n_sums = n * KZG_CELLS;
    uint8_t* d_c = nullptr;
    bls::G1Jac *d_sums = nullptr, *d_h = nullptr;
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_cell_scalars", n_sums * 2048, &d_c));
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_cell_sums", n_sums * 8, &d_sums));
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_cell_points", n_sums, &d_h));
    ZKW_LAUNCH_2D(ctx, k_kzg_cell_toeplitz, 16, n, KZG_CELL_FR_THREADS, src, poly_stride, d_tw, d_c);
    ZKW_LAUNCH_2D(ctx, k_kzg_cell_msm, KZG_CELLS, n, KZG_CELL_MSM_THREADS, (const uint8_t*)d_c, (const bls::G1Aff*)cs->table, d_sums);
    ZKW_LAUNCH(ctx, k_kzg_cell_horner, blocks_for(n_sums, 64), 64, (const bls::G1Jac*)d_sums, (u32)n_sums, d_h);
    ZKW_TRY(kzg_g1_fft_device(ctx, d_h, d_h, 7, n, true, false, false));   // h (its 1 / 128 is in the scalars); entries 64..127 are not h
    ZKW_TRY(kzg_g1_fft_device(ctx, d_h, d_h, 7, n, false, false, true));   // P[u] = sum_(j < 64) w128^(u j) h[j]
    ZKW_LAUNCH(ctx, k_kzg_g1_compress, blocks_for(n_sums, 64), 64, (const bls::G1Jac*)d_h, (u32)n_sums, 1u, d_proofs);
    return ZKW_OK;
}

static int kzg_cells_check_call(const char* who, const zkw_kzg_cell_settings* cs, zkw_ctx* ctx, size_t n) {
    if (cs && ctx->device != cs->ctx->device) return fail(ZKW_ERR_INVALID, "%s: the settings live on device %d, the context on device %d", who, cs->ctx->device, ctx->device);
    return kzg_blob_limit(who, n);
}

extern "C" int zkw_kzg_cells_blobs(zkw_ctx* ctx, const uint8_t* blob_evaluations, size_t n, uint8_t* cells) {
    if (!ctx || (n && (!blob_evaluations || !cells))) return fail(ZKW_ERR_INVALID, "zkw_kzg_cells_blobs: null argument");
    ZKW_TRY(kzg_cells_check_call("zkw_kzg_cells_blobs", nullptr, ctx, n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *d_ev = nullptr, *d_c = nullptr;
    ZKW_TRY(ctx->in("kzg_in_evals", blob_evaluations, n * KZG_EVAL_BYTES, &d_ev));
    ZKW_TRY(kzg_blob_coefficients_device("zkw_kzg_cells_blobs", ctx, d_ev, nullptr, n, &d_c));
    const bls::Fr *d_tw = nullptr, *d_wpow = nullptr;
    ZKW_TRY(kzg_twiddles_device(ctx, &d_tw, &d_wpow));
    uint8_t* d_cells = nullptr;
    ZKW_TRY(ctx->out("kzg_cells", cells, n * KZG_CELLS_BYTES, &d_cells));
    ZKW_TRY(kzg_cells_device(ctx, KzgSrc{d_c, (u32)KZG_BLOB_ELEMENTS, 0}, (u32)KZG_EVAL_BYTES, d_ev, d_tw, d_wpow, n, d_cells));
    ZKW_TRY(ctx->finish_out(cells, d_cells, n * KZG_CELLS_BYTES));
    return ctx->sync_if_host();
}

// the routine both proof calls share: it starts at the coefficients (src), on the device
static int kzg_cells_and_proofs(const zkw_kzg_cell_settings* cs, zkw_ctx* ctx, KzgSrc src, u32 poly_stride, const uint8_t* d_evals, size_t n, uint8_t* cells, uint8_t* proofs) {
    const bls::Fr *d_tw = nullptr, *d_wpow = nullptr;
    ZKW_TRY(kzg_twiddles_device(ctx, &d_tw, cells ? &d_wpow : nullptr));
    uint8_t *d_cells = nullptr, *d_proofs = nullptr;
    if (cells) {
        ZKW_TRY(ctx->out("kzg_cells", cells, n * KZG_CELLS_BYTES, &d_cells));
        ZKW_TRY(kzg_cells_device(ctx, src, poly_stride, d_evals, d_tw, d_wpow, n, d_cells));
    }
    ZKW_TRY(ctx->out("kzg_out", proofs, n * KZG_CELLS * 48, &d_proofs));
    ZKW_TRY(kzg_cell_proofs_device(cs, ctx, src, poly_stride, d_tw, n, d_proofs));
    if (cells) ZKW_TRY(ctx->finish_out(cells, d_cells, n * KZG_CELLS_BYTES));
    ZKW_TRY(ctx->finish_out(proofs, d_proofs, n * KZG_CELLS * 48));
    return ctx->sync_if_host();
}

extern "C" int zkw_kzg_cell_proofs_blobs(const zkw_kzg_cell_settings* cs, zkw_ctx* ctx, const uint8_t* blob_evaluations, size_t n, uint8_t* cells, uint8_t* proofs) {
    if (!cs || !ctx || (n && (!blob_evaluations || !proofs))) return fail(ZKW_ERR_INVALID, "zkw_kzg_cell_proofs_blobs: null argument");
    ZKW_TRY(kzg_cells_check_call("zkw_kzg_cell_proofs_blobs", cs, ctx, n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *d_ev = nullptr, *d_c = nullptr;
    ZKW_TRY(ctx->in("kzg_in_evals", blob_evaluations, n * KZG_EVAL_BYTES, &d_ev));
    ZKW_TRY(kzg_blob_coefficients_device("zkw_kzg_cell_proofs_blobs", ctx, d_ev, nullptr, n, &d_c));
    return kzg_cells_and_proofs(cs, ctx, KzgSrc{d_c, (u32)KZG_BLOB_ELEMENTS, 0}, (u32)KZG_EVAL_BYTES, d_ev, n, cells, proofs);
}

extern "C" int zkw_eip4844_cell_proofs(const zkw_kzg_cell_settings* cs, zkw_ctx* ctx, const uint8_t* blobs, size_t n, uint8_t* cells, uint8_t* proofs) {
    if (!cs || !ctx || (n && (!blobs || !proofs))) return fail(ZKW_ERR_INVALID, "zkw_eip4844_cell_proofs: null argument");
    ZKW_TRY(kzg_cells_check_call("zkw_eip4844_cell_proofs", cs, ctx, n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t* d_b = nullptr;
    ZKW_TRY(ctx->in("kzg_in_blobs", blobs, n * KZG_BLOB_BYTES, &d_b));  // (elements of 31 bytes: all below r)
    return kzg_cells_and_proofs(cs, ctx, KzgSrc{d_b, (u32)KZG_BLOB_ELEMENTS, 1}, (u32)KZG_BLOB_BYTES, nullptr, n, cells, proofs);
}

// ---- EIP-7594 recovery: every cell (and proof) of a blob from any 64 or more of its cells (kzg_recover_kernels.cuh) -----------------------
static_assert(sizeof(KzgSlots) == KZG_CELLS, "the slot table is 128 bytes of kernel argument");

extern "C" int zkw_kzg_recover_cells_blobs(const zkw_kzg_cell_settings* cs, zkw_ctx* ctx, const uint8_t* cell_indices, size_t n_cells, const uint8_t* cells, size_t n,
                                           uint8_t* recovered, uint8_t* proofs) {
    const char* who = "zkw_kzg_recover_cells_blobs";
    if (!ctx || (n && (!cells || !recovered))) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    if (n_cells < KZG_CELL_ELEMENTS || n_cells > KZG_CELLS) return fail(ZKW_ERR_INVALID, "%s: 64 to 128 cells, not %zu", who, n_cells);
    if (!cell_indices) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    KzgSlots slots;
    memset(slots.slot, KZG_RECOVER_ABSENT, sizeof slots.slot);
    for (size_t i = 0; i < n_cells; i++) {
        if (cell_indices[i] >= KZG_CELLS) return fail(ZKW_ERR_INVALID, "%s: cell_indices[%zu] is %u, a cell index is below 128", who, i, (unsigned)cell_indices[i]);
        if (i && cell_indices[i] <= cell_indices[i - 1])
            return fail(ZKW_ERR_INVALID, "%s: cell_indices[%zu] is %u after %u: the indices must ascend strictly", who, i, (unsigned)cell_indices[i], (unsigned)cell_indices[i - 1]);
        slots.slot[cell_indices[i]] = (uint8_t)i;
    }
    if (proofs && !cs) return fail(ZKW_ERR_INVALID, "%s: proofs need cell settings", who);
    ZKW_TRY(kzg_cells_check_call(who, cs, ctx, n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    ZKW_TRY(kzg_allow_ntt_lds(ctx));
    const uint8_t* d_in = nullptr;
    ZKW_TRY(ctx->in("kzg_in_cells", cells, n * n_cells * KZG_CELL_BYTES, &d_in));
    const bls::Fr *d_tw = nullptr, *d_wpow = nullptr;
    ZKW_TRY(kzg_twiddles_device(ctx, &d_tw, &d_wpow));
    bls::Fr* d_z = nullptr;  // z(c_k), k < 128, then the 64 inverses of Z on the coset
    uint8_t *d_ab = nullptr, *d_c = nullptr, *d_full = nullptr;
    u32* d_st = nullptr;  // [n][2] range words, then [n] consistency words
    ZKW_TRY(ctx->scratch_t<bls::Fr>("kzg_recover_vanish", KZG_CELLS + KZG_CELL_ELEMENTS, &d_z));
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_recover_halves", 2 * n * KZG_EVAL_BYTES, &d_ab));
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_blob_coeffs", n * KZG_EVAL_BYTES, &d_c));
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_recover_cells", n * KZG_CELLS_BYTES, &d_full));  // (scratch in both pointer modes: a refused call leaves `recovered` untouched)
    ZKW_TRY(ctx->scratch_t<u32>("kzg_recover_status", 3 * n, &d_st));
    const bls::Fr* d_zinv = d_z + KZG_CELLS;
    const unsigned nb = (unsigned)n;
    ZKW_LAUNCH(ctx, k_kzg_recover_vanish, 1, KZG_RECOVER_VANISH_THREADS, slots, d_tw, d_z, d_z + KZG_CELLS);
    ZKW_LAUNCH_D(ctx, k_kzg_recover_halves, "k_kzg_recover_halves", dim3(nb, 2), KZG_NTT_THREADS, KZG_NTT_LDS, slots, d_in, (u32)n_cells, (const bls::Fr*)d_z, d_tw, d_wpow,
                 d_ab, d_st);
    ZKW_LAUNCH_D(ctx, k_kzg_recover_quotient, "k_kzg_recover_quotient", dim3(nb), KZG_NTT_THREADS, KZG_NTT_LDS, (const uint8_t*)d_ab, d_zinv, d_tw, d_c, d_st + 2 * n);
    const KzgSrc src{d_c, (u32)KZG_BLOB_ELEMENTS, 0};
    ZKW_TRY(kzg_cells_device(ctx, src, (u32)KZG_EVAL_BYTES, nullptr, d_tw, d_wpow, n, d_full));
    ZKW_LAUNCH_2D(ctx, k_kzg_recover_check, KZG_CELLS, n, KZG_RECOVER_CHECK_THREADS, slots, d_in, (u32)n_cells, (const uint8_t*)d_full, d_st + 2 * n);
    std::vector<u32> st(3 * n);  // the call's ONE readback, ahead of anything that writes the caller's buffers
    ZKW_TRY(ctx->read_small(st.data(), d_st, 3 * n * sizeof(u32)));
    for (size_t j = 0; j < n; j++) {
        const u32 lo = st[2 * j] - 1u, hi = st[2 * j + 1] - 1u, bad = lo < hi ? lo : hi;  // (0 - 1: no offender)
        if (bad != ~0u)
            return fail(ZKW_ERR_INVALID, "%s: element %u of cell_indices[%u] (cell %u) of blob %zu is not below r", who, bad & 63u, bad >> 6, (unsigned)cell_indices[bad >> 6], j);
    }
    for (size_t j = 0; j < n; j++)
        if (st[2 * n + j]) return fail(ZKW_ERR_INVALID, "%s: the %zu cells of blob %zu do not lie on one polynomial of degree below 4096", who, n_cells, j);
    ZKW_TRY(ctx->copy_out(recovered, d_full, n * KZG_CELLS_BYTES));
    if (proofs) {
        uint8_t* d_proofs = nullptr;
        ZKW_TRY(ctx->out("kzg_out", proofs, n * KZG_CELLS * 48, &d_proofs));
        ZKW_TRY(kzg_cell_proofs_device(cs, ctx, src, (u32)KZG_EVAL_BYTES, d_tw, n, d_proofs));
        ZKW_TRY(ctx->finish_out(proofs, d_proofs, n * KZG_CELLS * 48));
    }
    return ctx->sync_if_host();
}

// ---- EIP-7594 verification: a verdict per (commitment, cell index, cell, proof) (kzg_cell_verify_kernels.cuh) ------------------------------
// [I_k(tau)] G1 of n >= 1 claims, Jacobian, at *d_h, and k_kzg_cell_interpolate's status words at *d_st: the twiddles, the interpolation,
// the 64-term sums over columns 0..63 of the settings' table, their Horner step. Nothing is read back
static int kzg_cell_commit_device(const zkw_kzg_settings* s, zkw_ctx* ctx, const uint8_t* d_idx, const uint8_t* d_cells, size_t n, const bls::Fr** d_tw,
                                  const bls::G1Jac** d_h, const u32** d_st) {
    const bls::Fr* d_wpow = nullptr;
    uint8_t* d_c = nullptr;
    bls::G1Jac *d_sums = nullptr, *d_pts = nullptr;
    u32* d_status = nullptr;
    ZKW_TRY(ctx->scratch_t<uint8_t>("kzg_cell_scalars", n * KZG_CELL_BYTES, &d_c));
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_cell_sums", n * 8, &d_sums));
    ZKW_TRY(ctx->scratch_t<bls::G1Jac>("kzg_cell_points", n, &d_pts));
    ZKW_TRY(ctx->scratch_t<u32>("kzg_cell_status", n, &d_status));
    ZKW_TRY(kzg_twiddles_device(ctx, d_tw, &d_wpow));
    ZKW_LAUNCH(ctx, k_kzg_cell_interpolate, blocks_for(n, KZG_CELL_INTERP_CLAIMS), KZG_CELL_INTERP_THREADS, d_idx, d_cells, (u32)n, *d_tw, d_wpow, d_c, d_status);
    ZKW_LAUNCH(ctx, k_kzg_cell_commit_msm, n, KZG_CELL_MSM_THREADS, (const uint8_t*)d_c, (const bls::G1Aff*)s->table, (u32)s->n, d_sums);
    ZKW_LAUNCH(ctx, k_kzg_cell_horner, blocks_for(n, 64), 64, (const bls::G1Jac*)d_sums, (u32)n, d_pts);
    *d_h = d_pts;
    *d_st = d_status;
    return ZKW_OK;
}

static int kzg_cell_claims_check_call(const char* who, const zkw_kzg_settings* s, zkw_ctx* ctx, size_t n) {
    ZKW_TRY(kzg_monomial_only(who, s));
    if (ctx->device != s->ctx->device) return fail(ZKW_ERR_INVALID, "%s: the settings live on device %d, the context on device %d", who, s->ctx->device, ctx->device);
    if (s->n < KZG_CELL_ELEMENTS) return fail(ZKW_ERR_INVALID, "%s: a cell's interpolant has 64 coefficients, the settings hold %zu points", who, s->n);
    if (n > (1u << 24)) return fail(ZKW_ERR_INVALID, "%s: at most %u claims per call, not %zu", who, 1u << 24, n);
    return ZKW_OK;
}

extern "C" int zkw_kzg_commit_cells(const zkw_kzg_settings* s, zkw_ctx* ctx, const uint64_t* cell_indices, const uint8_t* cells, size_t n, uint8_t* out) {
    const char* who = "zkw_kzg_commit_cells";
    if (!s || !ctx || (n && (!cell_indices || !cells || !out))) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    ZKW_TRY(kzg_cell_claims_check_call(who, s, ctx, n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint64_t* d_idx = nullptr;
    const uint8_t* d_cells = nullptr;
    ZKW_TRY(ctx->in("kzg_in_indices", cell_indices, n, &d_idx));
    ZKW_TRY(ctx->in("kzg_in_cells", cells, n * KZG_CELL_BYTES, &d_cells));
    const bls::Fr* d_tw = nullptr;
    const bls::G1Jac* d_h = nullptr;
    const u32* d_st = nullptr;
    ZKW_TRY(kzg_cell_commit_device(s, ctx, reinterpret_cast<const uint8_t*>(d_idx), d_cells, n, &d_tw, &d_h, &d_st));
    std::vector<u32> st(n);  // the call's ONE readback, ahead of anything that writes the caller's buffer
    ZKW_TRY(ctx->read_small(st.data(), d_st, n * sizeof(u32)));
    for (size_t i = 0; i < n; i++) {
        if (st[i] == KZG_CELL_ST_BAD_INDEX) return fail(ZKW_ERR_INVALID, "%s: cell_indices[%zu] is not below 128", who, i);
        if (st[i] != KZG_CELL_ST_OK) return fail(ZKW_ERR_INVALID, "%s: element %u of cells[%zu] is not below r", who, (unsigned)(st[i] - KZG_CELL_ST_BAD_ELEMENT), i);
    }
    uint8_t* d_out = nullptr;
    ZKW_TRY(ctx->out("kzg_out", out, n * 48, &d_out));
    ZKW_LAUNCH(ctx, k_kzg_g1_compress, blocks_for(n, 64), 64, d_h, (u32)n, 0u, d_out);
    ZKW_TRY(ctx->finish_out(out, d_out, n * 48));
    return ctx->sync_if_host();
}

extern "C" int zkw_kzg_verify_cells(const zkw_kzg_verifier* v64, const zkw_kzg_settings* s, zkw_ctx* ctx, const uint8_t* commitments, const uint64_t* cell_indices,
                                    const uint8_t* cells, const uint8_t* proofs, size_t n, uint8_t* verdicts) {
    const char* who = "zkw_kzg_verify_cells";
    if (!v64 || !s || !ctx || (n && (!commitments || !cell_indices || !cells || !proofs || !verdicts))) return fail(ZKW_ERR_INVALID, "%s: null argument", who);
    ZKW_TRY(kzg_verify_check_call(who, v64, ctx, n));
    ZKW_TRY(kzg_cell_claims_check_call(who, s, ctx, n));
    if (n == 0) return ZKW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint64_t* d_idx64 = nullptr;
    const uint8_t *d_cm = nullptr, *d_cells = nullptr, *d_pr = nullptr;
    ZKW_TRY(ctx->in("kzg_in_commitments", commitments, n * 48, &d_cm));
    ZKW_TRY(ctx->in("kzg_in_indices", cell_indices, n, &d_idx64));
    ZKW_TRY(ctx->in("kzg_in_cells", cells, n * KZG_CELL_BYTES, &d_cells));
    ZKW_TRY(ctx->in("kzg_in_proofs", proofs, n * 48, &d_pr));
    const uint8_t* d_idx = reinterpret_cast<const uint8_t*>(d_idx64);
    uint8_t* d_verdicts = nullptr;
    ZKW_TRY(ctx->out("kzg_verdicts", verdicts, n, &d_verdicts));
    const bls::Fr* d_tw = nullptr;
    const bls::G1Jac* d_h = nullptr;
    const u32* d_ist = nullptr;
    ZKW_TRY(kzg_cell_commit_device(s, ctx, d_idx, d_cells, n, &d_tw, &d_h, &d_ist));
    bls::G1Aff* d_pts = nullptr;
    u32* d_status = nullptr;
    ZKW_TRY(ctx->scratch_t<bls::G1Aff>("kzg_verify_points", 2 * n, &d_pts));
    ZKW_TRY(ctx->scratch_t<u32>("kzg_verify_status", n, &d_status));
    ZKW_LAUNCH(ctx, k_kzg_verify_cell_points, blocks_for(n, 64), 64, d_cm, d_idx, d_pr, d_ist, d_h, d_tw, (u32)n, d_pts, d_status);
    ZKW_LAUNCH_D(ctx, k_kzg_verify_pairing, "k_kzg_verify_pairing", dim3(blocks_for(n, KZG_VFY_CLAIMS_PER_BLOCK)), KZG_VFY_THREADS, bls::f12_lds_bytes(KZG_VFY_THREADS), (const bls::G1Aff*)d_pts, (const u32*)d_status, (const bls::G2Line*)v64->table, (u32)n, d_verdicts);
    ZKW_TRY(ctx->finish_out(verdicts, d_verdicts, n));
    return ctx->sync_if_host();
}
