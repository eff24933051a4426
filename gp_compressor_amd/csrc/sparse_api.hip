// sparse_api.hip -- the gpc_sparse_* entry points of the C-ABI (include/gpc.h): the object and its state, then the staged pairs, each a
// _dev entry on device pointers and a host-pointer twin.  Where things are:
//   - what a call is refused for: one *_rules function per pair, in the order the entry applies its rules, from the liveness of the object
//     (ctx: what sp_live, sparse_internal.h, said of it) to the nothing-to-do return.  The ragged batch (off, sizes, x0 / x1 / third array) is an SpBatch and its
//     rules are written once (sp_batch_shape_rules, sp_batch_null_rule).  Where the host twin and the _dev twin differ today, the rules
//     function says so in a condition on `host` with a comment;
//   - the critical section of a _dev entry: sp_locked -- the context's lock, its device, the LDS poison of diagnostic runs, the launcher
//     (beside its kernels: sparse.hip, sparse_rate.hip, sparse_predict.hip, sparse_scatter.hip);
//   - what a host twin stages: its list of up() / out(), the _dev twin, its list of down() (GpcStaging, gpc_internal.h), every size named
//     once above the list.  A host twin never takes ctx->mu itself: the _dev twin it calls does;
//   - the sizes of the state: sp_state_bytes.
#include <new>

#include "sparse_internal.h"

#define GPC_TRAIN_MAX_COUNTER 10000

static void sp_free_all(gpc_sparse* g)
{
    for (void* p : {(void*)g->alpha, (void*)g->C, (void*)g->Q, (void*)g->BV, (void*)g->b, (void*)g->count, (void*)g->stat, (void*)g->done_it, (void*)g->list})
        if (p) (void)hipFree(p);
    delete g;
}

// The bytes of the state arrays: alpha | C and Q, each | BV | b, count, stat and done_it, each.  An object of no patch is allocated as one.
struct SpStateBytes {
    size_t alpha, mat, bv, words;
};
static SpStateBytes sp_state_bytes(const gpc_sparse* g)
{
    const size_t ld = (size_t)g->ld, Pn = (size_t)(g->P > 0 ? g->P : 1);
    return SpStateBytes{8 * Pn * (size_t)g->ny * ld, 8 * Pn * ld * ld, 8 * Pn * ld * 2, 4 * Pn};
}

// every patch empty: no basis vector, no point seen, status OK
static hipError_t sp_empty_all(gpc_sparse* g, hipStream_t stream)
{
    hipError_t e = hipSuccess;
    for (int32_t* words : {g->b, g->count, g->stat})
        if (e == hipSuccess) e = hipMemsetAsync(words, 0, sp_state_bytes(g).words, stream);
    return e;
}

// gpc_sparse_remap: the state of patch i of `src` goes to patch map[i] of `dst` (same ld, same ny); one workgroup per source patch
__global__ __launch_bounds__(256) void sp_remap_kernel(const double* alpha, const double* C, const double* Q, const double* BV, const int32_t* b,
                                                       const int32_t* count, const int32_t* stat, const int32_t* map, int ny, int ld,
                                                       double* alpha_o, double* C_o, double* Q_o, double* BV_o, int32_t* b_o, int32_t* count_o,
                                                       int32_t* stat_o)
{
    const size_t i = blockIdx.x, j = (size_t)map[i];
    const size_t na = (size_t)ny * ld, nc = (size_t)ld * ld, nb = (size_t)ld * 2;
    for (size_t e = threadIdx.x; e < nc; e += 256) {
        C_o[j * nc + e] = C[i * nc + e];
        Q_o[j * nc + e] = Q[i * nc + e];
    }
    for (size_t e = threadIdx.x; e < na; e += 256) alpha_o[j * na + e] = alpha[i * na + e];
    for (size_t e = threadIdx.x; e < nb; e += 256) BV_o[j * nb + e] = BV[i * nb + e];
    if (threadIdx.x == 0) {
        b_o[j] = b[i];
        count_o[j] = count[i];
        stat_o[j] = stat[i];
    }
}

// ---- the rules.  A *_rules function answers an error code, GPC_OK -- go on -- or SP_NOTHING: the call is valid and there is nothing to do.
enum { SP_NOTHING = 1 };
static int sp_done(int rules) { return rules == SP_NOTHING ? GPC_OK : rules; }

// The ragged batch of a call; third: y, or the mean a predict call writes.  Host form: host pointers, n_max and n_total found from off.
struct SpBatch {
    const int32_t* off;
    int n_max, n_total;
    const double *x0, *x1, *third;
};

// off and the sizes.  size_first: the entry looks at its sizes before it looks at off.  Host form: off is read -- it starts at 0 and does
// not decrease -- and gives the sizes (all zero for an object of no patch, where off is not looked at).
static int sp_batch_shape_rules(gpc_ctx* ctx, const gpc_sparse* g, SpBatch& b, bool host, bool size_first)
{
    const bool bad_size = b.n_total < 0 || b.n_max < 0, bad_off = g->P > 0 && !b.off;
    if (bad_size && (size_first || !bad_off)) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (bad_off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    return host ? gpc_check_host_off(ctx, g->P, b.off, &b.n_max, &b.n_total) : GPC_OK;
}
// points without coordinates or without the third array
static int sp_batch_null_rule(gpc_ctx* ctx, const SpBatch& b, const char* text = nullptr)
{
    if (b.n_total > 0 && (!b.x0 || !b.x1 || !b.third)) return gpc_fail(ctx, GPC_EINVAL, "%s", text ? text : "x0/x1/y is NULL");
    return GPC_OK;
}
static int sp_batch_rules(gpc_ctx* ctx, const gpc_sparse* g, SpBatch& b, bool host, bool size_first, const char* text = nullptr)
{
    if (int rc = sp_batch_shape_rules(ctx, g, b, host, size_first)) return rc;
    return sp_batch_null_rule(ctx, b, text);
}

static int sp_add_rules(gpc_ctx* ctx, const gpc_sparse* g, SpBatch& b, const int32_t* perm, bool host)
{
    if (!ctx) return GPC_EINVAL;
    if (int rc = sp_batch_rules(ctx, g, b, host, false)) return rc;
    for (int i = 0; host && perm && i < g->P; ++i)      // (a device array cannot be validated without a synchronisation)
        for (int k = b.off[i]; k < b.off[i + 1]; ++k)
            if (perm[k] < 0 || perm[k] >= b.off[i + 1] - b.off[i])
                return gpc_fail(ctx, GPC_EINVAL, "perm[%d] = %d outside patch %d", k, perm[k], i);
    return g->P == 0 ? SP_NOTHING : GPC_OK;
}

static int sp_prune_rules(gpc_ctx* ctx, const gpc_sparse* g, int keep, const int32_t* target, double score_tol)
{
    if (!ctx) return GPC_EINVAL;
    if (!target && keep < 1) return gpc_fail(ctx, GPC_EINVAL, "keep must be >= 1 when target is NULL, got %d", keep);
    if (!(score_tol >= 0.0)) return gpc_fail(ctx, GPC_EINVAL, "score_tol must be >= 0 (+inf allowed), got %g", score_tol);
    return g->P == 0 ? SP_NOTHING : GPC_OK;
}

static int sp_prune_rd_rules(gpc_ctx* ctx, const gpc_sparse* g, SpBatch& b, int keep, const int32_t* target, double max_mse,
                             const double* max_mse_p, bool host)
{
    if (!ctx) return GPC_EINVAL;
    if (g->prm.noise_model != GPC_NOISE_GAUSSIAN)
        return gpc_fail(ctx, GPC_EINVAL, "prune_rd: the error is taken against the Gaussian read-out (noise_model 0), got %d", g->prm.noise_model);
    if (!target && keep < 1) return gpc_fail(ctx, GPC_EINVAL, "keep must be >= 1 when target is NULL, got %d", keep);
    if (!max_mse_p && !(max_mse >= 0.0)) return gpc_fail(ctx, GPC_EINVAL, "max_mse must be >= 0 (+inf allowed), got %g", max_mse);
    if (int rc = sp_batch_rules(ctx, g, b, host, true)) return rc;
    return g->P == 0 ? SP_NOTHING : GPC_OK;
}

static int sp_quantize_rd_rules(gpc_ctx* ctx, const gpc_sparse* g, SpBatch& b, int bits_min, int bits_max, double max_mse,
                                const double* max_mse_p, bool host)
{
    if (!ctx) return GPC_EINVAL;
    if (g->prm.noise_model != GPC_NOISE_GAUSSIAN)
        return gpc_fail(ctx, GPC_EINVAL, "quantize_rd: the error is taken against the Gaussian read-out (noise_model 0), got %d", g->prm.noise_model);
    if (bits_min < 1 || bits_max > 16 || bits_min > bits_max)
        return gpc_fail(ctx, GPC_EINVAL, "quantize_rd: widths must satisfy 1 <= bits_min <= bits_max <= 16, got %d .. %d", bits_min, bits_max);
    if (!max_mse_p && !(max_mse >= 0.0)) return gpc_fail(ctx, GPC_EINVAL, "max_mse must be >= 0 (+inf allowed), got %g", max_mse);
    if (int rc = sp_batch_rules(ctx, g, b, host, true)) return rc;
    return g->P == 0 ? SP_NOTHING : GPC_OK;
}

static int sp_dequantize_rules(gpc_ctx* ctx, const gpc_sparse* g, const int32_t* bv_count, const int32_t* bits, const uint16_t* q_alpha,
                               const uint16_t* q_bv, const float* range, bool host)
{
    if (!ctx) return GPC_EINVAL;
    if (g->P == 0) return SP_NOTHING;
    if (!bv_count || !bits || !q_alpha || !q_bv || !range) return gpc_fail(ctx, GPC_EINVAL, "bv_count/bits/q_alpha/q_bv/range is NULL");
    // the host twin checks the widths and counts it can read; the _dev twin cannot, and its kernel clamps them.  (A count out of range is
    // GPC_EINVAL here and GPC_ERANGE in gpc_sparse_set_state.)
    for (int i = 0; host && i < g->P; ++i) {
        if (bits[i] < 0 || bits[i] > 16) return gpc_fail(ctx, GPC_EINVAL, "bits[%d] = %d outside [0, 16]", i, bits[i]);
        if (bv_count[i] < 0 || bv_count[i] > g->ld)
            return gpc_fail(ctx, GPC_EINVAL, "bv_count[%d] = %d outside [0, %d]", i, bv_count[i], g->ld);
    }
    return GPC_OK;
}

static int sp_predict_rules(gpc_ctx* ctx, const gpc_sparse* g, int m, const double* xs0, const double* xs1, const double* f_star)
{
    if (!ctx) return GPC_EINVAL;
    if (m < 0) return gpc_fail(ctx, GPC_EINVAL, "negative m");
    if (m > 0 && (!xs0 || !xs1 || !f_star)) return gpc_fail(ctx, GPC_EINVAL, "xs0/xs1/f_star is NULL");
    return g->P == 0 || m == 0 ? SP_NOTHING : GPC_OK;
}

static int sp_predict_points_rules(gpc_ctx* ctx, const gpc_sparse* g, SpBatch& b, bool host)
{
    if (!ctx) return GPC_EINVAL;
    if (int rc = sp_batch_rules(ctx, g, b, host, false, "x0/x1/f is NULL")) return rc;
    return g->P == 0 ? SP_NOTHING : GPC_OK;
}

static int sp_scattered_rules(gpc_ctx* ctx, const gpc_sparse* g, int n, const int32_t* patch, const double* x0, const double* x1, int stride,
                              const int32_t* status)
{
    if (!ctx) return GPC_EINVAL;
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (stride < 1) return gpc_fail(ctx, GPC_EINVAL, "stride must be >= 1, got %d", stride);
    if (n > 0 && (!patch || !x0 || !x1)) return gpc_fail(ctx, GPC_EINVAL, "patch/x0/x1 is NULL");
    return n == 0 && (!status || g->P == 0) ? SP_NOTHING : GPC_OK;      // (with status the empty batch is still reported on)
}

static int sp_likelihood_rules(gpc_ctx* ctx, const gpc_sparse* g, SpBatch& b, const double* dX, const double* l, bool host)
{
    if (!ctx) return GPC_EINVAL;
    if (int rc = sp_batch_rules(ctx, g, b, host, false)) return rc;
    // the noise-model rule stands before the nothing-to-do return in the _dev twin only: a host call with nothing to do on a probit object
    // is GPC_OK, one with work meets the rule through the _dev twin
    if (!host && g->prm.noise_model != 0) return gpc_fail(ctx, GPC_EINVAL, "likelihoods are defined for the Gaussian noise model");
    return g->P == 0 || b.n_total == 0 || (!dX && !l) ? SP_NOTHING : GPC_OK;
}

static int sp_train_rules(gpc_ctx* ctx, const gpc_sparse* g, SpBatch& b, double step, int max_counter, const double* p0, const int32_t* iters,
                          const double* ls, const double* delta, bool host)
{
    if (!ctx) return GPC_EINVAL;
    // ny, the noise model and step are rules of the _dev twin alone: a host call meets them through it, behind its staging
    if (!host && g->ny != 1) return gpc_fail(ctx, GPC_EINVAL, "train_parameters exists for sparse_gp (ny == 1) only");
    if (!host && g->prm.noise_model != 0) return gpc_fail(ctx, GPC_EINVAL, "likelihoods are defined for the Gaussian noise model");
    if (int rc = sp_batch_shape_rules(ctx, g, b, host, false)) return rc;
    if (host && g->P == 0) return SP_NOTHING;      // the host twin returns here; the _dev twin applies the rules below first
    if (max_counter < 0 || max_counter > GPC_TRAIN_MAX_COUNTER) return gpc_fail(ctx, GPC_EINVAL, "max_counter must be in [0, %d]", GPC_TRAIN_MAX_COUNTER);
    if (!host && !(step == step)) return gpc_fail(ctx, GPC_EINVAL, "step is NaN");
    if (int rc = sp_batch_null_rule(ctx, b)) return rc;
    if (g->P > 0 && (!p0 || !iters || !ls || !delta)) return gpc_fail(ctx, GPC_EINVAL, "p0/iters/ls/delta is NULL");
    return g->P == 0 ? SP_NOTHING : GPC_OK;
}

// ---- what a _dev entry does with the answer of its rules: return it, or enter the critical section -- the context's lock, its device, the
// LDS poison of diagnostic runs (gpc_debug_poison_lds) -- and call the launcher, which expects exactly that of its caller (sparse_internal.h)
template <class Launch> static int sp_locked(const gpc_sparse* g, int rules, Launch launch)
{
    if (rules != GPC_OK) return sp_done(rules);
    gpc_ctx* ctx = g->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = gpc_debug_poison_lds(ctx)) return rc;
    return launch();
}

extern "C" {

// ---- the object and its state ---------------------------------------------------------------------------------------------------

int gpc_sparse_create(gpc_ctx* ctx, const gpc_params* params, int P, int ny, gpc_sparse** out)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!out) return gpc_fail(ctx, GPC_EINVAL, "out is NULL");
    *out = nullptr;
    if (!params) return gpc_fail(ctx, GPC_EINVAL, "params is NULL");
    if (P < 0) return gpc_fail(ctx, GPC_EINVAL, "negative P");
    if (ny != 1 && ny != 3) return gpc_fail(ctx, GPC_EINVAL, "ny must be 1 (sparse_gp) or 3 (sparse_gp_field), got %d", ny);
    if (params->capacity == 0 || params->capacity < -1) return gpc_fail(ctx, GPC_EINVAL, "capacity must be > 0 or -1");
    if (params->capacity > GPC_MAX_BV - 1) return gpc_fail(ctx, GPC_ERANGE, "capacity %d > %d", params->capacity, GPC_MAX_BV - 1);
    if (params->noise_model < 0 || params->noise_model > 2) return gpc_fail(ctx, GPC_EINVAL, "noise_model must be 0, 1 or 2");
    if (params->noise_model != 0 && ny != 1) return gpc_fail(ctx, GPC_EINVAL, "probit noise needs ny == 1");
    if (!(params->l_sq > 0.0) || !(params->sigmaf_sq > 0.0)) return gpc_fail(ctx, GPC_EINVAL, "kernel parameters out of range");
    gpc_sparse* g = new (std::nothrow) gpc_sparse();       // (every pointer null)
    if (!g) return GPC_ENOMEM;
    g->ctx = ctx; g->prm = *params; g->P = P; g->ny = ny;
    // capacity + 1 rows (a full update holds capacity + 1 basis vectors until the deletion that follows it), rounded up to 16
    // doubles = 128 B: every column of C and Q then starts on a cache line, and a wave's 64-row segment is exactly 4 lines.
    // With ld = 201 the segments straddled lines -- 5 fetched per 4 used, re-fetched from HBM by the next row trip -- and
    // the add path, which is bound by exactly this stream, read 27 % more than it consumed (profiles/r02_summary.json).
    g->ld = params->capacity == -1 ? GPC_MAX_BV : ((params->capacity + 1 + 15) & ~15);
    std::lock_guard<std::mutex> lk(ctx->mu);
    const SpStateBytes n = sp_state_bytes(g);
    const struct { void** p; size_t bytes; } bufs[] = {
        {(void**)&g->alpha, n.alpha}, {(void**)&g->C, n.mat}, {(void**)&g->Q, n.mat}, {(void**)&g->BV, n.bv}, {(void**)&g->b, n.words},
        {(void**)&g->count, n.words}, {(void**)&g->stat, n.words}, {(void**)&g->done_it, n.words},
        {(void**)&g->list, 3 * n.words + 4 * 12}};       // three work lists of P entries, then their 3 x 4 counters
    hipError_t e = hipSetDevice(ctx->device);
    for (const auto& buf : bufs)
        if (e == hipSuccess) e = hipMalloc(buf.p, buf.bytes);
    if (e == hipSuccess) e = sp_empty_all(g, ctx->stream);
    if (e != hipSuccess) {
        int rc = gpc_fail(ctx, e == hipErrorOutOfMemory ? GPC_ENOMEM : GPC_EHIP, "gpc_sparse_create: %s", hipGetErrorString(e));
        sp_free_all(g);
        return rc;
    }
    gpc_ctx_ref(ctx);
    g->serial = gpc_child_register(ctx, g);
    *out = g;
    return GPC_OK;
}

// Safe in either order with gpc_ctx_destroy: a context destroyed first has synchronised its stream already and stays
// allocated (dead) until its last child is gone.
void gpc_sparse_destroy(gpc_sparse* g)
{
    if (!g) return;
    gpc_ctx* ctx = g->ctx;
    (void)hipSetDevice(ctx->device);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (!ctx->dead.load()) (void)hipStreamSynchronize(ctx->stream);
        gpc_child_unregister(ctx, g);
    }
    sp_free_all(g);
    gpc_ctx_unref(ctx);
}

int gpc_sparse_ld(const gpc_sparse* g) { return g ? g->ld : GPC_EINVAL; }

int gpc_sparse_remap(gpc_sparse* old, int P_new, const int32_t* old_to_new, gpc_sparse** out)
{
    gpc_ctx* ctx = sp_live(old);
    if (!ctx) return GPC_EINVAL;
    if (!out) return gpc_fail(ctx, GPC_EINVAL, "out is NULL");
    *out = nullptr;
    const int P = old->P;
    if (P_new < P) return gpc_fail(ctx, GPC_EINVAL, "P_new %d is smaller than the object's P %d", P_new, P);
    if (P > 0 && !old_to_new) return gpc_fail(ctx, GPC_EINVAL, "old_to_new is NULL");
    for (int i = 0; i < P; ++i)
        if (old_to_new[i] < 0 || old_to_new[i] >= P_new || (i > 0 && old_to_new[i] <= old_to_new[i - 1]))
            return gpc_fail(ctx, GPC_EINVAL, "old_to_new[%d] = %d: the table must be strictly increasing within [0, %d)", i, old_to_new[i], P_new);
    gpc_sparse* g = nullptr;
    if (int rc = gpc_sparse_create(ctx, &old->prm, P_new, old->ny, &g)) return rc;      // every patch empty, as after gpc_sparse_reset
    if (P == 0) { *out = g; return GPC_OK; }
    hipError_t e;
    int rcp = GPC_OK;                                     // the poison call of diagnostic runs: its own code and text
    void* d_map = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        hipStream_t st = ctx->stream;
        const size_t n_map = 4 * (size_t)P;
        e = hipSetDevice(ctx->device);
        if (e == hipSuccess) rcp = gpc_debug_poison_lds(ctx);
        if (rcp != GPC_OK) e = hipErrorUnknown;
        if (e == hipSuccess) e = hipMalloc(&d_map, n_map);
        if (e == hipSuccess) e = hipMemcpyAsync(d_map, old_to_new, n_map, hipMemcpyHostToDevice, st);
        // the patches no old one moves into: a zero state, not what the allocation happened to hold (gpc_sparse_get_state reads it back)
        const SpStateBytes n = sp_state_bytes(g);
        if (e == hipSuccess) e = hipMemsetAsync(g->alpha, 0, n.alpha, st);
        if (e == hipSuccess) e = hipMemsetAsync(g->C, 0, n.mat, st);
        if (e == hipSuccess) e = hipMemsetAsync(g->Q, 0, n.mat, st);
        if (e == hipSuccess) e = hipMemsetAsync(g->BV, 0, n.bv, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(sp_remap_kernel, dim3(P), dim3(256), 0, st, old->alpha, old->C, old->Q, old->BV, old->b, old->count, old->stat,
                               (const int32_t*)d_map, old->ny, old->ld, g->alpha, g->C, g->Q, g->BV, g->b, g->count, g->stat);
            e = hipGetLastError();
        }
        const hipError_t es = hipStreamSynchronize(st);                                  // the table is the caller's again; d_map goes
        if (e == hipSuccess) e = es;
        if (d_map) (void)hipFree(d_map);
    }
    if (e != hipSuccess) {
        const int rc = rcp != GPC_OK ? rcp : gpc_fail(ctx, e == hipErrorOutOfMemory ? GPC_ENOMEM : GPC_EHIP, "gpc_sparse_remap: %s", hipGetErrorString(e));
        gpc_sparse_destroy(g);
        return rc;
    }
    *out = g;
    return GPC_OK;
}

int gpc_sparse_set_trace(gpc_sparse* g, uint8_t* trace_dev)
{
    gpc_ctx* ctx = sp_live(g);
    if (!ctx) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    g->trace = trace_dev;
    return GPC_OK;
}

int gpc_sparse_reset(gpc_sparse* g)
{
    gpc_ctx* ctx = sp_live(g);
    if (!ctx) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GPC_HIP(ctx, sp_empty_all(g, ctx->stream));
    return GPC_OK;
}

int gpc_sparse_sizes(gpc_sparse* g, int32_t* bv_count)
{
    gpc_ctx* ctx = sp_live(g);
    if (!ctx) return GPC_EINVAL;
    if (!bv_count) return gpc_fail(ctx, GPC_EINVAL, "bv_count is NULL");
    if (g->P == 0) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = gpc_stream_of(ctx);
    GPC_HIP(ctx, hipMemcpyAsync(bv_count, g->b, sp_state_bytes(g).words, hipMemcpyDeviceToHost, s));
    GPC_HIP(ctx, hipStreamSynchronize(s));
    return GPC_OK;
}

int gpc_sparse_get_state(gpc_sparse* g, double* alpha, double* C, double* Q, double* BV)
{
    gpc_ctx* ctx = sp_live(g);
    if (!ctx) return GPC_EINVAL;
    if (g->P == 0) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const SpStateBytes n = sp_state_bytes(g);
    hipStream_t s = gpc_stream_of(ctx);
    if (alpha) GPC_HIP(ctx, hipMemcpyAsync(alpha, g->alpha, n.alpha, hipMemcpyDeviceToHost, s));
    if (C) GPC_HIP(ctx, hipMemcpyAsync(C, g->C, n.mat, hipMemcpyDeviceToHost, s));
    if (Q) GPC_HIP(ctx, hipMemcpyAsync(Q, g->Q, n.mat, hipMemcpyDeviceToHost, s));
    if (BV) GPC_HIP(ctx, hipMemcpyAsync(BV, g->BV, n.bv, hipMemcpyDeviceToHost, s));
    GPC_HIP(ctx, hipStreamSynchronize(s));
    return GPC_OK;
}

// Inverse of gpc_sparse_get_state: loads a stored model (the compressed representation of row f3).  alpha and BV are
// required, C and Q may be NULL (zeroed: the mean prediction of the decompressor needs neither; sigma, likelihoods and
// further online growth do).
int gpc_sparse_set_state(gpc_sparse* g, const int32_t* bv_count, const double* alpha, const double* C, const double* Q,
                         const double* BV)
{
    gpc_ctx* ctx = sp_live(g);
    if (!ctx) return GPC_EINVAL;
    if (g->P == 0) return GPC_OK;
    if (!bv_count || !alpha || !BV) return gpc_fail(ctx, GPC_EINVAL, "bv_count/alpha/BV is NULL");
    for (int i = 0; i < g->P; ++i)      // (GPC_ERANGE here, GPC_EINVAL in gpc_sparse_dequantize: sp_dequantize_rules)
        if (bv_count[i] < 0 || bv_count[i] > g->ld) return gpc_fail(ctx, GPC_ERANGE, "bv_count[%d] = %d outside [0, %d]", i, bv_count[i], g->ld);
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const SpStateBytes n = sp_state_bytes(g);
    hipStream_t s = ctx->stream;
    GPC_HIP(ctx, hipMemcpyAsync(g->b, bv_count, n.words, hipMemcpyHostToDevice, s));
    GPC_HIP(ctx, hipMemcpyAsync(g->count, bv_count, n.words, hipMemcpyHostToDevice, s));
    GPC_HIP(ctx, hipMemsetAsync(g->stat, 0, n.words, s));
    GPC_HIP(ctx, hipMemcpyAsync(g->alpha, alpha, n.alpha, hipMemcpyHostToDevice, s));
    GPC_HIP(ctx, hipMemcpyAsync(g->BV, BV, n.bv, hipMemcpyHostToDevice, s));
    if (C) GPC_HIP(ctx, hipMemcpyAsync(g->C, C, n.mat, hipMemcpyHostToDevice, s));
    else GPC_HIP(ctx, hipMemsetAsync(g->C, 0, n.mat, s));
    if (Q) GPC_HIP(ctx, hipMemcpyAsync(g->Q, Q, n.mat, hipMemcpyHostToDevice, s));
    else GPC_HIP(ctx, hipMemsetAsync(g->Q, 0, n.mat, s));
    GPC_HIP(ctx, hipStreamSynchronize(s));
    return GPC_OK;
}

// ---- the staged pairs: the _dev entry (its rules, then sp_locked around the launcher) and the host twin (its rules, its staging) ------

int gpc_sparse_add_dev(gpc_sparse* g, const int32_t* off, int n_max, int n_total, const double* x0, const double* x1,
                       const double* y, const int32_t* perm, int32_t* status)
{
    SpBatch b{off, n_max, n_total, x0, x1, y};
    return sp_locked(g, sp_add_rules(sp_live(g), g, b, perm, false), [&] { return sp_add_launch(g, off, n_total, x0, x1, y, perm, status); });
}

int gpc_sparse_add(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y,
                   const int32_t* perm, int32_t* status)
{
    SpBatch b{off, 0, 0, x0, x1, y};
    if (int rc = sp_add_rules(sp_live(g), g, b, perm, true)) return sp_done(rc);
    GPC_HIP(g->ctx, hipSetDevice(g->ctx->device));
    const size_t P = (size_t)g->P, N = (size_t)b.n_total, n_y = N * (size_t)g->ny;
    GpcStaging st(g->ctx, "gpc_sparse_add");
    const int32_t* d_off = st.up(off, P + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N), *d_y = st.up(y, n_y);
    const int32_t* d_perm = perm ? st.up(perm, N) : nullptr;
    int32_t* d_st = st.out<int32_t>(P);
    if (st.ok()) st.rc = gpc_sparse_add_dev(g, d_off, b.n_max, b.n_total, d_x0, d_x1, d_y, d_perm, d_st);
    st.down(status, d_st, P);
    return st.finish();
}

int gpc_sparse_prune_dev(gpc_sparse* g, int keep, const int32_t* target, double score_tol, int32_t* removed, int32_t* order,
                         double* scores, int32_t* status)
{
    return sp_locked(g, sp_prune_rules(sp_live(g), g, keep, target, score_tol),
                     [&] { return sp_prune_launch(g, keep, target, score_tol, removed, order, scores, status); });
}

int gpc_sparse_prune(gpc_sparse* g, int keep, const int32_t* target, double score_tol, int32_t* removed, int32_t* order, double* scores,
                     int32_t* status)
{
    if (int rc = sp_prune_rules(sp_live(g), g, keep, target, score_tol)) return sp_done(rc);
    GPC_HIP(g->ctx, hipSetDevice(g->ctx->device));
    const size_t P = (size_t)g->P, n_trace = P * (size_t)g->ld;
    GpcStaging st(g->ctx, "gpc_sparse_prune");
    const int32_t* d_target = target ? st.up(target, P) : nullptr;
    int32_t* d_rm = removed ? st.out<int32_t>(P) : nullptr;
    // the trace goes up first: the entries at and beyond removed[p] come back as the caller left them
    int32_t* d_order = order ? st.up(order, n_trace) : nullptr;
    double* d_scores = scores ? st.up(scores, n_trace) : nullptr;
    int32_t* d_st = status ? st.out<int32_t>(P) : nullptr;
    if (st.ok()) st.rc = gpc_sparse_prune_dev(g, keep, d_target, score_tol, d_rm, d_order, d_scores, d_st);
    st.down(removed, d_rm, P);
    st.down(order, d_order, n_trace);
    st.down(scores, d_scores, n_trace);
    st.down(status, d_st, P);
    return st.finish();
}

int gpc_sparse_prune_rd_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y, int keep,
                            const int32_t* target, double max_mse, const double* max_mse_p, int32_t* removed, int32_t* order,
                            double* scores, double* mse, double* mse0, double* mse_next, int32_t* status)
{
    SpBatch b{off, 0, n_total, x0, x1, y};
    return sp_locked(g, sp_prune_rd_rules(sp_live(g), g, b, keep, target, max_mse, max_mse_p, false), [&] {
        return sp_prune_rd_launch(g, off, n_total, x0, x1, y, keep, target, max_mse, max_mse_p, removed, order, scores, mse, mse0, mse_next, status);
    });
}

int gpc_sparse_prune_rd(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y, int keep,
                        const int32_t* target, double max_mse, const double* max_mse_p, int32_t* removed, int32_t* order, double* scores,
                        double* mse, double* mse0, double* mse_next, int32_t* status)
{
    SpBatch b{off, 0, 0, x0, x1, y};
    if (int rc = sp_prune_rd_rules(sp_live(g), g, b, keep, target, max_mse, max_mse_p, true)) return sp_done(rc);
    GPC_HIP(g->ctx, hipSetDevice(g->ctx->device));
    const size_t P = (size_t)g->P, N = (size_t)b.n_total, n_trace = P * (size_t)g->ld, n_y = N * (size_t)g->ny;
    GpcStaging st(g->ctx, "gpc_sparse_prune_rd");
    const int32_t* d_off = st.up(off, P + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N), *d_y = st.up(y, n_y);
    const int32_t* d_target = target ? st.up(target, P) : nullptr;
    const double* d_bound = max_mse_p ? st.up(max_mse_p, P) : nullptr;
    int32_t* d_rm = removed ? st.out<int32_t>(P) : nullptr;
    // the traces go up first: the entries at and beyond removed[p] come back as the caller left them
    int32_t* d_order = order ? st.up(order, n_trace) : nullptr;
    double* d_scores = scores ? st.up(scores, n_trace) : nullptr;
    double* d_mse = mse ? st.up(mse, n_trace) : nullptr;
    double* d_mse0 = mse0 ? st.out<double>(P) : nullptr;
    double* d_next = mse_next ? st.out<double>(P) : nullptr;
    int32_t* d_st = status ? st.out<int32_t>(P) : nullptr;
    if (st.ok())
        st.rc = gpc_sparse_prune_rd_dev(g, d_off, b.n_total, d_x0, d_x1, d_y, keep, d_target, max_mse, d_bound, d_rm, d_order, d_scores, d_mse,
                                        d_mse0, d_next, d_st);
    st.down(removed, d_rm, P);
    st.down(order, d_order, n_trace);
    st.down(scores, d_scores, n_trace);
    st.down(mse, d_mse, n_trace);
    st.down(mse0, d_mse0, P);
    st.down(mse_next, d_next, P);
    st.down(status, d_st, P);
    return st.finish();
}

int gpc_sparse_quantize_rd_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y,
                               int bits_min, int bits_max, double max_mse, const double* max_mse_p, int32_t* bits, uint16_t* q_alpha,
                               uint16_t* q_bv, float* range, double* mse0, double* mse_q, double* curve, int32_t* status)
{
    SpBatch b{off, 0, n_total, x0, x1, y};
    return sp_locked(g, sp_quantize_rd_rules(sp_live(g), g, b, bits_min, bits_max, max_mse, max_mse_p, false), [&] {
        return sp_quantize_rd_launch(g, off, n_total, x0, x1, y, bits_min, bits_max, max_mse, max_mse_p, bits, q_alpha, q_bv, range, mse0, mse_q,
                                     curve, status);
    });
}

int gpc_sparse_quantize_rd(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y, int bits_min, int bits_max,
                           double max_mse, const double* max_mse_p, int32_t* bits, uint16_t* q_alpha, uint16_t* q_bv, float* range,
                           double* mse0, double* mse_q, double* curve, int32_t* status)
{
    SpBatch b{off, 0, 0, x0, x1, y};
    if (int rc = sp_quantize_rd_rules(sp_live(g), g, b, bits_min, bits_max, max_mse, max_mse_p, true)) return sp_done(rc);
    GPC_HIP(g->ctx, hipSetDevice(g->ctx->device));
    const size_t P = (size_t)g->P, N = (size_t)b.n_total, ld = (size_t)g->ld, ny = (size_t)g->ny;
    const size_t n_y = N * ny, n_qa = P * ny * ld, n_qb = P * ld * 2, n_rng = P * (ny + 2) * 2, n_curve = P * 16;
    GpcStaging st(g->ctx, "gpc_sparse_quantize_rd");
    const int32_t* d_off = st.up(off, P + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N), *d_y = st.up(y, n_y);
    const double* d_bound = max_mse_p ? st.up(max_mse_p, P) : nullptr;
    int32_t* d_bits = bits ? st.out<int32_t>(P) : nullptr;
    // what the call may leave unwritten goes up first: the codes at and beyond the basis count, everything of an escaped patch, the
    // curve entries of the widths not evaluated come back as the caller left them
    uint16_t* d_qa = q_alpha ? st.up(q_alpha, n_qa) : nullptr;
    uint16_t* d_qb = q_bv ? st.up(q_bv, n_qb) : nullptr;
    float* d_rng = range ? st.up(range, n_rng) : nullptr;
    double* d_curve = curve ? st.up(curve, n_curve) : nullptr;
    double* d_mse0 = mse0 ? st.out<double>(P) : nullptr;
    double* d_mseq = mse_q ? st.out<double>(P) : nullptr;
    int32_t* d_st = status ? st.out<int32_t>(P) : nullptr;
    if (st.ok())
        st.rc = gpc_sparse_quantize_rd_dev(g, d_off, b.n_total, d_x0, d_x1, d_y, bits_min, bits_max, max_mse, d_bound, d_bits, d_qa, d_qb, d_rng,
                                           d_mse0, d_mseq, d_curve, d_st);
    st.down(bits, d_bits, P);
    st.down(q_alpha, d_qa, n_qa);
    st.down(q_bv, d_qb, n_qb);
    st.down(range, d_rng, n_rng);
    st.down(curve, d_curve, n_curve);
    st.down(mse0, d_mse0, P);
    st.down(mse_q, d_mseq, P);
    st.down(status, d_st, P);
    return st.finish();
}

int gpc_sparse_dequantize_dev(gpc_sparse* g, const int32_t* bv_count, const int32_t* bits, const uint16_t* q_alpha, const uint16_t* q_bv,
                              const float* range)
{
    return sp_locked(g, sp_dequantize_rules(sp_live(g), g, bv_count, bits, q_alpha, q_bv, range, false),
                     [&] { return sp_dequantize_launch(g, bv_count, bits, q_alpha, q_bv, range); });
}

int gpc_sparse_dequantize(gpc_sparse* g, const int32_t* bv_count, const int32_t* bits, const uint16_t* q_alpha, const uint16_t* q_bv,
                          const float* range)
{
    if (int rc = sp_dequantize_rules(sp_live(g), g, bv_count, bits, q_alpha, q_bv, range, true)) return sp_done(rc);
    GPC_HIP(g->ctx, hipSetDevice(g->ctx->device));
    const size_t P = (size_t)g->P, ld = (size_t)g->ld, ny = (size_t)g->ny;
    GpcStaging st(g->ctx, "gpc_sparse_dequantize");
    const int32_t *d_b = st.up(bv_count, P), *d_w = st.up(bits, P);
    const uint16_t *d_qa = st.up(q_alpha, P * ny * ld), *d_qb = st.up(q_bv, P * ld * 2);
    const float* d_rng = st.up(range, P * (ny + 2) * 2);
    if (st.ok()) st.rc = gpc_sparse_dequantize_dev(g, d_b, d_w, d_qa, d_qb, d_rng);
    return st.finish();
}

int gpc_sparse_predict_dev(gpc_sparse* g, int m, const double* xs0, const double* xs1, double* f_star, double* sigma,
                           int conf, int32_t* status)
{
    // (mean only: a patch is a few hundred kernel evaluations, more resident blocks hide their latency)
    return sp_locked(g, sp_predict_rules(sp_live(g), g, m, xs0, xs1, f_star),
                     [&] { return sp_predict_launch(g, m, nullptr, 0, xs0, xs1, f_star, sigma, conf, status, sigma ? 4 : 8); });
}

int gpc_sparse_predict(gpc_sparse* g, int m, const double* xs0, const double* xs1, double* f_star, double* sigma,
                       int conf, int32_t* status)
{
    if (int rc = sp_predict_rules(sp_live(g), g, m, xs0, xs1, f_star)) return sp_done(rc);
    GPC_HIP(g->ctx, hipSetDevice(g->ctx->device));
    const size_t P = (size_t)g->P, n_xs = (size_t)m, n_s = P * n_xs, n_f = n_s * (size_t)g->ny;
    GpcStaging st(g->ctx, "gpc_sparse_predict");
    const double *d_xs0 = st.up(xs0, n_xs), *d_xs1 = st.up(xs1, n_xs);
    double *d_f = st.out<double>(n_f), *d_s = sigma ? st.out<double>(n_s) : nullptr;
    int32_t* d_st = st.out<int32_t>(P);
    if (st.ok()) st.rc = gpc_sparse_predict_dev(g, m, d_xs0, d_xs1, d_f, d_s, conf, d_st);
    st.down(f_star, d_f, n_f);
    st.down(sigma, d_s, n_s);
    st.down(status, d_st, P);
    return st.finish();
}

// predict_measurements on every patch's OWN point set (ragged, like the add call's batch): the reference's per-patch training-set
// RMS block (/root/reference/src/gp_compressor.cpp:303-315) calls gps[i].predict_measurements(f, X_i, sigma) exactly so.
int gpc_sparse_predict_points_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1,
                                  double* f, double* sigma, int conf, int32_t* status)
{
    SpBatch b{off, 0, n_total, x0, x1, f};
    return sp_locked(g, sp_predict_points_rules(sp_live(g), g, b, false),
                     [&] { return sp_predict_launch(g, 0, off, n_total, x0, x1, f, sigma, conf, status, 4); });
}

int gpc_sparse_predict_points(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, double* f, double* sigma,
                              int conf, int32_t* status)
{
    SpBatch b{off, 0, 0, x0, x1, f};
    if (int rc = sp_predict_points_rules(sp_live(g), g, b, true)) return sp_done(rc);
    GPC_HIP(g->ctx, hipSetDevice(g->ctx->device));
    const size_t P = (size_t)g->P, N = (size_t)b.n_total, n_f = N * (size_t)g->ny;
    GpcStaging st(g->ctx, "gpc_sparse_predict_points");
    const int32_t* d_off = st.up(off, P + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N);
    double *d_f = st.out<double>(n_f), *d_s = sigma ? st.out<double>(N) : nullptr;
    int32_t* d_st = st.out<int32_t>(P);
    if (st.ok()) st.rc = gpc_sparse_predict_points_dev(g, d_off, b.n_total, d_x0, d_x1, d_f, d_s, conf, d_st);
    st.down(f, d_f, n_f);
    st.down(sigma, d_s, N);
    st.down(status, d_st, P);
    return st.finish();
}

// predict_measurements at (patch, point) pairs in any order: bucketed on the device, then the kernels of the entry above (sparse_scatter.hip)
int gpc_sparse_predict_scattered_dev(gpc_sparse* g, int n, const int32_t* patch, const double* x0, const double* x1, int stride,
                                     double* f, double* sigma, int conf, int32_t* status)
{
    return sp_locked(g, sp_scattered_rules(sp_live(g), g, n, patch, x0, x1, stride, status),
                     [&] { return sp_scatter_launch(g, n, patch, x0, x1, stride, f, sigma, conf, status); });
}

int gpc_sparse_predict_scattered(gpc_sparse* g, int n, const int32_t* patch, const double* x0, const double* x1, int stride, double* f,
                                 double* sigma, int conf, int32_t* status)
{
    if (int rc = sp_scattered_rules(sp_live(g), g, n, patch, x0, x1, stride, status)) return sp_done(rc);
    GPC_HIP(g->ctx, hipSetDevice(g->ctx->device));
    const size_t N = (size_t)n, P = (size_t)g->P, n_f = N * (size_t)g->ny;
    GpcStaging st(g->ctx, "gpc_sparse_predict_scattered");
    const int32_t* d_patch = st.up(patch, N);
    // entry i reads x[i * stride]: (n - 1) * stride + 1 doubles each; interleaved coordinates (x1 inside the first stride of x0) go up once
    const size_t span = N ? (N - 1) * (size_t)stride + 1 : 0;
    const uintptr_t a0 = (uintptr_t)x0, a1 = (uintptr_t)x1;
    const size_t gap = (N && a1 >= a0 && (a1 - a0) % sizeof(double) == 0) ? (size_t)(a1 - a0) / sizeof(double) : (size_t)stride;
    const double *d_x0, *d_x1;
    if (gap < (size_t)stride) {
        d_x0 = st.up(x0, span + gap);
        d_x1 = d_x0 ? d_x0 + gap : nullptr;
    } else {
        d_x0 = st.up(x0, span);
        d_x1 = st.up(x1, span);
    }
    double *d_f = f ? st.out<double>(n_f) : nullptr, *d_s = sigma ? st.out<double>(N) : nullptr;
    int32_t* d_st = status ? st.out<int32_t>(P) : nullptr;
    if (st.ok()) st.rc = gpc_sparse_predict_scattered_dev(g, n, d_patch, d_x0, d_x1, stride, d_f, d_s, conf, d_st);
    st.down(f, d_f, n_f);
    st.down(sigma, d_s, N);
    st.down(status, d_st, P);
    return st.finish();
}

int gpc_sparse_likelihood_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1,
                              const double* y, double* dX, double* l)
{
    SpBatch b{off, 0, n_total, x0, x1, y};
    return sp_locked(g, sp_likelihood_rules(sp_live(g), g, b, dX, l, false),
                     [&] { return sp_likelihood_launch(g, off, n_total, x0, x1, y, dX, l, nullptr); });
}

int gpc_sparse_likelihood(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y,
                          double* dX, double* l)
{
    SpBatch b{off, 0, 0, x0, x1, y};
    if (int rc = sp_likelihood_rules(sp_live(g), g, b, dX, l, true)) return sp_done(rc);
    GPC_HIP(g->ctx, hipSetDevice(g->ctx->device));
    const size_t P = (size_t)g->P, N = (size_t)b.n_total, n_y = N * (size_t)g->ny, n_dX = N * 3;
    GpcStaging st(g->ctx, "gpc_sparse_likelihood");
    const int32_t* d_off = st.up(off, P + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N), *d_y = st.up(y, n_y);
    double *d_dX = dX ? st.out<double>(n_dX) : nullptr, *d_l = l ? st.out<double>(N) : nullptr;
    if (st.ok()) st.rc = gpc_sparse_likelihood_dev(g, d_off, b.n_total, d_x0, d_x1, d_y, d_dX, d_l);
    st.down(dX, d_dX, n_dX);
    st.down(l, d_l, N);
    return st.finish();
}

int gpc_sparse_train_sigmaf_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y,
                                double step, int max_counter, double* p0, int32_t* iters, double* ls, double* delta)
{
    SpBatch b{off, 0, n_total, x0, x1, y};
    return sp_locked(g, sp_train_rules(sp_live(g), g, b, step, max_counter, p0, iters, ls, delta, false), [&] {
        gpc_ctx* ctx = g->ctx;
        int rc = gpc_ws_reserve(ctx, sizeof(double) * 3 * (size_t)(n_total > 0 ? n_total : 1));
        if (rc != GPC_OK) return rc;
        double* raw = static_cast<double*>(ctx->ws);
        if (n_total > 0) {
            rc = sp_likelihood_launch(g, off, n_total, x0, x1, y, nullptr, nullptr, raw);
            if (rc != GPC_OK) return rc;
        }
        return sp_train_launch(g, off, y, raw, step, max_counter, p0, iters, ls, delta);
    });
}

int gpc_sparse_train_sigmaf(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y, double step,
                            int max_counter, double* p0, int32_t* iters, double* ls, double* delta)
{
    SpBatch b{off, 0, 0, x0, x1, y};
    if (int rc = sp_train_rules(sp_live(g), g, b, step, max_counter, p0, iters, ls, delta, true)) return sp_done(rc);
    GPC_HIP(g->ctx, hipSetDevice(g->ctx->device));
    // (y: one plane, whatever the object's ny -- the _dev twin refuses every other object)
    const size_t P = (size_t)g->P, N = (size_t)b.n_total, n_y = N, n_ls = P * ((size_t)max_counter + 2), n_delta = 2 * P;
    GpcStaging st(g->ctx, "gpc_sparse_train_sigmaf");
    const int32_t* d_off = st.up(off, P + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N), *d_y = st.up(y, n_y);
    double *d_p0 = st.out<double>(P), *d_ls = st.out<double>(n_ls, true), *d_de = st.out<double>(n_delta);
    int32_t* d_it = st.out<int32_t>(P);
    if (st.ok()) st.rc = gpc_sparse_train_sigmaf_dev(g, d_off, b.n_total, d_x0, d_x1, d_y, step, max_counter, d_p0, d_it, d_ls, d_de);
    st.down(p0, d_p0, P);
    st.down(iters, d_it, P);
    st.down(ls, d_ls, n_ls);
    st.down(delta, d_de, n_delta);
    return st.finish();
}

}  // extern "C"
