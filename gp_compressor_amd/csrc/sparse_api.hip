// sparse_api.hip -- the gpc_sparse_* entry points of the C-ABI (include/gpc.h): the object, the _dev entries (argument checks,
// locking, then the launcher beside the kernels: sparse.hip, sparse_rate.hip, sparse_predict.hip) and their host-pointer twins.
#include <new>

#include "sparse_internal.h"

static void sp_free_all(gpc_sparse* g)
{
    for (void* p : {(void*)g->alpha, (void*)g->C, (void*)g->Q, (void*)g->BV, (void*)g->b, (void*)g->count, (void*)g->stat, (void*)g->done_it, (void*)g->list})
        if (p) (void)hipFree(p);
    delete g;
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

extern "C" {

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
    gpc_sparse* g = new (std::nothrow) gpc_sparse();
    if (!g) return GPC_ENOMEM;
    g->ctx = ctx; g->prm = *params; g->P = P; g->ny = ny;
    // capacity + 1 rows (a full update holds capacity + 1 basis vectors until the deletion that follows it), rounded up to 16
    // doubles = 128 B: every column of C and Q then starts on a cache line, and a wave's 64-row segment is exactly 4 lines.
    // With ld = 201 the segments straddled lines -- 5 fetched per 4 used, re-fetched from HBM by the next row trip -- and
    // the add path, which is bound by exactly this stream, read 27 % more than it consumed (profiles/r02_summary.json).
    g->ld = params->capacity == -1 ? GPC_MAX_BV : ((params->capacity + 1 + 15) & ~15);
    g->alpha = g->C = g->Q = g->BV = nullptr;
    g->b = g->count = g->stat = nullptr;
    g->done_it = nullptr;
    g->list = nullptr;
    g->trace = nullptr;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t ld = (size_t)g->ld, Pn = (size_t)(P > 0 ? P : 1);
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(&g->alpha, 8 * Pn * ny * ld);
    if (e == hipSuccess) e = hipMalloc(&g->C, 8 * Pn * ld * ld);
    if (e == hipSuccess) e = hipMalloc(&g->Q, 8 * Pn * ld * ld);
    if (e == hipSuccess) e = hipMalloc(&g->BV, 8 * Pn * ld * 2);
    if (e == hipSuccess) e = hipMalloc(&g->b, 4 * Pn);
    if (e == hipSuccess) e = hipMalloc(&g->count, 4 * Pn);
    if (e == hipSuccess) e = hipMalloc(&g->stat, 4 * Pn);
    if (e == hipSuccess) e = hipMalloc(&g->done_it, 4 * Pn);
    if (e == hipSuccess) e = hipMalloc(&g->list, 4 * (3 * Pn + 12));      // three work lists of P entries, then their 3 x 4 counters
    if (e == hipSuccess) e = hipMemsetAsync(g->b, 0, 4 * Pn, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(g->count, 0, 4 * Pn, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(g->stat, 0, 4 * Pn, ctx->stream);
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
    if (!old) return GPC_EINVAL;
    gpc_ctx* ctx = old->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
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
    void* d_map = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        hipStream_t st = ctx->stream;
        e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipMalloc(&d_map, 4 * (size_t)P);
        if (e == hipSuccess) e = hipMemcpyAsync(d_map, old_to_new, 4 * (size_t)P, hipMemcpyHostToDevice, st);
        // the patches no old one moves into: a zero state, not what the allocation happened to hold (gpc_sparse_get_state reads it back)
        const size_t ldz = (size_t)g->ld, Pn = (size_t)P_new;
        if (e == hipSuccess) e = hipMemsetAsync(g->alpha, 0, 8 * Pn * (size_t)g->ny * ldz, st);
        if (e == hipSuccess) e = hipMemsetAsync(g->C, 0, 8 * Pn * ldz * ldz, st);
        if (e == hipSuccess) e = hipMemsetAsync(g->Q, 0, 8 * Pn * ldz * ldz, st);
        if (e == hipSuccess) e = hipMemsetAsync(g->BV, 0, 8 * Pn * ldz * 2, st);
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
        const int rc = gpc_fail(ctx, e == hipErrorOutOfMemory ? GPC_ENOMEM : GPC_EHIP, "gpc_sparse_remap: %s", hipGetErrorString(e));
        gpc_sparse_destroy(g);
        return rc;
    }
    *out = g;
    return GPC_OK;
}

int gpc_sparse_set_trace(gpc_sparse* g, uint8_t* trace_dev)
{
    if (!g) return GPC_EINVAL;
    if (g->ctx->dead.load()) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(g->ctx->mu);
    g->trace = trace_dev;
    return GPC_OK;
}

int gpc_sparse_reset(gpc_sparse* g)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t Pn = (size_t)(g->P > 0 ? g->P : 1);
    GPC_HIP(ctx, hipMemsetAsync(g->b, 0, 4 * Pn, ctx->stream));
    GPC_HIP(ctx, hipMemsetAsync(g->count, 0, 4 * Pn, ctx->stream));
    GPC_HIP(ctx, hipMemsetAsync(g->stat, 0, 4 * Pn, ctx->stream));
    return GPC_OK;
}


int gpc_sparse_add_dev(gpc_sparse* g, const int32_t* off, int n_max, int n_total, const double* x0, const double* x1,
                       const double* y, const int32_t* perm, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (g->P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (n_total < 0 || n_max < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (n_total > 0 && (!x0 || !x1 || !y)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/y is NULL");
    if (g->P == 0) return GPC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    return sp_add_launch(g, off, n_total, x0, x1, y, perm, status);
}

// what both prune entries check (include/gpc.h)
static int sp_prune_check(gpc_ctx* ctx, int keep, const int32_t* target, double score_tol)
{
    if (!target && keep < 1) return gpc_fail(ctx, GPC_EINVAL, "keep must be >= 1 when target is NULL, got %d", keep);
    if (!(score_tol >= 0.0)) return gpc_fail(ctx, GPC_EINVAL, "score_tol must be >= 0 (+inf allowed), got %g", score_tol);
    return GPC_OK;
}

int gpc_sparse_prune_dev(gpc_sparse* g, int keep, const int32_t* target, double score_tol, int32_t* removed, int32_t* order,
                         double* scores, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (int rc = sp_prune_check(ctx, keep, target, score_tol)) return rc;
    if (g->P == 0) return GPC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    return sp_prune_launch(g, keep, target, score_tol, removed, order, scores, status);
}

// what both distortion-bounded prune entries check before they look at the batch (include/gpc.h)
static int sp_prune_rd_check(gpc_sparse* g, int keep, const int32_t* target, double max_mse, const double* max_mse_p)
{
    gpc_ctx* ctx = g->ctx;
    if (g->prm.noise_model != GPC_NOISE_GAUSSIAN)
        return gpc_fail(ctx, GPC_EINVAL, "prune_rd: the error is taken against the Gaussian read-out (noise_model 0), got %d", g->prm.noise_model);
    if (!target && keep < 1) return gpc_fail(ctx, GPC_EINVAL, "keep must be >= 1 when target is NULL, got %d", keep);
    if (!max_mse_p && !(max_mse >= 0.0)) return gpc_fail(ctx, GPC_EINVAL, "max_mse must be >= 0 (+inf allowed), got %g", max_mse);
    return GPC_OK;
}

int gpc_sparse_prune_rd_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y, int keep,
                            const int32_t* target, double max_mse, const double* max_mse_p, int32_t* removed, int32_t* order,
                            double* scores, double* mse, double* mse0, double* mse_next, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (int rc = sp_prune_rd_check(g, keep, target, max_mse, max_mse_p)) return rc;
    if (n_total < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (g->P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (n_total > 0 && (!x0 || !x1 || !y)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/y is NULL");
    if (g->P == 0) return GPC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    return sp_prune_rd_launch(g, off, n_total, x0, x1, y, keep, target, max_mse, max_mse_p, removed, order, scores, mse, mse0, mse_next,
                              status);
}

// what both quantise entries check before they look at the batch (include/gpc.h)
static int sp_quantize_rd_check(gpc_sparse* g, int bits_min, int bits_max, double max_mse, const double* max_mse_p)
{
    gpc_ctx* ctx = g->ctx;
    if (g->prm.noise_model != GPC_NOISE_GAUSSIAN)
        return gpc_fail(ctx, GPC_EINVAL, "quantize_rd: the error is taken against the Gaussian read-out (noise_model 0), got %d", g->prm.noise_model);
    if (bits_min < 1 || bits_max > 16 || bits_min > bits_max)
        return gpc_fail(ctx, GPC_EINVAL, "quantize_rd: widths must satisfy 1 <= bits_min <= bits_max <= 16, got %d .. %d", bits_min, bits_max);
    if (!max_mse_p && !(max_mse >= 0.0)) return gpc_fail(ctx, GPC_EINVAL, "max_mse must be >= 0 (+inf allowed), got %g", max_mse);
    return GPC_OK;
}

int gpc_sparse_quantize_rd_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y,
                               int bits_min, int bits_max, double max_mse, const double* max_mse_p, int32_t* bits, uint16_t* q_alpha,
                               uint16_t* q_bv, float* range, double* mse0, double* mse_q, double* curve, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (int rc = sp_quantize_rd_check(g, bits_min, bits_max, max_mse, max_mse_p)) return rc;
    if (n_total < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (g->P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (n_total > 0 && (!x0 || !x1 || !y)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/y is NULL");
    if (g->P == 0) return GPC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    return sp_quantize_rd_launch(g, off, n_total, x0, x1, y, bits_min, bits_max, max_mse, max_mse_p, bits, q_alpha, q_bv, range, mse0, mse_q,
                                 curve, status);
}

int gpc_sparse_dequantize_dev(gpc_sparse* g, const int32_t* bv_count, const int32_t* bits, const uint16_t* q_alpha, const uint16_t* q_bv,
                              const float* range)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (g->P == 0) return GPC_OK;
    if (!bv_count || !bits || !q_alpha || !q_bv || !range) return gpc_fail(ctx, GPC_EINVAL, "bv_count/bits/q_alpha/q_bv/range is NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    return sp_dequantize_launch(g, bv_count, bits, q_alpha, q_bv, range);
}

int gpc_sparse_predict_dev(gpc_sparse* g, int m, const double* xs0, const double* xs1, double* f_star, double* sigma,
                           int conf, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (m < 0) return gpc_fail(ctx, GPC_EINVAL, "negative m");
    if (m > 0 && (!xs0 || !xs1 || !f_star)) return gpc_fail(ctx, GPC_EINVAL, "xs0/xs1/f_star is NULL");
    if (g->P == 0 || m == 0) return GPC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    // (mean only: a patch is a few hundred kernel evaluations, more resident blocks hide their latency)
    return sp_predict_launch(g, m, nullptr, 0, xs0, xs1, f_star, sigma, conf, status, sigma ? 4 : 8);
}

// predict_measurements on every patch's OWN point set (ragged, like the add call's batch): the reference's per-patch training-set
// RMS block (/root/reference/src/gp_compressor.cpp:303-315) calls gps[i].predict_measurements(f, X_i, sigma) exactly so.
int gpc_sparse_predict_points_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1,
                                  double* f, double* sigma, int conf, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (g->P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (n_total < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (n_total > 0 && (!x0 || !x1 || !f)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/f is NULL");
    if (g->P == 0) return GPC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    return sp_predict_launch(g, 0, off, n_total, x0, x1, f, sigma, conf, status, 4);
}

// what both scattered entries check (include/gpc.h)
static int sp_scattered_check(gpc_ctx* ctx, int n, const int32_t* patch, const double* x0, const double* x1, int stride)
{
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (stride < 1) return gpc_fail(ctx, GPC_EINVAL, "stride must be >= 1, got %d", stride);
    if (n > 0 && (!patch || !x0 || !x1)) return gpc_fail(ctx, GPC_EINVAL, "patch/x0/x1 is NULL");
    return GPC_OK;
}

// predict_measurements at (patch, point) pairs in any order: bucketed on the device, then the kernels of the entry above (sparse_scatter.hip)
int gpc_sparse_predict_scattered_dev(gpc_sparse* g, int n, const int32_t* patch, const double* x0, const double* x1, int stride,
                                     double* f, double* sigma, int conf, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (int rc = sp_scattered_check(ctx, n, patch, x0, x1, stride)) return rc;
    if (n == 0 && (!status || g->P == 0)) return GPC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    return sp_scatter_launch(g, n, patch, x0, x1, stride, f, sigma, conf, status);
}

int gpc_sparse_likelihood_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1,
                              const double* y, double* dX, double* l)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (g->P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (n_total < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (n_total > 0 && (!x0 || !x1 || !y)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/y is NULL");
    if (g->prm.noise_model != 0) return gpc_fail(ctx, GPC_EINVAL, "likelihoods are defined for the Gaussian noise model");
    if (g->P == 0 || n_total == 0 || (!dX && !l)) return GPC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    return sp_likelihood_launch(g, off, n_total, x0, x1, y, dX, l, nullptr);
}

#define GPC_TRAIN_MAX_COUNTER 10000

int gpc_sparse_train_sigmaf_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y,
                                double step, int max_counter, double* p0, int32_t* iters, double* ls, double* delta)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (g->ny != 1) return gpc_fail(ctx, GPC_EINVAL, "train_parameters exists for sparse_gp (ny == 1) only");
    if (g->prm.noise_model != 0) return gpc_fail(ctx, GPC_EINVAL, "likelihoods are defined for the Gaussian noise model");
    if (g->P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (n_total < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (max_counter < 0 || max_counter > GPC_TRAIN_MAX_COUNTER) return gpc_fail(ctx, GPC_EINVAL, "max_counter must be in [0, %d]", GPC_TRAIN_MAX_COUNTER);
    if (!(step == step)) return gpc_fail(ctx, GPC_EINVAL, "step is NaN");
    if (n_total > 0 && (!x0 || !x1 || !y)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/y is NULL");
    if (g->P > 0 && (!p0 || !iters || !ls || !delta)) return gpc_fail(ctx, GPC_EINVAL, "p0/iters/ls/delta is NULL");
    if (g->P == 0) return GPC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    int rc = gpc_ws_reserve(ctx, sizeof(double) * 3 * (size_t)(n_total > 0 ? n_total : 1));
    if (rc != GPC_OK) return rc;
    double* raw = static_cast<double*>(ctx->ws);
    if (n_total > 0) {
        rc = sp_likelihood_launch(g, off, n_total, x0, x1, y, nullptr, nullptr, raw);
        if (rc != GPC_OK) return rc;
    }
    return sp_train_launch(g, off, y, raw, step, max_counter, p0, iters, ls, delta);
}

// ---- host-pointer twins: validate, stage (GpcStaging, gpc_internal.h), the _dev entry, download

int gpc_sparse_train_sigmaf(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y, double step,
                            int max_counter, double* p0, int32_t* iters, double* ls, double* delta)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    const int P = g->P;
    if (P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (P == 0) return GPC_OK;
    if (int rc = gpc_check_host_off(ctx, P, off, nullptr, nullptr)) return rc;
    if (max_counter < 0 || max_counter > GPC_TRAIN_MAX_COUNTER) return gpc_fail(ctx, GPC_EINVAL, "max_counter must be in [0, %d]", GPC_TRAIN_MAX_COUNTER);
    const size_t N = (size_t)off[P], Pz = (size_t)P, W = (size_t)max_counter + 2;
    if (N > 0 && (!x0 || !x1 || !y)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/y is NULL");
    if (!p0 || !iters || !ls || !delta) return gpc_fail(ctx, GPC_EINVAL, "p0/iters/ls/delta is NULL");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_sparse_train_sigmaf");
    const int32_t* d_off = st.up(off, Pz + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N), *d_y = st.up(y, N);
    double *d_p0 = st.out<double>(Pz), *d_ls = st.out<double>(Pz * W, true), *d_de = st.out<double>(2 * Pz);
    int32_t* d_it = st.out<int32_t>(Pz);
    if (st.ok()) st.rc = gpc_sparse_train_sigmaf_dev(g, d_off, (int)N, d_x0, d_x1, d_y, step, max_counter, d_p0, d_it, d_ls, d_de);
    st.down(p0, d_p0, Pz);
    st.down(iters, d_it, Pz);
    st.down(ls, d_ls, Pz * W);
    st.down(delta, d_de, 2 * Pz);
    return st.finish();
}

int gpc_sparse_likelihood(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y,
                          double* dX, double* l)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    const int P = g->P;
    if (P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (P == 0) return GPC_OK;
    if (int rc = gpc_check_host_off(ctx, P, off, nullptr, nullptr)) return rc;
    const size_t N = (size_t)off[P], ny = (size_t)g->ny;
    if (N > 0 && (!x0 || !x1 || !y)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/y is NULL");
    if (N == 0 || (!dX && !l)) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_sparse_likelihood");
    const int32_t* d_off = st.up(off, (size_t)P + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N), *d_y = st.up(y, N * ny);
    double *d_dX = dX ? st.out<double>(N * 3) : nullptr, *d_l = l ? st.out<double>(N) : nullptr;
    if (st.ok()) st.rc = gpc_sparse_likelihood_dev(g, d_off, (int)N, d_x0, d_x1, d_y, d_dX, d_l);
    st.down(dX, d_dX, N * 3);
    st.down(l, d_l, N);
    return st.finish();
}

int gpc_sparse_add(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y,
                   const int32_t* perm, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    const int P = g->P;
    if (P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (P == 0) return GPC_OK;
    int n_max = 0;
    if (int rc = gpc_check_host_off(ctx, P, off, &n_max, nullptr)) return rc;
    const size_t N = (size_t)off[P], ny = (size_t)g->ny;
    if (N > 0 && (!x0 || !x1 || !y)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/y is NULL");
    if (perm)
        for (int i = 0; i < P; ++i)
            for (int k = off[i]; k < off[i + 1]; ++k)
                if (perm[k] < 0 || perm[k] >= off[i + 1] - off[i])
                    return gpc_fail(ctx, GPC_EINVAL, "perm[%d] = %d outside patch %d", k, perm[k], i);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_sparse_add");
    const int32_t* d_off = st.up(off, (size_t)P + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N), *d_y = st.up(y, N * ny);
    const int32_t* d_perm = perm ? st.up(perm, N) : nullptr;
    int32_t* d_st = st.out<int32_t>((size_t)P);
    if (st.ok()) st.rc = gpc_sparse_add_dev(g, d_off, n_max, (int)N, d_x0, d_x1, d_y, d_perm, d_st);
    st.down(status, d_st, (size_t)P);
    return st.finish();
}

int gpc_sparse_prune(gpc_sparse* g, int keep, const int32_t* target, double score_tol, int32_t* removed, int32_t* order, double* scores,
                     int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (int rc = sp_prune_check(ctx, keep, target, score_tol)) return rc;
    const size_t P = (size_t)g->P, W = P * (size_t)g->ld;
    if (P == 0) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_sparse_prune");
    const int32_t* d_target = target ? st.up(target, P) : nullptr;
    int32_t* d_rm = removed ? st.out<int32_t>(P) : nullptr;
    // the trace goes up first: the entries at and beyond removed[p] come back as the caller left them
    int32_t* d_order = order ? st.up(order, W) : nullptr;
    double* d_scores = scores ? st.up(scores, W) : nullptr;
    int32_t* d_st = status ? st.out<int32_t>(P) : nullptr;
    if (st.ok()) st.rc = gpc_sparse_prune_dev(g, keep, d_target, score_tol, d_rm, d_order, d_scores, d_st);
    st.down(removed, d_rm, P);
    st.down(order, d_order, W);
    st.down(scores, d_scores, W);
    st.down(status, d_st, P);
    return st.finish();
}

int gpc_sparse_prune_rd(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y, int keep,
                        const int32_t* target, double max_mse, const double* max_mse_p, int32_t* removed, int32_t* order, double* scores,
                        double* mse, double* mse0, double* mse_next, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (int rc = sp_prune_rd_check(g, keep, target, max_mse, max_mse_p)) return rc;
    const size_t P = (size_t)g->P, W = P * (size_t)g->ld, ny = (size_t)g->ny;
    if (P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (P == 0) return GPC_OK;
    if (int rc = gpc_check_host_off(ctx, (int)P, off, nullptr, nullptr)) return rc;
    const size_t N = (size_t)off[P];
    if (N > 0 && (!x0 || !x1 || !y)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/y is NULL");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_sparse_prune_rd");
    const int32_t* d_off = st.up(off, P + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N), *d_y = st.up(y, N * ny);
    const int32_t* d_target = target ? st.up(target, P) : nullptr;
    const double* d_bound = max_mse_p ? st.up(max_mse_p, P) : nullptr;
    int32_t* d_rm = removed ? st.out<int32_t>(P) : nullptr;
    // the traces go up first: the entries at and beyond removed[p] come back as the caller left them
    int32_t* d_order = order ? st.up(order, W) : nullptr;
    double* d_scores = scores ? st.up(scores, W) : nullptr;
    double* d_mse = mse ? st.up(mse, W) : nullptr;
    double* d_mse0 = mse0 ? st.out<double>(P) : nullptr;
    double* d_next = mse_next ? st.out<double>(P) : nullptr;
    int32_t* d_st = status ? st.out<int32_t>(P) : nullptr;
    if (st.ok())
        st.rc = gpc_sparse_prune_rd_dev(g, d_off, (int)N, d_x0, d_x1, d_y, keep, d_target, max_mse, d_bound, d_rm, d_order, d_scores, d_mse,
                                        d_mse0, d_next, d_st);
    st.down(removed, d_rm, P);
    st.down(order, d_order, W);
    st.down(scores, d_scores, W);
    st.down(mse, d_mse, W);
    st.down(mse0, d_mse0, P);
    st.down(mse_next, d_next, P);
    st.down(status, d_st, P);
    return st.finish();
}

int gpc_sparse_quantize_rd(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y, int bits_min, int bits_max,
                           double max_mse, const double* max_mse_p, int32_t* bits, uint16_t* q_alpha, uint16_t* q_bv, float* range,
                           double* mse0, double* mse_q, double* curve, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (int rc = sp_quantize_rd_check(g, bits_min, bits_max, max_mse, max_mse_p)) return rc;
    const size_t P = (size_t)g->P, ld = (size_t)g->ld, ny = (size_t)g->ny;
    if (P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (P == 0) return GPC_OK;
    if (int rc = gpc_check_host_off(ctx, (int)P, off, nullptr, nullptr)) return rc;
    const size_t N = (size_t)off[P];
    if (N > 0 && (!x0 || !x1 || !y)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/y is NULL");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_sparse_quantize_rd");
    const int32_t* d_off = st.up(off, P + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N), *d_y = st.up(y, N * ny);
    const double* d_bound = max_mse_p ? st.up(max_mse_p, P) : nullptr;
    int32_t* d_bits = bits ? st.out<int32_t>(P) : nullptr;
    // what the call may leave unwritten goes up first: the codes at and beyond the basis count, everything of an escaped patch, the
    // curve entries of the widths not evaluated come back as the caller left them
    uint16_t* d_qa = q_alpha ? st.up(q_alpha, P * ny * ld) : nullptr;
    uint16_t* d_qb = q_bv ? st.up(q_bv, P * ld * 2) : nullptr;
    float* d_rng = range ? st.up(range, P * (ny + 2) * 2) : nullptr;
    double* d_curve = curve ? st.up(curve, P * 16) : nullptr;
    double* d_mse0 = mse0 ? st.out<double>(P) : nullptr;
    double* d_mseq = mse_q ? st.out<double>(P) : nullptr;
    int32_t* d_st = status ? st.out<int32_t>(P) : nullptr;
    if (st.ok())
        st.rc = gpc_sparse_quantize_rd_dev(g, d_off, (int)N, d_x0, d_x1, d_y, bits_min, bits_max, max_mse, d_bound, d_bits, d_qa, d_qb, d_rng,
                                           d_mse0, d_mseq, d_curve, d_st);
    st.down(bits, d_bits, P);
    st.down(q_alpha, d_qa, P * ny * ld);
    st.down(q_bv, d_qb, P * ld * 2);
    st.down(range, d_rng, P * (ny + 2) * 2);
    st.down(curve, d_curve, P * 16);
    st.down(mse0, d_mse0, P);
    st.down(mse_q, d_mseq, P);
    st.down(status, d_st, P);
    return st.finish();
}

int gpc_sparse_dequantize(gpc_sparse* g, const int32_t* bv_count, const int32_t* bits, const uint16_t* q_alpha, const uint16_t* q_bv,
                          const float* range)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    const size_t P = (size_t)g->P, ld = (size_t)g->ld, ny = (size_t)g->ny;
    if (P == 0) return GPC_OK;
    if (!bv_count || !bits || !q_alpha || !q_bv || !range) return gpc_fail(ctx, GPC_EINVAL, "bv_count/bits/q_alpha/q_bv/range is NULL");
    for (size_t i = 0; i < P; ++i) {
        if (bits[i] < 0 || bits[i] > 16) return gpc_fail(ctx, GPC_EINVAL, "bits[%d] = %d outside [0, 16]", (int)i, bits[i]);
        if (bv_count[i] < 0 || bv_count[i] > g->ld)
            return gpc_fail(ctx, GPC_EINVAL, "bv_count[%d] = %d outside [0, %d]", (int)i, bv_count[i], g->ld);
    }
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_sparse_dequantize");
    const int32_t *d_b = st.up(bv_count, P), *d_w = st.up(bits, P);
    const uint16_t *d_qa = st.up(q_alpha, P * ny * ld), *d_qb = st.up(q_bv, P * ld * 2);
    const float* d_rng = st.up(range, P * (ny + 2) * 2);
    if (st.ok()) st.rc = gpc_sparse_dequantize_dev(g, d_b, d_w, d_qa, d_qb, d_rng);
    return st.finish();
}

int gpc_sparse_predict(gpc_sparse* g, int m, const double* xs0, const double* xs1, double* f_star, double* sigma,
                       int conf, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (m < 0) return gpc_fail(ctx, GPC_EINVAL, "negative m");
    if (m > 0 && (!xs0 || !xs1 || !f_star)) return gpc_fail(ctx, GPC_EINVAL, "xs0/xs1/f_star is NULL");
    const int P = g->P;
    if (P == 0 || m == 0) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t Pm = (size_t)P * (size_t)m, ny = (size_t)g->ny;
    GpcStaging st(ctx, "gpc_sparse_predict");
    const double *d_xs0 = st.up(xs0, (size_t)m), *d_xs1 = st.up(xs1, (size_t)m);
    double *d_f = st.out<double>(Pm * ny), *d_s = sigma ? st.out<double>(Pm) : nullptr;
    int32_t* d_st = st.out<int32_t>((size_t)P);
    if (st.ok()) st.rc = gpc_sparse_predict_dev(g, m, d_xs0, d_xs1, d_f, d_s, conf, d_st);
    st.down(f_star, d_f, Pm * ny);
    st.down(sigma, d_s, Pm);
    st.down(status, d_st, (size_t)P);
    return st.finish();
}

int gpc_sparse_predict_points(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, double* f, double* sigma,
                              int conf, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    const int P = g->P;
    if (P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (P == 0) return GPC_OK;
    if (int rc = gpc_check_host_off(ctx, P, off, nullptr, nullptr)) return rc;
    const size_t N = (size_t)off[P], ny = (size_t)g->ny;
    if (N > 0 && (!x0 || !x1 || !f)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/f is NULL");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_sparse_predict_points");
    const int32_t* d_off = st.up(off, (size_t)P + 1);
    const double *d_x0 = st.up(x0, N), *d_x1 = st.up(x1, N);
    double *d_f = st.out<double>(N * ny), *d_s = sigma ? st.out<double>(N) : nullptr;
    int32_t* d_st = st.out<int32_t>((size_t)P);
    if (st.ok()) st.rc = gpc_sparse_predict_points_dev(g, d_off, (int)N, d_x0, d_x1, d_f, d_s, conf, d_st);
    st.down(f, d_f, N * ny);
    st.down(sigma, d_s, N);
    st.down(status, d_st, (size_t)P);
    return st.finish();
}

int gpc_sparse_predict_scattered(gpc_sparse* g, int n, const int32_t* patch, const double* x0, const double* x1, int stride, double* f,
                                 double* sigma, int conf, int32_t* status)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (int rc = sp_scattered_check(ctx, n, patch, x0, x1, stride)) return rc;
    const size_t N = (size_t)n, ny = (size_t)g->ny, P = (size_t)g->P;
    if (n == 0 && (!status || P == 0)) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_sparse_predict_scattered");
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
    double *d_f = f ? st.out<double>(N * ny) : nullptr, *d_s = sigma ? st.out<double>(N) : nullptr;
    int32_t* d_st = status ? st.out<int32_t>(P) : nullptr;
    if (st.ok()) st.rc = gpc_sparse_predict_scattered_dev(g, n, d_patch, d_x0, d_x1, stride, d_f, d_s, conf, d_st);
    st.down(f, d_f, N * ny);
    st.down(sigma, d_s, N);
    st.down(status, d_st, P);
    return st.finish();
}

int gpc_sparse_sizes(gpc_sparse* g, int32_t* bv_count)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (!bv_count) return gpc_fail(ctx, GPC_EINVAL, "bv_count is NULL");
    if (g->P == 0) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = gpc_stream_of(ctx);
    GPC_HIP(ctx, hipMemcpyAsync(bv_count, g->b, 4 * (size_t)g->P, hipMemcpyDeviceToHost, s));
    GPC_HIP(ctx, hipStreamSynchronize(s));
    return GPC_OK;
}

int gpc_sparse_get_state(gpc_sparse* g, double* alpha, double* C, double* Q, double* BV)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (g->P == 0) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ld = (size_t)g->ld, P = (size_t)g->P;
    hipStream_t s = gpc_stream_of(ctx);
    if (alpha) GPC_HIP(ctx, hipMemcpyAsync(alpha, g->alpha, 8 * P * g->ny * ld, hipMemcpyDeviceToHost, s));
    if (C) GPC_HIP(ctx, hipMemcpyAsync(C, g->C, 8 * P * ld * ld, hipMemcpyDeviceToHost, s));
    if (Q) GPC_HIP(ctx, hipMemcpyAsync(Q, g->Q, 8 * P * ld * ld, hipMemcpyDeviceToHost, s));
    if (BV) GPC_HIP(ctx, hipMemcpyAsync(BV, g->BV, 8 * P * ld * 2, hipMemcpyDeviceToHost, s));
    GPC_HIP(ctx, hipStreamSynchronize(s));
    return GPC_OK;
}

// Inverse of gpc_sparse_get_state: loads a stored model (the compressed representation of row f3).  alpha and BV are
// required, C and Q may be NULL (zeroed: the mean prediction of the decompressor needs neither; sigma, likelihoods and
// further online growth do).
int gpc_sparse_set_state(gpc_sparse* g, const int32_t* bv_count, const double* alpha, const double* C, const double* Q,
                         const double* BV)
{
    if (!g) return GPC_EINVAL;
    gpc_ctx* ctx = g->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;   // the context went first: the object can only be destroyed (include/gpc.h)
    if (g->P == 0) return GPC_OK;
    if (!bv_count || !alpha || !BV) return gpc_fail(ctx, GPC_EINVAL, "bv_count/alpha/BV is NULL");
    for (int i = 0; i < g->P; ++i)
        if (bv_count[i] < 0 || bv_count[i] > g->ld) return gpc_fail(ctx, GPC_ERANGE, "bv_count[%d] = %d outside [0, %d]", i, bv_count[i], g->ld);
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ld = (size_t)g->ld, P = (size_t)g->P;
    hipStream_t s = ctx->stream;
    GPC_HIP(ctx, hipMemcpyAsync(g->b, bv_count, 4 * P, hipMemcpyHostToDevice, s));
    GPC_HIP(ctx, hipMemcpyAsync(g->count, bv_count, 4 * P, hipMemcpyHostToDevice, s));
    GPC_HIP(ctx, hipMemsetAsync(g->stat, 0, 4 * P, s));
    GPC_HIP(ctx, hipMemcpyAsync(g->alpha, alpha, 8 * P * g->ny * ld, hipMemcpyHostToDevice, s));
    GPC_HIP(ctx, hipMemcpyAsync(g->BV, BV, 8 * P * ld * 2, hipMemcpyHostToDevice, s));
    if (C) GPC_HIP(ctx, hipMemcpyAsync(g->C, C, 8 * P * ld * ld, hipMemcpyHostToDevice, s));
    else GPC_HIP(ctx, hipMemsetAsync(g->C, 0, 8 * P * ld * ld, s));
    if (Q) GPC_HIP(ctx, hipMemcpyAsync(g->Q, Q, 8 * P * ld * ld, hipMemcpyHostToDevice, s));
    else GPC_HIP(ctx, hipMemsetAsync(g->Q, 0, 8 * P * ld * ld, s));
    GPC_HIP(ctx, hipStreamSynchronize(s));
    return GPC_OK;
}

}  // extern "C"
