// dense_api.hip -- the dense path on device pointers: argument checks, the dispatcher that executes the route of a batch (the rule
// that chooses the kernels is dense_route, dense_route.h: nothing here decides), the two Gaussian _dev entries and the route test hook.
// The pipelined host-pointer dense entries are in dense_host.hip, the probit / IRLS entries in dense_irls_api.hip.
#include "dense_internal.h"

int dense_check(gpc_ctx* ctx, const gpc_params* prm, int P, const void* off, int n_max, int n_total,
                const void* x0, const void* x1, const void* y, int ny, int m, const void* f_star)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!prm) return gpc_fail(ctx, GPC_EINVAL, "params is NULL");
    if (P < 0 || m < 0 || n_total < 0 || n_max < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (ny != 1 && ny != 3) return gpc_fail(ctx, GPC_EINVAL, "ny must be 1 (depth) or 3 (RGB), got %d", ny);
    if (P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    if (n_total > 0 && (!x0 || !x1 || !y)) return gpc_fail(ctx, GPC_EINVAL, "x0/x1/y is NULL");
    if (P > 0 && m > 0 && !f_star) return gpc_fail(ctx, GPC_EINVAL, "f_star is NULL");
    if (n_max > GPC_MAX_POINTS) return gpc_fail(ctx, GPC_ERANGE, "n_max %d > GPC_MAX_POINTS %d", n_max, GPC_MAX_POINTS);
    if (!(prm->l_sq > 0.0) || !(prm->sigmaf_sq >= 0.0) || !(prm->noise >= 0.0))
        return gpc_fail(ctx, GPC_EINVAL, "kernel/noise parameters out of range");
    return GPC_OK;
}

DenseArgs dense_args(const gpc_params* prm, int P, const int32_t* off, int n_max, int n_total, const double* x0, const double* x1,
                     const double* y, int ny, int m, double* f_star, double* alpha_out, int32_t* status)
{
    DenseArgs a{};
    a.prm = *prm;
    a.P = P; a.n_max = n_max; a.n_total = n_total; a.ny = ny; a.m = m;
    a.off = off; a.x0 = x0; a.x1 = x1; a.y = y;
    a.f_star = f_star; a.alpha_out = alpha_out; a.status = status;
    return a;
}

// Ragged batches whose largest patch exceeds the register-resident kernel's 256 points: patches are sorted into size classes on
// the device (no host round trip: `off` lives there) -- n <= 256 -> the register-resident kernel, 256 < n <= 272 -> its NT = 17
// shape (depth plane only: the octree leaves of a cloud cut for 256-point patches scatter around that size, median 258, and
// would otherwise pay the tiled kernel's 4x cost per patch), the rest -> the tiled kernel.  Patches are independent, so the
// order inside a class does not matter.
extern "C" __global__ void dense_classify_kernel(int P, const int32_t* off, int bound0, int bound1, int32_t* sel0, int32_t* sel1, int32_t* sel2,
                                                 int32_t* counts)
{
    // one atomic per wave and class (a counter takes ~11 ns per atomic device-wide: with one per patch the 8192 patches of a
    // single-class batch spent 95 us here, 0.8 % of a C3 launch and 5 % of a C2-sized one)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int n = i < P ? off[i + 1] - off[i] : 0;
    const int cls = i >= P ? -1 : n <= bound0 ? 0 : n <= bound1 ? 1 : 2;
    int32_t* const sel[3] = {sel0, sel1, sel2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(cls == c);
        if (m == 0) continue;
        int base = 0;
        if (lane == __builtin_ctzll(m)) base = atomicAdd(&counts[c], __builtin_popcountll(m));
        base = __builtin_amdgcn_readlane(base, __builtin_ctzll(m));
        if (cls == c) sel[c][base + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = i;
    }
}

static inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// The size-class split of a ragged batch (DENSE_SPLIT): classify on the device, then one launch per class.  `hinted` sizes launches,
// it does not choose kernels.
static int dense_split(gpc_ctx* ctx, const DenseArgs& a, const DenseSite& site, const DenseRoute& route, bool no_hint)
{
    const bool nt17 = route.nt17, need_big = route.need_big;
    const DenseRoute big = dense_route_class(route, 2);
    int grid_b = 0;
    const size_t big_bytes = need_big ? al256(dense_big_ws_bytes(ctx, a, big, &grid_b)) : 0;
    // Class sizes known on the host (the batch came from gpc_project_cloud on this context): the class launches get exactly that
    // many workgroups.  The hint is matched by pointer and P only -- a caller that rewrites `off` IN PLACE keeps both -- so every
    // hinted launch is followed by an OVERFLOW launch of the generic kernel (a few workgroups that stride over
    // sel[hint .. count), count on the device: no patch when the hint was right, every patch the hint missed otherwise).
    const bool hinted = ctx->hint_off == a.off && ctx->hint_P == a.P && !no_hint;
    constexpr int OVF_GRID = 8;
    const size_t ovf_slot = sizeof(double) * (size_t)(17 * 16 + a.ny) * (size_t)(17 * 16 + a.ny);
    const size_t ovf_bytes = hinted ? al256(2 * OVF_GRID * ovf_slot) : 0;
    int rc = gpc_ws_reserve(ctx, site, big_bytes + ovf_bytes + sizeof(int32_t) * (3 * (size_t)a.P + 64));
    if (rc != GPC_OK) return rc;
    double* ovf_ws = reinterpret_cast<double*>(dense_ws(ctx, site) + big_bytes);
    int32_t* counts = reinterpret_cast<int32_t*>(dense_ws(ctx, site) + big_bytes + ovf_bytes);
    int32_t* sel0 = counts + 64;
    int32_t* sel1 = sel0 + a.P;
    int32_t* sel2 = sel1 + a.P;
    GPC_HIP(ctx, hipMemsetAsync(counts, 0, 3 * sizeof(int32_t), site.stream));
    hipLaunchKernelGGL(dense_classify_kernel, dim3((a.P + 255) / 256), dim3(256), 0, site.stream, a.P, a.off, 256, nt17 ? 17 * 16 : 256,
                       sel0, sel1, sel2, counts);
    GPC_HIP(ctx, hipGetLastError());
    // The classes are independent: they run on three streams (forked from and joined to the site's), so that
    // the tail of one kernel -- its last workgroups running on a mostly idle chip -- fills with the next one's work.
    const hipStream_t main_s = site.stream;
    const DenseSite on_in{ctx->s_in, site.ws_off, site.ws_len}, on_out{ctx->s_out, site.ws_off, site.ws_len};
    // an error after the fork must not leave work (or the caller's buffers) in flight on the side streams
    auto bail = [&](int code) {
        (void)hipStreamSynchronize(ctx->s_in);
        (void)hipStreamSynchronize(ctx->s_out);
        return code;
    };
    GPC_HIP(ctx, hipEventRecord(ctx->ev[0][GPC_EV_CLASS_FORK], main_s));
    GPC_HIP(ctx, hipStreamWaitEvent(ctx->s_in, ctx->ev[0][GPC_EV_CLASS_FORK], 0));
    GPC_HIP(ctx, hipStreamWaitEvent(ctx->s_out, ctx->ev[0][GPC_EV_CLASS_FORK], 0));
    // largest patches first: the tiled kernel's workgroups are the long ones
    if (need_big) {
        DenseArgs b = a;
        b.sel = sel2; b.sel_count = counts + 2;
        rc = dense_big_launch(ctx, on_out, b, big, grid_b);
        if (rc != GPC_OK) return bail(rc);
    }
    // Class `which` (0: n <= 256, 1: the NT = 17 shape) on the register kernel, `cnt` workgroups at `at`.  Without a hint cnt is P: the
    // workgroups beyond the class count leave at once, but each still waits for a CU with 158 KB of LDS free.  With one, the overflow
    // launch follows on the same stream; a class the hint calls empty is its overflow launch alone, on the main stream.
    auto run_class = [&](int which, int cnt, const DenseSite& at) -> int {
        DenseArgs s = a;
        s.n_max = which ? 17 * 16 : 256;       // the class bound: what the overflow launch sizes its LDS and its slots for
        s.sel = which ? sel1 : sel0; s.sel_count = counts + which;
        s.P = cnt;
        const int rcl = cnt > 0 ? dense_mfma_launch(ctx, at, s, dense_route_class(route, which)) : GPC_OK;
        if (rcl != GPC_OK || !hinted || cnt >= a.P) return rcl;
        s.sel_base = cnt;
        s.P = a.P;
        return dense_generic_launch(ctx, cnt > 0 ? at : site, s, OVF_GRID, ovf_ws + (size_t)which * OVF_GRID * (ovf_slot / sizeof(double)));
    };
    const int c0 = hinted ? ctx->hint_le256 : a.P;
    const int c1 = hinted ? ctx->hint_le272 - ctx->hint_le256 : a.P;
    if (nt17 && (rc = run_class(1, c1, on_in)) != GPC_OK) return bail(rc);
    if ((rc = run_class(0, c0, site)) != GPC_OK) return bail(rc);
    GPC_HIP(ctx, hipEventRecord(ctx->ev[1][GPC_EV_CLASS_FORK], ctx->s_in));
    GPC_HIP(ctx, hipEventRecord(ctx->ev[2][GPC_EV_CLASS_FORK], ctx->s_out));
    GPC_HIP(ctx, hipStreamWaitEvent(main_s, ctx->ev[1][GPC_EV_CLASS_FORK], 0));
    GPC_HIP(ctx, hipStreamWaitEvent(main_s, ctx->ev[2][GPC_EV_CLASS_FORK], 0));
    return rc;
}

// Executes the route of a batch: reserves what its kernel needs, launches it, records its name.  Caller holds ctx->mu.
int dense_dispatch(gpc_ctx* ctx, DenseArgs& a, const DenseSite& site, unsigned* seen_gen)
{
    const DenseSwitches sw = dense_switches_read();
    const DenseFacts facts = dense_facts(ctx, a);
    DenseRoute route = dense_route(facts, sw);
    if (route.kind == DENSE_NOTHING) return GPC_OK;
    if (a.n_max < 1) a.n_max = 1;
    if (seen_gen)      // a chunk of the two-stream host pipeline
        if (int rco = gpc_pipe_chunk_order(ctx, site.stream, seen_gen)) return rco;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (!a.prm.want_variance) a.v_star = nullptr;
    if (int rcp = gpc_debug_poison_lds(ctx, site)) return rcp;
    int grid = 0, rc = GPC_OK;
    if (route.kind == DENSE_ONE_WAVE) {
        // One factor slot (304 KB) per patch of a launch.  If the device cannot serve that, the batch goes
        // through in smaller launches that reuse fewer slots, and below two launches' worth of resident patches it takes the
        // route it would have had without this kernel -- the register-resident one needs no workspace at all.
        for (int cap_w1 = site.w1_cap;;) {      // (site.w1_cap: where the caller's own dense_reserve, which ran this loop, ended)
            rc = gpc_ws_reserve(ctx, site, al256(dense_w1_ws_bytes(facts, route, &grid, cap_w1)));
            if (rc != GPC_ENOMEM) break;
            cap_w1 = grid / 2;
            if (cap_w1 < 4 * ctx->num_cus) break;             // (below the batch-size rule of this kernel)
        }
        if (rc == GPC_ENOMEM) {
            route = dense_route(facts, sw, true);
            if (route.kind == DENSE_NO_ROUTE) return rc;
            (void)hipGetLastError();
        } else if (rc != GPC_OK) {
            return rc;
        }
    }
    switch (route.kind) {
        case DENSE_ONE_WAVE:
            rc = dense_w1_launch(ctx, site, a, route, grid);
            break;
        case DENSE_REGISTER:                                    // one shape for the whole batch
            rc = dense_mfma_launch(ctx, site, a, route);
            break;
        case DENSE_TILED:
            if ((rc = gpc_ws_reserve(ctx, site, al256(dense_big_ws_bytes(ctx, a, route, &grid)))) == GPC_OK)
                rc = dense_big_launch(ctx, site, a, route, grid);
            break;
        case DENSE_SPLIT:
            rc = dense_split(ctx, a, site, route, sw.no_hint);
            break;
        case DENSE_GENERIC:
            if ((rc = gpc_ws_reserve(ctx, site, dense_generic_ws_bytes(ctx, a, &grid))) == GPC_OK)
                rc = dense_generic_launch(ctx, site, a, grid);
            break;
        default:
            return gpc_fail(ctx, GPC_EINVAL, "no route for this batch");
    }
    if (rc == GPC_OK) ctx->last_dense_kernel = route.name;
    return rc;
}

// What dense_dispatch will reserve for a batch on the variance route, `front` bytes of the caller's own in front of it, reserved in one
// step at `site`: the caller may then fill its front region before the dispatch without a later grow moving the workspace from under it.
// The one-wave route runs the dispatcher's retry with fewer slots here and leaves where it ended in *w1_cap.  A batch off the variance
// route is GPC_EINVAL; DENSE_NO_ROUTE stays GPC_ENOMEM.
int dense_reserve(gpc_ctx* ctx, const DenseSite& site, size_t front, const DenseArgs& a, int* w1_cap)
{
    *w1_cap = 0;
    const DenseFacts facts = dense_facts(ctx, a);
    const DenseRoute route = dense_route(facts, dense_switches_read());
    int grid = 0, rc = GPC_ENOMEM;
    switch (route.kind) {
        case DENSE_NOTHING:
            return gpc_ws_reserve(ctx, site, front);
        case DENSE_ONE_WAVE:
            for (int cap_w1 = 0;;) {
                rc = gpc_ws_reserve(ctx, site, front + al256(dense_w1_ws_bytes(facts, route, &grid, cap_w1)));
                *w1_cap = cap_w1;
                if (rc != GPC_ENOMEM) break;
                cap_w1 = grid / 2;
                if (cap_w1 < 4 * ctx->num_cus) break;
            }
            return rc;
        case DENSE_REGISTER:
            return gpc_ws_reserve(ctx, site, front + dense_mfma_ws_bytes(a, route));
        case DENSE_TILED:
            return gpc_ws_reserve(ctx, site, front + al256(dense_big_ws_bytes(ctx, a, route, &grid)));
        case DENSE_GENERIC:
            return gpc_ws_reserve(ctx, site, front + dense_generic_ws_bytes(ctx, a, &grid));
        case DENSE_NO_ROUTE:
            return gpc_fail(ctx, GPC_ENOMEM, "no kernel computes the variance of this batch without the one-wave workspace");
        default:
            return gpc_fail(ctx, GPC_EINVAL, "dense_reserve: not a batch of the variance route");
    }
}

extern "C" {

int gpc_dense_fit_predict_dev(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off, int n_max, int n_total,
                              const double* x0, const double* x1, const double* y, int ny,
                              int m, const double* xs0, const double* xs1,
                              double* f_star, double* v_star, double* alpha_out, int32_t* status)
{
    int rc = dense_check(ctx, params, P, off, n_max, n_total, x0, x1, y, ny, m, f_star);
    if (rc != GPC_OK) return rc;
    if (m > 0 && (!xs0 || !xs1)) return gpc_fail(ctx, GPC_EINVAL, "xs0/xs1 is NULL");
    DenseArgs a = dense_args(params, P, off, n_max, n_total, x0, x1, y, ny, m, f_star, alpha_out, status);
    a.xs0 = xs0; a.xs1 = xs1;
    a.v_star = v_star;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return dense_dispatch(ctx, a, dense_site_of(ctx));
}

int gpc_dense_fit_predict_grid_dev(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off, int n_max,
                                   int n_total, const double* x0, const double* x1, const double* y, int ny,
                                   double res, int sz, double* f_star, double* alpha_out, int32_t* status)
{
    if (ctx && (sz < 0 || sz > 1024)) return gpc_fail(ctx, GPC_EINVAL, "sz out of range");
    int rc = dense_check(ctx, params, P, off, n_max, n_total, x0, x1, y, ny, sz * sz, f_star);
    if (rc != GPC_OK) return rc;
    DenseArgs a = dense_args(params, P, off, n_max, n_total, x0, x1, y, ny, sz * sz, f_star, alpha_out, status);
    a.prm.want_variance = 0;
    a.grid_res = res; a.grid_sz = sz;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return dense_dispatch(ctx, a, dense_site_of(ctx));
}

// host-only test hook: dense_route for the given facts under the switches of the environment (no HIP call: works without a GPU)
int gpc_test_dense_route(int P, int n_max, int n_total, int ny, int m, int variance, int pointwise, int alpha_out, int num_cus, int irls,
                         int w1_refused, char* name, int name_cap, int32_t* shape)
{
    const DenseFacts f{P, n_max, n_total, ny, m, variance != 0, pointwise != 0, alpha_out != 0, num_cus, irls != 0};
    const DenseRoute r = dense_route(f, dense_switches_read(), w1_refused != 0);
    if (name && name_cap > 0) snprintf(name, (size_t)name_cap, "%s", r.name);
    if (shape) {
        const int32_t v[GPC_TEST_ROUTE_SHAPE] = {r.w1_npad, r.w1_slots, r.nt, r.export_factor, r.waves, r.npad, r.per_cu, r.nt17, r.need_big};
        memcpy(shape, v, sizeof(v));
    }
    return (int)r.kind;
}

}  // extern "C"
