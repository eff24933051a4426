// dense_ev_api.hip -- the log marginal likelihood of the regression GP and the per-patch selection among candidate hyper-parameters built
// on it: gpc_dense_fit_predict_ev and gpc_dense_select, each on host and on device pointers (definitions: include/gpc.h).  Every entry
// fills one record (GaussCall) and hands it to gauss_run_host or gauss_run_dev; there is one list of argument rules (gauss_rules) and one
// staging list (gauss_run_host).  A call that asks for log_ev is a dense_dispatch on the variance route with DenseArgs::log_ev set: the
// launchers keep the factor export on and enqueue the read-out (dense_evidence.hip) where the factor is still in place.
#include "dense_internal.h"

// What any of the four entries received.  Host form: every pointer but params and cand is a host pointer, and n_max, n_total are found
// from off (gauss_rules).
struct GaussCall {
    const gpc_params* params;
    bool select;              // gpc_dense_select[_dev]: H candidates at cand (host memory in both forms)
    int H;
    const gpc_hyper* cand;
    int P;
    const int32_t* off;
    int n_max, n_total;
    const double *x0, *x1, *y;
    int ny;
    int m;                    // point-wise X*: as given; grid form (xs0 == nullptr): sz sz once gauss_rules has run
    const double *xs0, *xs1;
    double res;
    int sz;
    double *f_star, *v_star, *alpha_out;
    int32_t* status;
    double* log_ev;
    int32_t* best;
    double* log_ev_all;
};

// The argument rules of every entry, in the order include/gpc.h states them, and the record made ready for the run: m = sz sz in the
// grid form, n_max >= 1; host form: n_max and n_total from off.  GPC_OK with c.P == 0: the call is valid and there is nothing to do.
static int gauss_rules(gpc_ctx* ctx, GaussCall& c, bool host)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!c.params) return gpc_fail(ctx, GPC_EINVAL, "params is NULL");
    if (c.select) {
        if (c.H < 1 || !c.cand) return gpc_fail(ctx, GPC_EINVAL, "select needs H >= 1 candidates");
        for (int h = 0; h < c.H; ++h) {
            const gpc_hyper& k = c.cand[h];
            const bool finite = k.sigmaf_sq - k.sigmaf_sq == 0.0 && k.l_sq - k.l_sq == 0.0 && k.noise - k.noise == 0.0;
            if (!finite || !(k.sigmaf_sq > 0.0) || !(k.l_sq > 0.0) || !(k.noise >= 0.0))
                return gpc_fail(ctx, GPC_EINVAL, "candidate %d has a non-positive or non-finite field", h);
        }
    }
    const bool grid = (c.xs0 == nullptr);
    if (grid) {
        if (c.sz < 0 || c.sz > 1024) return gpc_fail(ctx, GPC_EINVAL, "sz out of range");
        c.m = c.sz * c.sz;
    }
    int rc;
    if (host) {
        if (c.P < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
        if (c.P > 0 && !c.off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
        if ((rc = gpc_check_host_off(ctx, c.P, c.off, &c.n_max, &c.n_total))) return rc;
    }
    // (select: f_star may be NULL, the candidates write into temporaries)
    if ((rc = dense_check(ctx, c.params, c.P, c.off, c.n_max, c.n_total, c.x0, c.x1, c.y, c.ny, c.select ? 0 : c.m, c.f_star))) return rc;
    if (c.m < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (c.n_max < 1) c.n_max = 1;
    if (!grid && c.m > 0 && !c.xs1) return gpc_fail(ctx, GPC_EINVAL, "xs1 is NULL");
    return GPC_OK;
}

// The front region of one fit's workspace, ahead of what the dispatch reserves: the status where the caller does not take it (the
// read-out needs it) and the grid as points.  alpha needs no place here: with the export on every launcher keeps it in its own region
// when alpha_out is NULL and hands that to the read-out, and the generic kernel reads its own copy -- except where nothing else is
// wanted (m == 0, no alpha_out), since a batch with neither a prediction nor the weights asked for has no route at all.
struct GaussFront {
    size_t o_al, o_st, o_xs, bytes;
};
static GaussFront gauss_front(const GaussCall& c)
{
    GaussFront w{};
    WsCarve cv;
    w.o_al = cv.take<double>(c.alpha_out || c.m > 0 ? 0 : (size_t)c.n_total * c.ny + 1);
    w.o_st = cv.take<int32_t>(c.status ? 0 : (size_t)c.P);
    w.o_xs = cv.take<double>(c.xs0 ? 0 : 2 * (size_t)c.m);
    w.bytes = cv.bytes;
    return w;
}

// The batch of a record under `prm` as the dispatcher takes it, the temporaries at `front`.  X* is point-wise throughout: the variance
// kernels have no separable form, so the grid form is evaluated on the materialised grid.  want_variance follows v_star.
static DenseArgs gauss_args(const GaussCall& c, const gpc_params& prm, char* front)
{
    const GaussFront w = gauss_front(c);
    DenseArgs a = dense_args(&prm, c.P, c.off, c.n_max, c.n_total, c.x0, c.x1, c.y, c.ny, c.m, c.f_star,
                             c.alpha_out || c.m > 0 ? c.alpha_out : ws_at<double>(front, w.o_al),
                             c.status ? c.status : ws_at<int32_t>(front, w.o_st));
    a.prm.want_variance = c.v_star != nullptr;
    a.v_star = c.v_star;
    a.log_ev = c.log_ev;
    a.xs0 = c.xs0 ? c.xs0 : ws_at<double>(front, w.o_xs);
    a.xs1 = c.xs0 ? c.xs1 : ws_at<double>(front, w.o_xs) + c.m;
    return a;
}

// What gpc_last_dense_kernel reports for a call with the evidence but without v_star: the route's names end in the variance kernel, which
// such a call does not run.  (With v_star the route's own name stands; the generic kernel forms the evidence itself.)
static const char* gauss_kernel_name(const char* route_name)
{
    static const char* const names[][2] = {{"dense_mfma_nt4 ", "dense_mfma_nt4 + dense_gauss_evidence"},
                                           {"dense_mfma_nt8 ", "dense_mfma_nt8 + dense_gauss_evidence"},
                                           {"dense_mfma_nt12 ", "dense_mfma_nt12 + dense_gauss_evidence"},
                                           {"dense_mfma_nt16 ", "dense_mfma_nt16 + dense_gauss_evidence"},
                                           {"dense_mfma_w1 ", "dense_mfma_w1 + dense_gauss_evidence"},
                                           {"dense_mfma_big ", "dense_mfma_big + dense_gauss_evidence"}};
    for (const auto& n : names)
        if (strncmp(route_name, n[0], strlen(n[0])) == 0) return n[1];
    return route_name;
}

// One fit of a record whose workspace is reserved (dense_reserve at `site` with gauss_front's bytes in front, which gave w1_cap): the grid
// as points, then the dispatch behind the front region.  Record checked (gauss_rules), P > 0; caller holds ctx->mu.
static int gauss_fit(gpc_ctx* ctx, const DenseSite& site, const GaussCall& c, const gpc_params& prm, int w1_cap)
{
    const GaussFront w = gauss_front(c);
    DenseArgs a = gauss_args(c, prm, dense_ws(ctx, site));
    int rc;
    if (!c.xs0 && c.m > 0 && (rc = dense_grid_points_launch(ctx, site, c.res, c.sz, const_cast<double*>(a.xs0), const_cast<double*>(a.xs1))))
        return rc;
    const DenseSite behind{site.stream, site.ws_off + w.bytes, 0, w1_cap};
    if ((rc = dense_dispatch(ctx, a, behind))) return rc;
    if (c.log_ev && !c.v_star) ctx->last_dense_kernel = gauss_kernel_name(ctx->last_dense_kernel);
    return GPC_OK;
}

// ... with the reserve in front of it.  Pointers into the workspace do not exist before the reserve; what the route looks at is which of
// them are set, so a placeholder base stands in for it.
static int gauss_reserve(gpc_ctx* ctx, const DenseSite& site, const GaussCall& c, int* w1_cap)
{
    const DenseArgs probe = gauss_args(c, *c.params, reinterpret_cast<char*>((uintptr_t)4096));
    return dense_reserve(ctx, site, gauss_front(c).bytes, probe, w1_cap);
}

// The selection loop: every candidate is an _ev fit into temporaries, and the keep-best step behind it copies the rows of the patches it
// won so far into the caller's outputs.  The workspace: the temporaries of one candidate and the state of the keep-best step in front,
// the fit's region behind them.
static int gauss_select(gpc_ctx* ctx, const DenseSite& whole, const GaussCall& c)
{
    const size_t Pz = (size_t)c.P, Pm = Pz * (size_t)c.m, N = (size_t)c.n_total, ny = (size_t)c.ny;
    WsCarve cv;
    const size_t o_f = cv.take<double>(Pm * ny + 1), o_v = cv.take<double>(c.v_star ? Pm : 0), o_al = cv.take<double>(N * ny + 1),
                 o_ev = cv.take<double>(Pz * ny), o_cur_ev = cv.take<double>(Pz), o_st = cv.take<int32_t>(Pz), o_cur_best = cv.take<int32_t>(Pz);
    const DenseSite site{whole.stream, whole.ws_off + cv.bytes, 0};
    const char* fake = reinterpret_cast<char*>((uintptr_t)4096);
    GaussCall k = c;               // one candidate: the _ev level on prm, into the temporaries
    k.select = false;
    k.best = nullptr; k.log_ev_all = nullptr;
    auto aim = [&](char* t) {
        k.f_star = ws_at<double>(t, o_f); k.v_star = c.v_star ? ws_at<double>(t, o_v) : nullptr; k.alpha_out = ws_at<double>(t, o_al);
        k.log_ev = ws_at<double>(t, o_ev); k.status = ws_at<int32_t>(t, o_st);
    };
    aim(const_cast<char*>(fake));
    int rc, w1_cap = 0;
    if ((rc = gauss_reserve(ctx, site, k, &w1_cap))) return rc;
    char* t = dense_ws(ctx, whole);
    aim(t);
    const GaussRows tmp{k.f_star, k.v_star, k.alpha_out, k.log_ev, k.status};
    const GaussRows out{c.f_star, c.v_star, c.alpha_out, c.log_ev, c.status};
    gpc_params prm = *c.params;
    for (int h = 0; h < c.H; ++h) {
        prm.sigmaf_sq = c.cand[h].sigmaf_sq; prm.l_sq = c.cand[h].l_sq; prm.noise = c.cand[h].noise;
        if ((rc = gauss_fit(ctx, site, k, prm, w1_cap))) return rc;
        if ((rc = dense_gauss_keep_launch(ctx, whole, h, c.P, c.ny, c.m, c.n_total, c.off, tmp, out, c.best,
                                          c.log_ev_all ? c.log_ev_all + (size_t)h * Pz * ny : nullptr, ws_at<int32_t>(t, o_cur_best),
                                          ws_at<double>(t, o_cur_ev))))
            return rc;
    }
    return GPC_OK;
}

// The device-pointer run of a record: the selection loop, or one fit with its reserve.
static int gauss_run_dev(gpc_ctx* ctx, GaussCall c)
{
    const int rc = gauss_rules(ctx, c, false);
    if (rc != GPC_OK || c.P == 0) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const DenseSite site = dense_site_of(ctx);
    if (c.select) return gauss_select(ctx, site, c);
    int w1_cap = 0;
    if (const int rcr = gauss_reserve(ctx, site, c, &w1_cap)) return rcr;
    return gauss_fit(ctx, site, c, *c.params, w1_cap);
}

// The host-pointer run: every input and every output the record asks for is staged, the device-pointer run does the work.  The mean is
// staged whether the caller takes it or not, as is log_ev under select; everything else only when requested.
static int gauss_run_host(gpc_ctx* ctx, const char* entry, GaussCall c)
{
    const int rc = gauss_rules(ctx, c, true);
    if (rc != GPC_OK || c.P == 0) return rc;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const bool grid = (c.xs0 == nullptr);
    const size_t N = (size_t)c.n_total, Pz = (size_t)c.P, Pm = Pz * (size_t)c.m, ny = (size_t)c.ny, HP = (size_t)c.H * Pz;
    GpcStaging st(ctx, entry);
    GaussCall d = c;
    d.off = st.up(c.off, Pz + 1);
    d.x0 = st.up(c.x0, N); d.x1 = st.up(c.x1, N); d.y = st.up(c.y, N * ny);
    d.xs0 = grid ? nullptr : st.up(c.xs0, (size_t)c.m); d.xs1 = grid ? nullptr : st.up(c.xs1, (size_t)c.m);
    d.f_star = st.out<double>(Pm * ny);
    d.v_star = c.v_star ? st.out<double>(Pm) : nullptr;
    d.alpha_out = c.alpha_out ? st.out<double>(N * ny) : nullptr;
    d.status = c.status ? st.out<int32_t>(Pz) : nullptr;
    d.log_ev = c.log_ev || c.select ? st.out<double>(Pz * ny) : nullptr;
    d.best = c.select && c.best ? st.out<int32_t>(Pz) : nullptr;
    d.log_ev_all = c.select && c.log_ev_all ? st.out<double>(HP * ny) : nullptr;
    if (st.ok()) st.rc = gauss_run_dev(ctx, d);
    st.down(c.f_star, d.f_star, Pm * ny);
    st.down(c.v_star, d.v_star, Pm);
    st.down(c.alpha_out, d.alpha_out, N * ny);
    st.down(c.status, d.status, Pz);
    st.down(c.log_ev, d.log_ev, Pz * ny);
    st.down(c.best, d.best, Pz);
    st.down(c.log_ev_all, d.log_ev_all, HP * ny);
    return st.finish();
}

extern "C" {

int gpc_dense_fit_predict_ev_dev(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off, int n_max, int n_total,
                                 const double* x0, const double* x1, const double* y, int ny, int m, const double* xs0, const double* xs1,
                                 double res, int sz, double* f_star, double* v_star, double* alpha_out, int32_t* status, double* log_ev)
{
    // without the evidence the call IS the plain entry: the same launches, the same bits
    if (!log_ev && xs0)
        return gpc_dense_fit_predict_dev(ctx, params, P, off, n_max, n_total, x0, x1, y, ny, m, xs0, xs1, f_star, v_star, alpha_out, status);
    if (!log_ev && !(params && params->want_variance && v_star))
        return gpc_dense_fit_predict_grid_dev(ctx, params, P, off, n_max, n_total, x0, x1, y, ny, res, sz, f_star, alpha_out, status);
    return gauss_run_dev(ctx, GaussCall{params, false, 0, nullptr, P, off, n_max, n_total, x0, x1, y, ny, m, xs0, xs1, res, sz,
                                        f_star, v_star, alpha_out, status, log_ev, nullptr, nullptr});
}

int gpc_dense_fit_predict_ev(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off, const double* x0, const double* x1,
                             const double* y, int ny, int m, const double* xs0, const double* xs1, double res, int sz, double* f_star,
                             double* v_star, double* alpha_out, int32_t* status, double* log_ev)
{
    if (!log_ev && xs0) return gpc_dense_fit_predict(ctx, params, P, off, x0, x1, y, ny, m, xs0, xs1, f_star, v_star, alpha_out, status);
    if (!log_ev && !(params && params->want_variance && v_star))
        return gpc_dense_fit_predict_grid(ctx, params, P, off, x0, x1, y, ny, res, sz, f_star, alpha_out, status);
    return gauss_run_host(ctx, "gpc_dense_fit_predict_ev",
                          GaussCall{params, false, 0, nullptr, P, off, 0, 0, x0, x1, y, ny, m, xs0, xs1, res, sz,
                                    f_star, v_star, alpha_out, status, log_ev, nullptr, nullptr});
}

int gpc_dense_select_dev(gpc_ctx* ctx, const gpc_params* params, int H, const gpc_hyper* cand, int P, const int32_t* off, int n_max,
                         int n_total, const double* x0, const double* x1, const double* y, int ny, int m, const double* xs0,
                         const double* xs1, double res, int sz, double* f_star, double* v_star, double* alpha_out, double* log_ev,
                         int32_t* best, double* log_ev_all, int32_t* status)
{
    return gauss_run_dev(ctx, GaussCall{params, true, H, cand, P, off, n_max, n_total, x0, x1, y, ny, m, xs0, xs1, res, sz,
                                        f_star, v_star, alpha_out, status, log_ev, best, log_ev_all});
}

int gpc_dense_select(gpc_ctx* ctx, const gpc_params* params, int H, const gpc_hyper* cand, int P, const int32_t* off, const double* x0,
                     const double* x1, const double* y, int ny, int m, const double* xs0, const double* xs1, double res, int sz,
                     double* f_star, double* v_star, double* alpha_out, double* log_ev, int32_t* best, double* log_ev_all, int32_t* status)
{
    return gauss_run_host(ctx, "gpc_dense_select",
                          GaussCall{params, true, H, cand, P, off, 0, 0, x0, x1, y, ny, m, xs0, xs1, res, sz,
                                    f_star, v_star, alpha_out, status, log_ev, best, log_ev_all});
}

}  // extern "C"
