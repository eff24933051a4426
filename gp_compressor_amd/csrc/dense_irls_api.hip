// dense_irls_api.hip -- the eight probit / IRLS entries of the C-ABI (BASELINE config 5; definitions: include/gpc.h): the plain fit, its
// _var and _ev forms and the selection among candidates, each on host and on device pointers.  Every entry fills one record (IrlsCall)
// and hands it to irls_run_host or irls_run_dev; there is one list of argument rules (irls_rules), one staging list (irls_run_host)
// and one place that chooses what a call launches (irls_run_dev).  The kernels and their launchers are in dense_mfma_big.hip,
// dense_variance.hip and dense_evidence.hip; which instance a batch runs on is dense_route's answer (dense_route.h).
#include "dense_internal.h"

// What any of the eight entries received.  Host form: every pointer but params, irls and cand is a host pointer, and n_max, n_total are
// found from off (irls_rules).
struct IrlsCall {
    const gpc_params* params;
    const gpc_irls_params* irls;
    bool select;              // gpc_dense_irls_select[_dev]: H candidates at cand (host memory in both forms)
    int H;
    const gpc_hyper* cand;
    int P;
    const int32_t* off;
    int n_max, n_total;
    const double *x0, *x1, *y;
    int m;                    // point-wise X*: as given; grid form (xs0 == nullptr): sz sz once irls_rules has run
    const double *xs0, *xs1;
    double res;
    int sz;
    double *f_star, *v_star, *p_star, *alpha_out, *fhat_out, *log_q;
    int32_t* best;
    double* log_q_all;
    int32_t *iters, *status;
};

// The argument rules of every entry, in the order include/gpc.h states them, and the record made ready for the run: m = sz sz in the
// grid form, n_max >= 1; host form: n_max and n_total from off.  GPC_OK with c.P == 0: the call is valid and there is nothing to do.
static int irls_rules(gpc_ctx* ctx, IrlsCall& c, bool host)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!c.params) return gpc_fail(ctx, GPC_EINVAL, "params is NULL");
    if (c.select) {
        if (c.H < 1 || !c.cand) return gpc_fail(ctx, GPC_EINVAL, "select needs H >= 1 candidates");
        if (c.params->noise_model != 2) return gpc_fail(ctx, GPC_EINVAL, "select needs noise_model 2, got %d", c.params->noise_model);
        for (int h = 0; h < c.H; ++h) {
            const double v[3] = {c.cand[h].sigmaf_sq, c.cand[h].l_sq, c.cand[h].noise};
            for (double x : v)
                if (!(x > 0.0) || !(x - x == 0.0)) return gpc_fail(ctx, GPC_EINVAL, "candidate %d has a non-positive or non-finite field", h);
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
    if ((rc = dense_check(ctx, c.params, c.P, c.off, c.n_max, c.n_total, c.x0, c.x1, c.y, 1, c.select ? 0 : c.m, c.f_star))) return rc;
    if (c.m < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (c.n_max < 1) c.n_max = 1;
    if (!c.irls) return gpc_fail(ctx, GPC_EINVAL, "irls is NULL");
    if (c.params->noise_model != 1 && c.params->noise_model != 2)
        return gpc_fail(ctx, GPC_EINVAL, "the IRLS loop needs a probit noise_model (1 or 2), got %d", c.params->noise_model);
    if ((c.p_star || c.log_q) && c.params->noise_model != 2)
        return gpc_fail(ctx, GPC_EINVAL, "%s needs noise_model 2: the \"Phi\" of model 1 is not a probability", c.p_star ? "p_star" : "log_q");
    if (c.irls->max_iter < 1 || !(c.irls->tol >= 0.0) || !(c.irls->f_init == c.irls->f_init))
        return gpc_fail(ctx, GPC_EINVAL, "irls parameters out of range");
    if (!(c.params->noise > 0.0)) return gpc_fail(ctx, GPC_EINVAL, "s20 (params->noise) must be positive");
    if (!grid && c.m > 0 && !c.xs1) return gpc_fail(ctx, GPC_EINVAL, "xs1 is NULL");
    return GPC_OK;
}

// The workspace of one fit.  Plain: a factor slot per workgroup.  With the export: a factor slot per patch | a (when the caller does not
// take it) | s of the last solve | the variance kernel's per-wave V scratch | the grid as points | the status (when the caller does not
// take it) | with the evidence wanted: fhat (when the caller does not take it)
struct IrlsFitWs {
    size_t slot, o_al, o_s, o_scr, o_xs, o_st, o_fh, bytes;
};
static IrlsFitWs irls_fit_ws(const gpc_ctx* ctx, const IrlsCall& c, bool exported, bool evidence, int workgroups)
{
    const int ntw = (c.n_max + 15) / 16;
    const size_t N = (size_t)c.n_total;
    IrlsFitWs w{};
    WsCarve cv;
    w.slot = big_slot_doubles(ntw);
    cv.take<double>(w.slot * (size_t)(exported ? c.P : workgroups));
    if (exported) {
        w.o_al = cv.take<double>(N);
        w.o_s = cv.take<double>(N);
        w.o_scr = cv.take<double>(dense_variance_big_scratch_doubles(ctx, ntw));
        w.o_xs = cv.take<double>(2 * (size_t)c.m);
        w.o_st = cv.take<int32_t>((size_t)c.P);
        w.o_fh = cv.take<double>(evidence ? N : 0);
    }
    w.bytes = cv.bytes;
    return w;
}

// what dense_route looks at for a fit: the batch as dense_facts sees it; with the export on, the variance path on point-wise X* (the grid
// is evaluated as points) over all m points, and the weights as the caller wants them, whatever the fit itself is handed
static DenseFacts irls_facts(const gpc_ctx* ctx, const DenseArgs& a, const IrlsCall& c, bool exported)
{
    DenseFacts f = dense_facts(ctx, a, true);
    if (exported) {
        f.m = c.m;
        f.variance = f.pointwise = true;
        f.alpha_out = c.alpha_out != nullptr;
    }
    return f;
}

// One fit at `site`.  Plain: the loop and the fit's own prediction of f*.  With the export on: the factor of the last solve is kept, the
// variance kernel follows when there is a v* or p* to write and the evidence read-out when log_q is wanted.  Record checked (irls_rules),
// P > 0; caller holds ctx->mu.
static int irls_fit(gpc_ctx* ctx, const DenseSite& site, const IrlsCall& c, bool exported)
{
    const bool grid = (c.xs0 == nullptr);
    // nothing for the variance kernel to write (the evidence alone, or with the mean): the fit predicts f* itself, as in the plain level
    const bool var = exported && (c.v_star || c.p_star) && c.m > 0;
    int rc;
    if (int rcp = gpc_debug_poison_lds(ctx, site)) return rcp;
    // with the variance the fit predicts nothing: the variance kernel forms the mean from the K* tiles it evaluates anyway
    DenseArgs a = dense_args(c.params, c.P, c.off, c.n_max, c.n_total, c.x0, c.x1, c.y, 1, var ? 0 : c.m, c.f_star, c.alpha_out, c.status);
    a.prm.want_variance = 0;
    const DenseRoute route = dense_route(irls_facts(ctx, a, c, exported), dense_switches_read());
    const int cap = ctx->num_cus * route.per_cu, workgroups = c.P < cap ? c.P : cap;
    const IrlsFitWs w = irls_fit_ws(ctx, c, exported, c.log_q != nullptr, workgroups);
    if ((rc = gpc_ws_reserve(ctx, site, w.bytes))) return rc;
    char* ws = dense_ws(ctx, site);
    IrlsArgs ir{c.irls->max_iter, c.irls->tol, c.irls->f_init, c.iters, c.fhat_out, nullptr};
    double* d_xs = ws_at<double>(ws, w.o_xs);
    if (exported) {
        if (!a.alpha_out) a.alpha_out = ws_at<double>(ws, w.o_al);
        if (!a.status) a.status = ws_at<int32_t>(ws, w.o_st);
        if (!ir.fhat && c.log_q) ir.fhat = ws_at<double>(ws, w.o_fh);
        ir.s_out = ws_at<double>(ws, w.o_s);
    }
    if (var) {
        if (grid && (rc = dense_grid_points_launch(ctx, site, c.res, c.sz, d_xs, d_xs + c.m))) return rc;
        a.xs0 = grid ? d_xs : c.xs0; a.xs1 = grid ? d_xs + c.m : c.xs1;
    } else {
        a.xs0 = c.xs0; a.xs1 = c.xs1;
        a.grid_res = grid ? c.res : 0.0; a.grid_sz = grid ? c.sz : 0;
    }
    if ((rc = dense_irls_launch(ctx, site, a, route, ir, workgroups))) return rc;
    const int ntw = (c.n_max + 15) / 16;
    const double* slots = reinterpret_cast<const double*>(ws);
    if (var) {
        a.m = c.m;
        if ((rc = dense_variance_big_scaled_launch(ctx, site, a, ntw, slots, w.slot, a.alpha_out, ir.s_out, ws_at<double>(ws, w.o_scr),
                                                   c.v_star, c.p_star)))
            return rc;
    }
    if (c.log_q && (rc = dense_evidence_launch(ctx, site, a, ntw, slots, w.slot, a.alpha_out, ir.fhat, c.log_q))) return rc;
    ctx->last_dense_kernel = route.name;
    return GPC_OK;
}

// The selection loop: every candidate is an export fit into temporaries, and the keep-best step behind it copies the rows of the patches
// it won so far into the caller's outputs.  The workspace: the temporaries of one candidate and the state of the keep-best step in
// front, the fit's region behind them.
static int irls_select(gpc_ctx* ctx, const DenseSite& whole, const IrlsCall& c)
{
    const size_t Pz = (size_t)c.P, Pm = Pz * (size_t)c.m, N = (size_t)c.n_total;
    WsCarve cv;
    const size_t o_f = cv.take<double>(Pm), o_v = cv.take<double>(Pm), o_p = cv.take<double>(Pm), o_al = cv.take<double>(N),
                 o_fh = cv.take<double>(N), o_lq = cv.take<double>(Pz), o_cur_lq = cv.take<double>(Pz), o_it = cv.take<int32_t>(Pz),
                 o_st = cv.take<int32_t>(Pz), o_cur_best = cv.take<int32_t>(Pz);
    const DenseSite site{whole.stream, whole.ws_off + cv.bytes, 0};
    int rc;
    if ((rc = gpc_ws_reserve(ctx, whole, cv.bytes + irls_fit_ws(ctx, c, true, true, 0).bytes))) return rc;
    char* t = dense_ws(ctx, whole);
    const SelectRows tmp{ws_at<double>(t, o_f), c.v_star ? ws_at<double>(t, o_v) : nullptr, c.p_star ? ws_at<double>(t, o_p) : nullptr,
                         ws_at<double>(t, o_al), ws_at<double>(t, o_fh), ws_at<double>(t, o_lq), ws_at<int32_t>(t, o_it), ws_at<int32_t>(t, o_st)};
    const SelectRows out{c.f_star, c.v_star, c.p_star, c.alpha_out, c.fhat_out, c.log_q, c.iters, c.status};
    gpc_params prm = *c.params;
    IrlsCall k = c;                // one candidate: the _ev level on prm, into the temporaries
    k.select = false;
    k.params = &prm;
    k.best = nullptr; k.log_q_all = nullptr;
    k.f_star = tmp.f; k.v_star = tmp.v; k.p_star = tmp.p; k.alpha_out = tmp.alpha; k.fhat_out = tmp.fhat; k.log_q = tmp.log_q;
    k.iters = tmp.iters; k.status = tmp.status;
    for (int h = 0; h < c.H; ++h) {
        prm.sigmaf_sq = c.cand[h].sigmaf_sq; prm.l_sq = c.cand[h].l_sq; prm.noise = c.cand[h].noise;
        if ((rc = irls_fit(ctx, site, k, true))) return rc;
        if ((rc = dense_select_keep_launch(ctx, whole, h, c.P, c.m, c.off, tmp, out, c.best, c.log_q_all ? c.log_q_all + (size_t)h * Pz : nullptr,
                                           ws_at<int32_t>(t, o_cur_best), ws_at<double>(t, o_cur_lq))))
            return rc;
    }
    return GPC_OK;
}

// The device-pointer run of a record, and the one place that chooses its level: the selection loop; the export fit when the evidence is
// wanted or there is a v* or p* to write; else the plain fit -- same launches, same bits whichever entry the call came through.
static int irls_run_dev(gpc_ctx* ctx, IrlsCall c)
{
    const int rc = irls_rules(ctx, c, false);
    if (rc != GPC_OK || c.P == 0) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const DenseSite site = dense_site_of(ctx);
    if (c.select) return irls_select(ctx, site, c);
    return irls_fit(ctx, site, c, c.log_q || ((c.v_star || c.p_star) && c.m > 0));
}

// The host-pointer run: every input and every output the record asks for is staged, the device-pointer run does the work.  alpha, fhat,
// iters and status are staged whether the caller takes them or not (as are f*, and log_q, best under select); v*, p* and log_q_all only
// when requested.
static int irls_run_host(gpc_ctx* ctx, const char* entry, IrlsCall c)
{
    const int rc = irls_rules(ctx, c, true);
    if (rc != GPC_OK || c.P == 0) return rc;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const bool grid = (c.xs0 == nullptr);
    const size_t N = (size_t)c.n_total, Pz = (size_t)c.P, Pm = Pz * (size_t)c.m, HP = (size_t)c.H * Pz;
    GpcStaging st(ctx, entry);
    IrlsCall d = c;
    d.off = st.up(c.off, Pz + 1);
    d.x0 = st.up(c.x0, N); d.x1 = st.up(c.x1, N); d.y = st.up(c.y, N);
    d.xs0 = grid ? nullptr : st.up(c.xs0, (size_t)c.m); d.xs1 = grid ? nullptr : st.up(c.xs1, (size_t)c.m);
    d.f_star = st.out<double>(Pm); d.alpha_out = st.out<double>(N); d.fhat_out = st.out<double>(N);
    d.log_q = c.log_q || c.select ? st.out<double>(Pz) : nullptr;
    d.v_star = c.v_star ? st.out<double>(Pm) : nullptr; d.p_star = c.p_star ? st.out<double>(Pm) : nullptr;
    d.iters = st.out<int32_t>(Pz); d.status = st.out<int32_t>(Pz);
    d.best = c.select ? st.out<int32_t>(Pz) : nullptr;
    d.log_q_all = c.select && c.log_q_all ? st.out<double>(HP) : nullptr;
    if (st.ok()) st.rc = irls_run_dev(ctx, d);
    st.down(c.f_star, d.f_star, Pm);
    st.down(c.v_star, d.v_star, Pm);
    st.down(c.p_star, d.p_star, Pm);
    st.down(c.alpha_out, d.alpha_out, N);
    st.down(c.fhat_out, d.fhat_out, N);
    st.down(c.log_q, d.log_q, Pz);
    st.down(c.best, d.best, Pz);
    st.down(c.log_q_all, d.log_q_all, HP);
    st.down(c.iters, d.iters, Pz);
    st.down(c.status, d.status, Pz);
    return st.finish();
}

extern "C" {

int gpc_dense_irls_fit_predict_dev(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                                   int n_max, int n_total, const double* x0, const double* x1, const double* y, int m,
                                   const double* xs0, const double* xs1, double res, int sz, double* f_star, double* alpha_out,
                                   double* fhat_out, int32_t* iters, int32_t* status)
{
    return irls_run_dev(ctx, IrlsCall{params, irls, false, 0, nullptr, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz,
                                      f_star, nullptr, nullptr, alpha_out, fhat_out, nullptr, nullptr, nullptr, iters, status});
}

int gpc_dense_irls_fit_predict(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                               const double* x0, const double* x1, const double* y, int m, const double* xs0, const double* xs1,
                               double res, int sz, double* f_star, double* alpha_out, double* fhat_out, int32_t* iters,
                               int32_t* status)
{
    return irls_run_host(ctx, "gpc_dense_irls_fit_predict",
                         IrlsCall{params, irls, false, 0, nullptr, P, off, 0, 0, x0, x1, y, m, xs0, xs1, res, sz,
                                  f_star, nullptr, nullptr, alpha_out, fhat_out, nullptr, nullptr, nullptr, iters, status});
}

int gpc_dense_irls_fit_predict_var_dev(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                                       int n_max, int n_total, const double* x0, const double* x1, const double* y, int m,
                                       const double* xs0, const double* xs1, double res, int sz, double* f_star, double* v_star,
                                       double* p_star, double* alpha_out, double* fhat_out, int32_t* iters, int32_t* status)
{
    return irls_run_dev(ctx, IrlsCall{params, irls, false, 0, nullptr, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz,
                                      f_star, v_star, p_star, alpha_out, fhat_out, nullptr, nullptr, nullptr, iters, status});
}

int gpc_dense_irls_fit_predict_var(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                                   const double* x0, const double* x1, const double* y, int m, const double* xs0, const double* xs1,
                                   double res, int sz, double* f_star, double* v_star, double* p_star, double* alpha_out,
                                   double* fhat_out, int32_t* iters, int32_t* status)
{
    return irls_run_host(ctx, "gpc_dense_irls_fit_predict_var",
                         IrlsCall{params, irls, false, 0, nullptr, P, off, 0, 0, x0, x1, y, m, xs0, xs1, res, sz,
                                  f_star, v_star, p_star, alpha_out, fhat_out, nullptr, nullptr, nullptr, iters, status});
}

int gpc_dense_irls_fit_predict_ev_dev(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                                      int n_max, int n_total, const double* x0, const double* x1, const double* y, int m,
                                      const double* xs0, const double* xs1, double res, int sz, double* f_star, double* v_star,
                                      double* p_star, double* alpha_out, double* fhat_out, int32_t* iters, int32_t* status, double* log_q)
{
    return irls_run_dev(ctx, IrlsCall{params, irls, false, 0, nullptr, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz,
                                      f_star, v_star, p_star, alpha_out, fhat_out, log_q, nullptr, nullptr, iters, status});
}

int gpc_dense_irls_fit_predict_ev(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                                  const double* x0, const double* x1, const double* y, int m, const double* xs0, const double* xs1,
                                  double res, int sz, double* f_star, double* v_star, double* p_star, double* alpha_out,
                                  double* fhat_out, int32_t* iters, int32_t* status, double* log_q)
{
    return irls_run_host(ctx, "gpc_dense_irls_fit_predict_ev",
                         IrlsCall{params, irls, false, 0, nullptr, P, off, 0, 0, x0, x1, y, m, xs0, xs1, res, sz,
                                  f_star, v_star, p_star, alpha_out, fhat_out, log_q, nullptr, nullptr, iters, status});
}

int gpc_dense_irls_select_dev(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int H, const gpc_hyper* cand, int P,
                              const int32_t* off, int n_max, int n_total, const double* x0, const double* x1, const double* y, int m,
                              const double* xs0, const double* xs1, double res, int sz, double* f_star, double* v_star,
                              double* p_star, double* alpha_out, double* fhat_out, double* log_q, int32_t* best, double* log_q_all,
                              int32_t* iters, int32_t* status)
{
    return irls_run_dev(ctx, IrlsCall{params, irls, true, H, cand, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz,
                                      f_star, v_star, p_star, alpha_out, fhat_out, log_q, best, log_q_all, iters, status});
}

int gpc_dense_irls_select(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int H, const gpc_hyper* cand, int P,
                          const int32_t* off, const double* x0, const double* x1, const double* y, int m, const double* xs0,
                          const double* xs1, double res, int sz, double* f_star, double* v_star, double* p_star, double* alpha_out,
                          double* fhat_out, double* log_q, int32_t* best, double* log_q_all, int32_t* iters, int32_t* status)
{
    return irls_run_host(ctx, "gpc_dense_irls_select",
                         IrlsCall{params, irls, true, H, cand, P, off, 0, 0, x0, x1, y, m, xs0, xs1, res, sz,
                                  f_star, v_star, p_star, alpha_out, fhat_out, log_q, best, log_q_all, iters, status});
}

}  // extern "C"
