// dense_internal.h -- host-side definitions of the dense path: the arguments of a batch, where a call runs, the dispatcher and the
// launchers of the kernel translation units (not part of the C-ABI).  Which kernel a batch runs on is decided in dense_route.h; the
// dispatcher executes that route and every launcher takes its shape from it.
#pragma once

#include "gpc_internal.h"
#include "dense_route.h"

struct DenseArgs {
    gpc_params prm;
    int P, n_max, n_total, ny, m;
    const int32_t* off;
    const double *x0, *x1, *y;
    const double *xs0, *xs1;   // point-wise X* (m entries) or nullptr when the grid form is used
    double grid_res;           // grid form: res, sz (m = sz*sz)
    int grid_sz;
    double *f_star, *v_star, *alpha_out;
    int32_t* status;
    // size-class dispatch of a ragged batch (dense_api.hip): when sel != nullptr a kernel works on the patches sel[0 .. *sel_count)
    // (both on the device) instead of 0 .. P-1
    const int32_t* sel;
    const int32_t* sel_count;
    int sel_base;              // generic kernel only: it works on sel[sel_base .. *sel_count) -- the overflow launch behind a class launch that
                               // was sized from a host-side hint (dense_api.hip)
    // gpc_dense_fit_predict_ev (include/gpc.h): the log marginal likelihood [P][ny], or nullptr.  A call that asks for it takes the
    // variance route (dense_facts) with the factor export on, and needs status and alpha_out (dense_ev_api.hip supplies temporaries)
    double* log_ev;
};

// Where a dense call runs.  A host-side value handed from the dispatcher to the launchers, never part of a kernel-parameter struct.
struct DenseSite {
    hipStream_t stream;     // every launch, memset and event record of the call in hand
    size_t ws_off, ws_len;  // the region of ctx->ws it may use; ws_len == 0: the whole workspace, not a chunk of the host-pointer pipeline
    int w1_cap = 0;         // one-wave route: the factor slots the caller's own dense_reserve settled on (0: the route's)
};

// a call on the context's stream that may use the whole workspace (caller holds ctx->mu)
static inline DenseSite dense_site_of(const gpc_ctx* ctx) { return DenseSite{ctx->stream, 0, 0}; }
// the site's region of the workspace; ask AFTER the reserve, which may move ctx->ws
static inline char* dense_ws(const gpc_ctx* ctx, const DenseSite& site) { return static_cast<char*>(ctx->ws) + site.ws_off; }
// ... and how much of it the workspace holds as it stands
static inline size_t dense_ws_len(const gpc_ctx* ctx, const DenseSite& site)
{
    const size_t rest = ctx->ws_bytes > site.ws_off ? ctx->ws_bytes - site.ws_off : 0;
    return site.ws_len && site.ws_len < rest ? site.ws_len : rest;
}
// `bytes` within the site's region
static inline int gpc_ws_reserve(gpc_ctx* ctx, const DenseSite& site, size_t bytes)
{
    return gpc_ws_reserve(ctx, site.stream, site.ws_len != 0, site.ws_off + bytes);
}
// GPC_POISON_LDS for a dense call: launched on the site's stream, and only the site's region of the workspace is filled
int gpc_debug_poison_lds(gpc_ctx* ctx, const DenseSite& site);

// Regions of the workspace, one behind the other, each rounded up to 256 bytes; take() answers the region's byte offset (pointers are
// formed after the reserve, which may move the workspace).
struct WsCarve {
    size_t bytes = 0;
    template <class T> size_t take(size_t count)
    {
        const size_t at = bytes;
        bytes += (sizeof(T) * count + 255) & ~(size_t)255;
        return at;
    }
};
template <class T> static inline T* ws_at(char* ws, size_t off) { return reinterpret_cast<T*>(ws + off); }

// ---- dispatcher (dense_api.hip), also used by the host-pointer pipeline (dense_host.hip); the argument check and dense_args also by
// ---- the probit / IRLS entries (dense_irls_api.hip) ------------------------------------------------------------

int dense_check(gpc_ctx* ctx, const gpc_params* prm, int P, const void* off, int n_max, int n_total,
                const void* x0, const void* x1, const void* y, int ny, int m, const void* f_star);
// the device-pointer arguments shared by the dense and IRLS entries; the rest of DenseArgs stays zero
DenseArgs dense_args(const gpc_params* prm, int P, const int32_t* off, int n_max, int n_total, const double* x0, const double* x1,
                     const double* y, int ny, int m, double* f_star, double* alpha_out, int32_t* status);
// what dense_route looks at, of a batch as its entry point received it
static inline DenseFacts dense_facts(const gpc_ctx* ctx, const DenseArgs& a, bool irls = false)
{
    return DenseFacts{a.P, a.n_max, a.n_total, a.ny, a.m, (a.prm.want_variance && a.v_star) || a.log_ev, a.xs0 != nullptr,
                      a.alpha_out != nullptr, ctx->num_cus, irls};
}
// Asks dense_route for the kernels of a batch and launches them at `site`; caller holds ctx->mu.  `seen_gen`: a chunk of the two-stream
// host-pointer pipeline hands in gpc_ctx::foreign_gen as its compute stream last saw it (gpc_pipe_chunk_order); nullptr everywhere else.
int dense_dispatch(gpc_ctx* ctx, DenseArgs& a, const DenseSite& site, unsigned* seen_gen = nullptr);
// `front` bytes of the caller's own plus everything the dispatch of `a` (a batch of the variance route) will reserve behind them, in one
// step.  *w1_cap: what the dispatch must find in its DenseSite::w1_cap.  The entries that keep temporaries in the workspace across a
// dispatch (dense_ev_api.hip) call it first.  It asks the same byte functions as the dispatcher and the launchers (dense_w1_ws_bytes,
// dense_mfma_ws_bytes, dense_big_ws_bytes, dense_generic_ws_bytes): a launcher that reserves anything else must say so here too.
int dense_reserve(gpc_ctx* ctx, const DenseSite& site, size_t front, const DenseArgs& a, int* w1_cap);

// ---- launchers implemented in the kernel translation units -------------------------------------------------

// generic kernel: any n <= GPC_MAX_POINTS, K/L in a global-memory workspace slot per workgroup
size_t dense_generic_ws_bytes(const gpc_ctx* ctx, const DenseArgs& a, int* grid_out);
int dense_generic_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, int grid, double* ws_override = nullptr);

// register-tile MFMA kernel: n <= 256, trailing matrix resident in VGPRs (see dense_mfma.hip)
// (what its launcher reserves with the factor export on -- v_star or log_ev wanted --, else 0)
size_t dense_mfma_ws_bytes(const DenseArgs& a, const DenseRoute& r);
int dense_mfma_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, const DenseRoute& r);

// predictive variance from the exported factor of the register-tile kernel (dense_variance.hip): V* [P][m]
// (var_w4: DenseSwitches::var_w4)
int dense_variance_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, int nt_max, int var_w4, const double* factor,
                          const double* alpha, double* v_star);

// ... and from the tiled kernel's per-patch factor slots (n <= 1024); scratch: V blocks of the waves in flight
size_t big_slot_doubles(int ntw);
size_t dense_variance_big_scratch_doubles(const gpc_ctx* ctx, int ntw);
int dense_variance_big_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, int ntw, const double* ws, size_t slot,
                              const double* alpha, double* scratch, double* v_star);

// ... and of the probit GP (row-scaled: v* = sigma_f^2 - |L^-1 (s o k*)|^2, L the factor of B = I + diag(s) K diag(s) that the IRLS
// instances exported, any n <= 1024); v_star or p_star (the occupancy probability) may be nullptr
int dense_variance_big_scaled_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, int ntw, const double* ws, size_t slot,
                                     const double* alpha, const double* s, double* scratch, double* v_star, double* p_star);
// the sz x sz grid of load_compressed as sz sz points (cell p = y sz + x) in xs0, xs1 on the device
int dense_grid_points_launch(gpc_ctx* ctx, const DenseSite& site, double res, int sz, double* xs0, double* xs1);

// the Laplace evidence log q(y | X, theta) of the probit GP from what such a fit left behind (dense_evidence.hip; definition:
// include/gpc.h): a, fhat, the labels a.y, the fit's status a.status and the L_kk^-1 images of the slots; log_q [P]
int dense_evidence_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, int ntw, const double* ws, size_t slot,
                          const double* alpha, const double* fhat, double* log_q);
// The log marginal likelihood of the regression GP from what a fit with the export on left behind (dense_evidence.hip; definition:
// include/gpc.h, gpc_dense_fit_predict_ev): y, alpha, the fit's status a.status and the diagonals of the L_kk^-1 images; log_ev [P][ny].
// The factor is in one of two layouts: tri_nt > 0: [P][tri_nt (tri_nt + 1) / 2] images, the lower triangle the register and the one-wave
// kernel export (image k (k + 1) / 2 + k is L_kk^-1); tri_nt == 0: the tiled kernel's slots of `slot` doubles (ntw tile columns).
int dense_gauss_evidence_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, int tri_nt, int ntw, const double* ws, size_t slot,
                                const double* alpha, double* log_ev);
// ... and the keep-best step of gpc_dense_select: candidate h's rows go from `cand` to `out` where it wins the patch by the sum of its
// planes' log_ev.  Any pointer of `out` may be nullptr; cur_best, cur_ev [P] hold the state between the candidates.
struct GaussRows {
    double *f;                // [P][ny][m]
    double *v;                // [P][m]
    double *alpha;            // [ny][n_total]
    double *log_ev;           // [P][ny]
    int32_t *status;          // [P]
};
int dense_gauss_keep_launch(gpc_ctx* ctx, const DenseSite& site, int h, int P, int ny, int m, int n_total, const int32_t* off,
                            const GaussRows& cand, const GaussRows& out, int32_t* best, double* log_ev_all_h, int32_t* cur_best,
                            double* cur_ev);
// One candidate's outputs (gpc_dense_irls_select, include/gpc.h) and the keep-best step behind it: where candidate h wins a patch its rows
// are copied from `cand` to `out`.  Any pointer of `out` may be nullptr; cur_best, cur_lq [P] hold the state between the candidates.
struct SelectRows {
    double *f, *v, *p;        // [P][m]
    double *alpha, *fhat;     // [n_total]
    double* log_q;            // [P]
    int32_t *iters, *status;  // [P]
};
int dense_select_keep_launch(gpc_ctx* ctx, const DenseSite& site, int h, int P, int m, const int32_t* off, const SelectRows& cand,
                             const SelectRows& out, int32_t* best, double* log_q_all_h, int32_t* cur_best, double* cur_lq);

// tiled left-looking MFMA kernel: 256 < n <= 1024, factor in a global-memory workspace slot per workgroup (see dense_mfma_big.hip)
size_t dense_big_ws_bytes(const gpc_ctx* ctx, const DenseArgs& a, const DenseRoute& r, int* grid_out);
int dense_big_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, const DenseRoute& r, int grid);
// one wave per patch, eight patches per CU: n <= 256, depth plane, mean only (see dense_mfma_w1.hip) -- the C2 headline kernel
// (cap > 0: fewer factor slots than the route's, the dispatcher's retry after GPC_ENOMEM)
size_t dense_w1_ws_bytes(const DenseFacts& f, const DenseRoute& r, int* grid_out, int cap = 0);
int dense_w1_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, const DenseRoute& r, int grid);
// the same kernel inside the Newton / IRLS loop of the probit variant (BASELINE config 5; any n <= 1024, ny == 1)
struct IrlsArgs {
    int max_iter;
    double tol, f_init;
    int32_t* iters;   // [P] or nullptr
    double* fhat;     // [n_total] or nullptr
    double* s_out;    // [n_total]: W^1/2 of the last solve, written when the route exports the factor (DenseRoute::export_factor)
};
int dense_irls_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, const DenseRoute& r, const IrlsArgs& ir, int grid);
