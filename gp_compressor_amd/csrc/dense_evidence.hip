// dense_evidence.hip -- model selection for the probit occupancy GP: the Laplace approximation of the log marginal likelihood read
// out of a finished fit, and the keep-best step of the loop over candidate hyper-parameters (definitions: include/gpc.h,
// gpc_dense_irls_fit_predict_ev and gpc_dense_irls_select).  Behind them, in the second half of the file, the same pair for the
// regression GP (gpc_dense_fit_predict_ev and gpc_dense_select): the exact log marginal likelihood from the factor the Gaussian fits export.
//
// Rasmussen & Williams 2006, Alg. 3.1 line 10 (eq. 3.32):
//     log q(y | X, theta) = -1/2 a^T fhat + sum_i log p(y_i | fhat_i) - sum_j log L_jj
// Everything in it is on the device after the IRLS instances of the tiled kernel ran with the factor export on (dense_mfma_big.hip):
// a and fhat are outputs, L is the factor of B = I + diag(s) K diag(s) of the last solve, and the slot of a patch keeps the L_kk^-1
// images behind its tiles, whose diagonals are 1 / L_jj.  The read-out re-runs nothing: 4 n doubles per patch (a, fhat, y, one diagonal
// element per point), one wave per patch, and no atomics -- lane l sums its points l, l + 64, ... in that order, then a fixed shuffle tree
// adds the 64 partial sums, so two calls give the same bits.
#include "gpc_device.h"
#include "dense_internal.h"
#include "mfma_tile.h"

#define EV_THREADS 256
#define EV_WAVES (EV_THREADS / 64)

struct EvParams {
    int P, ntw;
    size_t slot;              // doubles per factor slot (big_slot_doubles(ntw))
    double s20;
    const int32_t* off;       // [P + 1]
    const int32_t* status;    // [P]: the fit's
    const double *alpha, *fhat, *y;   // [n_total]
    const double* ws;         // [P][slot]
    double* log_q;            // [P]
};

// (ev_wave_sum, the one order of every sum here: gpc_device.h)

__global__ __launch_bounds__(EV_THREADS) void dense_evidence_kernel(EvParams g)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double sigma = sqrt(g.s20);                    // the functor's sigma at sigma_x = 0 (gpc_probit_q_r)
    for (int patch = blockIdx.x * EV_WAVES + wave; patch < g.P; patch += gridDim.x * EV_WAVES) {
        const int o = g.off[patch], n = g.off[patch + 1] - o;
        const int st = g.status[patch];
        if (n <= 0 || n > MF_TS * g.ntw || (st != GPC_STATUS_OK && st != GPC_STATUS_NOT_CONVERGED)) {
            if (lane == 0) g.log_q[patch] = (n == 0) ? 0.0 : __builtin_nan("");
            continue;
        }
        // the L_kk^-1 images sit behind the (ntw + 1) ntw tiles and the ntw L_kk^-T images of the slot
        const double* linv = g.ws + (size_t)patch * g.slot + ((size_t)(g.ntw + 1) * g.ntw + g.ntw) * MF_IMG;
        double quad = 0.0, lik = 0.0, ldet = 0.0;
        for (int j = lane; j < n; j += 64) {           // (rows j >= n of the last tile are padding)
            const double f = g.fhat[o + j];
            quad = __builtin_fma(g.alpha[o + j], f, quad);
            lik += log(gpc_probit_ef(GPC_NOISE_PROBIT_STD, g.y[o + j] * f / sigma));
            const int r = j & (MF_TS - 1);
            ldet += log(linv[(size_t)(j / MF_TS) * MF_IMG + mf_img_rc(r, r)]);      // = -log L_jj
        }
        quad = ev_wave_sum(quad);
        lik = ev_wave_sum(lik);
        ldet = ev_wave_sum(ldet);
        if (lane == 0) g.log_q[patch] = (-0.5 * quad + lik) + ldet;
    }
}

int dense_evidence_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, int ntw, const double* ws, size_t slot,
                          const double* alpha, const double* fhat, double* log_q)
{
    if (a.P == 0) return GPC_OK;
    if (!a.status || !alpha || !fhat || !log_q) return gpc_fail(ctx, GPC_EINVAL, "the evidence read-out needs the fit's status, a and fhat");
    EvParams g;
    g.P = a.P; g.ntw = ntw; g.slot = slot; g.s20 = a.prm.noise;
    g.off = a.off; g.status = a.status; g.alpha = alpha; g.fhat = fhat; g.y = a.y; g.ws = ws; g.log_q = log_q;
    const int need = (a.P + EV_WAVES - 1) / EV_WAVES, cap = ctx->num_cus * 8;
    hipLaunchKernelGGL(dense_evidence_kernel, dim3(need < cap ? need : cap), dim3(EV_THREADS), 0, site.stream, g);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}

// ---- gpc_dense_irls_select: keep the best candidate so far ----------------------------------------------------------------------
// One workgroup per patch at a time.  Candidate h is eligible iff its status is GPC_STATUS_OK and its log_q is finite; it takes the patch
// iff no candidate holds it yet or its log_q is strictly greater (ties stay with the lower index, NaN never wins).  Candidate 0 also
// lays down what a patch without any eligible candidate keeps: best = -1, NaN rows, its own iters and status.
struct KeepParams {
    int h, P, m;
    const int32_t* off;
    SelectRows cand, out;
    int32_t* best;            // [P] or nullptr
    double* log_q_all_h;      // [P] (row h of log_q_all) or nullptr
    int32_t* cur_best;        // [P]
    double* cur_lq;           // [P]
};

__global__ __launch_bounds__(EV_THREADS) void dense_select_keep_kernel(KeepParams g)
{
    const int tid = threadIdx.x;
    for (int patch = blockIdx.x; patch < g.P; patch += gridDim.x) {
        const double lq = g.cand.log_q[patch];
        const int st = g.cand.status[patch];
        const int held = g.h == 0 ? -1 : g.cur_best[patch];
        const double held_lq = g.h == 0 ? 0.0 : g.cur_lq[patch];
        __syncthreads();                                    // every thread has read the state before thread 0 replaces it
        if (tid == 0 && g.log_q_all_h) g.log_q_all_h[patch] = lq;
        const bool eligible = st == GPC_STATUS_OK && __builtin_isfinite(lq);
        const bool win = eligible && (held < 0 || lq > held_lq);
        if (!win && g.h != 0) continue;
        // candidate 0 without a win: the rows of "no eligible candidate"
        const double nan = __builtin_nan("");
        const int o = g.off[patch], n = g.off[patch + 1] - o;
        const size_t pm = (size_t)patch * g.m;
        for (int q = tid; q < g.m; q += EV_THREADS) {
            if (g.out.f) g.out.f[pm + q] = win ? g.cand.f[pm + q] : nan;
            if (g.out.v) g.out.v[pm + q] = win ? g.cand.v[pm + q] : nan;
            if (g.out.p) g.out.p[pm + q] = win ? g.cand.p[pm + q] : nan;
        }
        for (int j = tid; j < n; j += EV_THREADS) {
            if (g.out.alpha) g.out.alpha[o + j] = win ? g.cand.alpha[o + j] : nan;
            if (g.out.fhat) g.out.fhat[o + j] = win ? g.cand.fhat[o + j] : nan;
        }
        if (tid == 0) {
            if (g.out.log_q) g.out.log_q[patch] = win ? lq : nan;
            if (g.out.iters) g.out.iters[patch] = g.cand.iters[patch];
            if (g.out.status) g.out.status[patch] = st;
            if (g.best) g.best[patch] = win ? g.h : -1;
            g.cur_best[patch] = win ? g.h : -1;
            g.cur_lq[patch] = win ? lq : nan;
        }
    }
}

int dense_select_keep_launch(gpc_ctx* ctx, const DenseSite& site, int h, int P, int m, const int32_t* off, const SelectRows& cand,
                             const SelectRows& out, int32_t* best, double* log_q_all_h, int32_t* cur_best, double* cur_lq)
{
    if (P == 0) return GPC_OK;
    KeepParams g;
    g.h = h; g.P = P; g.m = m; g.off = off; g.cand = cand; g.out = out;
    g.best = best; g.log_q_all_h = log_q_all_h; g.cur_best = cur_best; g.cur_lq = cur_lq;
    const int cap = ctx->num_cus * 8;
    hipLaunchKernelGGL(dense_select_keep_kernel, dim3(P < cap ? P : cap), dim3(EV_THREADS), 0, site.stream, g);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}

// ---- gpc_dense_fit_predict_ev: the log marginal likelihood of the regression GP ----------------------------------------------------
// Rasmussen & Williams 2006, Alg. 2.1 line 7 (eq. 2.30), per patch of n points and per target plane c:
//     log p(y_c | X, theta) = -1/2 y_c^T alpha_c - sum_{j<n} log L_jj - n/2 log 2 pi
// L is the factor of A = K + noise I (twice the noise under ref_double_noise) that the fit exported; y and alpha are in place.  The
// read-out re-runs nothing: (2 ny + 1) n doubles per patch, one wave per patch, the sums in the order of dense_evidence_kernel (lane
// j mod 64, then ev_wave_sum), no atomics.  The factor comes in one of two layouts: the lower triangle of images that the register
// kernel's EXPORT instantiation and the one-wave kernel's slots hold (tri_nt > 0, what dense_variance_kernel reads), or the tiled
// kernel's slot (tri_nt == 0, as above).  Both keep L_kk^-1 as an operand image whose diagonal is 1 / L_jj (mf_diag_factor).

struct GaussEvParams {
    int P, ny, n_total, tri_nt, ntw;
    size_t slot;              // doubles per factor slot: tri_nt (tri_nt + 1) / 2 images, or big_slot_doubles(ntw)
    const int32_t* off;       // [P + 1]
    const int32_t* status;    // [P]: the fit's
    const double *alpha, *y;  // [ny][n_total]
    const double* ws;         // [P][slot]
    double* log_ev;           // [P][ny]
};

__global__ __launch_bounds__(EV_THREADS) void dense_gauss_evidence_kernel(GaussEvParams g)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cap = MF_TS * (g.tri_nt > 0 ? g.tri_nt : g.ntw);
    for (int patch = blockIdx.x * EV_WAVES + wave; patch < g.P; patch += gridDim.x * EV_WAVES) {
        const int o = g.off[patch], n = g.off[patch + 1] - o;
        double* out = g.log_ev + (size_t)patch * g.ny;
        if (n <= 0 || n > cap || g.status[patch] != GPC_STATUS_OK) {
            if (lane < g.ny) out[lane] = (n == 0) ? 0.0 : __builtin_nan("");
            continue;
        }
        const double* f = g.ws + (size_t)patch * g.slot;
        // tiled slot: the L_kk^-1 images sit behind the (ntw + 1) ntw tiles and the ntw L_kk^-T images
        if (g.tri_nt == 0) f += ((size_t)(g.ntw + 1) * g.ntw + g.ntw) * MF_IMG;
        double quad[3] = {0.0, 0.0, 0.0}, ldet = 0.0;
        for (int j = lane; j < n; j += 64) {           // (rows j >= n of the last tile are padding)
            const int k = j / MF_TS, r = j & (MF_TS - 1);
            const size_t img = g.tri_nt > 0 ? (size_t)(k * (k + 1) / 2 + k) : (size_t)k;
            ldet += log(f[img * MF_IMG + mf_img_rc(r, r)]);      // = -log L_jj
            for (int c = 0; c < g.ny; ++c)
                quad[c] = __builtin_fma(g.y[(size_t)c * g.n_total + o + j], g.alpha[(size_t)c * g.n_total + o + j], quad[c]);
        }
        ldet = ev_wave_sum(ldet);
        for (int c = 0; c < g.ny; ++c) {
            const double q = ev_wave_sum(quad[c]);
            if (lane == 0) out[c] = (-0.5 * q + ldet) - EV_HALF_LOG_2PI * (double)n;
        }
    }
}

int dense_gauss_evidence_launch(gpc_ctx* ctx, const DenseSite& site, const DenseArgs& a, int tri_nt, int ntw, const double* ws, size_t slot,
                                const double* alpha, double* log_ev)
{
    if (a.P == 0) return GPC_OK;
    if (!a.status || !alpha || !log_ev) return gpc_fail(ctx, GPC_EINVAL, "the evidence read-out needs the fit's status and alpha");
    GaussEvParams g;
    g.P = a.P; g.ny = a.ny; g.n_total = a.n_total; g.tri_nt = tri_nt; g.ntw = ntw;
    g.slot = tri_nt > 0 ? (size_t)(tri_nt * (tri_nt + 1) / 2) * MF_IMG : slot;
    g.off = a.off; g.status = a.status; g.alpha = alpha; g.y = a.y; g.ws = ws; g.log_ev = log_ev;
    const int need = (a.P + EV_WAVES - 1) / EV_WAVES, cap = ctx->num_cus * 8;
    hipLaunchKernelGGL(dense_gauss_evidence_kernel, dim3(need < cap ? need : cap), dim3(EV_THREADS), 0, site.stream, g);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}

// ---- gpc_dense_select: keep the best candidate so far ------------------------------------------------------------------------------
// dense_select_keep_kernel's rule on the Gaussian outputs.  The deciding value of a patch is the sum of its planes' log_ev in plane
// order; candidate h is eligible iff its status is GPC_STATUS_OK and that sum is finite, and takes the patch iff no candidate holds it
// yet or its sum is strictly greater.  Candidate 0 lays down what a patch without any eligible candidate keeps: best = -1, NaN rows,
// its own status.
struct GaussKeepParams {
    int h, P, ny, m, n_total;
    const int32_t* off;
    GaussRows cand, out;
    int32_t* best;            // [P] or nullptr
    double* log_ev_all_h;     // [P][ny] (row h of log_ev_all) or nullptr
    int32_t* cur_best;        // [P]
    double* cur_ev;           // [P]
};

__global__ __launch_bounds__(EV_THREADS) void dense_gauss_keep_kernel(GaussKeepParams g)
{
    const int tid = threadIdx.x;
    for (int patch = blockIdx.x; patch < g.P; patch += gridDim.x) {
        double ev = 0.0;
        for (int c = 0; c < g.ny; ++c) ev += g.cand.log_ev[(size_t)patch * g.ny + c];
        const int st = g.cand.status[patch];
        const int held = g.h == 0 ? -1 : g.cur_best[patch];
        const double held_ev = g.h == 0 ? 0.0 : g.cur_ev[patch];
        __syncthreads();                                    // every thread has read the state before thread 0 replaces it
        if (tid < g.ny && g.log_ev_all_h) g.log_ev_all_h[(size_t)patch * g.ny + tid] = g.cand.log_ev[(size_t)patch * g.ny + tid];
        const bool eligible = st == GPC_STATUS_OK && __builtin_isfinite(ev);
        const bool win = eligible && (held < 0 || ev > held_ev);
        if (!win && g.h != 0) continue;
        // candidate 0 without a win: the rows of "no eligible candidate"
        const double nan = __builtin_nan("");
        const int o = g.off[patch], n = g.off[patch + 1] - o;
        const size_t pm = (size_t)patch * g.m, pf = pm * g.ny;
        for (int q = tid; q < g.m * g.ny; q += EV_THREADS)
            if (g.out.f) g.out.f[pf + q] = win ? g.cand.f[pf + q] : nan;
        for (int q = tid; q < g.m; q += EV_THREADS)
            if (g.out.v) g.out.v[pm + q] = win ? g.cand.v[pm + q] : nan;
        for (int j = tid; j < n * g.ny; j += EV_THREADS) {
            const size_t at = (size_t)(j / n) * g.n_total + o + (j % n);
            if (g.out.alpha) g.out.alpha[at] = win ? g.cand.alpha[at] : nan;
        }
        if (tid < g.ny && g.out.log_ev) g.out.log_ev[(size_t)patch * g.ny + tid] = win ? g.cand.log_ev[(size_t)patch * g.ny + tid] : nan;
        if (tid == 0) {
            if (g.out.status) g.out.status[patch] = st;
            if (g.best) g.best[patch] = win ? g.h : -1;
            g.cur_best[patch] = win ? g.h : -1;
            g.cur_ev[patch] = win ? ev : nan;
        }
    }
}

int dense_gauss_keep_launch(gpc_ctx* ctx, const DenseSite& site, int h, int P, int ny, int m, int n_total, const int32_t* off,
                            const GaussRows& cand, const GaussRows& out, int32_t* best, double* log_ev_all_h, int32_t* cur_best,
                            double* cur_ev)
{
    if (P == 0) return GPC_OK;
    GaussKeepParams g;
    g.h = h; g.P = P; g.ny = ny; g.m = m; g.n_total = n_total; g.off = off; g.cand = cand; g.out = out;
    g.best = best; g.log_ev_all_h = log_ev_all_h; g.cur_best = cur_best; g.cur_ev = cur_ev;
    const int cap = ctx->num_cus * 8;
    hipLaunchKernelGGL(dense_gauss_keep_kernel, dim3(P < cap ? P : cap), dim3(EV_THREADS), 0, site.stream, g);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}
