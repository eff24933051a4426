// dense_evidence.hip -- model selection for the probit occupancy GP: the Laplace approximation of the log marginal likelihood read
// out of a finished fit, and the keep-best step of the loop over candidate hyper-parameters (definitions: include/gpc.h,
// gpc_dense_irls_fit_predict_ev and gpc_dense_irls_select).
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

// the 64 lanes' values in one fixed order; every lane gets the sum
__device__ static __forceinline__ double ev_wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

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
