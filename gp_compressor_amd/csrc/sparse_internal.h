// sparse_internal.h -- what the translation units of the sparse path share: sparse.hip (the add kernels), sparse_rate.hip (the prune and
// quantise kernels), sparse_predict.hip (the predict / likelihood / train kernels) and sparse_api.hip (the gpc_sparse_* C-ABI).  The
// device helpers of the kernels that change the state are in sparse_device.h.
#pragma once

#include "gpc_device.h"
#include "gpc_internal.h"

#define SP_THREADS 256

struct gpc_sparse {
    gpc_ctx* ctx;
    gpc_params prm;
    int P, ny, ld;
    double *alpha, *C, *Q, *BV;
    int32_t *b, *count, *stat;
    int32_t* done_it;   // P: hand-over between the phases of an add call (allocated with the object)
    int32_t* list;      // P + 4: work list of the phases after the rows phase, then its length and three ticket counters
    uint8_t* trace;     // diagnostic (gpc_sparse_set_trace): device buffer for the decision bytes of the next add calls, or nullptr
    uint64_t serial;    // gpc_child_register
};

// kernel_function(X, X) = p(0) exp(-0.5/p(1) |X - X|^2) (src/sparse_gp.hpp:98, :316): p(0) for a finite X (X - X = +0, exp(-0) is exactly 1,
// so finite data keeps its bits) and NaN when a coordinate is NaN or +-inf (X - X = NaN): no select, three operations.
__device__ static __forceinline__ double sp_kstar(double sf, double x0, double x1) { return sf + ((x0 - x0) + (x1 - x1)); }

// The live context of an object of the C-ABI (gpc_sparse, gpc_patches), or nullptr: the object is NULL, or the context went first and the
// object can only be destroyed (include/gpc.h).  The first question of every entry that takes an object.
template <class Object> static inline gpc_ctx* sp_live(const Object* g) { return g && !g->ctx->dead.load() ? g->ctx : nullptr; }

// ---- launchers implemented beside their kernels.  The caller has checked the arguments (the *_rules of sparse_api.hip) and is inside
// sp_locked (sparse_api.hip), which holds ctx->mu, has set the device and made the poison call; a caller elsewhere (render.hip,
// sparse_scatter.hip) has done the same itself.  All pointers are device pointers.

// sparse.hip: the phases of one add call
int sp_add_launch(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y, const int32_t* perm,
                  int32_t* status);
// sparse.hip: threads per patch (64, 128 or 256) of the add call's regular kernel and of every rate-control launch
int sp_workgroup_threads(const gpc_sparse* g);
// sparse_rate.hip: gpc_sparse_prune_dev behind its argument checks (removed / order / scores / status may be nullptr; target == nullptr: keep)
int sp_prune_launch(gpc_sparse* g, int keep, const int32_t* target, double score_tol, int32_t* removed, int32_t* order, double* scores,
                    int32_t* status);
// sparse_rate.hip: gpc_sparse_prune_rd_dev behind its argument checks (every output may be nullptr; max_mse_p == nullptr: max_mse)
int sp_prune_rd_launch(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y, int keep,
                       const int32_t* target, double max_mse, const double* max_mse_p, int32_t* removed, int32_t* order, double* scores,
                       double* mse, double* mse0, double* mse_next, int32_t* status);
// sparse_rate.hip: gpc_sparse_quantize_rd_dev behind its argument checks (every output may be nullptr; max_mse_p == nullptr: max_mse)
int sp_quantize_rd_launch(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y, int bits_min,
                          int bits_max, double max_mse, const double* max_mse_p, int32_t* bits, uint16_t* q_alpha, uint16_t* q_bv, float* range,
                          double* mse0, double* mse_q, double* curve, int32_t* status);
// sparse_rate.hip: gpc_sparse_dequantize_dev behind its argument checks (counts and widths are clamped by the kernel)
int sp_dequantize_launch(gpc_sparse* g, const int32_t* bv_count, const int32_t* bits, const uint16_t* q_alpha, const uint16_t* q_bv,
                         const float* range);
// sparse_predict.hip.  off == nullptr: every patch at the shared grid xs0 / xs1 [m]; else patch i at its own points off[i] .. off[i+1]-1 of
// xs0 / xs1 (m == 0, plane stride n_total).  max_blocks: cap on the resident workgroups per CU of the regular kernel.
int sp_predict_launch(gpc_sparse* g, int m, const int32_t* off, int n_total, const double* xs0, const double* xs1, double* f_star,
                      double* sigma, int conf, int32_t* status, int max_blocks);
// sparse_scatter.hip: gpc_sparse_predict_scattered_dev behind its argument checks (n >= 0, stride >= 1) -- buckets the n entries by patch in
// the context's workspace, runs sp_predict_launch on the bucketed batch and scatters the result back to entry order.  render.hip calls it
// for the sigma of a render's hits.
int sp_scatter_launch(gpc_sparse* g, int n, const int32_t* patch, const double* x0, const double* x1, int stride, double* f, double* sigma,
                      int conf, int32_t* status);
// raw != nullptr: the train_sigmaf pass (sigma_f^2 = 1, per-point sums only)
int sp_likelihood_launch(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y,
                         double* dX, double* l, double* raw);
// the iterations of train_sigmaf on the per-point sums `raw` of sp_likelihood_launch
int sp_train_launch(gpc_sparse* g, const int32_t* off, const double* y, const double* raw, double step, int max_counter, double* p0,
                    int32_t* iters, double* ls, double* delta);
