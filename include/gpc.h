/*
 * gpc.h -- C-ABI of the MI355X-native per-patch Gaussian-process hot path of gp_compressor.
 *
 * The reference (nilsbore/gp_compressor) has no FFI: its seam is the duck-typed contract that
 * gp_compressor uses on every element of `gps` / `RGB_gps` (src/gp_compressor.h:55-56):
 *
 *     add_measurements(X, y)                      src/sparse_gp.h:40, src/sparse_gp_field.h:37, src/gaussian_process.h:20
 *     predict_measurements(f_star, X_star, sig)   src/sparse_gp.h:41-42, src/sparse_gp_field.h:38-39, src/gaussian_process.h:19
 *     size(), reset()                             src/sparse_gp.h:36,39
 *
 * called once per octree-leaf patch from gp_compressor::train_processes (src/gp_compressor.cpp:121-175) and
 * gp_compressor::load_compressed (src/gp_compressor.cpp:298-380).  A per-object call per patch would serialise
 * the GPU, so the entry points below are the same calls BATCHED over patches: plain pointers and sizes, a ragged
 * CSR batch, no C++ / torch types.  All paths are relative to /root/reference.
 *
 * Layout conventions
 *   - patch i owns rows off[i] .. off[i+1]-1 of x0, x1, y   (off has P+1 entries, off[0] == 0)
 *   - X is SoA: x0[N], x1[N]  == Eigen column-major n x 2 (src/gp_compressor.cpp:146-155)
 *   - y is `ny` planes of N doubles (plane c at y + c*N): ny = 1 depth (VectorXd y), ny = 3 RGB (MatrixXd C n x 3,
 *     column-major), which is what sparse_gp_field::add_measurements takes (src/sparse_gp_field.hpp:46-57)
 *   - f_star is [P][ny][m]; v_star / sigma is [P][m]
 *   - every function returns 0 or a negative errno-style code and NEVER aborts (the reference exit(0)s,
 *     src/gp_compressor.cpp:138,215); per-patch conditions are reported in status[P]
 *   - *_dev entry points take DEVICE pointers and enqueue on the context's HIP stream without synchronising;
 *     the plain entry points take HOST pointers and are synchronous (H2D, launch, D2H).
 *
 * There is no CPU fallback: without a HIP device gpc_ctx_create() fails with GPC_ENODEV.
 */
#ifndef GPC_H
#define GPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPC_VERSION 100 /* 0.1.0 */

/* return codes */
#define GPC_OK 0
#define GPC_EINVAL (-22)  /* bad argument (NULL pointer, negative size, ny not in {1,3}, ...) */
#define GPC_ENOMEM (-12)  /* device or host allocation failed */
#define GPC_ENODEV (-19)  /* no HIP device / device index out of range */
#define GPC_EHIP (-5)     /* a HIP runtime call failed; see gpc_last_error() */
#define GPC_ERANGE (-34)  /* a size exceeds what the kernels support (n > GPC_MAX_POINTS, capacity > GPC_MAX_BV) */

/* per-patch status values */
#define GPC_STATUS_OK 0
#define GPC_STATUS_NOT_SPD 1      /* Cholesky pivot <= 1e-14 (sigmaf_sq + noise): numerically singular (Eigen::LLT would
                                     report NumericalIssue on a pivot <= 0); outputs are NaN */
#define GPC_STATUS_NAN 2          /* state became NaN ("sparse_gp::C has become Nan", src/sparse_gp.hpp:245) */
#define GPC_STATUS_SIGMA_CLAMPED 3 /* predictive sigma^2 < 0 was clamped to 0 (src/sparse_gp.hpp:334-337) */
#define GPC_STATUS_OVERFLOW 4     /* sparse, capacity == -1 only: basis set would exceed GPC_MAX_BV; point skipped */
#define GPC_STATUS_NOT_CONVERGED 5 /* gpc_dense_irls_fit_predict: max_iter Newton steps without max|df| <= tol; outputs are the last iterate */

#define GPC_MAX_POINTS 1024 /* largest n per patch of the dense path (BASELINE config 5) */
#define GPC_MAX_BV 256      /* largest sparse capacity (BASELINE config 4 uses 200) */

/* Hyper-parameters: exactly the constants the reference hard-codes per object. */
typedef struct gpc_params {
    double sigmaf_sq;             /* kernel amplitude: rbf_kernel p(0) (src/rbf_kernel.h:24) / gaussian_process sigmaf^2 */
    double l_sq;                  /* squared length scale: rbf_kernel p(1) / gaussian_process l^2 */
    double noise;                 /* dense: sigman_sq (src/gaussian_process.h:21);  sparse: s20 (src/sparse_gp.h:48) */
    double eps_tol;               /* sparse only: src/sparse_gp.hpp:30 (1e-6f), src/sparse_gp_field.hpp:16 (1e-4f) */
    int32_t capacity;             /* sparse only: max basis vectors; -1 = exact GP (src/sparse_gp.hpp:155,206) */
    int32_t noise_model;          /* 0 gaussian_noise(_3d); 1 probit_noise as written (src/probit_noise.cpp:11-31; its "Phi" is
                                     erf(z)/(2.0f*sqrt(2.0f)), not a CDF); 2 probit_noise with Phi(z) = (1 + erf(z/sqrt 2))/2,
                                     everything else as upstream.  1 and 2: ny == 1 only; never instantiated upstream */
    int32_t ref_double_noise;     /* dense: 1 = add sigman_sq twice like src/gaussian_process.cpp:19-22,59-61 */
    int32_t ref_field_delete_bug; /* sparse ny==3: 1 = multiply like src/sparse_gp_field.hpp:250-253, 0 = divide */
    int32_t want_variance;        /* dense: also compute V_star (src/gaussian_process.cpp:35-43) */
    int32_t reserved;
} gpc_params;

/* gaussian_process(double sigmaf = 0.05, double l = 3, double sigman = 0.04), squared (src/gaussian_process.h:21, .cpp:8-9) */
void gpc_default_params_dense(gpc_params* p);
/* sparse_gp(capacity=100, s0=1e-1f), eps_tol 1e-6f (ny==1)  |  sparse_gp_field(capacity=100, s0=1e2f), eps_tol 1e-4f (ny==3);
 * rbf_kernel(sigmaf_sq = 100e-0f, l_sq = 1) */
void gpc_default_params_sparse(gpc_params* p, int ny);

int gpc_version(void);

/* ---- context: one per process per GPU (owns the device workspace; thread-safe per context) ---------------- */
/* Ownership: objects created from a context (gpc_sparse, gpc_patches, gpc_registration) hold a reference on it and may be destroyed before
 * OR after gpc_ctx_destroy, in any order -- neither order aborts or touches freed memory.  gpc_ctx_destroy synchronises
 * the stream and releases the device workspace at once; from then on every call that takes the context, or one of its
 * surviving children, returns GPC_EINVAL, except the children's own destroy functions, which release their device
 * buffers as usual (the last one releases the context's host struct).  The context pointer itself must not be used
 * again once it AND all its children have been destroyed. */
typedef struct gpc_ctx gpc_ctx;
int gpc_ctx_create(gpc_ctx** out, int device);
/* hip_stream: a hipStream_t passed as void*, used as is (NULL is HIP's default stream); GPC_STREAM_OWN selects the
 * non-blocking stream the context created for itself (the initial setting).  Not owned.
 * The call only swaps the handle: work enqueued on the new stream is NOT ordered behind work still in flight on the old one, and both
 * use the context's workspace and events.  (The library cannot record an event on the old stream: it does not own that stream, and the
 * caller may have destroyed it.)  While work of this context is in flight, call gpc_ctx_synchronize before switching. */
#define GPC_STREAM_OWN ((void*)(intptr_t)-1)
int gpc_ctx_set_stream(gpc_ctx* ctx, void* hip_stream);
int gpc_ctx_synchronize(gpc_ctx* ctx);
/* Device buffers for callers built without the HIP toolchain (the reference is a g++ / CMake project): what the `_dev`
 * entry points need to be chained from plain C++.  gpc_dev_memcpy is synchronous and ordered after the work already
 * enqueued on the context's stream; kind: */
#define GPC_COPY_H2D 1
#define GPC_COPY_D2H 2
#define GPC_COPY_D2D 3
int gpc_dev_malloc(gpc_ctx* ctx, size_t bytes, void** out);
int gpc_dev_free(gpc_ctx* ctx, void* p);
int gpc_dev_memcpy(gpc_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);
/* Page-locked host memory for the buffers handed to the host-pointer entries (gpc_dense_fit_predict[_grid] ...).  Those entries
 * cut the batch into chunks and overlap upload, kernel and download on separate streams; from pinned memory the copies run in
 * place on the SDMA engines, from ordinary (pageable) memory they are first staged through pinned buffers of the context by a
 * threaded memcpy.  A reference-side binding assembles its X, y, C batch anyway (src/gp_compressor.cpp:146-155 copies the
 * lists into matrices): assembling it in gpc_host_alloc memory saves the staging copy. */
int gpc_host_alloc(gpc_ctx* ctx, size_t bytes, void** out);
int gpc_host_free(gpc_ctx* ctx, void* p);
void gpc_ctx_destroy(gpc_ctx* ctx);
/* text of the last failure on this context ("" if none); valid until the next call on the context */
const char* gpc_last_error(const gpc_ctx* ctx);
/* name of the kernel variant the last dense call dispatched to (for tests and profiles) */
const char* gpc_last_dense_kernel(const gpc_ctx* ctx);

/* ---- dense exact GP: gaussian_process::add_measurements + predict_measurements, batched ------------------- */
/* Replaces, per patch:  gp.add_measurements(X, y); gp.predict_measurements(f_star, X_star, V_star);
 * (src/gaussian_process.cpp:15-45).  Computes K (+noise), its Cholesky factor, alpha, f_star = K*^T alpha and,
 * when params->want_variance and v_star != NULL, V_star.  alpha_out (ny planes of N) may be NULL. */
int gpc_dense_fit_predict(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off,
                          const double* x0, const double* x1, const double* y, int ny,
                          int m, const double* xs0, const double* xs1,
                          double* f_star, double* v_star, double* alpha_out, int32_t* status);
/* Same with device pointers.  n_max >= max_i(off[i+1]-off[i]) and n_total == off[P] are passed by value because
 * `off` lives on the device. */
int gpc_dense_fit_predict_dev(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off, int n_max, int n_total,
                              const double* x0, const double* x1, const double* y, int ny,
                              int m, const double* xs0, const double* xs1,
                              double* f_star, double* v_star, double* alpha_out, int32_t* status);
/* The decompression grid of gp_compressor::load_compressed is the same for every patch and separable:
 * X*(p,0) = res*((x+.5)/sz-.5), X*(p,1) = res*((y+.5)/sz-.5), p = y*sz + x, m = sz*sz
 * (src/gp_compressor.cpp:317-332).  These entry points build it internally and evaluate K* as an outer product
 * of two sz x n factor tables (rounding differs from the point-wise kernel by O(1 ulp) per entry). */
int gpc_dense_fit_predict_grid(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off,
                               const double* x0, const double* x1, const double* y, int ny,
                               double res, int sz, double* f_star, double* alpha_out, int32_t* status);
int gpc_dense_fit_predict_grid_dev(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off, int n_max,
                                   int n_total, const double* x0, const double* x1, const double* y, int ny,
                                   double res, int sz, double* f_star, double* alpha_out, int32_t* status);
/* Non-finite data (all four entries, every kernel they dispatch to; hyper-parameters must be finite, see the argument rules).  The
 * arithmetic is the reference's, which takes no special case, and what a NaN or an infinity reaches is decided per patch, per target
 * plane and per X* column -- nothing else in the batch changes, and the variance of everything untouched keeps its bits:
 *   x0 / x1 of a training point NaN or +-inf: the point's diagonal entry is sf * exp(c (inf - inf)^2) = NaN, a NaN pivot is not
 *     positive: status[i] = GPC_STATUS_NOT_SPD, and f_star, v_star and alpha_out of patch i are NaN in every entry, every plane.
 *   y of a training point NaN or +-inf: status[i] stays GPC_STATUS_OK; alpha_out and f_star of THAT plane of patch i are non-finite
 *     in every entry (NaN or +-inf: where the infinities of a sum cancel depends on its order); the patch's other planes and its
 *     v_star, which does not depend on y, are as without the poison.
 *   a coordinate of X* column j NaN (point-wise entries): f_star[.][j] and v_star[j] are NaN for every patch with points.  +-inf: the
 *     kernel value against every training point is exp(-inf) = 0, so f_star[.][j] = 0, and v_star[j] = k(x*, x*) - 0 is NaN, since
 *     k(x*, x*) = sf * exp(c (inf - inf)^2) as gaussian_process::predict_measurements evaluates it.
 *   a patch without points writes the prior whatever X* holds, f_star = 0 and v_star = sigmaf_sq: nothing is evaluated for it.
 *     This is the one place where the contract is not the reference's arithmetic, which gives v_star = NaN there under a non-finite x*.
 * The other columns of a call with a non-finite X* agree with the clean call to rounding, not to the bit (the variance kernel bounds
 * its exponential by the extent of all of X*). */

/* ... with the log marginal likelihood log p(y | X, theta) (Rasmussen & Williams 2006, Alg. 2.1 line 7, eq. 2.30): what tells whether
 * sigmaf_sq, l_sq and noise fit the data of a patch.
 * Definition.  Let A be the matrix the fit factorises, K + noise I, or K + 2 noise I with ref_double_noise, and L its Cholesky factor.
 * Per patch i of n points and per target plane c
 *     log_ev[i][c] = -0.5 sum_j y_c[j] alpha_c[j]  -  sum_{j<n} log L_jj  -  0.5 n log(2 pi)
 *   - the padding rows j >= n of the last tile are never summed;
 *   - each sum has one fixed order: point j goes to lane j mod 64 of one wave, then a fixed shuffle tree; no atomics.  From the same
 *     alpha and factor two calls give the same bits: that is every call on the one-wave, the tiled and the generic kernel.  The register
 *     kernel (n_max <= 256 below the one-wave kernel's batch size, and every ny == 3 batch of that size) forms alpha with LDS atomic adds
 *     in no fixed order, so there alpha_out, f_star and the y^T alpha term repeat to a rounding or two, as in gpc_dense_fit_predict; the
 *     factor, v_star and sum log L_jj repeat bit for bit on every route;
 *   - an empty patch gives 0;
 *   - status GPC_STATUS_NOT_SPD (and GPC_STATUS_NAN) gives NaN in every plane;
 *   - a non-finite y in plane c gives a non-finite log_ev[i][c] and leaves the other planes as they are;
 *   - L_jj = 1 / (L_kk^-1)_jj is read from the L_kk^-1 image of tile k = j / 16 that the fit exported, so -log L_jj is taken as
 *     log (L_kk^-1)_jj, as the probit read-out below does.  (Under GPC_FORCE_GENERIC the generic kernel forms the same sums from its own
 *     pivots, without any export: the value the other routes are cross-checked against.)
 * Arguments: those of gpc_dense_fit_predict[_dev], plus res, sz and log_ev [P][ny].  X* is point-wise (xs0, xs1, m) or, when xs0 == NULL,
 * the sz x sz grid of load_compressed (res, sz; m is ignored, m = sz sz, cell p = y sz + x).  The variance kernels have no separable
 * form, so the library materialises the grid as m points in its workspace and evaluates point-wise throughout: f_star may differ from
 * gpc_dense_fit_predict_grid[_dev] by O(1 ulp) per kernel value.
 * A call with log_ev takes the variance route with the factor export on, whatever params->want_variance says: a caller who wants v_star
 * passes it, and NULL means no variance.
 *   - log_ev == NULL: the call IS gpc_dense_fit_predict[_dev] (point-wise form; grid form without a variance to compute:
 *     gpc_dense_fit_predict_grid[_dev]): the same launches, the same bits.
 *   - log_ev and v_star: f_star, v_star and alpha_out are bit for bit those of gpc_dense_fit_predict_dev with want_variance = 1.
 *   - log_ev without v_star: the fit runs with the export on and predicts f_star itself; no variance kernel runs, so the call costs a
 *     fit, not a fit plus an n^2 m solve.  f_star and alpha_out are the export-on fit's own: correct to the tolerances of the plain entry,
 *     not held to its bits (the one-wave kernel factorises K / sigmaf_sq without the export and K itself with it).
 *   - m == 0 is allowed: the call returns the evidence (and alpha_out, status) only.
 * Rules, checked in this order; the first one broken decides the code, and no output is written on an error:
 *   1. ctx NULL or dead                                                                              GPC_EINVAL (no text)
 *   2. params NULL
 *   3. select only: H < 1 or cand NULL; a candidate with a non-finite field, sigmaf_sq <= 0, l_sq <= 0 or noise < 0
 *   4. grid form (xs0 == NULL): sz outside 0 .. 1024
 *   5. host forms only: P < 0; off NULL with P > 0; off[0] != 0 or off decreasing
 *   6. the dense rules: a negative size; ny not 1 or 3; off, x0, x1 or y NULL where there is something to read; f_star NULL with P > 0
 *      and m > 0 (not under select, whose every output may be NULL); n_max > GPC_MAX_POINTS: GPC_ERANGE; l_sq <= 0, sigmaf_sq < 0 or
 *      noise < 0
 *   7. point-wise form: xs1 NULL with m > 0
 *   8. P == 0: GPC_OK, nothing is launched and nothing written
 * Everything but the one GPC_ERANGE is GPC_EINVAL.
 * Workspace.  In front: a status word per patch when status == NULL, alpha (ny n_total + 1 doubles) when alpha_out == NULL and m == 0
 * (with something to predict the kernels keep alpha in their own region, counted below), the grid
 * points (2 m doubles) in the grid form, each rounded up to 256 bytes; behind them what the route's kernel keeps for the variance path,
 * with nt = 4 ceil(n_max / 64), ntw = ceil(n_max / 16), slot(ntw) = 256 ((ntw + 1) ntw + 2 ntw):
 *     n_max <= 256, register kernel:    8 (128 nt (nt + 1) P + ny n_total + 2048)
 *     193 .. 256 points, one-wave:      8 (38912 min(P, 8192) + n_total)          (ny == 1, batches of at least four patches per CU)
 *     257 .. 1024 points, tiled kernel: 8 (slot(ntw) P + ny n_total + 2048 CUs ntw)
 *     GPC_FORCE_GENERIC:                8 ((n_max + ny)^2 + n_max ceil64(m) [with v_star]) per resident workgroup
 * A refusal returns GPC_ENOMEM.  The batch is not chunked beyond what the one-wave launcher already does (launches of at most 8192
 * patches that reuse the slots; the read-out follows each launch), and where only the one-wave kernel's workspace is refused the call
 * stays GPC_ENOMEM.  The _dev form enqueues on the context's stream and never synchronises; the host form stages its arguments through
 * device buffers of its own and returns when the outputs are in host memory. */
int gpc_dense_fit_predict_ev(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off, const double* x0, const double* x1,
                             const double* y, int ny, int m, const double* xs0, const double* xs1, double res, int sz, double* f_star,
                             double* v_star, double* alpha_out, int32_t* status, double* log_ev);
int gpc_dense_fit_predict_ev_dev(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off, int n_max, int n_total,
                                 const double* x0, const double* x1, const double* y, int ny, int m, const double* xs0, const double* xs1,
                                 double res, int sz, double* f_star, double* v_star, double* alpha_out, int32_t* status, double* log_ev);
/* Model selection among H candidate hyper-parameter sets, per patch, by that evidence.  params is the base; for candidate h its
 * sigmaf_sq, l_sq and noise are replaced by cand[h]'s (struct gpc_hyper).  cand is a HOST array of H >= 1 entries, read at call
 * time, in the _dev form too.
 * Rule per patch.  The deciding value is sum_c log_ev[c], taken in plane order.  Candidate h is eligible iff its fit ended with
 * GPC_STATUS_OK and that sum is finite.  best is the lowest h that attains the maximum over the eligible candidates (the comparison is a
 * strict >: ties and duplicates go to the lower index, a NaN never wins).  Every output of the patch is the winner's, bit for bit what
 * gpc_dense_fit_predict_ev[_dev] gives with that candidate's parameters and the same outputs requested.  With no eligible candidate
 * best = -1, f*, v*, alpha and log_ev are NaN and status is candidate 0's.  An empty patch has log_ev = 0 under every candidate:
 * best = 0 with candidate 0's outputs, f* = 0 and v* = cand[0].sigmaf_sq.
 * Outputs, each may be NULL: f_star [P][ny][m], v_star [P][m], alpha_out [ny][n_total], log_ev [P][ny], best [P],
 * log_ev_all [H][P][ny] (every candidate's log_ev), status [P].
 * The candidates run one after another on the context's stream into temporaries in the workspace, and after each a keep-best kernel
 * copies the rows of the patches it won so far into the outputs.  Workspace: that of gpc_dense_fit_predict_ev[_dev] with alpha_out and
 * status given, plus the temporaries and the state of the keep-best step --
 *     bytes = ev_bytes + 8 (ny P m + 1 + [P m with v_star] + ny n_total + 1 + ny P + P) + 4 (2 P)
 * (each term rounded up to 256 bytes); a refusal returns GPC_ENOMEM.  The _dev form never synchronises.
 * Errors: rule 3 above, then the shared rules. */
typedef struct gpc_hyper {
    double sigmaf_sq, l_sq, noise;
} gpc_hyper;
int gpc_dense_select(gpc_ctx* ctx, const gpc_params* params, int H, const gpc_hyper* cand, int P, const int32_t* off,
                     const double* x0, const double* x1, const double* y, int ny, int m, const double* xs0, const double* xs1, double res,
                     int sz, double* f_star, double* v_star, double* alpha_out, double* log_ev, int32_t* best, double* log_ev_all,
                     int32_t* status);
int gpc_dense_select_dev(gpc_ctx* ctx, const gpc_params* params, int H, const gpc_hyper* cand, int P, const int32_t* off, int n_max,
                         int n_total, const double* x0, const double* x1, const double* y, int ny, int m, const double* xs0,
                         const double* xs1, double res, int sz, double* f_star, double* v_star, double* alpha_out, double* log_ev,
                         int32_t* best, double* log_ev_all, int32_t* status);

/* ---- dense GP with the probit functor: Newton / IRLS loop on the GPU (BASELINE config 5) ---------------------------- */
/* The reference never instantiates probit_noise and holds no IRLS loop (its occupancy map is a ray-cast boolean mask,
 * src/gp_mapping.cpp:154-211 -- gpc_patches_raycast + gpc_occupancy_batch_dev below turn it into this entry's labels): what it fixes is the Noise contract, q = dx_ln(y, x, sigma_x), r = dx2_ln(y, x, sigma_x)
 * (src/probit_noise.cpp:11-31), and the kernel.  This entry runs the textbook loop those plug into -- Newton's method for
 * the mode of p(f | y) with labels y = +-1 (Rasmussen & Williams 2006, Alg. 3.1) in IRLS form: with W = -r, g = q at
 * sigma_x = 0, every step is one gaussian_process::add_measurements-style fit (src/gaussian_process.cpp:15-26) with
 * per-point noise 1 / W_i and working targets t_i = f_i + g_i / W_i:
 *     a = (K + W^-1)^-1 t,   f <- K a = t - W^-1 a;    start f = y * f_init;   stop: max_iter solves or max|df| <= tol.
 * params: sigmaf_sq, l_sq (rbf_kernel, src/rbf_kernel.cpp:15-18), noise = s20 of the functor, noise_model = 1 (as written;
 * singular at f = 0, needs f_init > 0) or 2 (proper CDF; f_init = 0 is the textbook start).  y: N labels.
 * Prediction: latent mean f* = K*^T a on X* -- point-wise (xs0, xs1, m) or, when xs0 == NULL, the sz x sz grid of
 * gp_compressor::load_compressed (res, sz; m is ignored).  f_star [P][m]; alpha_out [N] (= a), fhat_out [N] (the mode at the
 * training points), iters [P] (solves performed) and status [P] may be NULL.  Status GPC_STATUS_NOT_CONVERGED: the step cap ended
 * the loop (outputs are the last iterate).  Status GPC_STATUS_NAN: a weight W_i was not
 * finite and positive (with noise_model 1 this is the normal outcome when a step crosses f = 0); outputs of the patch are NaN.
 * Definition and CPU restatement: oracle/gpc_oracle.c (orc_dense_irls_fit).
 *
 * Shared arguments and rules of the eight probit entries (gpc_dense_irls_fit_predict, its _var and _ev forms and gpc_dense_irls_select,
 * each with its _dev twin).  All take ctx, params, irls, P, off, x0, x1, y, m, xs0, xs1, res, sz as described above; the _dev forms
 * also n_max (the largest patch) and n_total = off[P], which the host forms read from off.  Every entry checks the same rules in this
 * order, whichever outputs it was asked for, and the first one broken decides the code and the text of gpc_last_error:
 *   1. ctx NULL or dead                                                                              GPC_EINVAL (no text)
 *   2. params NULL
 *   3. select only: H < 1 or cand NULL; noise_model != 2; a candidate with a non-positive or non-finite field
 *   4. grid form (xs0 == NULL): sz outside 0 .. 1024
 *   5. host forms only: P < 0; off NULL with P > 0; off[0] != 0 or off decreasing
 *   6. the dense rules: a negative size; off, x0, x1 or y NULL where there is something to read; f_star NULL with P > 0 and m > 0
 *      (not under select, whose every output may be NULL); n_max > GPC_MAX_POINTS: GPC_ERANGE; l_sq <= 0, sigmaf_sq < 0 or noise < 0
 *   7. irls NULL; noise_model not 1 or 2; p_star or log_q with noise_model != 2 (the "Phi" of model 1 is not a probability);
 *      max_iter < 1, tol < 0 or NaN, f_init NaN; noise <= 0; point-wise form: xs1 NULL with m > 0
 *   8. P == 0: GPC_OK, nothing is launched and nothing written
 * Everything but the one GPC_ERANGE is GPC_EINVAL, and no output is written on an error.  The rules run in full before rule 8 in both
 * forms: an empty batch with invalid probit parameters is GPC_EINVAL from a host entry as from its _dev twin. */
typedef struct gpc_irls_params {
    int32_t max_iter;   /* >= 1 */
    int32_t reserved;
    double tol;         /* on max_i |f_new_i - f_i| */
    double f_init;      /* f_i = y_i * f_init before the first step */
} gpc_irls_params;
/* max_iter 20, tol 1e-9, f_init 0 */
void gpc_default_params_irls(gpc_irls_params* p);
int gpc_dense_irls_fit_predict(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                               const double* x0, const double* x1, const double* y, int m, const double* xs0, const double* xs1,
                               double res, int sz, double* f_star, double* alpha_out, double* fhat_out, int32_t* iters,
                               int32_t* status);
int gpc_dense_irls_fit_predict_dev(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                                   int n_max, int n_total, const double* x0, const double* x1, const double* y, int m,
                                   const double* xs0, const double* xs1, double res, int sz, double* f_star, double* alpha_out,
                                   double* fhat_out, int32_t* iters, int32_t* status);
/* ... with the latent predictive variance and the occupancy probability (Rasmussen & Williams 2006, Alg. 3.2).
 * Definition.  For every patch the Newton / IRLS loop runs exactly as in gpc_dense_irls_fit_predict_dev: the same rule, the same a,
 * fhat, iters and status.  Let W be the weights of the LAST SOLVE PERFORMED -- the functor's -r at the iterate the last step started
 * from; no factorisation is run after the loop, and on a converged patch W differs from W(fhat) by O(tol).  Let s = W^1/2 and L the
 * Cholesky factor of B = I + diag(s) K diag(s) that this solve left behind.  Then per prediction point
 *     f* = k*^T a                                   (as in the plain entry)
 *     v* = sigmaf_sq - | L^-1 (s o k*) |^2          (= k** - k*^T (K + W^-1)^-1 k*; not clamped: may be -O(eps) like the dense v_star)
 *     p* = 0.5 erfc(-z / sqrt 2),  z = f* / sqrt(s20 + max(v*, 0))       (the functor's own ef of noise_model 2 at sigma_x = v*:
 *                                                                          P(y = +1 | x*), the sigma_x slot of probit_noise::dx_ln)
 * Per patch: an empty patch gives f* = 0, v* = sigmaf_sq, p* = 0.5; status GPC_STATUS_NAN (and NOT_SPD) gives NaN in f*, v*, p*;
 * GPC_STATUS_NOT_CONVERGED gives the outputs of the last iterate, not NaN.
 * v_star and p_star are [P][m]; each may be NULL, and with both NULL (or nothing to predict) the call IS gpc_dense_irls_fit_predict[_dev]:
 * the same launches, the same bits.  p_star needs noise_model 2 (rule 7 above); v_star works with both models.
 * With xs0 == NULL the sz x sz grid of load_compressed is used (res, sz; m = sz*sz, cell p = y*sz + x).  The variance kernel has no
 * separable form, so the library then materialises the grid as m points in its workspace and evaluates point-wise throughout: f_star may
 * differ from the grid form of gpc_dense_irls_fit_predict[_dev] by O(1 ulp) per kernel value.
 * Workspace: one factor slot per patch, a and s (n_total doubles each), the variance kernel's per-wave scratch, the grid points, a
 * status word per patch --
 *     bytes = 8 (slot(ntw) P + 2 n_total + 2048 CUs ntw + 2 m) + 4 P,   slot(ntw) = 256 ((ntw + 1) ntw + 2 ntw),  ntw = ceil(n_max / 16)
 * (each term rounded up to 256 bytes; n_max = 1024: 8.8 MB per patch).  A refusal returns GPC_ENOMEM; the batch is not chunked.
 * The _dev form enqueues on the context's stream and never synchronises; the host form stages its arguments like
 * gpc_dense_irls_fit_predict. */
int gpc_dense_irls_fit_predict_var(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                                   const double* x0, const double* x1, const double* y, int m, const double* xs0, const double* xs1,
                                   double res, int sz, double* f_star, double* v_star, double* p_star, double* alpha_out,
                                   double* fhat_out, int32_t* iters, int32_t* status);
int gpc_dense_irls_fit_predict_var_dev(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                                       int n_max, int n_total, const double* x0, const double* x1, const double* y, int m,
                                       const double* xs0, const double* xs1, double res, int sz, double* f_star, double* v_star,
                                       double* p_star, double* alpha_out, double* fhat_out, int32_t* iters, int32_t* status);
/* ... and with the Laplace approximation of the log marginal likelihood (Rasmussen & Williams 2006, Alg. 3.1 line 10, eq. 3.32): what
 * tells whether sigmaf_sq, l_sq and s20 fit the labels of a patch.  noise_model 2 only.
 * Definition.  The loop, a, fhat, iters, status, f*, v* and p* are exactly those of gpc_dense_irls_fit_predict_var[_dev]; L is the factor
 * of the LAST SOLVE PERFORMED (R&W's own convention: the L of the last iteration with the updated f).  Per patch of n points
 *     log_q = -0.5 sum_j a_j fhat_j  +  sum_j log ef(y_j fhat_j / sqrt(s20))  -  sum_{j<n} log L_jj,    ef(z) = 0.5 erfc(-z / sqrt 2)
 * ef is the functor's own ef of noise_model 2 at sigma_x = 0; L_jj = 1 / (L_kk^-1)_jj is read from the L_kk^-1 image of tile k = j / 16
 * that the fit exported (so -log L_jj is taken as log (L_kk^-1)_jj); the padding rows j >= n of the last tile are not summed.  Each of
 * the three sums has a fixed order (point j goes to lane j mod 64 of one wave, then a fixed shuffle tree): two calls give the same bits.
 * Per patch: an empty patch gives log_q = 0; status GPC_STATUS_NAN (and NOT_SPD) gives NaN; GPC_STATUS_NOT_CONVERGED gives the value at
 * the last iterate; an ef that underflows gives -inf, a valid output.
 * log_q is [P].  log_q == NULL: the call IS gpc_dense_irls_fit_predict_var[_dev], the same launches and the same bits.  log_q != NULL:
 * every other output is bit for bit what that entry gives; noise_model 2 only (rule 7 above).  v_star and p_star may both be NULL and m
 * may be 0: the fit still runs with the factor export on (f_star is then the plain entry's), and the variance kernel is skipped.
 * Workspace: that of gpc_dense_irls_fit_predict_var[_dev] plus fhat (n_total doubles) when fhat_out == NULL --
 *     bytes = 8 (slot(ntw) P + 3 n_total + 2048 CUs ntw + 2 m) + 4 P
 * (each term rounded up to 256 bytes).  A refusal returns GPC_ENOMEM; the batch is not chunked.  The read-out re-runs nothing: it reads
 * a, fhat, y and the diagonals of the L_kk^-1 images, 4 n doubles per patch. */
int gpc_dense_irls_fit_predict_ev(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                                  const double* x0, const double* x1, const double* y, int m, const double* xs0, const double* xs1,
                                  double res, int sz, double* f_star, double* v_star, double* p_star, double* alpha_out,
                                  double* fhat_out, int32_t* iters, int32_t* status, double* log_q);
int gpc_dense_irls_fit_predict_ev_dev(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int P, const int32_t* off,
                                      int n_max, int n_total, const double* x0, const double* x1, const double* y, int m,
                                      const double* xs0, const double* xs1, double res, int sz, double* f_star, double* v_star,
                                      double* p_star, double* alpha_out, double* fhat_out, int32_t* iters, int32_t* status,
                                      double* log_q);
/* Model selection among H candidate hyper-parameter sets, per patch, by that evidence.  params is the base (noise_model must be 2); for
 * candidate h its sigmaf_sq, l_sq and noise (= s20) are replaced by cand[h]'s.  cand is a HOST array of H >= 1 entries, read at call
 * time, in the _dev form too.
 * Rule per patch.  Candidate h is eligible iff its fit ended with GPC_STATUS_OK and its log_q is finite.  best is the lowest h that
 * attains the maximum of log_q over the eligible candidates (the comparison is a strict >: ties and duplicates go to the lower index, a
 * NaN never wins).  Every output of the patch is the winner's, bit for bit what gpc_dense_irls_fit_predict_ev[_dev] gives with that
 * candidate's parameters and the same v_star / p_star requested.  With no eligible candidate best = -1, f*, v*, p*, alpha, fhat and log_q
 * are NaN, and iters and status are those of candidate 0.  An empty patch has log_q = 0 under every candidate: best = 0 with candidate
 * 0's outputs, f* = 0, v* = cand[0].sigmaf_sq, p* = 0.5.
 * Outputs, each may be NULL: f_star, v_star, p_star [P][m]; alpha_out, fhat_out [N]; log_q [P]; best [P]; log_q_all [H][P] (every
 * candidate's log_q); iters, status [P].
 * The candidates run one after another on the context's stream into temporaries in the workspace, and after each a keep-best kernel
 * copies the rows of the patches it won so far into the outputs.  Workspace: that of gpc_dense_irls_fit_predict_ev[_dev] plus the
 * temporaries --
 *     bytes = ev_bytes + 8 (3 P m + 2 n_total + 2 P) + 4 (3 P)
 * (each term rounded up to 256 bytes); not chunked over patches, a refusal returns GPC_ENOMEM.  The _dev form never synchronises.
 * Errors: rule 3 above, then the shared rules. */
/* (struct gpc_hyper: with gpc_dense_select above) */
int gpc_dense_irls_select(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int H, const gpc_hyper* cand, int P,
                          const int32_t* off, const double* x0, const double* x1, const double* y, int m, const double* xs0,
                          const double* xs1, double res, int sz, double* f_star, double* v_star, double* p_star, double* alpha_out,
                          double* fhat_out, double* log_q, int32_t* best, double* log_q_all, int32_t* iters, int32_t* status);
int gpc_dense_irls_select_dev(gpc_ctx* ctx, const gpc_params* params, const gpc_irls_params* irls, int H, const gpc_hyper* cand, int P,
                              const int32_t* off, int n_max, int n_total, const double* x0, const double* x1, const double* y, int m,
                              const double* xs0, const double* xs1, double res, int sz, double* f_star, double* v_star,
                              double* p_star, double* alpha_out, double* fhat_out, double* log_q, int32_t* best, double* log_q_all,
                              int32_t* iters, int32_t* status);
/* The Noise contract itself, evaluated on the DEVICE by the very functions the kernels inline (csrc/gpc_device.h):
 * q[i] = dx_ln(y[i], x[i], sigma_x[i]), r[i] = dx2_ln(...) for noise_model 0 (src/gaussian_noise.cpp:9-18), 1 or 2
 * (src/probit_noise.cpp:11-31).  Host pointers, n triples.  This is what pins the device functors to the compiled
 * reference objects (tests/golden/noise_ref.json). */
int gpc_noise_eval(gpc_ctx* ctx, int noise_model, double s20, int n, const double* y, const double* x, const double* sigma_x,
                   double* q, double* r);

/* ---- sparse online GP: sparse_gp<rbf_kernel, gaussian_noise> / sparse_gp_field<rbf_kernel, gaussian_noise_3d> */
/* One handle holds the persistent state (alpha, C, Q, BV, current_size) of P independent patch GPs on the
 * device: the batched equivalent of `std::vector<sparse_gp<...>> gps` (src/gp_compressor.h:55-56). */
typedef struct gpc_sparse gpc_sparse;
int gpc_sparse_create(gpc_ctx* ctx, const gpc_params* params, int P, int ny, gpc_sparse** out);
void gpc_sparse_destroy(gpc_sparse* g);
/* reset(): src/sparse_gp.hpp:573-582, for all patches */
int gpc_sparse_reset(gpc_sparse* g);
/* add_measurements(X, y) for every patch (src/sparse_gp.hpp:59-86); may be called repeatedly (online growth,
 * src/gp_mapping.cpp:338-339).  perm holds, per patch, the insertion order as patch-local row indices
 * (the reference draws it from libc rand(), src/sparse_gp.hpp:43-56; here it is an explicit input, NULL = identity). */
int gpc_sparse_add(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y,
                   const int32_t* perm, int32_t* status);
int gpc_sparse_add_dev(gpc_sparse* g, const int32_t* off, int n_max, int n_total, const double* x0, const double* x1,
                       const double* y, const int32_t* perm, int32_t* status);
/* Diagnostic: record the branch decisions of the following add calls.  trace_dev is a DEVICE buffer of n_total bytes (the
 * n_total of those calls), NULL switches it off.  Byte off[i] + t belongs to the t-th point patch i inserted in the call:
 * bit 0: 1 = full update (basis grew, src/sparse_gp.hpp:164-203), 0 = sparse update (:155-163); bits 1-3: capacity
 * deletions that followed (:206-223); bits 4-6: geometric deletions (:226-242); 0x81: first point of an empty GP (:100-114).
 * The CPU oracle and its binary128 arbiter emit the same bytes (oracle/gpc_oracle_hp.c), which is how the tests count the
 * decisions an fp64 implementation takes differently from the exact recursion. */
int gpc_sparse_set_trace(gpc_sparse* g, uint8_t* trace_dev);
/* predict_measurements(f_star, X_star, sigconf, conf) for every patch on one shared X_star (src/sparse_gp.hpp:299-351).
 * sigma may be NULL (the caller in src/gp_compressor.cpp:333-334 discards it); conf selects the 0-100 confidence form. */
int gpc_sparse_predict(gpc_sparse* g, int m, const double* xs0, const double* xs1, double* f_star, double* sigma,
                       int conf, int32_t* status);
int gpc_sparse_predict_dev(gpc_sparse* g, int m, const double* xs0, const double* xs1, double* f_star, double* sigma,
                           int conf, int32_t* status);
/* predict_measurements(f, X_i, sigconf, conf) with every patch on ITS OWN point set (ragged like the add call's batch): what the
 * reference's per-patch training-set RMS block does (src/gp_compressor.cpp:303-315, printed at :381).  Patch i reads rows
 * off[i]..off[i+1]-1 of x0, x1 and writes the same rows of f (ny planes of n_total) and sigma (n_total, may be NULL). */
int gpc_sparse_predict_points(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, double* f, double* sigma,
                              int conf, int32_t* status);
int gpc_sparse_predict_points_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1,
                                  double* f, double* sigma, int conf, int32_t* status);
/* predict_measurements at n UNBUCKETED (patch, point) pairs, in any order: entry i is the point (x0[i stride], x1[i stride]) under patch
 * patch[i].  stride >= 1 counts doubles: 1 is the SoA layout of the entries above; (local + 1, local + 2, 3) reads the `local` output
 * of gpc_patches_render in place.  f: ny planes of n in ENTRY order, sigma: n; either may be NULL.  status: P words or NULL; conf as in
 * gpc_sparse_predict.
 *   skipped  an entry with patch[i] < 0 or patch[i] >= P is skipped: its f (every plane) and sigma are NaN.  That is the miss
 *            convention of gpc_patches_render and no error.
 *   result   f, sigma and status are, bit for bit, those of gpc_sparse_predict_points_dev on the batch in which patch p owns the
 *            entries with patch[i] == p in ascending i: the entries are bucketed on the device (keys, a stable radix sort over
 *            ceil(log2(P + 1)) bits, a binary search per patch for `off`, a gather), the same kernels run on that batch, and the
 *            result is scattered back.  No atomics: the same inputs give the same bits.
 *   errors   n == 0: GPC_OK.  GPC_EINVAL: a NULL or dead object, n < 0, stride < 1, NULL patch / x0 / x1 with n > 0.  Outputs must
 *            not overlap inputs.
 * gpc_sparse_predict_scattered_dev takes DEVICE pointers, enqueues on the context's stream and never synchronises (the number of
 * valid entries is never read back); the scratch is the context's workspace.  gpc_sparse_predict_scattered takes HOST pointers and is
 * synchronous. */
int gpc_sparse_predict_scattered(gpc_sparse* g, int n, const int32_t* patch, const double* x0, const double* x1, int stride, double* f,
                                 double* sigma, int conf, int32_t* status);
int gpc_sparse_predict_scattered_dev(gpc_sparse* g, int n, const int32_t* patch, const double* x0, const double* x1, int stride,
                                     double* f, double* sigma, int conf, int32_t* status);
/* Registration inner loop: sparse_gp::compute_derivatives + compute_likelihoods
 * (src/sparse_gp.h:44-45 -> src/sparse_gp.hpp:387-427, 463-508; field: src/sparse_gp_field.h:40-41 -> .hpp:322-392; call site
 * src/gp_registration.cpp:175-195), batched over patches: patch i evaluates its own rows off[i]..off[i+1]-1 of x0, x1 and
 * the ny planes of y against its current state.  dX is [N][3], row = point, columns as the reference fills them
 * (d/dy -- 0 in the field variant --, d/dx0, d/dx1); l is [N].  Either output may be NULL.  Gaussian noise model only. */
int gpc_sparse_likelihood(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y,
                          double* dX, double* l);
int gpc_sparse_likelihood_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1,
                              const double* y, double* dX, double* l);
/* size() of every patch GP (src/sparse_gp.hpp:35-39) -- host pointer */
int gpc_sparse_sizes(gpc_sparse* g, int32_t* bv_count);
/* state read-back for tests (host pointers; each may be NULL): alpha [P][ny][cap1], C,Q [P][cap1][cap1] column-major,
 * BV [P][cap1][2], with cap1 = gpc_sparse_ld(g).  C and Q are symmetric matrices stored in full; the add kernels may work on
 * one triangle and mirror it (a state that went through them at capacity > 64 comes back exactly symmetric, a smaller one
 * carries the rounding of its rank-one updates in both triangles): a state handed to gpc_sparse_set_state must be symmetric
 * to rounding, as every state of the recursion is. */
int gpc_sparse_get_state(gpc_sparse* g, double* alpha, double* C, double* Q, double* BV);
int gpc_sparse_ld(const gpc_sparse* g);
/* inverse of gpc_sparse_get_state, for loading a stored model (row f3; the reference's save_compressed writes nothing,
 * src/gp_compressor.cpp:21-27): same layouts, host pointers; C and Q may be NULL (zeroed -- enough for the mean prediction) */
int gpc_sparse_set_state(gpc_sparse* g, const int32_t* bv_count, const double* alpha, const double* C, const double* Q,
                         const double* BV);
/* The map grew (gpc_patches_insert_cloud): a NEW object of P_new patches with old's parameters, ny and leading dimension, in which
 * patch old_to_new[i] holds the state of old's patch i -- alpha, C, Q, BV, basis count and the per-patch counters, copied exactly
 * on the device -- and every other patch is empty, as after gpc_sparse_reset, its state zero.  old_to_new: host, old's P entries, strictly
 * increasing, < P_new (else GPC_EINVAL).  old is untouched; the two objects are destroyed independently.  Synchronises the stream. */
int gpc_sparse_remap(gpc_sparse* old, int P_new, const int32_t* old_to_new, gpc_sparse** out);
/* Rate control: prune every patch's basis IN PLACE by continuing the reference's capacity deletion (src/sparse_gp.hpp:206-223 with
 * delete_bv :252-295; field variant src/sparse_gp_field.hpp:219-263) as a step of its own.  Per patch, with b its basis count and
 * t = max(1, target[p]) (target == NULL: t = keep):
 *     loop:
 *       if b <= 1: stop
 *       scan i = 0 .. b-1 ascending:  s_i = (sum_c alpha[c][i]^2) / (Q_ii + C_ii)
 *       (minscore, loc) = the reference's arg-min: `if (i == 0 || s_i < minscore)` -- a NaN score at index 0 sticks, a NaN score
 *                         at any other index is never chosen, equal scores go to the lower index
 *       if b > t:                      remove
 *       else if minscore < score_tol:  remove              (a NaN minscore compares false: stop)
 *       else:                          stop
 *       order[p][step] = loc;  scores[p][step] = minscore;  delete_bv(loc);  b -= 1;  step += 1
 * Afterwards the patch's basis count is b and removed[p] = step; its point counter is untouched.  If at least one vector was removed
 * and C(0,0) is NaN the patch's sticky status becomes GPC_STATUS_NAN, as after an add.  An empty patch is left alone.  delete_bv runs
 * on the full matrices in every workgroup shape and there are no atomics: the same state gives the same bits, whatever the shape.
 *   keep      used when target == NULL; must then be >= 1 (else GPC_EINVAL)
 *   target    [P] or NULL.  Entries below 1 count as 1 (a device array cannot be validated without a synchronisation)
 *   score_tol >= 0; +inf prunes every patch down to one vector; NaN or a negative value is GPC_EINVAL.  0 removes by count only
 *   removed   [P], may be NULL
 *   order, scores  [P][ld] with ld = gpc_sparse_ld(g), each may be NULL: the removal trace.  `order` holds the index each removed
 *             vector had when it went (delete_bv moves the last vector into its place).  Entries at and beyond removed[p] are left
 *             as they were
 *   status    [P], may be NULL: the sticky status of every patch after the call
 * ny = 1 and ny = 3; params.ref_field_delete_bug applies as in the add path (with it set, the field variant multiplies by q* + c* where
 * the derivation divides: a few removals per patch stay finite, a long chain diverges as it does while training).  The capacity of the object is unchanged, so later
 * gpc_sparse_add calls may grow the basis again.  The call is destructive: gpc_sparse_remap with P_new = P and the identity table is
 * the non-destructive copy to prune from (one trained object then gives every rate below it).
 * gpc_sparse_prune_dev takes DEVICE pointers, enqueues on the context's stream and never synchronises; gpc_sparse_prune takes HOST
 * pointers and is synchronous.  P == 0: GPC_OK.  GPC_EINVAL: a NULL or dead object, and the argument errors above. */
int gpc_sparse_prune(gpc_sparse* g, int keep, const int32_t* target, double score_tol, int32_t* removed, int32_t* order, double* scores,
                     int32_t* status);
int gpc_sparse_prune_dev(gpc_sparse* g, int keep, const int32_t* target, double score_tol, int32_t* removed, int32_t* order,
                         double* scores, int32_t* status);
/* Rate control against a distortion bound: the removals of gpc_sparse_prune, each taken only if the mean square error of the state it
 * would leave, on the patch's own points, stays within the patch's bound ("the smallest model whose error stays below X").  IN PLACE.
 * The batch is ragged like gpc_sparse_predict_points: patch p owns rows off[p] .. off[p+1]-1 of x0, x1 and of the ny planes of y (plane c
 * at y + c * n_total) -- normally the points the object was trained on.  With n = off[p+1] - off[p], b the patch's basis count,
 * t = max(1, target ? target[p] : keep) and B = max_mse_p ? max_mse_p[p] : max_mse:
 *     mse0[p] = mse(current state)            (n == 0: NaN, and the patch is left alone: removed = 0, not a byte of its state moves)
 *     loop:
 *       if b <= 1 or b <= t: stop              (mse_next[p] = NaN)
 *       (minscore, loc) = the arg-min of gpc_sparse_prune, exactly
 *       alpha' = the alpha that delete_bv(loc) would write;  BV' = BV with vector b-1 moved to loc
 *       e = mse(alpha', BV', b-1)              (a look-ahead: nothing has been written yet)
 *       if !(e <= B): mse_next[p] = e; stop    (a NaN e, or a NaN entry of max_mse_p, compares false: stop)
 *       order[p][step] = loc; scores[p][step] = minscore; mse[p][step] = e; delete_bv(loc); b -= 1; step += 1
 * mse of a state (alpha, BV, b), in a summation order that is fixed and does not depend on the workgroup shape:
 *     k_ij = sigmaf_sq * exp(c_exp * ((x0_i-BV_j0)^2 + (x1_i-BV_j1)^2)), c_exp = (double)(-0.5f) / l_sq, the library's exp
 *     f_ci = sum_j alpha_cj k_ij, j ascending in the state's own index order;   e_i = sum_c (y_ci - f_ci)^2, c ascending
 *     point i goes to class i mod 64, each class sums its e_i in ascending i, the 64 class sums are added by the xor-shuffle tree
 *     d = 32, 16, .. 1;   mse = sse / (double)(n * ny)
 * Afterwards removed[p] = step; the basis count, the sticky status, the untouched point counter and the untouched trace entries at and
 * beyond removed[p] follow gpc_sparse_prune.  Every output pointer may be NULL; order, scores and mse are [P][ld], mse0 and mse_next [P].
 *   - The loop stops at the FIRST look-ahead that exceeds the bound.  The error is not monotone along the chain (removing a vector can
 *     lower it), so a later state might have been inside the bound again; the call does not search for it.
 *   - With max_mse = +inf and max_mse_p == NULL the call leaves, bit for bit, the state, removed, order and scores of
 *     gpc_sparse_prune(keep, target, score_tol = 0), and mse is the patch's rate-distortion curve.  Run it on a gpc_sparse_remap identity
 *     copy to get the curve without touching the model.
 *   - target >= b removes nothing and still returns mse0: that is how a caller forms relative bounds such as max_mse_p = 2 * mse0.
 *   - The same inputs give the same bits in every workgroup shape; there are no atomics.
 * GPC_EINVAL: a NULL or dead object; keep < 1 with target == NULL; max_mse NaN or negative with max_mse_p == NULL; n_total < 0; NULL off
 * with P > 0; NULL x0, x1 or y with n_total > 0; an object whose noise_model is not 0.  P == 0: GPC_OK.
 * gpc_sparse_prune_rd_dev takes DEVICE pointers, enqueues on the context's stream and never synchronises; gpc_sparse_prune_rd takes HOST
 * pointers (n_total = off[P]) and is synchronous. */
int gpc_sparse_prune_rd(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y, int keep,
                        const int32_t* target, double max_mse, const double* max_mse_p, int32_t* removed, int32_t* order, double* scores,
                        double* mse, double* mse0, double* mse_next, int32_t* status);
int gpc_sparse_prune_rd_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y, int keep,
                            const int32_t* target, double max_mse, const double* max_mse_p, int32_t* removed, int32_t* order,
                            double* scores, double* mse, double* mse0, double* mse_next, int32_t* status);
/* Rate control by precision: the fewest bits per coefficient whose error stays within the patch's bound.  Pruning decides how many
 * coefficients a leaf keeps, this call how precisely each is stored.  NOT in place: g is only read.  The batch (off, x0, x1, y in ny
 * planes, n_total) and the error mse(alpha, BV, b) -- definition and summation order -- are those of gpc_sparse_prune_rd.
 * The scalar quantiser, for an array v[0..b) of finite doubles and a width w in 1..16 (one definition for the kernels and the host,
 * csrc/gpc_device.h):
 *     lo = (double)(float) of min v rounded toward -inf;  hi = (double)(float) of max v rounded toward +inf     (independent of w)
 *     step = (hi - lo) / (double)(2^w - 1)
 *     q_i = step > 0 ? clamp(rint((v_i - lo) / step), 0, 2^w - 1) : 0          (rint: round-half-even)
 *     v'_i = lo + (double)q_i * step                                            (every operation rounded once, no FMA)
 * A patch's ny + 2 arrays are quantised separately at ONE width: BV column 0, BV column 1, then the alpha planes.
 * Per patch, with b its basis count (clamped to ld), n = off[p+1] - off[p] and B = max_mse_p ? max_mse_p[p] : max_mse:
 *     mse0[p] = mse(current state)                  (n == 0: NaN);  status[p] = the object's sticky status
 *     the patch ESCAPES if b == 0, n == 0 or any of its b (ny + 2) values is not finite: bits[p] = 0, mse_q[p] = NaN, and nothing else
 *     of the patch is written -- the caller stores such a leaf raw
 *     otherwise range[p] is written, and for w = bits_min .. bits_max ascending:
 *       e = mse(alpha', BV', b) with every array quantised at w, the state's index order unchanged;  curve[p][w-1] = e
 *       if e <= B: bits[p] = w, mse_q[p] = e, the codes of this width go to q_alpha[p] / q_bv[p] (entries at and beyond b are left as
 *       they were); stop                             (a NaN e or a NaN B compares false)
 *     no width accepted: bits[p] = 0, mse_q[p] = NaN (range and the evaluated curve entries are written)
 * Outputs, each may be NULL: bits [P], q_alpha [P][ny][ld] and q_bv [P][ld][2] uint16, range [P][ny+2][2] float (rows in the array
 * order above, each (lo, hi)), mse0, mse_q [P], curve [P][16] (entries of widths not evaluated are left as they were), status [P].
 *   - The FIRST accepted width wins.  The error is not monotone in w (a coarser grid can happen to fit better), and the call does not
 *     search further.
 *   - max_mse = 0 evaluates every width of bits_min .. bits_max and so yields the whole rate-distortion curve (on noisy data).
 *   - max_mse = +inf accepts bits_min.
 *   - The same inputs give the same bits in every workgroup shape; there are no atomics.
 * GPC_EINVAL: a NULL or dead object; bits_min < 1, bits_max > 16 or bits_min > bits_max; max_mse NaN or negative with max_mse_p == NULL;
 * n_total < 0; NULL off with P > 0; NULL x0, x1 or y with n_total > 0; an object whose noise_model is not 0.  P == 0: GPC_OK.
 * gpc_sparse_quantize_rd_dev takes DEVICE pointers, enqueues on the context's stream and never synchronises; gpc_sparse_quantize_rd
 * takes HOST pointers (n_total = off[P]) and is synchronous. */
int gpc_sparse_quantize_rd(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y, int bits_min, int bits_max,
                           double max_mse, const double* max_mse_p, int32_t* bits, uint16_t* q_alpha, uint16_t* q_bv, float* range,
                           double* mse0, double* mse_q, double* curve, int32_t* status);
int gpc_sparse_quantize_rd_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y,
                               int bits_min, int bits_max, double max_mse, const double* max_mse_p, int32_t* bits, uint16_t* q_alpha,
                               uint16_t* q_bv, float* range, double* mse0, double* mse_q, double* curve, int32_t* status);
/* The decoder.  For every patch with bits[p] in 1..16: alpha and BV become the dequantised values v' of the codes (layouts and range as
 * above; entries at and beyond bv_count[p] are zero), the basis count becomes bv_count[p], and C and Q are zeroed -- the patch is as
 * gpc_sparse_set_state with NULL C and Q leaves it.  A patch with bits[p] == 0 is not touched: load the raw leaves with
 * gpc_sparse_set_state first.  GPC_EINVAL: a NULL or dead object; a NULL array with P > 0; in the host form a count outside 0..ld or
 * a width outside 0..16 (the _dev form clamps both).  P == 0: GPC_OK.  _dev: DEVICE pointers, the context's stream, no synchronisation. */
int gpc_sparse_dequantize(gpc_sparse* g, const int32_t* bv_count, const int32_t* bits, const uint16_t* q_alpha, const uint16_t* q_bv,
                          const float* range);
int gpc_sparse_dequantize_dev(gpc_sparse* g, const int32_t* bv_count, const int32_t* bits, const uint16_t* q_alpha, const uint16_t* q_bv,
                              const float* range);
/* Rate control to a byte budget: the allocator.  The calls above decide leaf by leaf; this one decides ACROSS rows -- a row is one GP of
 * one leaf -- how many removals each takes, so that at least `need` bytes are saved and the total weighted error is smallest.  It only
 * allocates: the curves come from gpc_sparse_prune_rd (max_mse = +inf on a gpc_sparse_remap identity copy: kmax = removed, d0 = mse0,
 * d = mse), and gpc_sparse_prune_dev(target = b - k, score_tol = 0) replays exactly the first k removals of that chain.
 * Row r of R has
 *     kmax[r] >= 0 removals on its curve (clamped to 0 .. ld): the options are k = 0 .. kmax[r]
 *     the error after k removals  e_r(k) = (k == 0 ? d0[r] : d[r * ld + k - 1])
 *     a weight w[r] (w == NULL: w_all for every row) and unit[r] bytes saved per removal (unit == NULL: unit_all; entries < 1 count as 1)
 * and, at a multiplier lambda >= 0 (one definition for the kernels and the host, csrc/gpc_device.h):
 *     D(k) = w_r * e_r(k)                                                       (one rounded product)
 *     rate(k) = unit_r * (kmax_r - k)                                           (int64)
 *     c(k) = D(k) + (rate(k) == 0 ? 0.0 : lambda * (double)rate(k))             (product and sum rounded once each, no FMA)
 *     choice_r(lambda) = 0 if c(0) is NaN (the row is fixed), else the LARGEST k that attains the minimum of c over the options whose
 *       cost is not NaN -- the scan "k ascending, replace the best iff c(k) <= c(best)": ties go to fewer bytes, a NaN is never chosen
 *     S(lambda) = sum_r unit_r * choice_r(lambda)                               (int64, exact: the order of the sum is free)
 * Given `need` bytes to save:
 *     S(+inf) < need:  INFEASIBLE.  k = choice(+inf), feasible = 0, lambda = +inf
 *     S(0) >= need:    FREE (always so for need <= 0).  k = choice(0), feasible = 1, lambda = 0; it may remove vectors where a removal
 *                      does not raise the error
 *     otherwise bisect on the BIT PATTERN of lambda: lo = bits(0.0), hi = bits(+inf); while hi - lo > 1: mid = lo + (hi - lo) / 2,
 *       hi = mid if S(double(mid)) >= need, else lo = mid.  At most 63 steps; the outcome is defined by this procedure, not by a
 *       property of S.  lambda = double(hi), k_hi = choice(lambda), feasible = 1
 *       refine == 0: k = k_hi
 *       refine != 0: k_lo = choice(double(lo)), delta_r = unit_r (k_hi(r) - k_lo(r)), E_r = S(double(lo)) + sum_{q < r} delta_q (an int64
 *         exclusive scan in ascending r), k(r) = E_r < need ? k_hi(r) : k_lo(r); if that saves less than need (only possible with a
 *         negative delta), k = k_hi.  Rows whose curves tie at lambda are so switched in ascending row order only until the saving is
 *         met: the overshoot is less than one row's step.
 * Outputs (each may be NULL): k [R]; target [R] = max(1, count[r] - k[r]), ready for gpc_sparse_prune_dev (needs count [R], the rows'
 * basis counts); and *result: lambda as above, saved = sum unit_r k(r), max_saving = S(+inf), feasible, switched_rows = the rows
 * whose k differs from k_lo(r) (0 outside a refined bisection).
 * GPC_EINVAL: a NULL or dead ctx; R < 0; ld < 1; NULL kmax, d0 or d with R > 0; w_all NaN or negative with w == NULL; unit_all < 1 with
 * unit == NULL; target without count.  R == 0: GPC_OK, nothing is written.
 * gpc_rate_allocate_dev takes DEVICE pointers (result too), enqueues a fixed sequence of launches on the context's stream -- the two end
 * points, 63 sweeps that are no-ops once the bracket has closed, k_hi and k_lo, the scan, the write-out -- and never reads back or
 * synchronises; scratch is the context's workspace.  The totals are integer atomics: the same inputs give the same bits in every
 * grid shape.  gpc_rate_allocate takes HOST pointers and is synchronous. */
typedef struct gpc_rate_result {
    double lambda;
    int64_t saved, max_saving;
    int32_t feasible, switched_rows;
} gpc_rate_result;
int gpc_rate_allocate(gpc_ctx* ctx, int R, int ld, const int32_t* kmax, const double* d0, const double* d, const double* w, double w_all,
                      const int32_t* unit, int unit_all, int64_t need, int refine, const int32_t* count, int32_t* k, int32_t* target,
                      gpc_rate_result* result);
int gpc_rate_allocate_dev(gpc_ctx* ctx, int R, int ld, const int32_t* kmax, const double* d0, const double* d, const double* w, double w_all,
                          const int32_t* unit, int unit_all, int64_t need, int refine, const int32_t* count, int32_t* k, int32_t* target,
                          gpc_rate_result* result);

/* ---- hyper-parameter training: the live part of sparse_gp::train_parameters ---------------- */
/* src/sparse_gp.hpp:586-640 up to the exit(0) at :640 (the call site is commented out upstream, src/gp_compressor.cpp:161):
 * gradient ascent on kernel.param()(0) = sigma_f^2 with the trained state held fixed, per patch and entirely on the device,
 *     do { delta = sum_i likelihood_dtheta(x_i, y_i);          (:510-519, kernel_dtheta src/rbf_kernel.cpp:49-58)
 *          p(0) += step * delta(0);                            (:624, step = 1e-4f upstream)
 *          ls.push_back(sum_i log_likelihood(x_i, y_i));       (:625-627, :356-385)
 *          if (counter > max_counter) break; ++counter;        (:630-633, max_counter = 100 upstream)
 *     } while (delta.norm() > 1e-2f);                          (:636)
 * A patch with fewer than 20 basis vectors is left alone like upstream (:609-611): iters = 0, p0 = the object's value.
 * ny == 1 only.  Outputs per patch: p0[P] the trained sigma_f^2, iters[P], ls[P][max_counter + 2] the likelihood trace the
 * reference plots, delta[P][2] the last gradient.  The object itself is not modified (upstream re-trains in the outer loop
 * the exit(0) cuts off): create a new gpc_sparse with the trained parameter to use it. */
int gpc_sparse_train_sigmaf(gpc_sparse* g, const int32_t* off, const double* x0, const double* x1, const double* y, double step,
                            int max_counter, double* p0, int32_t* iters, double* ls, double* delta);
int gpc_sparse_train_sigmaf_dev(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y,
                                double step, int max_counter, double* p0, int32_t* iters, double* ls, double* delta);

/* ---- the step after the path: reprojection + colour clamp, fused ------------------------ */
/* The tail of the patch loop of gp_compressor::load_compressed (src/gp_compressor.cpp:335-373, flatten_colors :251-265):
 * pt = R_i (f*, x*_0, x*_1) + mean_i as float, rgb = clamp(short(C* + RGB_mean_i)), written as pcl::PointXYZRGB records.
 * Patches with bv_count[i] == 0 are skipped and the output is compacted in patch order (the reference's `counter`,
 * :299-301); bv_count == NULL means every patch is trained.  f_star [P][m]; c_star [P][3][m] or NULL (colours 0);
 * rotations [P][9] column-major (columns = normal, u, v); means, rgb_means [P][3].  cloud must hold P*m records;
 * n_points receives the number written (device pointer in the _dev variant).  Bit-identical to the CPU oracle. */
typedef struct gpc_point_xyzrgb {   /* memory layout of pcl::PointXYZRGB: 32 bytes */
    float x, y, z, w;               /* w = 1.0f (PCL_ADD_POINT4D) */
    uint8_t b, g, r, a;             /* PCL_ADD_RGB; a = 255 */
    float pad[3];
} gpc_point_xyzrgb;
int gpc_reproject(gpc_ctx* ctx, int P, int m, const int32_t* bv_count, const double* xs0, const double* xs1, const double* f_star,
                  const double* c_star, const double* rotations, const double* means, const double* rgb_means,
                  gpc_point_xyzrgb* cloud, int32_t* n_points);
int gpc_reproject_dev(gpc_ctx* ctx, int P, int m, const int32_t* bv_count, const double* xs0, const double* xs1,
                      const double* f_star, const double* c_star, const double* rotations, const double* means,
                      const double* rgb_means, gpc_point_xyzrgb* cloud, int32_t* n_points);

/* ---- the step before the path: the patch producer on the GPU ---------------------------- */
/* gp_compressor::project_cloud + compute_rotation + project_points (src/gp_compressor.cpp:177-249, 29-64, 66-118): a
 * pcl::PointXYZRGB cloud in, the ragged patch batch of the entry points above out, resident in HBM -- voxel leaves of
 * side `res` (anchored at the cloud's minimum corner, visited in ascending (z, y, x) order), radiusSearch(center,
 * sqrt(3)/2 res) over the 27 neighbouring voxels, plane frame R_i from the smallest singular vector of the homogeneous
 * points (:35-61), exclusive point ownership in leaf order (occupied_indices, :81-89), the +-res/2 window (:85-87), depth
 * and colour mean removal (:101-107), centre shift (:116) and the sz x sz occupancy mask W (:90-92, :117).
 * The arithmetic is the oracle's operation for operation (no FMA contraction): every output is bit-identical to it.
 * gpc_project_cloud takes a HOST cloud, gpc_project_cloud_dev a DEVICE cloud; both synchronise (the sizes of the
 * result depend on the data) and return an object owning the device buffers.  Errors: GPC_EINVAL (res <= 0, sz < 1,
 * a non-finite coordinate), GPC_ERANGE (more than 2^21 voxels along an axis, or 2^62 in total). */
typedef struct gpc_patches gpc_patches;
typedef struct gpc_patches_view {
    int32_t P, n_total, n_max, m;     /* patches (= leaves), points owned in total, largest patch, sz*sz */
    const int32_t* off;               /* P + 1 */
    const double *x0, *x1, *y;        /* n_total: pt(1), pt(2), mean-removed pt(0)   (X and y of :146-155) */
    const double* rgb;                /* 3 planes of n_total: mean-removed colours   (C of :146-155) */
    const double* rotations;          /* P x 9 column-major (columns = normal, u, v) */
    const double *means, *rgb_means;  /* P x 3 */
    const uint8_t* W;                 /* P x m occupancy mask */
    const int32_t* src;               /* n_total: index of the cloud point behind each patch point */
} gpc_patches_view;
int gpc_project_cloud(gpc_ctx* ctx, const gpc_point_xyzrgb* cloud, int n, double res, int sz, gpc_patches** out);
int gpc_project_cloud_dev(gpc_ctx* ctx, const gpc_point_xyzrgb* cloud, int n, double res, int sz, gpc_patches** out);
/* sizes + DEVICE pointers (valid until gpc_patches_destroy): feed them to gpc_dense_fit_predict_grid_dev /
 * gpc_sparse_add_dev / gpc_reproject_dev without a host round trip.  The buffers are READ-ONLY for the caller: the dense entry
 * points recognise the context's most recent batch by its `off` buffer and P, and size their per-size-class launches from the
 * counts the producer took while cutting it. */
int gpc_patches_view_dev(const gpc_patches* p, gpc_patches_view* view);
/* copy to HOST buffers sized by the view's counts; NULL pointers are skipped */
int gpc_patches_fetch(const gpc_patches* p, int32_t* off, double* x0, double* x1, double* y, double* rgb, double* rotations,
                      double* means, double* rgb_means, uint8_t* W, int32_t* src);
void gpc_patches_destroy(gpc_patches* p);

/* ---- mapping (gp_mapping::insert_into_map, src/gp_mapping.cpp:37-152): a registered scan goes into the map ---------------------
 * Cuts `cloud` (n records; _dev: device pointer) against the leaf table of `model` and returns a NEW batch; `model` is untouched
 * and both are destroyed independently.  Synchronous, like gpc_project_cloud (sizes depend on the data).
 *   leaves   every leaf of the model, plus every voxel new to it whose search sphere holds >= min_nbr scan points (:126; upstream
 *            min_nbr = 100).  The leaf table is the merge of the two sorted key lists, leaf id = position in it (the reference
 *            appends instead, :88-95); old_to_new (host, the model's P entries) is the resulting monotone renumbering.
 *   grid     res, sz and the anchor are the model's; the grid grows by whole voxels to cover the scan, below the anchor too.
 *            Non-finite coordinate: GPC_EINVAL; more than 2^21 voxels along an axis: GPC_ERANGE.
 *   frames   kept  = old leaf whose depth GP (`depth`, ny == 1, the model's P; NULL: every leaf counts as trained) is not empty
 *                    (:115): keeps R_i, mean_i, rgb_mean_i (transform_to_old, :213-243);
 *            fresh = new leaf, or old leaf with an empty depth GP and >= min_nbr scan points in its sphere (:121-137): the
 *                    producer's treatment on the scan's points (frame of the sphere's moment matrix, origin at the voxel centre,
 *                    depth-mean shift and colour mean over what it owns, transform_to_new :245-291);
 *            an old untrained leaf below min_nbr keeps its frame and gets no points.
 *   points   every scan point goes to the first kept or fresh leaf in leaf order, out of the <= 27 around its voxel, whose search
 *            sphere (around the voxel centre, :96) holds it and whose +-res/2 window -- around the stored mean for a kept leaf
 *            (:227-228), around the voxel centre for a fresh one (:266-267) -- accepts it.
 *   batch    off / x0 / x1 / y / rgb / src hold the SCAN's points only (what S[i] holds when train_processes runs), ascending scan
 *            index inside a leaf, src = scan index.  Kept leaf: depth as is, colours minus the stored rgb_mean (:237); fresh leaf:
 *            mean-removed depth and colours.  W: old mask | cells hit now (kept, :242), cells hit now (fresh, :290), old mask (other).
 * Deviations: upstream lets to_be_added of a leaf below min_nbr pile up across scans and pairs it with a mis-indexed last_inds
 * (:261); here the threshold looks at the current scan only -- the reference's behaviour for a leaf's first scan.
 * train_classification (the ray-cast free mask, :154-211) is its own entry: gpc_patches_raycast below.
 * The same inputs give the same bits.  Follow with gpc_sparse_remap on both GPs and gpc_sparse_add_dev on the new batch.
 * Both forms synchronise the context's stream, like the cutters: the sizes of the new batch and old_to_new go to the host. */
int gpc_patches_insert_cloud(gpc_ctx* ctx, const gpc_patches* model, const gpc_sparse* depth, const gpc_point_xyzrgb* cloud, int n,
                             int min_nbr, gpc_patches** out, int32_t* old_to_new);
int gpc_patches_insert_cloud_dev(gpc_ctx* ctx, const gpc_patches* model, const gpc_sparse* depth, const gpc_point_xyzrgb* cloud,
                                 int n, int min_nbr, gpc_patches** out, int32_t* old_to_new);

/* ---- mapping (gp_mapping::train_classification, src/gp_mapping.cpp:154-211): the scan's rays label the cells of the leaves ------
 * Every scan ray, from the sensor `origin` to its point, is cast through the leaf table of `map`; on the plane of every trained
 * leaf it crosses between the sensor and the leaf that owns the point, the cell it meets is recorded as seen through (free), on the
 * owner's plane as hit (occupied).  Upstream keeps one boolean per cell (`free`, :203-208), which cannot tell "never seen" from
 * "occupied"; here a cell has three states: */
#define GPC_CELL_UNOBSERVED 0   /* no ray of any scan met the cell: the initial value of a cell buffer */
#define GPC_CELL_OCCUPIED 1     /* free(ind, m) = false, :204: the last ray that met the cell ended in this leaf */
#define GPC_CELL_FREE 2         /* free(ind, m) = true, :207: the last ray that met the cell went on to another leaf */
/* `map` is the batch gpc_patches_insert_cloud (or gpc_project_cloud) cut from THIS cloud: the owner of scan point i is the leaf whose
 * bucket holds it (gp_indices, :66-69, :233, :273), taken from the batch's off / src.  A batch that holds more points than n, or
 * a src entry >= n, is another cloud's: GPC_EINVAL.
 *   trained  a leaf whose depth GP (`depth`, ny == 1, the map's P) has a basis vector (gps[m].size() > 0, :180) at the time of the
 *            call -- upstream that is before train_processes, so pass the remapped object before gpc_sparse_add_dev.  NULL: every leaf.
 *   rays     o32 = float(origin), delta = p - o32 in float (:169), both widened to double for the walk.  A ray does nothing when its
 *            point is unowned (:176), its owner is untrained (:180) or it does not meet the owner's voxel (slab test; :183-190).
 *   walk     from the owner's voxel back towards the sensor, one face at a time: at voxel k the entry parameters
 *            n_a = (face_a - o_a) / delta_a (low face if delta_a > 0, else high; -inf if delta_a == 0) are recomputed from the
 *            integer coordinate; max n_a <= 0: the sensor is in or behind the voxel, stop; else step across the first axis that
 *            attains the maximum; stop on leaving the grid.  This is the reference's j loop (:175) from the far end once reached_gp
 *            is set (:183-190), without the list.
 *   planes   every visited voxel that is a trained leaf m, the owner included (:191-202): normal = column 0 of R_m,
 *            d = normal . (mean_m - origin) / normal . delta with the DOUBLE origin (:194-195), loc = R_m^T (origin + d delta - mean_m),
 *            the +-res/2 window on loc(1), loc(2) (:197), cell = sz * gx + gy with the clipped cell function of W.  A non-finite d or
 *            loc skips the leaf (upstream: undefined behaviour in int(nan)).  As upstream, d is NOT range-checked: a plane that the
 *            ray meets outside the voxel, or behind the sensor, but inside the window, is labelled all the same.
 *   write    upstream's loop is sequential, so the last scan index wins a cell; here integer atomicMax of (i + 1) << 1 | is_free
 *            per (leaf, cell), then touched cells of `cells` become GPC_CELL_OCCUPIED / GPC_CELL_FREE and the others keep what they
 *            held.  The same inputs give the same bits.  n > 2^30: GPC_ERANGE.
 * cells: P x m uint8 in the layout of W, in/out (DEVICE in _dev, HOST otherwise).  origin: host, 3 doubles.  counts: host int32[4] or
 * NULL: rays cast, rays that did nothing, occupied writes, free writes (per ray and leaf, before the tie rule).
 * gpc_patches_raycast_dev enqueues on the context's stream; it synchronises -- and reports what only the device can find: a
 * non-finite coordinate, a src entry >= n -- only when counts != NULL.  In those two cases `cells` is left untouched either way.
 * GPC_EINVAL: a non-finite origin or coordinate, objects of different contexts, a depth with another P or ny != 1, a cloud that is
 * not the batch's.  n == 0: GPC_OK, cells as they were. */
int gpc_patches_raycast(gpc_ctx* ctx, const gpc_patches* map, const gpc_sparse* depth, const gpc_point_xyzrgb* cloud, int n,
                        const double origin[3], uint8_t* cells, int32_t* counts);
int gpc_patches_raycast_dev(gpc_ctx* ctx, const gpc_patches* map, const gpc_sparse* depth, const gpc_point_xyzrgb* cloud, int n,
                            const double origin[3], uint8_t* cells, int32_t* counts);
/* The labelled batch the occupancy GP (gpc_dense_irls_fit_predict_dev) trains on, from a cell buffer: per leaf the observed cells in
 * ascending cell index, at the cell centres of the decompression grid (src/gp_compressor.cpp:326-327),
 * x0 = res*((gx+.5)/sz-.5), x1 = res*((gy+.5)/sz-.5), cell = sz*gx + gy, y = +1 (occupied) / -1 (free).  A leaf without an observed cell
 * is an empty patch.  All buffers on the DEVICE: cells P x m, off P + 1, x0 / x1 / y of capacity P * m.  n_total = off[P] and n_max (the
 * largest patch) are written to the host: the call synchronises, like the cutters. */
int gpc_occupancy_batch_dev(gpc_ctx* ctx, const gpc_patches* map, const uint8_t* cells, int32_t* off, double* x0, double* x1, double* y,
                            int32_t* n_total, int32_t* n_max);

/* ---- rendering: the map as a sensor at a pose would see it ------------------------------------------------------------------------
 * The inverse of a scan: n rays o + t d from one origin are cast through the leaf table of `map`, front to back, and each stops at
 * the first leaf whose depth GP's MEAN SURFACE it meets inside that leaf's window.  Output is organised (record i belongs to ray i):
 * with gpc_camera_rays_dev the cloud is the width x height image a depth camera at that pose would report.  The reference has no
 * such read-out (its only one is load_compressed, every leaf's whole grid); the rule below is this library's, stated per ray with no
 * order left to the scheduler, like the rules of gpc_patches_insert_cloud and gpc_patches_raycast.
 *   objects  map; depth (ny == 1, the map's P) REQUIRED; rgb (ny == 3, the map's P) or NULL (colours 0); cells: P x m uint8 labels
 *            in the layout of W (gpc_patches_raycast) or NULL.  All live objects of ctx, else GPC_EINVAL.
 *   ray      origin o (host, 3 doubles, finite, else GPC_EINVAL) and direction d = dirs[3 i .. 3 i + 2], NOT normalised: t counts in
 *            units of |d|.  A direction with a non-finite component, or all zero, is a miss (images carry masked pixels), not an error.
 *   entry    slab test of o + t d, t >= 0, against the grid box, whose faces on axis a are mn_a + (k - koff_a) res for k = 0 and
 *            kmax_a + 1: per axis with d_a != 0 the two face parameters (face - o_a) / d_a, tn = max of the smaller ones, tf = min of
 *            the larger ones; an axis with d_a == 0 needs lo <= o_a < hi.  The ray meets the box iff tn <= tf and tf >= 0.
 *            t_in = max(tn, 0); start voxel k_a = clamp(floor((o_a + t_in d_a - mn_a) / res) + koff_a, 0, kmax_a).
 *   walk     at voxel k: if k is a leaf L whose depth GP has a basis vector, run the surface test of L; an accepted test ends the
 *            ray (a hit).  Otherwise the exit parameters x_a = (face_a - o_a) / d_a (the HIGH face mn_a + (k_a - koff_a + 1) res if
 *            d_a > 0, else the low face; axes with d_a == 0 are skipped) are recomputed from the integer coordinate, and the ray
 *            steps across the first axis that attains the minimum.  Leaving [0, kmax] is a miss.  At most
 *            kmax_x + kmax_y + kmax_z + 1 voxels are visited (every step moves one coordinate away from the origin).
 *   surface  with R_L = (n, u, v) column-major and mean_L:  a = R_L^T (o - mean_L), c = R_L^T d (each a three-term sum, left to
 *   test     right); t starts on the leaf's plane, t = n.(mean_L - o) / n.d as gpc_patches_raycast evaluates it.  Then exactly
 *            newton_iters times, with no early exit:  q = (a1 + t c1, a2 + t c2);  k_j = sigmaf_sq exp(-0.5f / l_sq |q - BV_j|^2)
 *            with the library's exp;  f = sum_j alpha_j k_j,  (fx, fy) = (sum_j alpha_j k_j (BV_j - q)) / l_sq, j ascending over the
 *            min(basis count, ld) basis vectors;  g = (a0 + t c0) - f;  g' = c0 - (fx c1 + fy c2);  t <- t - g / g'.  One last
 *            evaluation of q, f, g at the final t.  The test is ACCEPTED iff all of:
 *              t, q, f, g finite;   |g| <= eps_rel res;   0 < t <= t_max;
 *              not (q1 > res/2 or q1 < -res/2 or q2 > res/2 or q2 < -res/2)                          (upstream's window form);
 *              x = R_L (f, q1, q2) + mean_L (in gpc_reproject's association, in double) has squared distance <= radius^2 to the
 *              centre of voxel k, radius = float(sqrt(3.0f) / 2.0f) res                            (the producer's membership rule);
 *              use_w != 0:  W[L][cell] != 0, cell = sz gx + gy, gx = clip(int(sz (q1 / res + 0.5)), 0, sz - 1), gy from q2;
 *              cells != NULL:  cells[L][cell] != GPC_CELL_FREE.
 *            A rejected test lets the ray go on to the next voxel.
 *   hit      cloud[i]: xyz = float(x), w = 1, a = 255; r, g, b = flatten_colors(c_k + rgb_mean_L[k]) as gpc_reproject, c the colour
 *            GP's mean at q under ITS parameters and basis (empty basis: the mean colour); 0 without rgb.  leaf[i] = L,
 *            range[i] = t, local[3 i ..] = (f, q1, q2).
 *   miss     x = y = z = NaN (PCL's organised-cloud convention), w = 1, a = 255, colours 0, leaf = -1, range = NaN, local = NaN.
 *   counts   host int32[5] or NULL: rays; hits; rays that never met the grid (invalid directions included); surface tests run;
 *            tests with finite t, q, f, g and |g| > eps_rel res.
 * Deviations: only the leaves of the voxels a ray visits are tested (as train_classification does): the sliver of a patch that
 * protrudes into a neighbouring voxel that is no trained leaf is not seen.  The predictive sigma and the surface normal at the hits
 * are a second call on the render's leaf and local outputs: gpc_patches_render_attrs below.
 * The same inputs give the same bits: integer atomics (the counters) only.  gpc_patches_render takes HOST dirs / cells / outputs and
 * is synchronous; gpc_patches_render_dev takes DEVICE dirs, cells and per-ray outputs (leaf, range, local may each be NULL), enqueues
 * on the context's stream and synchronises only when counts != NULL.  n == 0: GPC_OK.  GPC_EINVAL: a NULL or destroyed object, objects
 * of different contexts, depth with another P or ny != 1, rgb with another P or ny != 3, a non-finite origin, newton_iters < 0,
 * n < 0, NULL dirs or cloud with n > 0.  GPC_ERANGE: newton_iters > 64. */
typedef struct gpc_render_params {
    int32_t newton_iters;   /* 4 */
    int32_t use_w;          /* 1: a cell the producer's mask W never saw a point in does not stop a ray */
    double eps_rel;         /* 1e-6: accept |g| <= eps_rel * res */
    double t_max;           /* +inf */
} gpc_render_params;
void gpc_default_params_render(gpc_render_params* p);
int gpc_patches_render(gpc_ctx* ctx, const gpc_patches* map, const gpc_sparse* depth, const gpc_sparse* rgb, const uint8_t* cells,
                       const gpc_render_params* params, const double origin[3], const double* dirs, int n, gpc_point_xyzrgb* cloud,
                       int32_t* leaf, double* range, double* local, int32_t* counts);
int gpc_patches_render_dev(gpc_ctx* ctx, const gpc_patches* map, const gpc_sparse* depth, const gpc_sparse* rgb, const uint8_t* cells,
                           const gpc_render_params* params, const double origin[3], const double* dirs, int n,
                           gpc_point_xyzrgb* cloud, int32_t* leaf, double* range, double* local, int32_t* counts);
/* Confidence and surface normal at the hits of a render.  leaf (n) and local (n x 3) are the outputs of gpc_patches_render[_dev], or
 * any arrays of that form: nothing is walked again.  Either output may be NULL.
 *   sigma    [n]: gpc_sparse_predict_scattered_dev(depth, n, leaf, local + 1, local + 2, 3, NULL, sigma, conf, NULL) -- the
 *            predictive sigma of the depth GP at the hit, sqrt(s20 + k* + k^T C k) (src/sparse_gp.hpp:299-351), or with conf != 0 the
 *            0-100 confidence form.  NaN at a miss.
 *   normal   [n][3], unit length, in the world.  With L = leaf[i], q = (local[3 i + 1], local[3 i + 2]) and R_L = (n, u, v):
 *            (fx, fy) = (sum_j alpha_j k_j (BV_j - q)) / l_sq exactly as the surface test of the render forms it (j ascending over the
 *            min(basis count, ld) basis vectors, the library's exp);  frame normal v = (1, -fx, -fy);  w_a = (R[a] + R[a + 3] v1) +
 *            R[a + 6] v2 (gpc_reproject's association);  len = sqrt((w0 w0 + w1 w1) + w2 w2);  normal = w / len.
 *            origin != NULL (host, 3 doubles, finite): x = R_L (local[3 i], q1, q2) + mean_L as the hit rule forms it, e = origin - x,
 *            and when (normal_0 e_0 + normal_1 e_1) + normal_2 e_2 < 0 every component is negated: the normal faces the sensor.
 *            origin == NULL: the normal keeps the sign of the frame's first column.
 *            A miss (leaf outside [0, P)) or a non-finite intermediate gives three NaN.  An empty basis gives the normalised first
 *            column of R_L.
 * gpc_patches_render_attrs takes HOST arrays and is synchronous; gpc_patches_render_attrs_dev takes DEVICE arrays, enqueues on the
 * context's stream and never synchronises.  n == 0: GPC_OK.  GPC_EINVAL: a NULL or destroyed object, objects of different contexts,
 * depth with another P or ny != 1, a non-finite origin, n < 0, NULL leaf or local with n > 0. */
int gpc_patches_render_attrs(gpc_ctx* ctx, const gpc_patches* map, gpc_sparse* depth, int n, const int32_t* leaf, const double* local,
                             const double* origin, int conf, double* sigma, double* normal);
int gpc_patches_render_attrs_dev(gpc_ctx* ctx, const gpc_patches* map, gpc_sparse* depth, int n, const int32_t* leaf,
                                 const double* local, const double* origin, int conf, double* sigma, double* normal);
/* Pinhole rays for gpc_patches_render_dev: pixel i = v width + u gets dir = R ((u - cx) / fx, (v - cy) / fy, 1), R host, column-major
 * (the camera's axes in the world).  Not normalised, so `range` is the depth along the optical axis, as a depth camera reports it.
 * dirs_dev: DEVICE, width * height x 3.  Enqueued on the context's stream.  GPC_EINVAL: negative sizes, fx or fy zero or not finite,
 * a non-finite R, cx or cy; GPC_ERANGE: more than 2^31 - 1 pixels. */
int gpc_camera_rays_dev(gpc_ctx* ctx, const double R[9], double fx, double fy, double cx, double cy, int width, int height,
                        double* dirs_dev);

/* ---- masked decode: the map to a cloud in one pass, only the cells that hold data ------------------------------------------------ */
/* The patch loop of gp_compressor::load_compressed (src/gp_compressor.cpp:298-380) -- predict the depth GP and the colour GP of every
 * trained leaf on its sz x sz grid, reproject, clamp -- fused, and restricted to the grid points whose cell holds data: the producer's
 * occupancy mask W (its use upstream is commented out, :323-325) and / or the ray cast's cell labels.  depth (ny == 1) is required; rgb
 * (ny == 3, the same P) may be NULL: the colours are then 0 and rgb_means may be NULL.  Both are live objects of one context.
 *   grid     m = sz * sz.  Grid point p has gx = p % sz, gy = p / sz and the coordinates q0 = res (((double)gx + 0.5) / (double)sz - 0.5),
 *            q1 likewise from gy: the grid of gpc_dense_fit_predict_grid.  Its cell in the layout of W and of `cells` is
 *            c(p) = sz gx + gy: the producer's cell function (gpc_patches_raycast), transposed against p.
 *   kept     Leaf L is decoded iff depth's basis count of L is > 0 (the reference's `gps[i].size() == 0` skip, :299-301).  Point (L, p)
 *            is kept iff L is decoded, and W == NULL or W[L m + c(p)] != 0, and cells == NULL or cells[L m + c(p)] != GPC_CELL_FREE.
 *   order    The kept points are written in ascending (L, p).  No atomics: the same inputs give the same bytes.
 *   record   Record j of kept (L, p) is, bit for bit, the record gpc_reproject_dev writes for that point from the outputs of
 *            gpc_sparse_predict_dev on the two objects: f = sum_j alpha_j k_j, j ascending over the min(basis count, ld) vectors, k_j =
 *            sigma_f^2 exp((double)(-0.5f) / l^2 |q - BV_j|^2) with the library's exp, accumulated as the predict kernels accumulate it; the
 *            colour mean likewise per plane under rgb's own parameters and basis (an empty colour basis gives the mean colour);
 *            xyz[i] = (float)(((R[i] f + R[i + 3] q0) + R[i + 6] q1) + mean[i]) with no contraction, rgb = flatten_colors(c + rgb_mean),
 *            w = 1, a = 255, pad zero.  leaf[j] = L, point[j] = p.
 *   counts   count[L] is the number of kept points of L (0 for a leaf that is not decoded); *n_points = sum_L count[L], the FULL count
 *            even where it exceeds capacity.  Records and leaf / point entries with index >= capacity are not written; entries at and
 *            beyond n_points are left as they were.  cloud == NULL is the sizing call: only count and n_points are written and no GP is
 *            evaluated; the caller allocates exactly n_points records for a second call (P m records are always enough).
 *   outputs  W, cells [P][m]; rotations [P][9] column-major, means, rgb_means [P][3] as gpc_reproject takes them; cloud [capacity];
 *            leaf, point [capacity] and count [P] may each be NULL; n_points must not be.
 *   errors   On an error nothing is written.  GPC_EINVAL: a NULL depth or one whose context is gone, rgb of another context, with
 *            another P or with ny != 3, depth with ny != 1, sz < 1, a res that is not finite, capacity < 0, NULL rotations or means
 *            with P > 0 and cloud != NULL, rgb without rgb_means, NULL n_points.  GPC_ERANGE: P m > 2^31 - 1.  P == 0: *n_points = 0,
 *            GPC_OK.
 * gpc_sparse_decode_dev takes DEVICE pointers (n_points included), enqueues on the context's stream and never synchronises or reads
 * back; its scratch (the per-leaf counts and first records) is the context's workspace.  gpc_sparse_decode takes HOST pointers and is
 * synchronous; like gpc_reproject it downloads the count first and then only min(n_points, capacity) records. */
int gpc_sparse_decode(gpc_sparse* depth, gpc_sparse* rgb, double res, int sz, const uint8_t* W, const uint8_t* cells,
                      const double* rotations, const double* means, const double* rgb_means, int capacity, gpc_point_xyzrgb* cloud,
                      int32_t* leaf, int32_t* point, int32_t* count, int32_t* n_points);
int gpc_sparse_decode_dev(gpc_sparse* depth, gpc_sparse* rgb, double res, int sz, const uint8_t* W, const uint8_t* cells,
                          const double* rotations, const double* means, const double* rgb_means, int capacity, gpc_point_xyzrgb* cloud,
                          int32_t* leaf, int32_t* point, int32_t* count, int32_t* n_points);

/* ---- cloud-to-cloud distortion: exact nearest neighbour, D1 / D2 / colour ------------------------------------------------------------ */
/* What a point-cloud codec reports: for every point of cloud A (na records) its nearest neighbour in cloud B (nb records), and from it
 * the point-to-point error D1, the point-to-plane error D2 and the colour error, summed over A.  ONE direction, A -> B, per call; a
 * symmetric figure is two calls.  The rule is stated per point, with nothing left to the scheduler, and no number it gives depends on
 * `cell`, which only sizes the search table.
 *   valid    A record is valid iff x, y and z are all finite.  Invalid records of B are never a neighbour; invalid records of A get
 *            nn = -1, d2 = e2 = NaN and count nowhere.  (The organised clouds of gpc_patches_render carry NaN misses: usable as either.)
 *   d2       For valid a, b:  dx = (double)a.x - (double)b.x, dy, dz likewise;  d2(a, b) = (dx dx + dy dy) + dz dz, no contraction.
 *   nn       nn[i] = the valid record of B with the smallest d2(a_i, .); of several with that d2, the LOWEST index in B: the EXACT
 *            nearest neighbour, as a scan of B in ascending index gives it.  Not approximate at any cell, density or position of A
 *            (inside B's box, on a voxel face, far outside it): the ring search stops only when (r - 2^-20)^2 cell^2 plus A's squared
 *            distance outside the table's box, less the rounding of its own terms, STRICTLY exceeds the best d2.
 *   none     If that d2 > max_dist max_dist (formed in double), or B has no valid record: nn = -1, d2 = e2 = NaN; the point counts
 *            in n_valid, not in n_matched.  max_dist = +inf (the default) searches exhaustively; max_dist = 0 matches coincident points.
 *   e2       With normals_b != NULL (nb x 3 floats, indexed like B) and the neighbour's normal finite in all three components:
 *            e2 = ((dx n0 + dy n1) + dz n2)^2, the normal widened to double, used as given and NOT renormalised.  Otherwise e2 = NaN
 *            and the point is not in n_plane.
 *   colour   Per matched point, from the integer channel differences dr, dg, db (a minus b):  (double)dc (double)dc per channel, in
 *            r, g, b order, and ((0.2126 dr + 0.7152 dg) + 0.0722 db)^2.
 *   sums     A sum over an array of values indexed by i (the record index of A; entries that do not take part contribute +0.0) is
 *            taken in chunks of 4096 consecutive entries: inside a chunk entry i goes to class i mod 64, each class adds its entries in
 *            ascending i starting from +0.0, and the 64 class sums s go through the xor-shuffle tree  s[c] <- s[c] + s[c ^ d],
 *            d = 32, 16, .. 1 (the tree of gpc_sparse_prune_rd's mse), whose s[0] is the chunk's sum.  The array of chunk sums is
 *            summed by the same rule, and again, until one value is left.  Maxima are 0 where nothing takes part.  No atomics: the
 *            same inputs give the same bytes, at every cell.
 *   outputs  nn (int32), d2, e2 (double): na entries each, any may be NULL.  result: see the struct.  na == 0: result all zero, GPC_OK.
 *   errors   On an error nothing is written.  GPC_EINVAL: a NULL or destroyed ctx, negative na or nb, NULL A with na > 0, NULL B with
 *            nb > 0, NULL result, cell negative or not finite, max_dist NaN or negative.  GPC_ERANGE: a cell so small that B's box
 *            spans more than 2^21 voxels along an axis (the cutters' key limit); cell = 0, the library's choice, never does: it is
 *            c0 = max(sqrt(4 e1 e2 / nv), e1 / 2^20) with e1 >= e2 the two largest extents of B's box and nv its valid records (four
 *            points per voxel if B were a surface filling its box), and where that table holds more than 8 points per OCCUPIED voxel
 *            on average (a patchy or folded surface), max(c0 sqrt(4 / that average), e1 / 2^20).  params == NULL: the defaults.
 * gpc_cloud_distortion_dev takes DEVICE pointers, result included, works on the context's stream and in its workspace, and
 * SYNCHRONISES the stream while it builds the table (its size depends on the data), as the cutters do; the search and the sums are
 * enqueued behind that, so the outputs are complete once the stream is.  gpc_cloud_distortion takes HOST pointers and is synchronous. */
typedef struct gpc_distortion_params {
    double cell;       /* voxel side of the search table over B; 0 = chosen by the library.  A PERFORMANCE knob only */
    double max_dist;   /* a neighbour counts only if d2 <= max_dist * max_dist; +inf = exhaustive (the default) */
} gpc_distortion_params;
typedef struct gpc_distortion_result {
    int64_t n_valid, n_matched, n_plane;     /* A points with finite xyz; of those, with a neighbour; of those, with a finite normal */
    double sse_d1, max_d1;                   /* over matched points: sum and max of d2 */
    double sse_d2, max_d2;                   /* over plane points: sum and max of e2 */
    double sse_rgb[3], sse_luma;             /* over matched points */
} gpc_distortion_result;
void gpc_default_params_distortion(gpc_distortion_params* p);
int gpc_cloud_distortion(gpc_ctx* ctx, const gpc_point_xyzrgb* a, int na, const gpc_point_xyzrgb* b, int nb, const float* normals_b,
                         const gpc_distortion_params* params, int32_t* nn, double* d2, double* e2, gpc_distortion_result* result);
int gpc_cloud_distortion_dev(gpc_ctx* ctx, const gpc_point_xyzrgb* a, int na, const gpc_point_xyzrgb* b, int nb, const float* normals_b,
                             const gpc_distortion_params* params, int32_t* nn, double* d2, double* e2, gpc_distortion_result* result);
/* The normals that make D2 usable on a cloud this library cut: for a batch cut from a cloud of n points, normals[n][3] (float): point
 * src[j] of leaf L (off[L] <= j < off[L + 1]) gets (float) of column 0 of R_L, the plane normal the producer fitted over the leaf's
 * sphere; a point no leaf owns gets three NaN.  GPC_EINVAL: a NULL or destroyed batch, NULL normals with n > 0, n < 0, a batch that
 * holds more points than n or a src entry >= n (gpc_patches_raycast's test: the batch was cut from another cloud); nothing is written
 * then.  gpc_patches_normals_dev takes a DEVICE buffer, works on the context's stream and synchronises it once (the src test);
 * gpc_patches_normals takes a HOST buffer and is synchronous. */
int gpc_patches_normals(const gpc_patches* p, int n, float* normals);
int gpc_patches_normals_dev(const gpc_patches* p, int n, float* normals);

/* ---- scan-to-model registration (SURVEY section 8, row f): gp_registration on the GPU ------------------------------------ */
/* gp_registration (src/gp_registration.h, src/gp_registration.cpp) aligns a scan to a trained model by gradient ascent on the
 * mean likelihood of the scan's points under the per-leaf depth and colour GPs.  One step (registration_step, :73-92) is
 *     assign   every scan point to the first leaf, in leaf order, whose search sphere holds it and whose +-res/2 window accepts
 *              it in that leaf's frame (compute_transformation's leaf walk :146-174 + get_local_points :94-113; leaves whose
 *              depth GP is empty are skipped, :158);
 *     evaluate compute_derivatives + compute_likelihoods of both GPs on every leaf's points (:175-195; the kernel behind
 *              gpc_sparse_likelihood);
 *     reduce   dX = l dCX + cl dX (:196), rotated to the global frame (:202-206), times the 3 x 6 Jacobian of :40-49, averaged
 *              over the points used (:211-215, :245)  ->  delta[6], ls, cls;
 *     update   R = Rx Ry Rz, t (gradient_step :51-58), R_cloud = R R_cloud, t_cloud (+)= t (:83-84), cloud <- R cloud + t as
 *              float (transform_pointcloud :32-38),
 * and here it is enqueued on the context's stream from end to end: no host pass over the points, one 72-byte read-back.
 * The model is what the other entry points produced: a gpc_patches (its voxel table decides the candidate leaves the way the
 * reference's octree does: the <= 27 voxels around the point's own, in ascending leaf order; a point may lie one voxel outside
 * the model's grid and still be inside a leaf's sphere) and two gpc_sparse objects trained on it, depth (ny == 1) and colour
 * (ny == 3), Gaussian noise.  The registration object REFERS to the three and owns none of them: they must belong to the same
 * context and have the same P (else GPC_EINVAL), and once one of them has been destroyed every call on the registration object
 * except its own destroy returns GPC_EINVAL.  It is a child of the context like the others (destroy order is free). */
typedef struct gpc_registration gpc_registration;
typedef struct gpc_registration_params {
    double step;                    /* 1e-1f, src/gp_registration.cpp:10 */
    double tol;                     /* 0.1 on both norms, :69 */
    int32_t min_steps, max_steps;   /* 10, 300 (:69, :10) */
    int32_t ref_translation_sum;    /* 1 = t_cloud += t as written (:84); 0 = t_cloud = R t_cloud + t */
    int32_t reserved;
} gpc_registration_params;
/* step 1e-1f, tol 0.1, min_steps 10, max_steps 300, ref_translation_sum 1 (src/gp_registration.cpp:10, :69, :84) */
void gpc_default_params_registration(gpc_registration_params* p);
/* the constructor's tail (src/gp_registration.cpp:7-16) without the training, which the caller has done */
int gpc_registration_create(gpc_ctx* ctx, const gpc_patches* patches, gpc_sparse* depth, gpc_sparse* rgb, gpc_registration** out);
void gpc_registration_destroy(gpc_registration* r);
/* add_cloud (:60-65): the scan, n records.  Resets R_cloud = I, t_cloud = 0 and the step count.  The object keeps its own
 * working copy (the steps move it): set_cloud takes a HOST buffer, set_cloud_dev a DEVICE buffer that it copies on the stream. */
int gpc_registration_set_cloud(gpc_registration* r, const gpc_point_xyzrgb* cloud, int n);
int gpc_registration_set_cloud_dev(gpc_registration* r, const gpc_point_xyzrgb* cloud, int n);
/* one registration_step (:73-92).  out (host): delta[6] (translation, rotation), ls, cls (get_likelihood, get_color_likelihood
 * :248-256), n_used (points that found a leaf).  No point used: all zero.  The same state gives the same bits.
 * The call synchronises the context's stream: `out` is read back before it returns. */
int gpc_registration_step(gpc_registration* r, const gpc_registration_params* params, double out[9]);
/* steps until registration_done() (:67-70): after a step has raised the step count to s, stop when s > min_steps and either
 * s >= max_steps or both |delta[0:3]| < tol and |delta[3:6]| < tol.  trace (host, [max_steps][9], may be NULL): row k = the out
 * of the k-th step of this call (rows beyond max_steps, possible when min_steps >= max_steps, are not written); steps: how many.
 * Synchronises the context's stream once per step, as gpc_registration_step does. */
int gpc_registration_run(gpc_registration* r, const gpc_registration_params* params, double* trace, int32_t* steps);
/* get_cloud_transformation (:18-22): the accumulated R_cloud [9] column-major and t_cloud [3] (host) */
int gpc_registration_get_transform(gpc_registration* r, double R[9], double t[3]);
/* the working cloud, n records (host) */
int gpc_registration_get_cloud(gpc_registration* r, gpc_point_xyzrgb* cloud);
/* ... as a DEVICE pointer (read-only for the caller; valid until the next set_cloud or destroy): the registered scan goes into
 * gpc_patches_insert_cloud_dev without a host round trip */
int gpc_registration_cloud_dev(gpc_registration* r, const gpc_point_xyzrgb** cloud, int* n);
/* Diagnostic, like gpc_sparse_set_trace: what the LAST step assigned.  owner [n]: the leaf of every scan point, -1 = unused;
 * local [n][3]: its coordinates in that leaf's frame (depth, x0, x1).  Host pointers, each may be NULL. */
int gpc_registration_get_assignment(gpc_registration* r, int32_t* owner, double* local);

/* ---- patch -> rank partition for one process per GPU (src/gp_compressor.cpp:146-163: patches are independent) ----- */
/* Longest-processing-time assignment of P patches with per-patch cost n_i^3 (dense) or n_i*cap^2 (sparse) onto
 * `world` ranks, every rank padded to ceil(P/world) slots so that the single all-gather of f_star is fixed-size.
 * slot_patch has world*ceil(P/world) entries (patch id or -1 for padding), rank r owns slots [r*S, (r+1)*S). */
int gpc_partition_patches(int P, const int32_t* off, int world, int sparse_capacity, int32_t* slot_patch);

/* ---- multi-GPU: the one exchange step ------------------------------------------------------- */
/* Every rank fits + predicts the S = ceil(P / world) slots gpc_partition_patches gave it; ONE ncclAllGather of the slot buffers
 * over RCCL / xGMI, then a device gather to patch order, reassembles f_star [P][row] on every rank.  RCCL is bound at run time
 * (no link-time dependency; a copy already loaded in the process, e.g. PyTorch's, is shared).
 *   one process per GPU:      rank 0 calls gpc_comm_unique_id and hands the 128 bytes to the other ranks by whatever channel
 *                             the host has (file, socket, MPI); every rank: gpc_comm_create(ctx, world, rank, id, &c).
 *                             A communicator the host created itself goes through gpc_comm_adopt (ncclComm_t as void*; not owned).
 *   one process, N GPUs (how the single-process reference would use a node): one gpc_ctx per device, gpc_comm_create_all, and
 *                             the per-device calls bracketed by gpc_group_start / gpc_group_end.  Inside a bracket the
 *                             collectives are only enqueued at gpc_group_end, so pass f_star = NULL to gpc_allgather_fstar_dev
 *                             there and run gpc_unpermute_fstar_dev per device after the bracket.
 * gpc_comm_set_partition(c, P, slot_patch) takes the table gpc_partition_patches filled (host pointer, world * S entries) and
 * keeps its inverse on the device.  gpc_allgather_fstar_dev: local_f [S][row_doubles] (this rank's slots, padding slots
 * included), gathered [world * S][row_doubles] scratch, f_star [P][row_doubles] or NULL; all DEVICE pointers, enqueued on the
 * context's stream, no synchronisation.  A gpc_comm holds a reference on its context like the other children. */
typedef struct gpc_comm gpc_comm;
#define GPC_UNIQUE_ID_BYTES 128
int gpc_comm_unique_id(void* id128);
int gpc_comm_create(gpc_ctx* ctx, int world, int rank, const void* id128, gpc_comm** out);
int gpc_comm_create_all(int ndev, gpc_ctx* const* ctxs, gpc_comm** out /* ndev */);
int gpc_comm_adopt(gpc_ctx* ctx, void* nccl_comm, int world, int rank, gpc_comm** out);
void gpc_comm_destroy(gpc_comm* c);
int gpc_comm_world(const gpc_comm* c);
int gpc_comm_rank(const gpc_comm* c);
/* path of the RCCL library in use ("" before the first communicator) */
const char* gpc_comm_library(void);
int gpc_comm_set_partition(gpc_comm* c, int P, const int32_t* slot_patch);
int gpc_group_start(void);
int gpc_group_end(void);
int gpc_allgather_fstar_dev(gpc_comm* c, int row_doubles, const double* local_f, double* gathered, double* f_star);
int gpc_unpermute_fstar_dev(gpc_comm* c, int row_doubles, const double* gathered, double* f_star);

/* ---- diagnostics ------------------------------------------------------------------------------------------------ */
/* Host-side evaluation of the table-driven exp() the kernels use for the RBF kernel (same source, csrc/gpc_device.h),
 * so that its error against libm -- which the reference calls, src/rbf_kernel.cpp:17 -- can be bounded without a GPU. */
void gpc_test_exp_host(const double* x, double* out, int n);
/* Same for the small-argument polynomial (-2^-5 <= x <= 0) the register-tile kernel switches to when the patch extent
 * proves the range. */
void gpc_test_exp_small_host(const double* x, double* out, int n);
/* Host-side evaluation of the scalar quantiser of gpc_sparse_quantize_rd (same source) on one array v[0..b) at width w: the codes
 * q [b], range = (lo, hi) and the dequantised values deq [b]; each output may be NULL.  GPC_EINVAL: NULL v, b < 1, w outside 1..16. */
int gpc_test_quantize_host(const double* v, int b, int w, uint16_t* q, float* range, double* deq);
/* gpc_rate_allocate on the CPU: the same rule from the same source, no context and no device (host pointers; GPC_EINVAL as there). */
int gpc_test_rate_allocate_host(int R, int ld, const int32_t* kmax, const double* d0, const double* d, const double* w, double w_all,
                                const int32_t* unit, int unit_all, int64_t need, int refine, const int32_t* count, int32_t* k, int32_t* target,
                                gpc_rate_result* result);
/* the multi-threaded staging copy of the host-pointer entries (pageable caller buffers), callable without a GPU: concurrency test */
void gpc_test_par_memcpy(void* dst, const void* src, size_t bytes);
/* The rule that chooses the kernels of a dense batch, callable without a GPU.  The facts of the batch: its sizes, whether the
 * variance is computed, point-wise (1) or grid (0) X*, whether the weights are wanted, the device's CU count, the IRLS entry (1) or
 * the plain one (0); w1_refused: the route after the one-wave kernel's workspace was refused.  The GPC_* switches are read from the
 * environment, as by the entry points.  Returns the kind (-1 no route, 0 nothing to do, 1 one-wave, 2 register, 3 tiled, 4 generic,
 * 5 size-class split); name (if not NULL, name_cap bytes) receives what gpc_last_dense_kernel would report; shape (if not NULL,
 * GPC_TEST_ROUTE_SHAPE entries): one-wave padding and slots per launch | register tile count, factor exported | tiled waves, padding,
 * workgroups per CU | split: with the 257..272 class, with the tiled class. */
#define GPC_TEST_ROUTE_SHAPE 9
int gpc_test_dense_route(int P, int n_max, int n_total, int ny, int m, int variance, int pointwise, int alpha_out, int num_cus,
                         int irls, int w1_refused, char* name, int name_cap, int32_t* shape);

#ifdef __cplusplus
}
#endif
#endif /* GPC_H */
