// sparse_rate.hip -- RATE CONTROL of the batched online sparse GP: what makes a trained state (layout: sparse.hip) smaller, one patch per
// workgroup.  Prune to a count or below a score (gpc_sparse_prune), prune to a distortion bound (gpc_sparse_prune_rd), quantise to the fewest
// bits in a distortion bound (gpc_sparse_quantize_rd), decode the quantised model (gpc_sparse_dequantize).  The removal is the add path's
// own sp_delete_bv and arg-min (sparse_device.h).  The allocator across leaves is rate_alloc.hip, the entry points are in sparse_api.hip.
#include <algorithm>

#include "sparse_device.h"

// The layout of a kernel's dynamic LDS, in doubles, is stated ONCE, as an Sp*Lds below: take(n) gives the offset of the next region, `total`
// what the launch asks for.  The kernel's carve-up and the launcher's byte count both read it.
struct SpCarve {
    int total = 0;
    __host__ __device__ constexpr int take(int n) { const int o = total; total += n; return o; }
};

// ---- what the two prune kernels share -------------------------------------------------------------------------------------------
struct SpPruneCore {
    int P, ny, ld, keep, field_bug;
    const int32_t* target;     // [P] or nullptr (every patch: keep)
    double *alpha, *C, *Q, *BV;
    int32_t *b, *stat;
    int32_t *removed, *order, *status_out;   // each may be nullptr
    double* scores;                          // may be nullptr
};

// opens a patch: its state in HBM, its basis count b, its sticky status st and the count t = max(1, target) it may be pruned to
__device__ static __forceinline__ SpState sp_prune_open(const SpPruneCore& K, int patch, int& b, int& st, int& t)
{
    SpState S;
    S.ld = K.ld; S.ny = K.ny; S.ldm = K.ld;
    S.alpha = K.alpha + (size_t)patch * K.ny * K.ld;
    S.C = K.C + (size_t)patch * K.ld * K.ld;
    S.Q = K.Q + (size_t)patch * K.ld * K.ld;
    S.BV = K.BV + (size_t)patch * K.ld * 2;
    b = K.b[patch];
    if (b > K.ld) b = K.ld;                             // (gpc_sparse_set_state admits no more)
    st = K.stat[patch];
    const int tp = K.target ? K.target[patch] : K.keep;
    t = tp > 1 ? tp : 1;
    return S;
}

// The removal candidate of a patch with b vectors: argmin |alpha_i|^2 / (Q_ii + C_ii) as the reference scans; returns its index, `best` its
// score.  (ny from the kernel argument -- S.ny -- in every kernel, never a template constant: unrolled over a constant, the compiler
// may fuse another product of the sum, and the scores are promised bit for bit between the prune kernels.)
__device__ static __forceinline__ int sp_prune_scan(const SpState& S, int b, double* sval, int* sidx, double& best)
{
    const int ld = S.ld, ny = S.ny;
    int loc = 0x7fffffff;
    bool have = false;
    best = 0.0;
    for (int i = threadIdx.x; i < b; i += SP_NTH) {
        double a2 = 0.0;
        for (int c = 0; c < ny; ++c) { const double a = S.alpha[c * ld + i]; a2 += a * a; }
        const double score = a2 / (S.Q[sp_at<false>(i, i, ld)] + S.C[sp_at<false>(i, i, ld)]);
        if (!have || SP_TAKE(score, i, best, loc)) { best = score; loc = i; have = true; }
    }
    if (!have) best = __builtin_inf();
    sp_block_argmin(best, loc, sval, sidx);
    return (loc < 0 || loc >= b) ? 0 : loc;
}

// closes a patch after `step` removals: isnan(C(0,0)) -> "sparse_gp::C has become Nan" (:245), as after a point of the add path
__device__ static __forceinline__ void sp_prune_close(const SpPruneCore& K, const SpState& S, int patch, int b, int st, int step)
{
    if (step > 0) {
        const double c00 = S.C[0];
        if (c00 != c00 && st == GPC_STATUS_OK) st = GPC_STATUS_NAN;
    }
    if (threadIdx.x == 0) {
        if (step > 0) {
            K.b[patch] = b;
            K.stat[patch] = st;
        }
        if (K.removed) K.removed[patch] = step;
        if (K.status_out) K.status_out[patch] = st;
    }
}

// ---- prune: the capacity deletion of the add path (:206-223 -> delete_bv :252-295 / field :219-263) as a step of its own ---------
// A trained patch keeps removing the vector with the smallest score |alpha_i|^2 / (Q_ii + C_ii) until it holds max(1, target) vectors,
// then goes on while the smallest score is below score_tol (include/gpc.h, gpc_sparse_prune_dev).  One workgroup per patch at a time;
// the state stays in HBM and every removal is the full-matrix sp_delete_bv (TRI = false, PK = false) in every workgroup shape: states
// loaded with gpc_sparse_set_state and states trained at capacity <= 64 are symmetric only to rounding, and the triangular passes would
// read the other triangle.  The scan, the arg-min and the element updates do not depend on the shape, so 64, 128 and 256 threads leave
// the same bits.  No atomics.
struct SpPruneParams { SpPruneCore K; double score_tol; };

struct SpPruneLds : SpCarve {
    int sval, sidx, Cstar, Qstar, Crep, Qrep;   // 4; 4 ints (2 doubles); delete_bv scratch, [ld] each
    __host__ __device__ constexpr explicit SpPruneLds(int ld)
        : sval(take(4)), sidx(take(2)), Cstar(take(ld)), Qstar(take(ld)), Crep(take(ld)), Qrep(take(ld)) {}
};

__global__ __launch_bounds__(SP_THREADS) void sparse_prune_kernel(SpPruneParams A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SpPruneCore& K = A.K;
    const SpPruneLds L(K.ld);
    double* const W = reinterpret_cast<double*>(smem);
    for (int patch = blockIdx.x; patch < K.P; patch += gridDim.x) {
        int b, st, t, step = 0;
        const SpState S = sp_prune_open(K, patch, b, st, t);
        __syncthreads();                                // the scratch of the previous patch is free
        while (b > 1) {
            double best;
            const int loc = sp_prune_scan(S, b, W + L.sval, reinterpret_cast<int*>(W + L.sidx), best);
            if (!(b > t || best < A.score_tol)) break;  // (a NaN minimum compares false: the score branch stops)
            if (threadIdx.x == 0) {
                if (K.order) K.order[(size_t)patch * K.ld + step] = loc;
                if (K.scores) K.scores[(size_t)patch * K.ld + step] = best;
            }
            b = sp_delete_bv<SP_RMW, false, false>(S, b, loc, K.field_bug, W + L.Cstar, W + L.Qstar, W + L.Crep, W + L.Qrep);
            ++step;
        }
        sp_prune_close(K, S, patch, b, st, step);
    }
}

// ---- what the two distortion-bounded kernels share: the batch their error is taken on ------------------------------------------------
struct SpBatch {
    int n_total;
    const int32_t* off;
    const double *x0, *x1, *y;
    double max_mse;
    const double* max_mse_p;   // [P] or nullptr (every patch: max_mse)
    double sf, c_exp;
};

// mean square error of the state (al [NY][ld], bv [ld][2], both in LDS, nb vectors) on the n points of the batch from o on; every thread
// calls and gets the result.
// Summation order (fixed, independent of the workgroup shape): f_ci over j ascending, e_i over c ascending, point i into class i mod 64,
// each class in ascending i (one wave walks the chunks of per-point errors that the workgroup leaves in LDS), the 64 classes by the xor
// tree 32, 16, .. 1 (gpc_wave_sum).  No atomics.
template <int NY>
__device__ static double sp_rd_mse(const double* al, const double* bv, int nb, int ld, const SpBatch& B, int o, int n, const double* T,
                                   double* ebuf, double* sres)
{
    const int tid = threadIdx.x, nth = SP_NTH;
    const double *x0 = B.x0 + o, *x1 = B.x1 + o, *y = B.y + o;
    double acc = 0.0;                                   // wave 0: lane l holds class l
    __syncthreads();                                    // al / bv are written, ebuf / sres of the previous call are free
    for (int i0 = 0; i0 < n; i0 += nth) {
        const int i = i0 + tid;
        double e = 0.0;
        if (i < n) {
            const double px0 = x0[i], px1 = x1[i];
            double f[NY];
#pragma unroll
            for (int c = 0; c < NY; ++c) f[c] = 0.0;
            for (int j = 0; j < nb; ++j) {
                const double k = gpc_rbf_neg(B.sf, B.c_exp, px0, px1, bv[2 * j], bv[2 * j + 1], T);
#pragma unroll
                for (int c = 0; c < NY; ++c) f[c] += al[c * ld + j] * k;
            }
#pragma unroll
            for (int c = 0; c < NY; ++c) {
                const double d = y[(size_t)c * B.n_total + i] - f[c];
                e += d * d;
            }
        }
        ebuf[tid] = e;
        __syncthreads();
        if (tid < 64)
            for (int q = 0; q < nth; q += 64)
                if (i0 + q + tid < n) acc += ebuf[q + tid];       // i0 and q are multiples of 64: class tid, ascending i
        __syncthreads();
    }
    if (tid < 64) {
        acc = gpc_wave_sum(acc);
        if (tid == 0) sres[0] = acc;
    }
    __syncthreads();
    return sres[0] / (double)(n * NY);
}

// ---- prune to a distortion bound (include/gpc.h, gpc_sparse_prune_rd_dev) -----------------------------------------------------------
// The removals of sparse_prune_kernel -- its scan and arg-min (sp_prune_scan), the unchanged full-matrix sp_delete_bv -- but before a
// vector goes the kernel LOOKS AHEAD (sp_delete_bv_ahead, beside the sp_delete_bv it mirrors): it forms the alpha and BV that
// delete_bv(loc) would leave, evaluates the mean square error of that state on the patch's own points (sp_rd_mse: f_ci over j ascending
// in the post-removal index order), and removes only if the error stays within the patch's bound.
// The kernel values k_ij are recomputed at every step: keeping the patch's n x b table in a per-workgroup region of the workspace and
// reading it back was measured and lost (40.9 against 23.0 ms), and is not kept.
struct SpPruneRdParams { SpPruneCore K; SpBatch B; double *mse, *mse0, *mse_next; /* each may be nullptr */ };

struct SpPruneRdLds : SpCarve {
    int sval, sidx, sres, T;            // 4; 4 ints (2 doubles); 2 (the base of what follows stays 16-byte aligned); the exp table
    int Cstar, Qstar, Crep, Qrep;       // delete_bv scratch, [ld] each; the look-ahead writes the first two
    int al, bv, ebuf;                   // [ny][ld], [ld][2]: the state whose error is taken; [nth]: per-point errors of a chunk
    __host__ __device__ constexpr SpPruneRdLds(int ld, int ny, int nth)
        : sval(take(4)), sidx(take(2)), sres(take(2)), T(take(GPC_EXP_TABLE_SIZE)), Cstar(take(ld)), Qstar(take(ld)), Crep(take(ld)),
          Qrep(take(ld)), al(take(ny * ld)), bv(take(2 * ld)), ebuf(take(nth)) {}
};

template <int NY>
__global__ __launch_bounds__(SP_THREADS) void sparse_prune_rd_kernel(SpPruneRdParams A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SpPruneCore& K = A.K;
    const SpBatch& B = A.B;
    const int tid = threadIdx.x, ld = K.ld;             // (K.ny == NY)
    const SpPruneRdLds L(ld, NY, SP_NTH);
    double* const W = reinterpret_cast<double*>(smem);
    double *const sres = W + L.sres, *const T = W + L.T, *const Cstar = W + L.Cstar, *const Qstar = W + L.Qstar;
    double *const al = W + L.al, *const bv = W + L.bv, *const ebuf = W + L.ebuf;
    gpc_exp_table_init(T);
    for (int patch = blockIdx.x; patch < K.P; patch += gridDim.x) {
        // (S.ny from the kernel argument, not NY: sp_delete_bv is then compiled as it is in sparse_prune_kernel.  With the constant the
        // compiler drops the select between its two alpha updates and fuses the ny = 1 one into an FMA: other bits than the prune's)
        int b, st, t, step = 0;
        const SpState S = sp_prune_open(K, patch, b, st, t);
        const int o = B.off[patch], n = B.off[patch + 1] - o;
        const double bound = B.max_mse_p ? B.max_mse_p[patch] : B.max_mse;
        const double nan = __builtin_nan("");
        double e0 = nan, enext = nan;
        __syncthreads();                                // the scratch of the previous patch is free
        if (n > 0) {
            for (int i = tid; i < b; i += SP_NTH) {
                bv[2 * i] = S.BV[2 * i];
                bv[2 * i + 1] = S.BV[2 * i + 1];
#pragma unroll
                for (int c = 0; c < NY; ++c) al[c * ld + i] = S.alpha[c * ld + i];
            }
            e0 = sp_rd_mse<NY>(al, bv, b, ld, B, o, n, T, ebuf, sres);
            while (b > 1 && b > t) {
                double best;
                const int loc = sp_prune_scan(S, b, W + L.sval, reinterpret_cast<int*>(W + L.sidx), best);
                sp_delete_bv_ahead(S, b, loc, K.field_bug, Cstar, Qstar, al, bv);
                const double e = sp_rd_mse<NY>(al, bv, b - 1, ld, B, o, n, T, ebuf, sres);
                if (!(e <= bound)) { enext = e; break; }       // (a NaN error or a NaN bound compares false: stop)
                if (tid == 0) {
                    if (K.order) K.order[(size_t)patch * ld + step] = loc;
                    if (K.scores) K.scores[(size_t)patch * ld + step] = best;
                    if (A.mse) A.mse[(size_t)patch * ld + step] = e;
                }
                b = sp_delete_bv<SP_RMW, false, false>(S, b, loc, K.field_bug, Cstar, Qstar, W + L.Crep, W + L.Qrep);
                ++step;
            }
        }
        if (tid == 0) {
            if (A.mse0) A.mse0[patch] = e0;
            if (A.mse_next) A.mse_next[patch] = enext;
        }
        sp_prune_close(K, S, patch, b, st, step);
    }
}

// ---- quantise to the fewest bits in a distortion bound (include/gpc.h, gpc_sparse_quantize_rd_dev) ----------------------------------
// The search of sparse_prune_rd_kernel over another axis: not which vector goes, but how many bits each coefficient keeps.  Per patch the
// ny + 2 arrays (BV column 0, BV column 1, the alpha planes) get their float range once; then, width by width, the dequantised alpha' and
// BV' go where the look-ahead keeps its al / bv and sp_rd_mse gives their error in its fixed order.  The state is only read: the raw
// values are re-read from memory at every width (b (ny + 2) doubles, in L2 after the first), and the accepted width's codes are formed
// from them once more at the end.  Ranges: a block min / max (exact, so the tree does not matter).
#define SP_Q_MAXBITS 16
struct SpQuantParams {
    int P, ny, ld, bits_min, bits_max;
    SpBatch B;
    const double *alpha, *BV;
    const int32_t *b, *stat;
    int32_t *bits, *status_out;          // each output may be nullptr
    uint16_t *q_alpha, *q_bv;
    float* range;
    double *mse0, *mse_q, *curve;
};

struct SpQuantLds : SpCarve {
    int sres, red, rng, T;              // 2; [na][2][4]: per-wave min / max of each of the na = ny + 2 arrays; [na][2] floats (na doubles, + 1
                                        // when na is odd: the table stays 16-byte aligned); the exp table
    int al, bv, ebuf;                   // as in SpPruneRdLds
    __host__ __device__ constexpr SpQuantLds(int ld, int ny, int nth)
        : sres(take(2)), red(take((ny + 2) * 8)), rng(take((ny + 2) + ((ny + 2) & 1))), T(take(GPC_EXP_TABLE_SIZE)), al(take(ny * ld)),
          bv(take(2 * ld)), ebuf(take(nth)) {}
};

// array a of the patch (0, 1: the BV columns, 2 + c: alpha plane c), element i
__device__ static __forceinline__ double sp_q_raw(const double* alpha, const double* BV, int ld, int a, int i)
{
    return a < 2 ? BV[2 * i + a] : alpha[(a - 2) * ld + i];
}

template <int NY>
__global__ __launch_bounds__(SP_THREADS) void sparse_quantize_rd_kernel(SpQuantParams A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NA = NY + 2;
    const SpBatch& B = A.B;
    const int tid = threadIdx.x, ld = A.ld, nw = SP_NTH >> 6;
    const SpQuantLds L(ld, NY, SP_NTH);
    double* const W = reinterpret_cast<double*>(smem);
    double *const sres = W + L.sres, *const red = W + L.red, *const T = W + L.T;
    float* const rng = reinterpret_cast<float*>(W + L.rng);
    double *const al = W + L.al, *const bv = W + L.bv, *const ebuf = W + L.ebuf;
    gpc_exp_table_init(T);
    for (int patch = blockIdx.x; patch < A.P; patch += gridDim.x) {
        const double* alpha = A.alpha + (size_t)patch * NY * ld;
        const double* BV = A.BV + (size_t)patch * ld * 2;
        int b = A.b[patch];
        if (b > ld) b = ld;                             // (gpc_sparse_set_state admits no more)
        if (b < 0) b = 0;
        const int o = B.off[patch], n = B.off[patch + 1] - o;
        const double bound = B.max_mse_p ? B.max_mse_p[patch] : B.max_mse;
        const double nan = __builtin_nan("");
        double e0 = nan, eq = nan;
        int bits = 0;
        __syncthreads();                                // the scratch of the previous patch is free
        // the raw state into LDS: mse0, and whether every value is finite
        int bad = 0;
        double mn[NA], mx[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) { mn[a] = __builtin_inf(); mx[a] = -__builtin_inf(); }
        for (int i = tid; i < b; i += SP_NTH) {
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const double v = sp_q_raw(alpha, BV, ld, a, i);
                if (a < 2) bv[2 * i + a] = v;
                else al[(a - 2) * ld + i] = v;
                bad |= !__builtin_isfinite(v);
                mn[a] = v < mn[a] ? v : mn[a];
                mx[a] = v > mx[a] ? v : mx[a];
            }
        }
        if (n > 0) e0 = sp_rd_mse<NY>(al, bv, b, ld, B, o, n, T, ebuf, sres);
        const bool escape = __syncthreads_or(bad) != 0 || b == 0 || n == 0;
        if (!escape) {
            // the ranges: wave min / max by the xor tree, then across the waves through LDS
#pragma unroll
            for (int a = 0; a < NA; ++a) {
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) {
                    const double m0 = __shfl_xor(mn[a], d, 64), m1 = __shfl_xor(mx[a], d, 64);
                    mn[a] = m0 < mn[a] ? m0 : mn[a];
                    mx[a] = m1 > mx[a] ? m1 : mx[a];
                }
                if ((tid & 63) == 0) {
                    red[(a * 2 + 0) * 4 + (tid >> 6)] = mn[a];
                    red[(a * 2 + 1) * 4 + (tid >> 6)] = mx[a];
                }
            }
            __syncthreads();
            if (tid < NA) {
                double m0 = red[(tid * 2) * 4], m1 = red[(tid * 2 + 1) * 4];
                for (int k = 1; k < nw; ++k) {
                    const double u0 = red[(tid * 2) * 4 + k], u1 = red[(tid * 2 + 1) * 4 + k];
                    m0 = u0 < m0 ? u0 : m0;
                    m1 = u1 > m1 ? u1 : m1;
                }
                const float lo = gpc_q_lo(m0), hi = gpc_q_hi(m1);
                rng[2 * tid] = lo;
                rng[2 * tid + 1] = hi;
                if (A.range) {
                    A.range[((size_t)patch * NA + tid) * 2] = lo;
                    A.range[((size_t)patch * NA + tid) * 2 + 1] = hi;
                }
            }
            __syncthreads();
            for (int w = A.bits_min; w <= A.bits_max; ++w) {
                // (sp_rd_mse has left every thread behind a barrier: the readers of al / bv of the previous width are through)
                for (int i = tid; i < b; i += SP_NTH) {
#pragma unroll
                    for (int a = 0; a < NA; ++a) {
                        const float lo = rng[2 * a];
                        const double step = gpc_q_step(lo, rng[2 * a + 1], w);
                        const double v = gpc_q_value(gpc_q_code(sp_q_raw(alpha, BV, ld, a, i), lo, step, w), lo, step);
                        if (a < 2) bv[2 * i + a] = v;
                        else al[(a - 2) * ld + i] = v;
                    }
                }
                const double e = sp_rd_mse<NY>(al, bv, b, ld, B, o, n, T, ebuf, sres);
                if (tid == 0 && A.curve) A.curve[(size_t)patch * SP_Q_MAXBITS + (w - 1)] = e;
                if (e <= bound) { bits = w; eq = e; break; }       // (a NaN error or a NaN bound compares false: on to the next width)
            }
            // the accepted width's codes, from the raw state
            if (bits > 0 && (A.q_alpha || A.q_bv)) {
                for (int i = tid; i < b; i += SP_NTH) {
#pragma unroll
                    for (int a = 0; a < NA; ++a) {
                        const float lo = rng[2 * a];
                        const uint16_t q = gpc_q_code(sp_q_raw(alpha, BV, ld, a, i), lo, gpc_q_step(lo, rng[2 * a + 1], bits), bits);
                        if (a < 2) { if (A.q_bv) A.q_bv[((size_t)patch * ld + i) * 2 + a] = q; }
                        else if (A.q_alpha) A.q_alpha[((size_t)patch * NY + (a - 2)) * ld + i] = q;
                    }
                }
            }
        }
        if (tid == 0) {
            if (A.bits) A.bits[patch] = bits;
            if (A.mse0) A.mse0[patch] = e0;
            if (A.mse_q) A.mse_q[patch] = eq;
            if (A.status_out) A.status_out[patch] = A.stat[patch];
        }
    }
}

// ---- the decoder of the bit-packed model (include/gpc.h, gpc_sparse_dequantize_dev): one workgroup per patch -------------------------
struct SpDequantParams {
    int P, ny, ld;
    const int32_t *bv_count, *bits;
    const uint16_t *q_alpha, *q_bv;
    const float* range;
    double *alpha, *C, *Q, *BV;
    int32_t *b, *count, *stat;
};

__global__ __launch_bounds__(SP_THREADS) void sparse_dequantize_kernel(SpDequantParams A)
{
    const int patch = blockIdx.x, tid = threadIdx.x, ld = A.ld, ny = A.ny, na = ny + 2;
    int w = A.bits[patch];
    if (w <= 0) return;                                 // a raw leaf: not touched
    if (w > SP_Q_MAXBITS) w = SP_Q_MAXBITS;
    int b = A.bv_count[patch];
    b = b < 0 ? 0 : (b > ld ? ld : b);
    const float* rng = A.range + (size_t)patch * na * 2;
    double* alpha = A.alpha + (size_t)patch * ny * ld;
    double* BV = A.BV + (size_t)patch * ld * 2;
    for (int e = tid; e < na * ld; e += SP_THREADS) {
        const int a = e / ld, i = e - a * ld;
        double v = 0.0;
        if (i < b) {
            const float lo = rng[2 * a];
            const double step = gpc_q_step(lo, rng[2 * a + 1], w);
            const uint16_t q = a < 2 ? A.q_bv[((size_t)patch * ld + i) * 2 + a] : A.q_alpha[((size_t)patch * ny + (a - 2)) * ld + i];
            v = gpc_q_value(q, lo, step);
        }
        if (a < 2) BV[2 * i + a] = v;
        else alpha[(a - 2) * ld + i] = v;
    }
    double* Cp = A.C + (size_t)patch * ld * ld;
    double* Qp = A.Q + (size_t)patch * ld * ld;
    for (int e = tid; e < ld * ld; e += SP_THREADS) {
        Cp[e] = 0.0;
        Qp[e] = 0.0;
    }
    if (tid == 0) {
        A.b[patch] = b;
        A.count[patch] = b;
        A.stat[patch] = GPC_STATUS_OK;
    }
}

// the layouts against the closed forms of DESIGN 5.4e-g, at the corners of (ld, ny, threads)
#define SP_LDS_IS(ld, ny, nth)                                                                                                          \
    static_assert(SpPruneLds(ld).total == 6 + 4 * (ld) && SpPruneRdLds(ld, ny, nth).total == 8 + GPC_EXP_TABLE_SIZE + (6 + (ny)) * (ld) + (nth) && \
                  SpQuantLds(ld, ny, nth).total == 2 + 9 * ((ny) + 2) + (((ny) + 2) & 1) + GPC_EXP_TABLE_SIZE + ((ny) + 2) * (ld) + (nth), "LDS")
SP_LDS_IS(32, 1, 64); SP_LDS_IS(48, 3, 64); SP_LDS_IS(112, 1, 128); SP_LDS_IS(112, 3, 128); SP_LDS_IS(GPC_MAX_BV, 1, 256);
#undef SP_LDS_IS

// ------------------------------------------------------------------------------------------------ host side
// Every launch takes the workgroup shape of sp_add_launch (sp_workgroup_threads): a thread owns at most one basis row in each, and the
// scan, the removal and the error sum are laid out so that the shapes give the same bits.

static SpPruneCore sp_prune_core(const gpc_sparse* g, int keep, const int32_t* target, int32_t* removed, int32_t* order, double* scores,
                                 int32_t* status)
{
    SpPruneCore K;
    K.P = g->P; K.ny = g->ny; K.ld = g->ld; K.keep = keep; K.field_bug = g->prm.ref_field_delete_bug;
    K.target = target;
    K.alpha = g->alpha; K.C = g->C; K.Q = g->Q; K.BV = g->BV;
    K.b = g->b; K.stat = g->stat;
    K.removed = removed; K.order = order; K.scores = scores; K.status_out = status;
    return K;
}

static SpBatch sp_batch(const gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y,
                        double max_mse, const double* max_mse_p)
{
    return SpBatch{n_total, off, x0, x1, y, max_mse, max_mse_p, g->prm.sigmaf_sq, (double)(-0.5f) / g->prm.l_sq};   // (in the struct's order)
}

// The grid of the distortion-bounded kernels: as many workgroups as the device holds at once.  Their registers admit fewer waves per SIMD
// than sparse_prune_kernel's, and workgroups beyond the resident ones would only queue behind them (asked of the runtime per call:
// host-side only, no synchronisation).
template <class Kernel>
static int sp_resident_grid(const gpc_sparse* g, Kernel kernel, int nth, size_t lds)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, nth, lds) != hipSuccess || per_cu < 1) per_cu = 768 / nth;
    return std::min(g->P, g->ctx->num_cus * std::min(per_cu, 1024 / nth));
}

int sp_prune_launch(gpc_sparse* g, int keep, const int32_t* target, double score_tol, int32_t* removed, int32_t* order, double* scores,
                    int32_t* status)
{
    gpc_ctx* ctx = g->ctx;
    SpPruneParams A;
    A.K = sp_prune_core(g, keep, target, removed, order, scores, status);
    A.score_tol = score_tol;
    const int nth = sp_workgroup_threads(g);
    const size_t lds = sizeof(double) * (size_t)SpPruneLds(g->ld).total;
    // a removal is a chain of short barrier-separated phases on one patch: as many patches in flight as a CU holds (the kernel's
    // registers leave room for four waves per SIMD)
    const int grid = std::min(g->P, ctx->num_cus * (1024 / nth));
    hipLaunchKernelGGL(sparse_prune_kernel, dim3(grid), dim3(nth), lds, ctx->stream, A);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}

int sp_prune_rd_launch(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y, int keep,
                       const int32_t* target, double max_mse, const double* max_mse_p, int32_t* removed, int32_t* order, double* scores,
                       double* mse, double* mse0, double* mse_next, int32_t* status)
{
    gpc_ctx* ctx = g->ctx;
    SpPruneRdParams A;
    A.K = sp_prune_core(g, keep, target, removed, order, scores, status);
    A.B = sp_batch(g, off, n_total, x0, x1, y, max_mse, max_mse_p);
    A.mse = mse; A.mse0 = mse0; A.mse_next = mse_next;
    const int nth = sp_workgroup_threads(g);
    const size_t lds = sizeof(double) * (size_t)SpPruneRdLds(g->ld, g->ny, nth).total;
    void (*const kernel)(SpPruneRdParams) = g->ny == 1 ? sparse_prune_rd_kernel<1> : sparse_prune_rd_kernel<3>;
    hipLaunchKernelGGL(kernel, dim3(sp_resident_grid(g, kernel, nth, lds)), dim3(nth), lds, ctx->stream, A);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}

int sp_quantize_rd_launch(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y, int bits_min,
                          int bits_max, double max_mse, const double* max_mse_p, int32_t* bits, uint16_t* q_alpha, uint16_t* q_bv, float* range,
                          double* mse0, double* mse_q, double* curve, int32_t* status)
{
    gpc_ctx* ctx = g->ctx;
    SpQuantParams A;
    A.P = g->P; A.ny = g->ny; A.ld = g->ld; A.bits_min = bits_min; A.bits_max = bits_max;
    A.B = sp_batch(g, off, n_total, x0, x1, y, max_mse, max_mse_p);
    A.alpha = g->alpha; A.BV = g->BV; A.b = g->b; A.stat = g->stat;
    A.bits = bits; A.status_out = status; A.q_alpha = q_alpha; A.q_bv = q_bv; A.range = range;
    A.mse0 = mse0; A.mse_q = mse_q; A.curve = curve;
    const int nth = sp_workgroup_threads(g);
    const size_t lds = sizeof(double) * (size_t)SpQuantLds(g->ld, g->ny, nth).total;
    void (*const kernel)(SpQuantParams) = g->ny == 1 ? sparse_quantize_rd_kernel<1> : sparse_quantize_rd_kernel<3>;
    hipLaunchKernelGGL(kernel, dim3(sp_resident_grid(g, kernel, nth, lds)), dim3(nth), lds, ctx->stream, A);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}

int sp_dequantize_launch(gpc_sparse* g, const int32_t* bv_count, const int32_t* bits, const uint16_t* q_alpha, const uint16_t* q_bv,
                         const float* range)
{
    gpc_ctx* ctx = g->ctx;
    SpDequantParams A;
    A.P = g->P; A.ny = g->ny; A.ld = g->ld;
    A.bv_count = bv_count; A.bits = bits; A.q_alpha = q_alpha; A.q_bv = q_bv; A.range = range;
    A.alpha = g->alpha; A.C = g->C; A.Q = g->Q; A.BV = g->BV;
    A.b = g->b; A.count = g->count; A.stat = g->stat;
    hipLaunchKernelGGL(sparse_dequantize_kernel, dim3(g->P), dim3(SP_THREADS), 0, ctx->stream, A);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}
