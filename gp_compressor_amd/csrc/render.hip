// render.hip -- the map as a sensor at a pose would see it: gpc_patches_render casts n rays from one origin through the leaf table of
// a map, front to back, and stops each at the first leaf whose depth GP's mean surface it meets inside that leaf's window.  The
// reference has no such read-out (load_compressed, src/gp_compressor.cpp:298-380, dumps every leaf's whole grid); the rule is this
// library's and is stated in full in include/gpc.h.  As in raycast.hip it is a per-ray rule with no order left to the scheduler:
//   entry    slab test against the grid box, start voxel from the entry point
//   walk     a thread per ray, forwards: the exit parameters x_a = (face_a - o_a) / d_a are recomputed from the integer voxel coordinate
//            at every step (nothing accumulates); ties go to the first axis; leaving the grid is a miss.  At most
//            kmax[0] + kmax[1] + kmax[2] + 1 voxels: every step moves one coordinate away from the origin.  No list per ray.
//   surface  in a trained leaf: Newton on g(t) = depth of the ray point above the plane - f(q(t)), from the plane, a fixed number of
//            iterations; every evaluation is a sum over the leaf's basis (rn_eval).  Neighbouring rays meet the same leaf, so alpha / BV
//            are loads of one address per wave; the exp table sits in LDS.
//   accept   residual, range, window, the producer's sphere, W, the occupancy labels; a rejected test lets the ray go on
// The walk and frame arithmetic is compiled with contraction off (producer_internal.h); tests/render_ref.py evaluates the same
// expressions in the same association.  The GP sums use the library's exp, which NumPy's differs from by an ulp: decisions within
// that distance of a boundary are what the restatement's margin names.  Integer atomics (the counters) only: same inputs, same bits.
// gpc_patches_render_attrs reads a render's leaf / local outputs again, without a walk: the depth GP's predictive sigma at the hits
// through the scattered read-out (sp_scatter_launch, sparse_scatter.hip) and the world normal from rn_eval's gradient (rn_normal_kernel).
#include <cmath>
#include <cstring>

#include "gpc_device.h"
#include "producer_internal.h"   // (switches floating-point contraction off)
#include "sparse_internal.h"

// counters in the workspace
enum { RN_HITS = 0, RN_OUTSIDE = 1, RN_TESTS = 2, RN_RESID = 3, RN_WORDS = 8 };
#define RN_MAX_NEWTON 64

struct RnGp {                     // one gpc_sparse as the kernel reads it
    const double *alpha, *BV;     // [P][ny][ld], [P][ld][2]
    const int32_t* b;
    int ld;
    double sf, c_exp, l_sq;       // sigma_f^2, (double)(-0.5f) / l^2, l^2
};

struct RnArgs {
    PcGrid g;
    int n, P, m;
    const uint64_t* leaf_key;
    const double *R, *mean, *rgb_mean;
    const uint8_t *W, *cells;     // W: nullptr when use_w == 0
    RnGp depth, rgb;              // rgb.alpha == nullptr: no colour
    double org[3];
    const double* dirs;
    int newton;
    double tol_g, t_max;
    gpc_point_xyzrgb* cloud;
    int32_t* leaf;
    double *range, *local;
    int32_t* cnt;
};

// f = sum_j alpha_j k_j and s = sum_j alpha_j k_j (BV_j - q) at q, over the first b basis vectors of one leaf
__device__ static inline void rn_eval(const RnGp& G, const double* __restrict__ al, const double* __restrict__ bv, int b, double q1, double q2,
                                      const double* T, double& f, double& s1, double& s2)
{
    f = 0.0; s1 = 0.0; s2 = 0.0;
    for (int j = 0; j < b; ++j) {
        const double b0 = bv[2 * j], b1 = bv[2 * j + 1];
        const double w = al[j] * gpc_rbf_neg(G.sf, G.c_exp, q1, q2, b0, b1, T);
        f += w;
        s1 += w * (b0 - q1);
        s2 += w * (b1 - q2);
    }
}

__device__ static inline bool rn_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

struct RnHit {
    double t, f, q1, q2, x[3];
};

// the surface test of leaf L in voxel k: 1 = accepted; resid = 1 when t, q, f, g were finite and |g| > tol_g
__device__ static inline int rn_surface(const RnArgs& A, int L, const int k[3], const double d[3], const double* T, RnHit& h, int& resid)
{
    const PcGrid& g = A.g;
    const double* R = A.R + (size_t)L * 9;                    // column-major: R[0..2] = normal
    const double* mu = A.mean + (size_t)L * 3;
    double a[3], c[3];
    {
        const double e[3] = {A.org[0] - mu[0], A.org[1] - mu[1], A.org[2] - mu[2]};
        pc_to_frame(R, e, a);
        pc_to_frame(R, d, c);
    }
    // the plane (rc_plane_cell's association)
    const double num = R[0] * (mu[0] - A.org[0]) + R[1] * (mu[1] - A.org[1]) + R[2] * (mu[2] - A.org[2]);
    double t = num / c[0];
    const int b = min(A.depth.b[L], A.depth.ld);
    const double* al = A.depth.alpha + (size_t)L * A.depth.ld;
    const double* bv = A.depth.BV + (size_t)L * A.depth.ld * 2;
    double q1 = 0, q2 = 0, f = 0, gv = 0;
    for (int it = 0; it <= A.newton; ++it) {                  // newton updates, then the final evaluation
        double s1, s2;
        q1 = a[1] + t * c[1];
        q2 = a[2] + t * c[2];
        rn_eval(A.depth, al, bv, b, q1, q2, T, f, s1, s2);
        gv = (a[0] + t * c[0]) - f;
        if (it < A.newton) {
            const double fx = s1 / A.depth.l_sq, fy = s2 / A.depth.l_sq;
            const double gp = c[0] - (fx * c[1] + fy * c[2]);
            t = t - gv / gp;
        }
    }
    resid = 0;
    if (!rn_finite(t) || !rn_finite(q1) || !rn_finite(q2) || !rn_finite(f) || !rn_finite(gv)) return 0;
    bool ok = true;
    if (!(fabs(gv) <= A.tol_g)) { resid = 1; ok = false; }
    if (!(t > 0.0 && t <= A.t_max)) ok = false;
    if (q1 > g.half || q1 < -g.half || q2 > g.half || q2 < -g.half) ok = false;
    if (!ok) return 0;
    double cen[3];
    pc_center(g, k, cen);
    double r2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {                             // reproject_kernel's association
        const double v = __dadd_rn(__dadd_rn(__dmul_rn(R[i], f), __dmul_rn(R[i + 3], q1)), __dmul_rn(R[i + 6], q2));
        h.x[i] = __dadd_rn(v, mu[i]);
    }
    {
        const double ex = h.x[0] - cen[0], ey = h.x[1] - cen[1], ez = h.x[2] - cen[2];
        r2 = ex * ex + ey * ey + ez * ez;
    }
    if (!(r2 <= g.radius * g.radius)) return 0;
    if (A.W || A.cells) {
        const size_t cell = (size_t)L * (size_t)A.m + (size_t)pc_mask_cell(g, q1, q2);
        if (A.W && A.W[cell] == 0) return 0;
        if (A.cells && A.cells[cell] == GPC_CELL_FREE) return 0;
    }
    h.t = t; h.f = f; h.q1 = q1; h.q2 = q2;
    return 1;
}

// ---- a thread per ray ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void rn_render_kernel(RnArgs A)
{
    __shared__ double T[GPC_EXP_TABLE_SIZE];
    gpc_exp_table_init(T);
    __syncthreads();
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    const PcGrid& g = A.g;
    int nhit = 0, nout = 0, ntest = 0, nres = 0;
    if (i < A.n) {
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const double d[3] = {A.dirs[(size_t)i * 3], A.dirs[(size_t)i * 3 + 1], A.dirs[(size_t)i * 3 + 2]};
        bool meets = rn_finite(d[0]) && rn_finite(d[1]) && rn_finite(d[2]) && !(d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0) && A.P > 0;
        double tn = -inf, tf = inf;
        if (meets) {                                          // the grid box against the ray
            double lo[3], hi[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = g.mn[a] + (double)(0 - g.koff[a]) * g.res;
                hi[a] = g.mn[a] + (double)(g.kmax[a] + 1 - g.koff[a]) * g.res;
            }
            meets = pc_ray_box(lo, hi, A.org, d, tn, tf);
        }
        RnHit h;
        int hitL = -1;
        if (!meets) {
            nout = 1;
        } else {
            const double t_in = fmax(tn, 0.0);
            int k[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double kd = floor(((A.org[a] + t_in * d[a]) - g.mn[a]) / g.res) + (double)g.koff[a];
                k[a] = (int)fmin(fmax(kd, 0.0), (double)g.kmax[a]);          // (finite: the ray meets the box)
            }
            const int max_steps = g.kmax[0] + g.kmax[1] + g.kmax[2] + 1;     // voxels a monotone walk can visit
            for (int step = 0; step < max_steps; ++step) {
                const int L = pc_find_leaf(A.leaf_key, A.P, pc_pack(g, k[0], k[1], k[2]));
                if (L >= 0 && A.depth.b[L] > 0) {
                    int resid;
                    ++ntest;
                    const int acc = rn_surface(A, L, k, d, T, h, resid);
                    nres += resid;
                    if (acc) { hitL = L; break; }
                }
                // the face the ray leaves this voxel through
                double best = inf;
                int ax = -1;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (d[a] == 0.0) continue;
                    const int kf = d[a] > 0.0 ? k[a] - g.koff[a] + 1 : k[a] - g.koff[a];
                    const double xa = ((g.mn[a] + (double)kf * g.res) - A.org[a]) / d[a];
                    if (xa < best || ax < 0) { best = xa; ax = a; }   // (strict: the first axis that attains the minimum)
                }
                if (ax < 0) break;
                k[ax] += d[ax] > 0.0 ? 1 : -1;
                if (k[ax] < 0 || k[ax] > g.kmax[ax]) break;
            }
        }
        gpc_point_xyzrgb p;
        p.w = 1.0f; p.a = 255; p.r = p.g = p.b = 0;
        p.pad[0] = p.pad[1] = p.pad[2] = 0.0f;
        if (hitL >= 0) {
            nhit = 1;
            p.x = (float)h.x[0]; p.y = (float)h.x[1]; p.z = (float)h.x[2];
            if (A.rgb.alpha) {
                const int bc = min(A.rgb.b[hitL], A.rgb.ld);
                const double* al = A.rgb.alpha + (size_t)hitL * 3 * A.rgb.ld;
                const double* bv = A.rgb.BV + (size_t)hitL * A.rgb.ld * 2;
                double cs[3] = {0.0, 0.0, 0.0};
                for (int j = 0; j < bc; ++j) {
                    const double kj = gpc_rbf_neg(A.rgb.sf, A.rgb.c_exp, h.q1, h.q2, bv[2 * j], bv[2 * j + 1], T);
#pragma unroll
                    for (int c = 0; c < 3; ++c) cs[c] += al[c * A.rgb.ld + j] * kj;
                }
                const double* cm = A.rgb_mean + (size_t)hitL * 3;
                p.r = rp_flatten(__dadd_rn(cs[0], cm[0]));
                p.g = rp_flatten(__dadd_rn(cs[1], cm[1]));
                p.b = rp_flatten(__dadd_rn(cs[2], cm[2]));
            }
        } else {
            p.x = p.y = p.z = __int_as_float(0x7fc00000);
        }
        A.cloud[i] = p;
        if (A.leaf) A.leaf[i] = hitL;
        if (A.range) A.range[i] = hitL >= 0 ? h.t : nan;
        if (A.local) {
            A.local[(size_t)i * 3] = hitL >= 0 ? h.f : nan;
            A.local[(size_t)i * 3 + 1] = hitL >= 0 ? h.q1 : nan;
            A.local[(size_t)i * 3 + 2] = hitL >= 0 ? h.q2 : nan;
        }
    }
    // counters: one atomic per wave and word
    for (int o = 32; o > 0; o >>= 1) {
        nhit += __shfl_xor(nhit, o);
        nout += __shfl_xor(nout, o);
        ntest += __shfl_xor(ntest, o);
        nres += __shfl_xor(nres, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nhit) atomicAdd(&A.cnt[RN_HITS], nhit);
        if (nout) atomicAdd(&A.cnt[RN_OUTSIDE], nout);
        if (ntest) atomicAdd(&A.cnt[RN_TESTS], ntest);
        if (nres) atomicAdd(&A.cnt[RN_RESID], nres);
    }
}

// pixel i = v * width + u: dir = R ((u - cx) / fx, (v - cy) / fy, 1)
__global__ __launch_bounds__(PC_THREADS) void rn_camera_kernel(int width, size_t total, double fx, double fy, double cx, double cy, const double R0,
                                                               const double R1, const double R2, const double R3, const double R4, const double R5,
                                                               const double R6, const double R7, const double R8, double* dirs)
{
    const size_t i = (size_t)blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= total) return;
    const int u = (int)(i % (size_t)width), v = (int)(i / (size_t)width);
    const double x = ((double)u - cx) / fx, y = ((double)v - cy) / fy;
    dirs[i * 3] = (R0 * x + R3 * y) + R6;
    dirs[i * 3 + 1] = (R1 * x + R4 * y) + R7;
    dirs[i * 3 + 2] = (R2 * x + R5 * y) + R8;
}

// ---- the surface normal at the hits of a render: a thread per ray, nothing is walked again ---------------------------------------------
struct RnNormalArgs {
    int n, P;
    const int32_t* leaf;
    const double *local, *R, *mean;
    RnGp depth;
    int has_org;                  // 0: the normal keeps the sign of the frame's first column
    double org[3];
    double* normal;
};

__global__ __launch_bounds__(PC_THREADS) void rn_normal_kernel(RnNormalArgs A)
{
    __shared__ double T[GPC_EXP_TABLE_SIZE];
    gpc_exp_table_init(T);
    __syncthreads();
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= A.n) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double out[3] = {nan, nan, nan};
    const int L = A.leaf[i];
    if (L >= 0 && L < A.P) {
        const double* R = A.R + (size_t)L * 9;                // column-major: R[0..2] = normal
        const double f0 = A.local[(size_t)i * 3], q1 = A.local[(size_t)i * 3 + 1], q2 = A.local[(size_t)i * 3 + 2];
        const int b = min(A.depth.b[L], A.depth.ld);
        double f, s1, s2;
        rn_eval(A.depth, A.depth.alpha + (size_t)L * A.depth.ld, A.depth.BV + (size_t)L * A.depth.ld * 2, b, q1, q2, T, f, s1, s2);
        const double fx = s1 / A.depth.l_sq, fy = s2 / A.depth.l_sq;
        const double v1 = -fx, v2 = -fy;                      // the frame normal (1, -fx, -fy)
        double w[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) w[a] = __dadd_rn(__dadd_rn(R[a], __dmul_rn(R[a + 3], v1)), __dmul_rn(R[a + 6], v2));
        const double len = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
        double nr[3] = {w[0] / len, w[1] / len, w[2] / len};
        bool ok = rn_finite(nr[0]) && rn_finite(nr[1]) && rn_finite(nr[2]);
        if (A.has_org) {
            const double* mu = A.mean + (size_t)L * 3;
            double e[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {                     // the hit rule's x (reproject_kernel's association)
                const double v = __dadd_rn(__dadd_rn(__dmul_rn(R[a], f0), __dmul_rn(R[a + 3], q1)), __dmul_rn(R[a + 6], q2));
                e[a] = A.org[a] - __dadd_rn(v, mu[a]);
            }
            const double dot = (nr[0] * e[0] + nr[1] * e[1]) + nr[2] * e[2];
            ok = ok && rn_finite(dot);
            if (dot < 0.0) { nr[0] = -nr[0]; nr[1] = -nr[1]; nr[2] = -nr[2]; }
        }
        if (ok) { out[0] = nr[0]; out[1] = nr[1]; out[2] = nr[2]; }
    }
    A.normal[(size_t)i * 3] = out[0];
    A.normal[(size_t)i * 3 + 1] = out[1];
    A.normal[(size_t)i * 3 + 2] = out[2];
}

static RnGp rn_gp_of(const gpc_sparse* s)
{
    RnGp G;
    G.alpha = s->alpha; G.BV = s->BV; G.b = s->b; G.ld = s->ld;
    G.sf = s->prm.sigmaf_sq; G.l_sq = s->prm.l_sq;
    G.c_exp = (double)(-0.5f) / s->prm.l_sq;                  // as sparse_predict.hip forms it
    return G;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
extern "C" {

void gpc_default_params_render(gpc_render_params* p)
{
    if (!p) return;
    p->newton_iters = 4;
    p->use_w = 1;
    p->eps_rel = 1e-6;
    p->t_max = HUGE_VAL;
}

// what both entries check before they touch a buffer (the caller holds ctx->mu)
static int rn_check(gpc_ctx* ctx, const gpc_patches* map, const gpc_sparse* depth, const gpc_sparse* rgb, const gpc_render_params* prm,
                    const double origin[3], int n)
{
    if (!map || !depth) return gpc_fail(ctx, GPC_EINVAL, "map and depth must not be NULL");
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative ray count");
    if (!origin) return gpc_fail(ctx, GPC_EINVAL, "origin is NULL");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(origin[a])) return gpc_fail(ctx, GPC_EINVAL, "the origin is not finite");
    if (prm && prm->newton_iters < 0) return gpc_fail(ctx, GPC_EINVAL, "newton_iters is negative");
    if (prm && prm->newton_iters > RN_MAX_NEWTON) return gpc_fail(ctx, GPC_ERANGE, "newton_iters exceeds %d", RN_MAX_NEWTON);
    // (an object of another context, or a destroyed one, is not in this context's list: found out without touching it)
    if (!gpc_child_listed(ctx, map) || !gpc_child_listed(ctx, depth) || (rgb && !gpc_child_listed(ctx, rgb)))
        return gpc_fail(ctx, GPC_EINVAL, "map, depth and rgb must be live objects of this context");
    const int P = map->v.P;
    if (depth->ny != 1 || depth->P != P)
        return gpc_fail(ctx, GPC_EINVAL, "depth must have ny == 1 and the map's P (%d), got ny %d, P %d", P, depth->ny, depth->P);
    if (rgb && (rgb->ny != 3 || rgb->P != P))
        return gpc_fail(ctx, GPC_EINVAL, "rgb must have ny == 3 and the map's P (%d), got ny %d, P %d", P, rgb->ny, rgb->P);
    return GPC_OK;
}

int gpc_patches_render_dev(gpc_ctx* ctx, const gpc_patches* map, const gpc_sparse* depth, const gpc_sparse* rgb, const uint8_t* cells,
                           const gpc_render_params* params, const double origin[3], const double* dirs, int n,
                           gpc_point_xyzrgb* cloud, int32_t* leaf, double* range, double* local, int32_t* counts)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = rn_check(ctx, map, depth, rgb, params, origin, n)) return rc;
    if (n > 0 && (!dirs || !cloud)) return gpc_fail(ctx, GPC_EINVAL, "dirs and cloud must not be NULL");
    gpc_render_params prm;
    gpc_default_params_render(&prm);
    if (params) prm = *params;
    if (counts) {
        counts[0] = n;
        counts[1] = counts[2] = counts[3] = counts[4] = 0;
    }
    if (n == 0) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    hipStream_t st = ctx->stream;
    int32_t* cnt = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        PcCarver c(pass ? ctx->ws : nullptr);
        cnt = c.take<int32_t>(RN_WORDS);
        if (!pass) {
            const int rc = gpc_ws_reserve(ctx, c.used);
            if (rc != GPC_OK) return rc;
        }
    }
    RnArgs A;
    memset(&A, 0, sizeof(A));
    A.g = map->grid; A.n = n; A.P = map->v.P; A.m = map->v.m;
    A.leaf_key = map->leaf_key;
    A.R = map->v.rotations; A.mean = map->v.means; A.rgb_mean = map->v.rgb_means;
    A.W = prm.use_w ? map->v.W : nullptr;
    A.cells = cells;
    A.depth = rn_gp_of(depth);
    if (rgb) A.rgb = rn_gp_of(rgb);
    for (int a = 0; a < 3; ++a) A.org[a] = origin[a];
    A.dirs = dirs;
    A.newton = prm.newton_iters;
    A.tol_g = prm.eps_rel * A.g.res;
    A.t_max = prm.t_max;
    A.cloud = cloud; A.leaf = leaf; A.range = range; A.local = local;
    A.cnt = cnt;
    GPC_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(int32_t) * RN_WORDS, st));
    hipLaunchKernelGGL(rn_render_kernel, dim3((n + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, st, A);
    GPC_HIP(ctx, hipGetLastError());
    if (counts) {
        int32_t h[RN_WORDS];
        GPC_HIP(ctx, hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
        GPC_HIP(ctx, hipStreamSynchronize(st));
        counts[1] = h[RN_HITS]; counts[2] = h[RN_OUTSIDE]; counts[3] = h[RN_TESTS]; counts[4] = h[RN_RESID];
    }
    return GPC_OK;
}

int gpc_patches_render(gpc_ctx* ctx, const gpc_patches* map, const gpc_sparse* depth, const gpc_sparse* rgb, const uint8_t* cells,
                       const gpc_render_params* params, const double origin[3], const double* dirs, int n, gpc_point_xyzrgb* cloud,
                       int32_t* leaf, double* range, double* local, int32_t* counts)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    size_t total = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (int rc = rn_check(ctx, map, depth, rgb, params, origin, n)) return rc;
        total = (size_t)map->v.P * (size_t)map->v.m;
    }
    if (n > 0 && (!dirs || !cloud)) return gpc_fail(ctx, GPC_EINVAL, "dirs and cloud must not be NULL");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nz = (size_t)n;
    int32_t got[5];                                           // the host entry is synchronous anyway
    GpcStaging st(ctx, "gpc_patches_render");
    const double* d_dirs = st.up(dirs, nz * 3);
    const uint8_t* d_cells = cells ? st.up(cells, total) : nullptr;
    gpc_point_xyzrgb* d_cloud = st.out<gpc_point_xyzrgb>(nz);
    int32_t* d_leaf = leaf ? st.out<int32_t>(nz) : nullptr;
    double* d_range = range ? st.out<double>(nz) : nullptr;
    double* d_local = local ? st.out<double>(nz * 3) : nullptr;
    if (st.ok()) st.rc = gpc_patches_render_dev(ctx, map, depth, rgb, d_cells, params, origin, d_dirs, n, d_cloud, d_leaf, d_range, d_local, got);
    st.down(cloud, d_cloud, nz);
    st.down(leaf, d_leaf, nz);
    st.down(range, d_range, nz);
    st.down(local, d_local, nz * 3);
    if (st.ok() && counts) memcpy(counts, got, sizeof(got));
    return st.finish();
}

// what both attrs entries check before they touch a buffer (the caller holds ctx->mu)
static int rn_attrs_check(gpc_ctx* ctx, const gpc_patches* map, const gpc_sparse* depth, int n, const double* origin)
{
    if (!map || !depth) return gpc_fail(ctx, GPC_EINVAL, "map and depth must not be NULL");
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative ray count");
    for (int a = 0; origin && a < 3; ++a)
        if (!std::isfinite(origin[a])) return gpc_fail(ctx, GPC_EINVAL, "the origin is not finite");
    if (!gpc_child_listed(ctx, map) || !gpc_child_listed(ctx, depth))
        return gpc_fail(ctx, GPC_EINVAL, "map and depth must be live objects of this context");
    if (depth->ny != 1 || depth->P != map->v.P)
        return gpc_fail(ctx, GPC_EINVAL, "depth must have ny == 1 and the map's P (%d), got ny %d, P %d", map->v.P, depth->ny, depth->P);
    return GPC_OK;
}

int gpc_patches_render_attrs_dev(gpc_ctx* ctx, const gpc_patches* map, gpc_sparse* depth, int n, const int32_t* leaf, const double* local,
                                 const double* origin, int conf, double* sigma, double* normal)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = rn_attrs_check(ctx, map, depth, n, origin)) return rc;
    if (n > 0 && (!leaf || !local)) return gpc_fail(ctx, GPC_EINVAL, "leaf and local must not be NULL");
    if (n == 0 || (!sigma && !normal)) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    if (sigma)
        if (int rc = sp_scatter_launch(depth, n, leaf, local + 1, local + 2, 3, nullptr, sigma, conf, nullptr)) return rc;
    if (normal) {
        RnNormalArgs A;
        memset(&A, 0, sizeof(A));
        A.n = n; A.P = map->v.P;
        A.leaf = leaf; A.local = local;
        A.R = map->v.rotations; A.mean = map->v.means;
        A.depth = rn_gp_of(depth);
        A.has_org = origin ? 1 : 0;
        for (int a = 0; origin && a < 3; ++a) A.org[a] = origin[a];
        A.normal = normal;
        hipLaunchKernelGGL(rn_normal_kernel, dim3((n + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, ctx->stream, A);
        GPC_HIP(ctx, hipGetLastError());
    }
    return GPC_OK;
}

int gpc_patches_render_attrs(gpc_ctx* ctx, const gpc_patches* map, gpc_sparse* depth, int n, const int32_t* leaf, const double* local,
                             const double* origin, int conf, double* sigma, double* normal)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (int rc = rn_attrs_check(ctx, map, depth, n, origin)) return rc;
    }
    if (n > 0 && (!leaf || !local)) return gpc_fail(ctx, GPC_EINVAL, "leaf and local must not be NULL");
    if (n == 0 || (!sigma && !normal)) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nz = (size_t)n;
    GpcStaging st(ctx, "gpc_patches_render_attrs");
    const int32_t* d_leaf = st.up(leaf, nz);
    const double* d_local = st.up(local, nz * 3);
    double *d_sigma = sigma ? st.out<double>(nz) : nullptr, *d_normal = normal ? st.out<double>(nz * 3) : nullptr;
    if (st.ok()) st.rc = gpc_patches_render_attrs_dev(ctx, map, depth, n, d_leaf, d_local, origin, conf, d_sigma, d_normal);
    st.down(sigma, d_sigma, nz);
    st.down(normal, d_normal, nz * 3);
    return st.finish();
}

int gpc_camera_rays_dev(gpc_ctx* ctx, const double R[9], double fx, double fy, double cx, double cy, int width, int height, double* dirs_dev)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!R) return gpc_fail(ctx, GPC_EINVAL, "R is NULL");
    if (width < 0 || height < 0) return gpc_fail(ctx, GPC_EINVAL, "negative image size");
    for (int a = 0; a < 9; ++a)
        if (!std::isfinite(R[a])) return gpc_fail(ctx, GPC_EINVAL, "R is not finite");
    if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.0 || fy == 0.0 || !std::isfinite(cx) || !std::isfinite(cy))
        return gpc_fail(ctx, GPC_EINVAL, "fx and fy must be finite and not zero, cx and cy finite");
    const long long total = (long long)width * (long long)height;
    if (total > 0x7fffffffLL) return gpc_fail(ctx, GPC_ERANGE, "more than 2^31 - 1 pixels");
    if (total == 0) return GPC_OK;
    if (!dirs_dev) return gpc_fail(ctx, GPC_EINVAL, "dirs_dev is NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    hipLaunchKernelGGL(rn_camera_kernel, dim3((unsigned)((total + PC_THREADS - 1) / PC_THREADS)), dim3(PC_THREADS), 0, ctx->stream, width,
                       (size_t)total, fx, fy, cx, cy, R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], dirs_dev);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}

}  // extern "C"
