// registration.hip -- SURVEY section 8, row f: gp_registration (/root/reference/src/gp_registration.cpp) on the GPU.  One
// registration_step (:73-92) -- compute_transformation (:115-246), gradient_step (:51-58), transform_pointcloud (:32-38) -- is
// enqueued on the context's stream from end to end; the host reads back 9 doubles.
//
// The reference adds the scan to the model's PCL octree, walks the model's leaves in order and lets each trained leaf claim, out of
// radiusSearch(centre, sqrt(3)/2 res), the points nobody claimed before that pass the +-res/2 window in the leaf's frame
// (occupied_indices, :101-108).  As in the producer (producer.hip) the serial walk is a per-point minimum: a point belongs to the
// FIRST leaf in leaf order that accepts it, and only the <= 27 leaves around the point's own voxel can.  The model's voxel table
// (PcGrid + sorted leaf keys, kept by gpc_patches) stands in for the octree; leaf id = patch id = GP index.
// Pipeline (wave64, integer / gather work except the two likelihood launches):
//   1 rg_assign_kernel    a lane per scan point: voxel key, then pc_first_accepting_leaf (producer_internal.h): one binary search per
//                         (dz, dy) row of the 3 x 3 x 3 neighbourhood (the <= 3 leaves of a row are neighbours in the sorted table),
//                         candidates in ascending leaf order, untrained leaves skipped (:158), sphere test against the voxel centre,
//                         q = R_i^T (p - mean_i) (:104), window (:105)
//   2 bucket              rocPRIM's stable radix sort of (owner, scan index) -- patch order, ascending scan index within a patch, the
//                         unused points (key P) behind off[P]; pc_bucket_offsets: off[j] = first sorted position whose key is >= j
//                         (the exclusive scan of the per-patch counts, read off the sorted keys: no atomics);
//     rg_gather_kernel    X, depth and mean-removed colours (:166-171) in bucket order, planes of pitch n
//   3 sparse_likelihood_kernel twice (sparse_predict.hip): dX, l of the depth GP, dCX, cl of the colour field (:175-195)
//   4 rg_reduce_kernel    per used point d = l dCX + cl dX (:196), d_glob = R_i d, x = R_i q + mean_i (:202-206), g = d_glob^T J(x)
//                         (:40-49, :214); wave shuffles, then the waves of a workgroup in order: one partial per workgroup
//   5 rg_update_kernel    one wave: the partials in a fixed order, delta = sum g / n_used, ls, cls (the running mean of :211-214 IS this
//                         mean), gradient_step, R_cloud, t_cloud (:83-84);  rg_transform_kernel: the working cloud (:36)
// Every buffer is sized by the scan size n, off[P] = n_used is read on the device only.  No floating-point atomics: the same state
// gives the same bits.  Scratch: the context's grow-only workspace; the object owns what outlives a step (working cloud, last
// assignment, pose).
#include <algorithm>
#include <cmath>
#include <new>

#include <rocprim/device/device_radix_sort.hpp>

#include "producer_internal.h"   // (switches floating-point contraction off)
#include "sparse_internal.h"

#define RG_THREADS 256
#define RG_WAVES (RG_THREADS / 64)
#define RG_NQ 8            // sums of the reduction: g[6], l, cl

// device state of an object, doubles
#define RG_S_RC 0          // R_cloud, column-major
#define RG_S_TC 9          // t_cloud
#define RG_S_OUT 12        // delta[6], ls, cls, n_used of the last step
#define RG_S_R 21          // this step's R, row-major
#define RG_S_T 30          // ... and t
#define RG_S_LEN 40

struct gpc_registration {
    gpc_ctx* ctx = nullptr;
    const gpc_patches* pt = nullptr;      // referred to, not owned; alive while (address, serial) is in ctx->children
    gpc_sparse *gd = nullptr, *gc = nullptr;
    uint64_t pt_serial = 0, gd_serial = 0, gc_serial = 0;
    int P = 0;
    int n = 0, cap = 0;                   // scan size, records allocated
    int steps = 0;                        // step_nbr
    gpc_point_xyzrgb* cloud = nullptr;    // working cloud
    int32_t* owner = nullptr;             // [n] of the last step
    double* local = nullptr;              // [n][3]
    double* state = nullptr;              // RG_S_LEN
};

struct RgArgs {
    PcGrid g;
    int n, P;
    const uint64_t* leaf_key;
    const int32_t* bv;                    // basis sizes of the depth GPs
    const double *R, *mean, *rgb_mean;
    gpc_point_xyzrgb* cloud;
    int32_t* owner;
    double* local;
    uint32_t *key, *skey;                 // owner (P = unused) per scan point; sorted
    int32_t *val, *sval;                  // scan index; in bucket order
    int32_t* off;                         // P + 1
    double *x0, *x1, *y, *rgb;            // bucket order, pitch n
    double *dXd, *ld, *dXc, *lc;
    double* part;                         // [workgroups][RG_NQ]
};

// ---- 1: assign ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void rg_assign_kernel(RgArgs A)
{
    const int i = blockIdx.x * RG_THREADS + threadIdx.x;
    if (i >= A.n) return;
    const PcGrid& g = A.g;
    const float4 f = *reinterpret_cast<const float4*>(&A.cloud[i]);
    const double p[3] = {(double)f.x, (double)f.y, (double)f.z};
    // the point's voxel in the model's grid; one voxel beyond the grid a leaf's sphere can still reach it (radius < 1.5 res), further
    // out (or not finite) nothing can
    double kd[3];
    bool near = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        kd[a] = floor((p[a] - g.mn[a]) / g.res) + (double)g.koff[a];       // (koff: producer_internal.h; 0 unless the map grew downwards)
        near = near && kd[a] >= -1.0 && kd[a] <= (double)g.kmax[a] + 1.0;
    }
    int owner = -1;
    double q[3] = {0.0, 0.0, 0.0};
    if (near) {
        const int k[3] = {(int)kd[0], (int)kd[1], (int)kd[2]};
        const int32_t* bv = A.bv;                                           // skipped: gps[i].size() == 0 (:158); q = R^T (p - mean) (:104)
        owner = pc_first_accepting_leaf(g, A.leaf_key, A.P, p, k, A.R, A.mean, [bv](int L) { return bv[L] == 0; }, q);
    }
    A.owner[i] = owner;
    A.local[(size_t)i * 3] = q[0];
    A.local[(size_t)i * 3 + 1] = q[1];
    A.local[(size_t)i * 3 + 2] = q[2];
    A.key[i] = owner < 0 ? (uint32_t)A.P : (uint32_t)owner;
    A.val[i] = i;
}

// ---- 2: bucket ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void rg_gather_kernel(RgArgs A)
{
    const int s = blockIdx.x * RG_THREADS + threadIdx.x;
    if (s >= A.n) return;
    const uint32_t o = A.skey[s];
    double y = 0.0, x0 = 0.0, x1 = 0.0, c[3] = {0.0, 0.0, 0.0};
    if (o < (uint32_t)A.P) {
        const int i = A.sval[s];
        y = A.local[(size_t)i * 3];
        x0 = A.local[(size_t)i * 3 + 1];
        x1 = A.local[(size_t)i * 3 + 2];
        const uint32_t w = pc_rgb_of(&A.cloud[i]);
        const double* cm = A.rgb_mean + (size_t)o * 3;
        c[0] = (double)(w & 0xffu) - cm[0];                                       // :169-171
        c[1] = (double)((w >> 8) & 0xffu) - cm[1];
        c[2] = (double)((w >> 16) & 0xffu) - cm[2];
    }
    A.y[s] = y;
    A.x0[s] = x0;
    A.x1[s] = x1;
    A.rgb[s] = c[0];
    A.rgb[(size_t)A.n + s] = c[1];
    A.rgb[2 * (size_t)A.n + s] = c[2];
}

// ---- 4: combine and reduce -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void rg_reduce_kernel(RgArgs A)
{
    __shared__ double red[RG_WAVES][RG_NQ];
    const int used = A.off[A.P];
    double acc[RG_NQ];
#pragma unroll
    for (int k = 0; k < RG_NQ; ++k) acc[k] = 0.0;
    for (int s = blockIdx.x * RG_THREADS + threadIdx.x; s < used; s += gridDim.x * RG_THREADS) {
        const uint32_t o = A.skey[s];
        const double* R = A.R + (size_t)o * 9;                              // R(r, c) = R[3 c + r]
        const double* mu = A.mean + (size_t)o * 3;
        const double l = A.ld[s], cl = A.lc[s];
        double d[3], dg[3], x[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = l * A.dXc[(size_t)s * 3 + a] + cl * A.dXd[(size_t)s * 3 + a];        // :196
        const double loc[3] = {A.y[s], A.x0[s], A.x1[s]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            dg[r] = R[r] * d[0] + R[3 + r] * d[1] + R[6 + r] * d[2];                                            // :204
            x[r] = R[r] * loc[0] + R[3 + r] * loc[1] + R[6 + r] * loc[2] + mu[r];                               // :206
        }
        acc[0] += dg[0];
        acc[1] += dg[1];
        acc[2] += dg[2];
        acc[3] += dg[2] * x[1] - dg[1] * x[2];                              // d_glob^T J(x), J of :40-49
        acc[4] += dg[0] * x[2] - dg[2] * x[0];
        acc[5] += dg[1] * x[0] - dg[0] * x[1];
        acc[6] += l;
        acc[7] += cl;
    }
#pragma unroll
    for (int k = 0; k < RG_NQ; ++k)
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < RG_NQ; ++k) red[w][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < RG_NQ) {
        double v = red[0][threadIdx.x];
        for (int q = 1; q < RG_WAVES; ++q) v += red[q][threadIdx.x];
        A.part[(size_t)blockIdx.x * RG_NQ + threadIdx.x] = v;
    }
}

// ---- 5: update ---------------------------------------------------------------------------------------------------------------
__device__ static inline void rg_mul33(const double a[9], const double b[9], double c[9])     // row-major
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[3 * r + k] = a[3 * r] * b[k] + a[3 * r + 1] * b[3 + k] + a[3 * r + 2] * b[6 + k];
}

// one wave.  part: nblk partials (nblk == 0: nothing was evaluated); used: off + P on the device, or nullptr
__global__ __launch_bounds__(64) void rg_update_kernel(const double* part, int nblk, const int32_t* used, double step, int ref_sum,
                                                       double* state)
{
    const int lane = threadIdx.x;
    double s[RG_NQ];
#pragma unroll
    for (int k = 0; k < RG_NQ; ++k) {
        double v = 0.0;
        for (int b = lane; b < nblk; b += 64) v += part[(size_t)b * RG_NQ + k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        s[k] = v;
    }
    if (lane != 0) return;
    const int nu = (used && nblk > 0) ? *used : 0;
    double out[9];
#pragma unroll
    for (int k = 0; k < RG_NQ; ++k) out[k] = nu > 0 ? s[k] / (double)nu : 0.0;
    out[8] = (double)nu;
#pragma unroll
    for (int k = 0; k < 9; ++k) state[RG_S_OUT + k] = out[k];
    // gradient_step (:51-58)
    const double a = step * out[3], b = step * out[4], c = step * out[5];
    const double ca = cos(a), sa = sin(a), cb = cos(b), sb = sin(b), cc = cos(c), sc = sin(c);
    const double Rx[9] = {1, 0, 0, 0, ca, -sa, 0, sa, ca};
    const double Ry[9] = {cb, 0, sb, 0, 1, 0, -sb, 0, cb};
    const double Rz[9] = {cc, -sc, 0, sc, cc, 0, 0, 0, 1};
    double Rxy[9], R[9];
    rg_mul33(Rx, Ry, Rxy);
    rg_mul33(Rxy, Rz, R);
    const double t[3] = {step * out[0], step * out[1], step * out[2]};
    // R_cloud = R R_cloud (:83), column-major in the state
    double Rc[9], Rn[9], tc[3], tn[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) Rc[3 * r + k] = state[RG_S_RC + 3 * k + r];
    rg_mul33(R, Rc, Rn);
#pragma unroll
    for (int k = 0; k < 3; ++k) tc[k] = state[RG_S_TC + k];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        tn[r] = ref_sum ? tc[r] + t[r] : R[3 * r] * tc[0] + R[3 * r + 1] * tc[1] + R[3 * r + 2] * tc[2] + t[r];   // :84 | the composition
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            state[RG_S_RC + 3 * k + r] = Rn[3 * r + k];
            state[RG_S_R + 3 * r + k] = R[3 * r + k];
        }
        state[RG_S_TC + r] = tn[r];
        state[RG_S_T + r] = t[r];
    }
}

// (R * p.cast<double>() + t).cast<float>()  (:36)
__global__ __launch_bounds__(RG_THREADS) void rg_transform_kernel(gpc_point_xyzrgb* cloud, int n, const double* state)
{
    const int i = blockIdx.x * RG_THREADS + threadIdx.x;
    if (i >= n) return;
    const double* R = state + RG_S_R;
    const double* t = state + RG_S_T;
    float4 f = *reinterpret_cast<const float4*>(&cloud[i]);
    const double p[3] = {(double)f.x, (double)f.y, (double)f.z};
    f.x = (float)(R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + t[0]);
    f.y = (float)(R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + t[1]);
    f.z = (float)(R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + t[2]);
    *reinterpret_cast<float4*>(&cloud[i]) = f;
}

__global__ __launch_bounds__(64) void rg_reset_kernel(double* state)
{
    const int k = threadIdx.x;
    if (k >= RG_S_LEN) return;
    const bool diag = k == RG_S_RC || k == RG_S_RC + 4 || k == RG_S_RC + 8 || k == RG_S_R || k == RG_S_R + 4 || k == RG_S_R + 8;
    state[k] = diag ? 1.0 : 0.0;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
namespace {

// the caller holds ctx->mu
bool rg_usable(const gpc_registration* r)
{
    const gpc_ctx* ctx = r->ctx;
    return !ctx->dead.load() && gpc_child_alive(ctx, r->pt, r->pt_serial) && gpc_child_alive(ctx, r->gd, r->gd_serial) &&
           gpc_child_alive(ctx, r->gc, r->gc_serial);
}

int rg_check_params(gpc_ctx* ctx, const gpc_registration_params* p)
{
    if (!p) return gpc_fail(ctx, GPC_EINVAL, "params is NULL");
    if (!(std::fabs(p->step) < 1e300)) return gpc_fail(ctx, GPC_EINVAL, "step must be finite");
    if (p->min_steps < 0 || p->max_steps < 1) return gpc_fail(ctx, GPC_EINVAL, "min_steps must be >= 0 and max_steps >= 1");
    return GPC_OK;
}

// one step; the caller holds ctx->mu and has checked rg_usable and the parameters
int rg_step_locked(gpc_registration* r, const gpc_registration_params* prm, double out[9])
{
    gpc_ctx* ctx = r->ctx;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    hipStream_t st = ctx->stream;
    const int n = r->n, P = r->P;
    const size_t N = (size_t)n, Pz = (size_t)P;
    const bool work = n > 0 && P > 0;
    RgArgs A;
    memset(&A, 0, sizeof(A));
    int nred = 0;
    if (work) {
        const unsigned key_bits = (unsigned)pc_bits_for(P);
        size_t sort_bytes = 0;
        GPC_HIP(ctx, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr,
                                               (int32_t*)nullptr, N, 0u, key_bits, st));
        const int nblk = (n + RG_THREADS - 1) / RG_THREADS;
        nred = std::min(nblk, ctx->num_cus * 8);
        void* prim = nullptr;
        for (int pass = 0; pass < 2; ++pass) {            // measure, reserve, carve
            PcCarver c(pass ? ctx->ws : nullptr);
            A.key = c.take<uint32_t>(N); A.skey = c.take<uint32_t>(N);
            A.val = c.take<int32_t>(N); A.sval = c.take<int32_t>(N);
            A.off = c.take<int32_t>(Pz + 1);
            A.x0 = c.take<double>(N); A.x1 = c.take<double>(N); A.y = c.take<double>(N); A.rgb = c.take<double>(3 * N);
            A.dXd = c.take<double>(3 * N); A.ld = c.take<double>(N); A.dXc = c.take<double>(3 * N); A.lc = c.take<double>(N);
            A.part = c.take<double>((size_t)nred * RG_NQ);
            prim = c.take<char>(sort_bytes);
            if (!pass)
                if (int rc = gpc_ws_reserve(ctx, c.used)) return rc;
        }
        const gpc_patches* pt = r->pt;
        A.g = pt->grid; A.n = n; A.P = P;
        A.leaf_key = pt->leaf_key; A.bv = r->gd->b;
        A.R = pt->v.rotations; A.mean = pt->v.means; A.rgb_mean = pt->v.rgb_means;
        A.cloud = r->cloud; A.owner = r->owner; A.local = r->local;
        hipLaunchKernelGGL(rg_assign_kernel, dim3(nblk), dim3(RG_THREADS), 0, st, A);
        GPC_HIP(ctx, hipGetLastError());
        GPC_HIP(ctx, rocprim::radix_sort_pairs(prim, sort_bytes, A.key, A.skey, A.val, A.sval, N, 0u, key_bits, st));
        GPC_HIP(ctx, pc_bucket_offsets(st, A.skey, n, P, A.off));
        hipLaunchKernelGGL(rg_gather_kernel, dim3(nblk), dim3(RG_THREADS), 0, st, A);
        GPC_HIP(ctx, hipGetLastError());
        // 3: the registration inner loop on the bucketed scan (plane pitch n; the kernel reads off on the device)
        if (int rc = sp_likelihood_launch(r->gd, A.off, n, A.x0, A.x1, A.y, A.dXd, A.ld, nullptr)) return rc;
        if (int rc = sp_likelihood_launch(r->gc, A.off, n, A.x0, A.x1, A.rgb, A.dXc, A.lc, nullptr)) return rc;
        hipLaunchKernelGGL(rg_reduce_kernel, dim3(nred), dim3(RG_THREADS), 0, st, A);
        GPC_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(rg_update_kernel, dim3(1), dim3(64), 0, st, A.part, nred, work ? A.off + P : nullptr, prm->step,
                       prm->ref_translation_sum ? 1 : 0, r->state);
    GPC_HIP(ctx, hipGetLastError());
    if (n > 0) {
        hipLaunchKernelGGL(rg_transform_kernel, dim3((n + RG_THREADS - 1) / RG_THREADS), dim3(RG_THREADS), 0, st, r->cloud, n, r->state);
        GPC_HIP(ctx, hipGetLastError());
    }
    GPC_HIP(ctx, hipMemcpyAsync(out, r->state + RG_S_OUT, 9 * sizeof(double), hipMemcpyDeviceToHost, st));
    GPC_HIP(ctx, hipStreamSynchronize(st));
    ++r->steps;
    return GPC_OK;
}

// the scan: (re)allocates for n records, copies them in and resets the pose.  The caller holds ctx->mu.
int rg_set_cloud_locked(gpc_registration* r, const gpc_point_xyzrgb* cloud, int n, hipMemcpyKind kind)
{
    gpc_ctx* ctx = r->ctx;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    hipStream_t st = ctx->stream;
    if (n > r->cap) {
        GPC_HIP(ctx, hipStreamSynchronize(st));
        for (void* q : {(void*)r->cloud, (void*)r->owner, (void*)r->local})
            if (q) (void)hipFree(q);
        r->cloud = nullptr; r->owner = nullptr; r->local = nullptr;
        r->cap = r->n = 0;
        GPC_HIP(ctx, hipMalloc(&r->cloud, sizeof(gpc_point_xyzrgb) * (size_t)n));
        GPC_HIP(ctx, hipMalloc(&r->owner, sizeof(int32_t) * (size_t)n));
        GPC_HIP(ctx, hipMalloc(&r->local, sizeof(double) * 3 * (size_t)n));
        r->cap = n;
    }
    r->n = n;
    r->steps = 0;
    if (n > 0) {
        GPC_HIP(ctx, hipMemcpyAsync(r->cloud, cloud, sizeof(gpc_point_xyzrgb) * (size_t)n, kind, st));
        GPC_HIP(ctx, hipMemsetAsync(r->owner, 0xFF, sizeof(int32_t) * (size_t)n, st));          // -1: no step has assigned anything
        GPC_HIP(ctx, hipMemsetAsync(r->local, 0, sizeof(double) * 3 * (size_t)n, st));
    }
    hipLaunchKernelGGL(rg_reset_kernel, dim3(1), dim3(64), 0, st, r->state);
    GPC_HIP(ctx, hipGetLastError());
    if (kind == hipMemcpyHostToDevice) GPC_HIP(ctx, hipStreamSynchronize(st));                  // the host buffer is the caller's again
    return GPC_OK;
}

}  // namespace

extern "C" {

void gpc_default_params_registration(gpc_registration_params* p)
{
    if (!p) return;
    p->step = (double)1e-1f;
    p->tol = 0.1;
    p->min_steps = 10;
    p->max_steps = 300;
    p->ref_translation_sum = 1;
    p->reserved = 0;
}

int gpc_registration_create(gpc_ctx* ctx, const gpc_patches* patches, gpc_sparse* depth, gpc_sparse* rgb, gpc_registration** out)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!out) return gpc_fail(ctx, GPC_EINVAL, "out is NULL");
    *out = nullptr;
    if (!patches || !depth || !rgb) return gpc_fail(ctx, GPC_EINVAL, "patches/depth/rgb is NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    // (an object of another context is not in this context's list: found out without touching it)
    if (!gpc_child_listed(ctx, patches) || !gpc_child_listed(ctx, depth) || !gpc_child_listed(ctx, rgb))
        return gpc_fail(ctx, GPC_EINVAL, "patches, depth and rgb must be live objects of this context");
    if (depth->ny != 1 || rgb->ny != 3) return gpc_fail(ctx, GPC_EINVAL, "depth must have ny == 1 and rgb ny == 3");
    if (depth->P != patches->v.P || rgb->P != patches->v.P)
        return gpc_fail(ctx, GPC_EINVAL, "P differs: patches %d, depth %d, rgb %d", patches->v.P, depth->P, rgb->P);
    if (depth->prm.noise_model != 0 || rgb->prm.noise_model != 0)
        return gpc_fail(ctx, GPC_EINVAL, "likelihoods are defined for the Gaussian noise model");
    gpc_registration* r = new (std::nothrow) gpc_registration();
    if (!r) return GPC_ENOMEM;
    r->ctx = ctx;
    r->pt = patches; r->gd = depth; r->gc = rgb;
    r->pt_serial = patches->serial; r->gd_serial = depth->serial; r->gc_serial = rgb->serial;
    r->P = patches->v.P;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(&r->state, sizeof(double) * RG_S_LEN);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rg_reset_kernel, dim3(1), dim3(64), 0, ctx->stream, r->state);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        if (r->state) (void)hipFree(r->state);
        delete r;
        return gpc_fail(ctx, e == hipErrorOutOfMemory ? GPC_ENOMEM : GPC_EHIP, "gpc_registration_create: %s", hipGetErrorString(e));
    }
    gpc_ctx_ref(ctx);
    *out = r;
    return GPC_OK;
}

// Safe in either order with gpc_ctx_destroy and with the destroy calls of the objects it refers to (it touches none of them).
void gpc_registration_destroy(gpc_registration* r)
{
    if (!r) return;
    gpc_ctx* ctx = r->ctx;
    (void)hipSetDevice(ctx->device);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (!ctx->dead.load()) (void)hipStreamSynchronize(ctx->stream);
    }
    for (void* q : {(void*)r->cloud, (void*)r->owner, (void*)r->local, (void*)r->state})
        if (q) (void)hipFree(q);
    delete r;
    gpc_ctx_unref(ctx);
}

static int rg_set_cloud(gpc_registration* r, const gpc_point_xyzrgb* cloud, int n, hipMemcpyKind kind)
{
    if (!r) return GPC_EINVAL;
    gpc_ctx* ctx = r->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!rg_usable(r)) return GPC_EINVAL;
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative point count");
    if (n > 0 && !cloud) return gpc_fail(ctx, GPC_EINVAL, "cloud is NULL");
    return rg_set_cloud_locked(r, cloud, n, kind);
}

int gpc_registration_set_cloud(gpc_registration* r, const gpc_point_xyzrgb* cloud, int n)
{
    return rg_set_cloud(r, cloud, n, hipMemcpyHostToDevice);
}

int gpc_registration_set_cloud_dev(gpc_registration* r, const gpc_point_xyzrgb* cloud, int n)
{
    return rg_set_cloud(r, cloud, n, hipMemcpyDeviceToDevice);
}

int gpc_registration_step(gpc_registration* r, const gpc_registration_params* params, double out[9])
{
    if (!r) return GPC_EINVAL;
    gpc_ctx* ctx = r->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!rg_usable(r)) return GPC_EINVAL;
    if (int rc = rg_check_params(ctx, params)) return rc;
    if (!out) return gpc_fail(ctx, GPC_EINVAL, "out is NULL");
    return rg_step_locked(r, params, out);
}

int gpc_registration_run(gpc_registration* r, const gpc_registration_params* params, double* trace, int32_t* steps)
{
    if (!r) return GPC_EINVAL;
    gpc_ctx* ctx = r->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;
    if (steps) *steps = 0;
    for (int k = 0;; ++k) {
        double out[9];
        int s;
        {
            std::lock_guard<std::mutex> lk(ctx->mu);           // per step: other calls on the context get their turn
            if (!rg_usable(r)) return GPC_EINVAL;
            if (int rc = rg_check_params(ctx, params)) return rc;
            if (int rc = rg_step_locked(r, params, out)) return rc;
            s = r->steps;
        }
        if (trace && k < params->max_steps) memcpy(trace + (size_t)k * 9, out, sizeof(out));
        if (steps) *steps = k + 1;
        const double nt = std::sqrt(out[0] * out[0] + out[1] * out[1] + out[2] * out[2]);
        const double na = std::sqrt(out[3] * out[3] + out[4] * out[4] + out[5] * out[5]);
        if (s > params->min_steps && (s >= params->max_steps || (nt < params->tol && na < params->tol))) break;    // :69
    }
    return GPC_OK;
}

int gpc_registration_get_transform(gpc_registration* r, double R[9], double t[3])
{
    if (!r) return GPC_EINVAL;
    gpc_ctx* ctx = r->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!rg_usable(r)) return GPC_EINVAL;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (R) GPC_HIP(ctx, hipMemcpyAsync(R, r->state + RG_S_RC, 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (t) GPC_HIP(ctx, hipMemcpyAsync(t, r->state + RG_S_TC, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GPC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GPC_OK;
}

int gpc_registration_get_cloud(gpc_registration* r, gpc_point_xyzrgb* cloud)
{
    if (!r) return GPC_EINVAL;
    gpc_ctx* ctx = r->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!rg_usable(r)) return GPC_EINVAL;
    if (r->n == 0) return GPC_OK;
    if (!cloud) return gpc_fail(ctx, GPC_EINVAL, "cloud is NULL");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GPC_HIP(ctx, hipMemcpyAsync(cloud, r->cloud, sizeof(gpc_point_xyzrgb) * (size_t)r->n, hipMemcpyDeviceToHost, ctx->stream));
    GPC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GPC_OK;
}

int gpc_registration_cloud_dev(gpc_registration* r, const gpc_point_xyzrgb** cloud, int* n)
{
    if (!r) return GPC_EINVAL;
    gpc_ctx* ctx = r->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!rg_usable(r)) return GPC_EINVAL;
    if (!cloud || !n) return gpc_fail(ctx, GPC_EINVAL, "cloud/n is NULL");
    *cloud = r->n > 0 ? r->cloud : nullptr;
    *n = r->n;
    return GPC_OK;
}

int gpc_registration_get_assignment(gpc_registration* r, int32_t* owner, double* local)
{
    if (!r) return GPC_EINVAL;
    gpc_ctx* ctx = r->ctx;
    if (ctx->dead.load()) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!rg_usable(r)) return GPC_EINVAL;
    if (r->n == 0) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (owner) GPC_HIP(ctx, hipMemcpyAsync(owner, r->owner, sizeof(int32_t) * (size_t)r->n, hipMemcpyDeviceToHost, ctx->stream));
    if (local) GPC_HIP(ctx, hipMemcpyAsync(local, r->local, sizeof(double) * 3 * (size_t)r->n, hipMemcpyDeviceToHost, ctx->stream));
    GPC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GPC_OK;
}

}  // extern "C"
