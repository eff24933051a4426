// raycast.hip -- gp_mapping::train_classification (src/gp_mapping.cpp:154-211) on the GPU: every ray of a registered
// scan, from the sensor to its point, is cast through the leaf table of the map, and on the plane of every trained leaf it crosses the
// cell it meets is labelled: occupied where the ray ends (the leaf that owns the point), free where it goes on.  The labelled cells are
// what the occupancy GP (gpc_dense_irls_fit_predict_dev, BASELINE config 5) trains on; gpc_occupancy_batch_dev lays them out for it.
//
// The reference asks its octree for the leaves a ray intersects (get_intersected_gps, :170), walks that list from the far end (:175),
// waits for the owner of the point (reached_gp, :183-190) and handles every trained leaf from there to the sensor (:191-208), one scan
// point after the other, so that the last scan index wins a cell.  As in producer.hip, registration.hip and mapping.hip the walk is
// restated as a per-ray rule with no order left to the scheduler:
//   owner    gp_indices (:66-69, :233, :273) = the leaf whose bucket of the batch holds the point: a scatter of the batch's src over off
//   trained  gps[m].size() > 0 (:180): the depth GP's basis count, nullptr = every leaf
//   no-op    the point is unowned (:176), the owner is untrained (:180), or the ray does not meet the owner's voxel (slab test)
//   walk     a thread per ray: from the owner's voxel back towards the sensor, across the entry face of the voxel in hand.  The entry
//            parameters n_a = (face_a - o_a) / delta_a are recomputed from the integer voxel coordinate at every step (nothing
//            accumulates); max n_a <= 0: the sensor is in or behind this voxel, stop; ties go to the first axis; leaving the grid stops.
//            At most kmax[0] + kmax[1] + kmax[2] + 1 voxels: every step moves one coordinate towards the sensor.  No list per ray.
//   plane    :191-202 in one fixed association (rc_plane_cell); a non-finite d or loc skips the leaf (upstream: int(nan)); as upstream d is
//            not range-checked, so a plane met outside its voxel but inside the +-res/2 window is labelled all the same
//   write    atomicMax of (i + 1) << 1 | is_free on a zeroed uint32 per (leaf, cell): the largest scan index wins, as in the sequential loop
//            (one ray visits a leaf once, so a key is written once); rc_resolve_kernel turns the keys into the caller's bytes
// Integer atomics only: the same inputs give the same bits.  Contraction is off (producer_internal.h); tests/raycast_ref.py evaluates the
// same expressions in the same association.
#include <cmath>
#include <cstring>

#include <rocprim/device/device_scan.hpp>

#include "producer_internal.h"   // (switches floating-point contraction off)
#include "sparse_internal.h"

// flags / counters in the workspace: [0] a src entry >= n, [1] a non-finite coordinate, [2] no-op rays, [3] occupied writes, [4] free writes
enum { RC_BAD_SRC = 0, RC_BAD_XYZ = 1, RC_NOOP = 2, RC_OCC = 3, RC_FREE = 4, RC_WORDS = 8 };

struct RcArgs {
    PcGrid g;
    int n, P, n_total;
    const gpc_point_xyzrgb* cloud;
    const uint64_t* leaf_key;
    const int32_t *off, *src;
    const int32_t* bv;            // basis counts of the depth GPs, nullptr: every leaf trained
    const double *R, *mean;
    float o32[3];                 // the sensor as the octree sees it (:170)
    double org[3];                // ... and as the plane arithmetic does (:194-195)
    int32_t* owner;               // n
    uint32_t* key;                // P x m
    int32_t* cnt;                 // RC_WORDS
    uint8_t* cells;               // P x m, the caller's
};

// ---- owner of every scan point: bucket position s of leaf L holds scan point src[s] ------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void rc_owner_kernel(RcArgs A)
{
    const int s = blockIdx.x * PC_THREADS + threadIdx.x;
    if (s >= A.n_total) return;
    const int i = A.src[s];
    if (i < 0 || i >= A.n) {                                  // another cloud's batch
        atomicOr(&A.cnt[RC_BAD_SRC], 1);
        return;
    }
    int lo = 0, hi = A.P;                                     // the leaf with off[L] <= s < off[L + 1]: last L with off[L] <= s
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.off[mid] <= s) lo = mid; else hi = mid;
    }
    A.owner[i] = lo;
}

// the plane of leaf L against the ray org + d * delta (:191-202): the cell it meets, or -1
__device__ static inline int rc_plane_cell(const RcArgs& A, int L, const double delta[3])
{
    const PcGrid& g = A.g;
    const double* R = A.R + (size_t)L * 9;                    // column-major: R[0..2] = normal (:192)
    const double* mu = A.mean + (size_t)L * 3;
    const double num = R[0] * (mu[0] - A.org[0]) + R[1] * (mu[1] - A.org[1]) + R[2] * (mu[2] - A.org[2]);
    const double den = R[0] * delta[0] + R[1] * delta[1] + R[2] * delta[2];
    const double d = num / den;                               // :194
    const double e[3] = {(A.org[0] + d * delta[0]) - mu[0], (A.org[1] + d * delta[1]) - mu[1], (A.org[2] + d * delta[2]) - mu[2]};   // :195
    double t[3];
    pc_to_frame(R, e, t);                                     // R^T (x - mean), :196
    if (!(fabs(d) <= 1.7976931348623157e308) || !(fabs(t[0]) <= 1.7976931348623157e308) || !(fabs(t[1]) <= 1.7976931348623157e308) ||
        !(fabs(t[2]) <= 1.7976931348623157e308))
        return -1;
    if (t[1] > g.half || t[1] < -g.half || t[2] > g.half || t[2] < -g.half) return -1;                        // :197
    return pc_mask_cell(g, t[1], t[2]);                       // :200-201
}

// ---- a thread per ray ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void rc_cast_kernel(RcArgs A)
{
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    const PcGrid& g = A.g;
    int noop = 0, nocc = 0, nfree = 0, bad = 0;
    if (i < A.n) {
        const float4 f = *reinterpret_cast<const float4*>(&A.cloud[i]);
        const float pf[3] = {f.x, f.y, f.z};
        bad = !(fabsf(pf[0]) <= 3.4028234e38f) || !(fabsf(pf[1]) <= 3.4028234e38f) || !(fabsf(pf[2]) <= 3.4028234e38f);
        const int own = A.owner[i];
        noop = 1;
        if (!bad && own >= 0 && (!A.bv || A.bv[own] > 0)) {
            double o[3], delta[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                o[a] = (double)A.o32[a];
                delta[a] = (double)(pf[a] - A.o32[a]);        // :169, in float
            }
            int k[3];
            pc_unpack(g, A.leaf_key[own], k);
            // the owner's voxel against the ray
            double lo[3], hi[3], tn, tf;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = g.mn[a] + (double)(k[a] - g.koff[a]) * g.res;
                hi[a] = g.mn[a] + (double)(k[a] - g.koff[a] + 1) * g.res;
            }
            const double inf = __longlong_as_double(0x7ff0000000000000ll);
            const bool meets = pc_ray_box(lo, hi, o, delta, tn, tf);
            if (meets) {
                noop = 0;
                const int m = g.sz * g.sz;
                const int max_steps = g.kmax[0] + g.kmax[1] + g.kmax[2] + 1;     // voxels a monotone walk can visit
                for (int step = 0; step < max_steps; ++step) {
                    const int L = pc_find_leaf(A.leaf_key, A.P, pc_pack(g, k[0], k[1], k[2]));
                    if (L >= 0 && (!A.bv || A.bv[L] > 0)) {
                        const int cell = rc_plane_cell(A, L, delta);
                        if (cell >= 0) {
                            const uint32_t is_free = L == own ? 0u : 1u;        // :203-208
                            atomicMax(&A.key[(size_t)L * (size_t)m + (size_t)cell], ((uint32_t)(i + 1) << 1) | is_free);
                            if (is_free) ++nfree; else ++nocc;
                        }
                    }
                    // the face the ray entered this voxel through
                    double best = -inf;
                    int ax = -1;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        if (delta[a] == 0.0) continue;
                        const int kf = delta[a] > 0.0 ? k[a] - g.koff[a] : k[a] - g.koff[a] + 1;
                        const double na = ((g.mn[a] + (double)kf * g.res) - o[a]) / delta[a];
                        if (na > best) { best = na; ax = a; }  // (strict: the first axis that attains the maximum)
                    }
                    if (ax < 0 || !(best > 0.0)) break;        // the sensor is in or behind this voxel
                    k[ax] += delta[ax] > 0.0 ? -1 : 1;
                    if (k[ax] < 0 || k[ax] > g.kmax[ax]) break;
                }
            }
        }
    }
    // counters: one atomic per wave and word
    const int any_bad = __any(bad);
    for (int o = 32; o > 0; o >>= 1) {
        noop += __shfl_xor(noop, o);
        nocc += __shfl_xor(nocc, o);
        nfree += __shfl_xor(nfree, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (any_bad) atomicOr(&A.cnt[RC_BAD_XYZ], 1);
        if (noop) atomicAdd(&A.cnt[RC_NOOP], noop);
        if (nocc) atomicAdd(&A.cnt[RC_OCC], nocc);
        if (nfree) atomicAdd(&A.cnt[RC_FREE], nfree);
    }
}

// ---- keys -> the caller's bytes; nothing is written when the inputs were refused ------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void rc_resolve_kernel(RcArgs A, size_t total)
{
    if (A.cnt[RC_BAD_SRC] | A.cnt[RC_BAD_XYZ]) return;
    const size_t c = (size_t)blockIdx.x * PC_THREADS + threadIdx.x;
    if (c >= total) return;
    const uint32_t key = A.key[c];
    if (key) A.cells[c] = (key & 1u) ? (uint8_t)GPC_CELL_FREE : (uint8_t)GPC_CELL_OCCUPIED;
}

// ---- the occupancy batch: a wave per leaf, observed cells in ascending cell index --------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void rc_count_kernel(const uint8_t* cells, int P, int m, int32_t* cnt, int32_t* nmax)
{
    const int lane = threadIdx.x & 63;
    const int L = blockIdx.x * PC_WAVES + (threadIdx.x >> 6);
    if (L > P) return;
    int c = 0;
    if (L < P) {
        const uint8_t* row = cells + (size_t)L * (size_t)m;
        for (int j = lane; j < m; j += 64) c += row[j] != GPC_CELL_UNOBSERVED;
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    }
    if (lane == 0) {
        cnt[L] = c;                                           // cnt[P] = 0: the exclusive scan's last entry is the total
        if (c) atomicMax(nmax, c);
    }
}

__global__ __launch_bounds__(PC_THREADS) void rc_batch_kernel(const uint8_t* cells, int P, int m, int sz, double res, const int32_t* off,
                                                              double* x0, double* x1, double* y)
{
    const int lane = threadIdx.x & 63;
    const int L = blockIdx.x * PC_WAVES + (threadIdx.x >> 6);
    if (L >= P) return;
    const uint8_t* row = cells + (size_t)L * (size_t)m;
    int base = off[L];
    for (int j0 = 0; j0 < m; j0 += 64) {
        const int j = j0 + lane;
        const uint8_t v = j < m ? row[j] : (uint8_t)GPC_CELL_UNOBSERVED;
        const bool obs = v != GPC_CELL_UNOBSERVED;
        const unsigned long long mask = __ballot(obs);
        if (obs) {
            const int s = base + __popcll(mask & ((1ull << lane) - 1));
            const int gx = j / sz, gy = j % sz;
            x0[s] = res * (((double)gx + 0.5) / (double)sz - 0.5);        // src/gp_compressor.cpp:326-327
            x1[s] = res * (((double)gy + 0.5) / (double)sz - 0.5);
            y[s] = v == GPC_CELL_OCCUPIED ? 1.0 : -1.0;
        }
        base += __popcll(mask);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
extern "C" {

int gpc_patches_raycast_dev(gpc_ctx* ctx, const gpc_patches* map, const gpc_sparse* depth, const gpc_point_xyzrgb* cloud, int n,
                            const double origin[3], uint8_t* cells, int32_t* counts)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!map) return gpc_fail(ctx, GPC_EINVAL, "map is NULL");
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative point count");
    if (n > 0 && !cloud) return gpc_fail(ctx, GPC_EINVAL, "cloud is NULL");
    if (!origin) return gpc_fail(ctx, GPC_EINVAL, "origin is NULL");
    if (!cells) return gpc_fail(ctx, GPC_EINVAL, "cells is NULL");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(origin[a])) return gpc_fail(ctx, GPC_EINVAL, "the origin is not finite");
    if (n > (1 << 30)) return gpc_fail(ctx, GPC_ERANGE, "more than 2^30 rays: the cell key holds the scan index in 31 bits");
    std::lock_guard<std::mutex> lk(ctx->mu);
    // (an object of another context is not in this context's list: found out without touching it)
    if (!gpc_child_listed(ctx, map) || (depth && !gpc_child_listed(ctx, depth)))
        return gpc_fail(ctx, GPC_EINVAL, "map and depth must be live objects of this context");
    const int P = map->v.P;
    if (depth && (depth->ny != 1 || depth->P != P))
        return gpc_fail(ctx, GPC_EINVAL, "depth must have ny == 1 and the map's P (%d), got ny %d, P %d", P, depth->ny, depth->P);
    if (counts) {
        counts[0] = n;
        counts[1] = counts[2] = counts[3] = 0;
    }
    if (n == 0) return GPC_OK;                                // no ray: the cells stay as they are
    const int n_total = map->v.n_total;
    if (n_total > n) return gpc_fail(ctx, GPC_EINVAL, "the batch holds %d points, the cloud %d: it was cut from another cloud", n_total, n);
    if (P == 0) {
        if (counts) counts[1] = n;
        return GPC_OK;
    }
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    hipStream_t st = ctx->stream;
    const size_t total = (size_t)P * (size_t)map->v.m;       // <= 2^31 - 1 (the cutters refuse more)
    RcArgs A;
    memset(&A, 0, sizeof(A));
    {
        int32_t *owner = nullptr, *cnt = nullptr;
        uint32_t* key = nullptr;
        for (int pass = 0; pass < 2; ++pass) {
            PcCarver c(pass ? ctx->ws : nullptr);
            cnt = c.take<int32_t>(RC_WORDS);
            key = c.take<uint32_t>(total);                    // (contiguous with cnt: one memset clears both)
            owner = c.take<int32_t>((size_t)n);
            if (!pass) {
                const int rc = gpc_ws_reserve(ctx, c.used);
                if (rc != GPC_OK) return rc;
            }
        }
        A.owner = owner; A.key = key; A.cnt = cnt;
    }
    A.g = map->grid; A.n = n; A.P = P; A.n_total = n_total;
    A.cloud = cloud; A.leaf_key = map->leaf_key; A.off = map->v.off; A.src = map->v.src;
    A.bv = depth ? depth->b : nullptr;
    A.R = map->v.rotations; A.mean = map->v.means;
    for (int a = 0; a < 3; ++a) {
        A.o32[a] = (float)origin[a];
        A.org[a] = origin[a];
    }
    A.cells = cells;
    GPC_HIP(ctx, hipMemsetAsync(A.cnt, 0, (size_t)((char*)(A.key + total) - (char*)A.cnt), st));
    GPC_HIP(ctx, hipMemsetAsync(A.owner, 0xff, sizeof(int32_t) * (size_t)n, st));                             // -1: unowned
    if (n_total > 0) {
        hipLaunchKernelGGL(rc_owner_kernel, dim3((n_total + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, st, A);
        GPC_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(rc_cast_kernel, dim3((n + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, st, A);
    GPC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(rc_resolve_kernel, dim3((unsigned)((total + PC_THREADS - 1) / PC_THREADS)), dim3(PC_THREADS), 0, st, A, total);
    GPC_HIP(ctx, hipGetLastError());
    if (counts) {
        int32_t h[RC_WORDS];
        GPC_HIP(ctx, hipMemcpyAsync(h, A.cnt, sizeof(h), hipMemcpyDeviceToHost, st));
        GPC_HIP(ctx, hipStreamSynchronize(st));
        if (h[RC_BAD_SRC]) return gpc_fail(ctx, GPC_EINVAL, "the batch names a point beyond the cloud's %d: it was cut from another cloud", n);
        if (h[RC_BAD_XYZ]) return gpc_fail(ctx, GPC_EINVAL, "the cloud holds a non-finite coordinate");
        counts[1] = h[RC_NOOP]; counts[2] = h[RC_OCC]; counts[3] = h[RC_FREE];
    }
    return GPC_OK;
}

int gpc_patches_raycast(gpc_ctx* ctx, const gpc_patches* map, const gpc_sparse* depth, const gpc_point_xyzrgb* cloud, int n,
                        const double origin[3], uint8_t* cells, int32_t* counts)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!map) return gpc_fail(ctx, GPC_EINVAL, "map is NULL");
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative point count");
    if (n > 0 && !cloud) return gpc_fail(ctx, GPC_EINVAL, "cloud is NULL");
    if (!cells) return gpc_fail(ctx, GPC_EINVAL, "cells is NULL");
    size_t total = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (!gpc_child_listed(ctx, map)) return gpc_fail(ctx, GPC_EINVAL, "map must be a live object of this context");
        total = (size_t)map->v.P * (size_t)map->v.m;
    }
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    int32_t local[4];                                         // the host entry always learns what only the device can find
    GpcStaging st(ctx, "gpc_patches_raycast");
    const gpc_point_xyzrgb* d_cloud = st.up(cloud, (size_t)n);
    uint8_t* d_cells = st.up(cells, total);
    if (st.ok()) st.rc = gpc_patches_raycast_dev(ctx, map, depth, d_cloud, n, origin, d_cells, local);
    st.down(cells, d_cells, total);
    if (st.ok() && counts) memcpy(counts, local, sizeof(local));
    return st.finish();
}

int gpc_occupancy_batch_dev(gpc_ctx* ctx, const gpc_patches* map, const uint8_t* cells, int32_t* off, double* x0, double* x1, double* y,
                            int32_t* n_total, int32_t* n_max)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!map) return gpc_fail(ctx, GPC_EINVAL, "map is NULL");
    if (!cells || !off || !x0 || !x1 || !y) return gpc_fail(ctx, GPC_EINVAL, "cells, off, x0, x1 and y must not be NULL");
    if (!n_total || !n_max) return gpc_fail(ctx, GPC_EINVAL, "n_total and n_max must not be NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!gpc_child_listed(ctx, map)) return gpc_fail(ctx, GPC_EINVAL, "map must be a live object of this context");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    hipStream_t st = ctx->stream;
    const int P = map->v.P, m = map->v.m;
    const PcGrid& g = map->grid;
    size_t scan_bytes = 0;
    GPC_HIP(ctx, rocprim::exclusive_scan(nullptr, scan_bytes, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, (size_t)P + 1,
                                         rocprim::plus<int32_t>(), st));
    int32_t *cnt = nullptr, *nmax = nullptr;
    void* prim = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        PcCarver c(pass ? ctx->ws : nullptr);
        nmax = c.take<int32_t>(1);
        cnt = c.take<int32_t>((size_t)P + 1);
        prim = c.take<char>(scan_bytes);
        if (!pass) {
            const int rc = gpc_ws_reserve(ctx, c.used);
            if (rc != GPC_OK) return rc;
        }
    }
    GPC_HIP(ctx, hipMemsetAsync(nmax, 0, sizeof(int32_t), st));
    const int lblk = (P + 1 + PC_WAVES - 1) / PC_WAVES;
    hipLaunchKernelGGL(rc_count_kernel, dim3(lblk), dim3(PC_THREADS), 0, st, cells, P, m, cnt, nmax);
    GPC_HIP(ctx, hipGetLastError());
    GPC_HIP(ctx, rocprim::exclusive_scan(prim, scan_bytes, cnt, off, (int32_t)0, (size_t)P + 1, rocprim::plus<int32_t>(), st));
    if (P > 0) {
        hipLaunchKernelGGL(rc_batch_kernel, dim3((P + PC_WAVES - 1) / PC_WAVES), dim3(PC_THREADS), 0, st, cells, P, m, g.sz, g.res,
                           (const int32_t*)off, x0, x1, y);
        GPC_HIP(ctx, hipGetLastError());
    }
    int32_t h_total = 0, h_max = 0;
    GPC_HIP(ctx, hipMemcpyAsync(&h_total, off + P, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GPC_HIP(ctx, hipMemcpyAsync(&h_max, nmax, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GPC_HIP(ctx, hipStreamSynchronize(st));
    *n_total = h_total;
    *n_max = h_max;
    return GPC_OK;
}

}  // extern "C"
