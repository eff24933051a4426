// producer.hip -- the step before the hot path: gp_compressor::project_cloud with
// compute_rotation and project_points (/root/reference/src/gp_compressor.cpp:177-249, 29-64, 66-118) on the GPU.
// A pcl::PointXYZRGB cloud goes in; the ragged patch batch the GP kernels consume (off, X, y, C, R_i, mean_i, RGB mean,
// W) comes out resident in HBM, so that cloud -> patches -> GP -> cloud needs no host pass over the points.
//
// The reference walks the leaves of a PCL octree one after the other and lets each leaf claim the points of its
// search sphere that nobody claimed before (occupied_indices): a serial dependence in its letter, not in its substance --
//   * the frame R_i of a leaf depends on every point of its sphere, claimed or not (:220-236), so frames are independent;
//   * a point is claimed by the FIRST leaf in leaf order whose sphere holds it and whose +-res/2 window accepts it
//     (:81-89); candidates are the <= 27 leaves around the point's voxel, so ownership is a per-point minimum.
// Pipeline (all HBM-bound integer / gather work; nothing here is GEMM-shaped):
//   1 pc_bounds_kernel    min / max corner, finiteness: one pass over the cloud, one set of atomics per workgroup
//   2 pc_keys_kernel      voxel key (z, y, x packed) per point, then rocPRIM's stable radix sort of (key, index) over
//                         exactly the key's bits, pc_heads/pc_leaves: leaf table (sorted unique keys + segment starts)
//   3 pc_gather_kernel    points re-laid in sorted order as 16-byte records (x, y, z, rgb): every later access to a
//                         voxel's points is one contiguous, coalesced segment
//   4 pc_moment_kernel    one wave per leaf: 27 neighbour segments (binary search in the leaf table), sphere test by
//                         ballot; the hits' exact products go to LDS in hit order and 16 lanes (one matrix entry each)
//                         add them up in the oracle's order -- the only serial chain is one f64 add per hit
//     pc_frame_kernel     one thread per leaf: cyclic Jacobi eigen-solve of the 4x4 moment matrix, frame (:37-63)
//   5 pc_claim_kernel     one wave per leaf: the 27 candidate frames sit in LDS, the leaf's own points test them in
//                         leaf order and stop at the first that accepts; patch-frame coordinates; counts
//   6 pc_emit_kernel      one wave per leaf: ordered compaction (ballot + prefix popcount) of the points it owns, depth
//                         mean as the oracle's sequential sum, colour means, mean removal, centre shift, mask W
// Scratch lives in the context's grow-only workspace and the result in one allocation: a call costs three small
// device->host reads (bounds, leaf count, totals) and no allocation in steady state beyond the result's.
// Stages 1-3, the layout of the result and the tail that publishes it are host functions of their own (pc_cloud_bounds,
// pc_voxel_table_*, pc_patches_alloc, pc_patches_publish: producer_internal.h), which gpc_patches_insert_cloud (mapping.hip) runs
// too; so are the launchers of the bucket kernels every cutter uses (pc_bucket_offsets, pc_nmax).  Their kernels are defined here, once.
// Bit-exactness: floating-point contraction is off for this file and every expression is written in the association of
// oracle/gpc_oracle_producer.c; products of two floats are exact in double, so the moment sums only fix the ORDER.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "producer_internal.h"   // (switches floating-point contraction off)
#include "sparse_internal.h"     // sp_live

// ---- 1: bounds; 2: keys, leaf table (PcGrid and the key arithmetic: producer_internal.h) -------------------------------------
// out[0..2] = ordered min, out[3..5] = ordered max, out[6] = 1 if a coordinate is not finite
__global__ __launch_bounds__(PC_THREADS) void pc_bounds_kernel(const gpc_point_xyzrgb* cloud, int n, uint32_t* out)
{
    __shared__ uint32_t red[PC_WAVES][8];
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0, 0, 0};
    int bad = 0;
    for (int i = blockIdx.x * PC_THREADS + threadIdx.x; i < n; i += gridDim.x * PC_THREADS) {
        const float4 p = *reinterpret_cast<const float4*>(&cloud[i]);
        const float c[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            bad |= !(fabsf(c[a]) <= 3.4028234e38f);
            const uint32_t o = pc_ordered(c[a]);
            lo[a] = min(lo[a], o);
            hi[a] = max(hi[a], o);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], o));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], o));
        }
    }
    bad = __any(bad);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[w][a] = lo[a]; red[w][3 + a] = hi[a]; }
        red[w][6] = (uint32_t)bad;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int a = threadIdx.x;
        uint32_t v = red[0][a];
        for (int q = 1; q < PC_WAVES; ++q) v = a < 3 ? min(v, red[q][a]) : max(v, red[q][a]);   // [6]: 0 / 1, max == or
        if (a < 3) atomicMin(&out[a], v); else if (a < 6) atomicMax(&out[a], v); else if (v) atomicOr(&out[6], 1u);
    }
}

__global__ __launch_bounds__(PC_THREADS) void pc_keys_kernel(PcGrid g, const gpc_point_xyzrgb* cloud, int n, uint64_t* keys, int32_t* vals)
{
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= n) return;
    const float4 p = *reinterpret_cast<const float4*>(&cloud[i]);
    int k[3];
    pc_voxel(g, p.x, p.y, p.z, k);
    keys[i] = pc_pack(g, k[0], k[1], k[2]);
    vals[i] = i;
}

__global__ __launch_bounds__(PC_THREADS) void pc_heads_kernel(const uint64_t* keys, int n, int32_t* head)
{
    const int s = blockIdx.x * PC_THREADS + threadIdx.x;
    if (s < n) head[s] = (s == 0 || keys[s] != keys[s - 1]) ? 1 : 0;
}

// leaf_of[s] holds the inclusive scan of head[] on entry (leaf id + 1) and the leaf id on exit
__global__ __launch_bounds__(PC_THREADS) void pc_leaves_kernel(const uint64_t* keys, int n, int P, int32_t* leaf_of, uint64_t* leaf_key,
                                                        int32_t* leaf_start)
{
    const int s = blockIdx.x * PC_THREADS + threadIdx.x;
    if (s >= n) return;
    const int id = leaf_of[s] - 1;
    leaf_of[s] = id;
    if (s == 0 || keys[s] != keys[s - 1]) {
        leaf_key[id] = keys[s];
        leaf_start[id] = s;
    }
    if (s == n - 1) leaf_start[P] = n;
}

// ---- 3: sorted-order copy ------------------------------------------------------------------------------------------------
// points re-laid in sorted order
__global__ __launch_bounds__(PC_THREADS) void pc_gather_kernel(const gpc_point_xyzrgb* cloud, const int32_t* vals, int n, PcPoint* sp)
{
    const int s = blockIdx.x * PC_THREADS + threadIdx.x;
    if (s >= n) return;
    const gpc_point_xyzrgb* q = &cloud[vals[s]];
    const float4 p = *reinterpret_cast<const float4*>(q);
    PcPoint o;
    o.x = p.x; o.y = p.y; o.z = p.z;
    o.rgb = pc_rgb_of(q);
    *reinterpret_cast<float4*>(&sp[s]) = *reinterpret_cast<const float4*>(&o);
}

// ---- 4: frames -------------------------------------------------------------------------------------------------------------
struct PcArgs {
    PcGrid g;
    int n, P;
    const uint64_t* leaf_key;
    const int32_t* leaf_start;
    const int32_t* leaf_of;
    const int32_t* vals;
    const PcPoint* sp;
    int32_t* nbr;          // P x 27 neighbour leaf ids (-1: empty voxel), (dz, dy, dx) order = ascending leaf order
    double* M;             // P x 16 moment matrices
    int32_t* kcount;       // P: points in the search sphere
    double* cen;           // P x 3 voxel centres
    int32_t* owner;        // per sorted position: owning leaf or -1
    double *py, *px0, *px1;   // per sorted position: patch-frame coordinates in the owner's frame
    int32_t* cnt;          // P + 1: points owned per leaf (cnt[P] = 0)
    int32_t* off;          // P + 1: exclusive scan of cnt
    int32_t* nmax;
    double *R, *mean, *rgb_mean;
    uint8_t* W;
    double *x0, *x1, *y, *rgb;
    int32_t* src;
};

__global__ __launch_bounds__(PC_THREADS) void pc_moment_kernel(PcArgs A)
{
    // per wave: 10 rows (xx xy xz x yy yz y zz z 1) of the hits of one 64-point chunk, in hit order
    __shared__ double prod[PC_WAVES][10 * PC_LROW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int leaf = blockIdx.x * PC_WAVES + w;
    if (leaf >= A.P) return;                                  // whole waves leave; no block-level synchronisation below
    const PcGrid& g = A.g;
    double* pr = prod[w];
    int k3[3];
    pc_unpack(g, A.leaf_key[leaf], k3);
    double center[3];
    pc_center(g, k3, center);
    // the 27 neighbour segments: lane j looks up voxel (dz, dy, dx) = (j / 9, j / 3 % 3, j % 3) - 1
    int seg0 = 0, seg1 = 0;
    if (lane < 27) {
        const int nx = k3[0] + lane % 3 - 1, ny = k3[1] + (lane / 3) % 3 - 1, nz = k3[2] + lane / 9 - 1;
        int nb = -1;
        if (nx >= 0 && nx <= g.kmax[0] && ny >= 0 && ny <= g.kmax[1] && nz >= 0 && nz <= g.kmax[2])
            nb = pc_find_leaf(A.leaf_key, A.P, pc_pack(g, nx, ny, nz));
        A.nbr[(size_t)leaf * 27 + lane] = nb;
        if (nb >= 0) { seg0 = A.leaf_start[nb]; seg1 = A.leaf_start[nb + 1]; }
    }
    if (lane < 3) A.cen[(size_t)leaf * 3 + lane] = lane == 0 ? center[0] : (lane == 1 ? center[1] : center[2]);
    double M;
    int k;
    pc_sphere_moments(g, center, seg0, seg1, A.sp, pr, lane, M, k);
    if (lane < 16) A.M[(size_t)leaf * 16 + lane] = M;
    if (lane == 0) A.kcount[leaf] = k;
}

#define PC_FRAME_THREADS 64     // one wave per workgroup: the leaves spread over as many CUs as possible

__global__ __launch_bounds__(PC_FRAME_THREADS) void pc_frame_kernel(PcArgs A)
{
    const int leaf = blockIdx.x * PC_FRAME_THREADS + threadIdx.x;
    if (leaf >= A.P) return;
    double R[9];
    pc_frame_of_moments(A.M + (size_t)leaf * 16, A.kcount[leaf], R);
#pragma unroll
    for (int i = 0; i < 9; ++i) A.R[(size_t)leaf * 9 + i] = R[i];
}

// ---- 5: ownership ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void pc_claim_kernel(PcArgs A)
{
    __shared__ double frames[PC_WAVES][27][12];               // per wave: centre (3) + R (9) of the 27 candidate leaves
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int leaf = blockIdx.x * PC_WAVES + w;
    if (leaf >= A.P) return;
    const PcGrid& g = A.g;
    int nb = -1;
    if (lane < 27) {
        nb = A.nbr[(size_t)leaf * 27 + lane];
        if (nb >= 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) frames[w][lane][i] = A.cen[(size_t)nb * 3 + i];
#pragma unroll
            for (int i = 0; i < 9; ++i) frames[w][lane][3 + i] = A.R[(size_t)nb * 9 + i];
        }
    }
    __builtin_amdgcn_wave_barrier();
    const double r2 = g.radius * g.radius;
    const int s0 = A.leaf_start[leaf], s1 = A.leaf_start[leaf + 1];
    for (int base = s0; base < s1; base += 64) {
        const int s = base + lane;
        const bool valid = s < s1;
        double p[3] = {0, 0, 0};
        if (valid) {
            const float4 f = *reinterpret_cast<const float4*>(&A.sp[s]);
            p[0] = (double)f.x; p[1] = (double)f.y; p[2] = (double)f.z;
        }
        int owner = -1;
        double pt[3] = {0, 0, 0};
        for (int j = 0; j < 27; ++j) {                        // candidates in leaf order: the first that accepts owns the point
            const int L = __builtin_amdgcn_readlane(nb, j);
            if (L < 0) continue;
            if (!__any(valid && owner < 0)) break;
            const double* fr = frames[w][j];
            const double d[3] = {p[0] - fr[0], p[1] - fr[1], p[2] - fr[2]};
            const bool in = valid && owner < 0 && d[0] * d[0] + d[1] * d[1] + d[2] * d[2] <= r2;    // in L's search sphere
            if (!__any(in)) continue;
            double q[3];
            pc_to_frame(fr + 3, d, q);                        // R^T d  (:84)
            const bool acc = in && !(q[1] > g.half || q[1] < -g.half || q[2] > g.half || q[2] < -g.half);     // :85-87
            if (acc) { owner = L; pt[0] = q[0]; pt[1] = q[1]; pt[2] = q[2]; }
            const int c = __popcll(__ballot(acc));
            if (c && lane == 0) atomicAdd(&A.cnt[L], c);
        }
        if (valid) {
            A.owner[s] = owner;
            A.py[s] = pt[0];
            A.px0[s] = pt[1];
            A.px1[s] = pt[2];
        }
    }
}

// ---- the bucket kernels of every cutter (pc_bucket_offsets, pc_nmax: producer_internal.h) -----------------------------------------
__global__ __launch_bounds__(PC_THREADS) void pc_bucket_offsets_kernel(const uint32_t* skey, int n, int P, int32_t* off)
{
    const int j = blockIdx.x * PC_THREADS + threadIdx.x;
    if (j <= P) off[j] = pc_lower_bound(skey, n, (uint32_t)j);
}

__global__ __launch_bounds__(PC_THREADS) void pc_nmax_kernel(const int32_t* off, int P, int32_t* nmax)
{
    int m = 0, c0 = 0, c1 = 0;
    for (int i = blockIdx.x * PC_THREADS + threadIdx.x; i < P; i += gridDim.x * PC_THREADS) {
        const int n = off[i + 1] - off[i];
        m = max(m, n);
        c0 += n <= 256;
        c1 += n <= 272;
    }
    for (int o = 32; o > 0; o >>= 1) {
        m = max(m, __shfl_xor(m, o));
        c0 += __shfl_xor(c0, o);
        c1 += __shfl_xor(c1, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(nmax, m);
        atomicAdd(nmax + 1, c0);
        atomicAdd(nmax + 2, c1);
    }
}

// ---- 6: ordered compaction, means, mask ------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void pc_emit_kernel(PcArgs A)
{
    const int lane = threadIdx.x & 63;
    const int leaf = blockIdx.x * PC_WAVES + (threadIdx.x >> 6);
    if (leaf >= A.P) return;
    const PcGrid& g = A.g;
    const int base_q = A.off[leaf], cnt = A.off[leaf + 1] - base_q, total = A.off[A.P];
    int seg0 = 0, seg1 = 0;
    if (lane < 27) {
        const int nb = A.nbr[(size_t)leaf * 27 + lane];
        if (nb >= 0) { seg0 = A.leaf_start[nb]; seg1 = A.leaf_start[nb + 1]; }
    }
    int k3[3];
    pc_unpack(g, A.leaf_key[leaf], k3);
    double mid[3];
    pc_center(g, k3, mid);
    // pass 1: depth sum in patch order (the oracle's sequential sum), colour sums (integers: any order)
    double mnd = 0.0;
    int cs[3] = {0, 0, 0};
    for (int j = 0; j < 27; ++j) {
        const int s0 = __builtin_amdgcn_readlane(seg0, j), s1 = __builtin_amdgcn_readlane(seg1, j);
        for (int b0 = s0; b0 < s1; b0 += 64) {
            const int s = b0 + lane;
            const bool mine = s < s1 && A.owner[s] == leaf;
            double d = 0.0;
            if (mine) {
                d = A.py[s];
                const uint32_t c = A.sp[s].rgb;
                cs[0] += (int)(c & 0xffu); cs[1] += (int)((c >> 8) & 0xffu); cs[2] += (int)((c >> 16) & 0xffu);
            }
            unsigned long long mask = __ballot(mine);
            while (mask) {
                const int b = __builtin_ctzll(mask);
                mask &= mask - 1;
                mnd += pc_readlane_d(d, b);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int o = 32; o > 0; o >>= 1) cs[a] += __shfl_xor(cs[a], o);
    double cmean[3] = {0, 0, 0};
    if (cnt > 0) {                                                           // :101-107, :116
        mnd /= (double)cnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) cmean[a] = (double)cs[a] / (double)cnt;
        const double* R = A.R + (size_t)leaf * 9;
#pragma unroll
        for (int a = 0; a < 3; ++a) mid[a] += mnd * R[a];
    }
    if (lane < 3) {
        A.mean[(size_t)leaf * 3 + lane] = lane == 0 ? mid[0] : (lane == 1 ? mid[1] : mid[2]);
        A.rgb_mean[(size_t)leaf * 3 + lane] = lane == 0 ? cmean[0] : (lane == 1 ? cmean[1] : cmean[2]);
    }
    // pass 2: the same walk, writing the patch in hit order
    uint8_t* W = A.W + (size_t)leaf * (size_t)(g.sz * g.sz);
    int run = 0;
    for (int j = 0; j < 27; ++j) {
        const int s0 = __builtin_amdgcn_readlane(seg0, j), s1 = __builtin_amdgcn_readlane(seg1, j);
        for (int b0 = s0; b0 < s1; b0 += 64) {
            const int s = b0 + lane;
            const bool mine = s < s1 && A.owner[s] == leaf;
            const unsigned long long mask = __ballot(mine);
            if (mine) {
                const size_t q = (size_t)base_q + run + __popcll(mask & ((1ull << lane) - 1));
                const double u = A.px0[s], w = A.px1[s];
                A.y[q] = A.py[s] - mnd;
                A.x0[q] = u;
                A.x1[q] = w;
                A.src[q] = A.vals[s];
                const uint32_t c = A.sp[s].rgb;
                A.rgb[q] = (double)(c & 0xffu) - cmean[0];
                A.rgb[(size_t)total + q] = (double)((c >> 8) & 0xffu) - cmean[1];
                A.rgb[2 * (size_t)total + q] = (double)((c >> 16) & 0xffu) - cmean[2];
                W[pc_mask_cell(g, u, w)] = 1;                 // :90-92
            }
            run += __popcll(mask);
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// (struct gpc_patches and the stages' contracts: producer_internal.h)
int pc_cloud_bounds(gpc_ctx* ctx, const char* entry, const gpc_point_xyzrgb* cloud, int n, uint32_t hb[8])
{
    if (int rc = gpc_ws_reserve(ctx, 4096)) return rc;
    hipStream_t st = ctx->stream;
    uint32_t* d_bounds = static_cast<uint32_t*>(ctx->ws);
    const uint32_t init[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0, 0, 0, 0, 0};
    const int nblk = (n + PC_THREADS - 1) / PC_THREADS;
    hipError_t e = hipMemcpyAsync(d_bounds, init, sizeof(init), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pc_bounds_kernel, dim3(nblk < ctx->num_cus * 4 ? nblk : ctx->num_cus * 4), dim3(PC_THREADS), 0, st, cloud, n, d_bounds);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hb, d_bounds, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess)
        return gpc_fail(ctx, e == hipErrorOutOfMemory ? GPC_ENOMEM : GPC_EHIP, "%s: the bounds pass failed: %s", entry, hipGetErrorString(e));
    if (hb[6]) return gpc_fail(ctx, GPC_EINVAL, "the cloud holds a non-finite coordinate");
    return GPC_OK;
}

#define PC_RET(call)                      \
    do {                                  \
        hipError_t e_ = (call);           \
        if (e_ != hipSuccess) return e_;  \
    } while (0)

hipError_t pc_voxel_table_prim_bytes(gpc_ctx* ctx, const PcGrid& g, size_t n, size_t* bytes)
{
    size_t sort_bytes = 0, scan_bytes = 0;
    PC_RET(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, n, 0u,
                                     (unsigned)(g.bx + g.by + g.bz), ctx->stream));
    PC_RET(rocprim::inclusive_scan(nullptr, scan_bytes, (int32_t*)nullptr, (int32_t*)nullptr, n, rocprim::plus<int32_t>(), ctx->stream));
    *bytes = std::max(sort_bytes, scan_bytes);
    return hipSuccess;
}

hipError_t pc_voxel_table_build(gpc_ctx* ctx, const PcGrid& g, const gpc_point_xyzrgb* cloud, int n, const PcVoxelTable& T, void* prim,
                                size_t prim_bytes, int32_t* count)
{
    hipStream_t st = ctx->stream;
    const int nblk = (n + PC_THREADS - 1) / PC_THREADS;
    const size_t N = (size_t)n;
    // 2: keys, stable sort over exactly the key's bits (<= 63), heads, leaf id + 1 per sorted position
    hipLaunchKernelGGL(pc_keys_kernel, dim3(nblk), dim3(PC_THREADS), 0, st, g, cloud, n, T.k0, T.v0);
    PC_RET(hipGetLastError());
    size_t tb = prim_bytes;
    PC_RET(rocprim::radix_sort_pairs(prim, tb, T.k0, T.keys, T.v0, T.vals, N, 0u, (unsigned)(g.bx + g.by + g.bz), st));
    hipLaunchKernelGGL(pc_heads_kernel, dim3(nblk), dim3(PC_THREADS), 0, st, T.keys, n, T.head);
    PC_RET(hipGetLastError());
    tb = prim_bytes;
    PC_RET(rocprim::inclusive_scan(prim, tb, T.head, T.leaf_of, N, rocprim::plus<int32_t>(), st));
    PC_RET(hipMemcpyAsync(count, T.leaf_of + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    // 3: sorted-order copy (does not need the count: overlaps the read-back)
    hipLaunchKernelGGL(pc_gather_kernel, dim3(nblk), dim3(PC_THREADS), 0, st, cloud, T.vals, n, T.sp);
    PC_RET(hipGetLastError());
    return hipStreamSynchronize(st);
}

hipError_t pc_voxel_table_leaves(gpc_ctx* ctx, int n, const PcVoxelTable& T, int count, uint64_t* leaf_key, int32_t* leaf_start)
{
    hipLaunchKernelGGL(pc_leaves_kernel, dim3((n + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, ctx->stream, T.keys, n, count, T.leaf_of,
                       leaf_key, leaf_start);
    return hipGetLastError();
}

// per-point arrays are sized by N (an upper bound of the points owned)
hipError_t pc_patches_alloc(gpc_patches* o, size_t P, size_t N, size_t m)
{
    for (int pass = 0; pass < 2; ++pass) {
        PcCarver oc(pass ? o->block : nullptr);
        o->v.off = oc.take<int32_t>(P + 1);
        o->v.rotations = oc.take<double>(9 * P);
        o->v.means = oc.take<double>(3 * P);
        o->v.rgb_means = oc.take<double>(3 * P);
        o->v.W = oc.take<uint8_t>(P * m);
        o->v.x0 = oc.take<double>(N);
        o->v.x1 = oc.take<double>(N);
        o->v.y = oc.take<double>(N);
        o->v.rgb = oc.take<double>(3 * N);
        o->v.src = oc.take<int32_t>(N);
        o->leaf_key = oc.take<uint64_t>(P);             // (last: the batch's own arrays keep their places)
        if (!pass) PC_RET(hipMalloc(&o->block, oc.used));
    }
    return hipSuccess;
}

hipError_t pc_patches_publish(gpc_ctx* ctx, gpc_patches* o, int P, const int32_t* nmax_dev)
{
    hipStream_t st = ctx->stream;
    int32_t total = 0, nmax[3] = {0, 0, 0};
    PC_RET(hipMemcpyAsync(&total, o->v.off + P, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PC_RET(hipMemcpyAsync(nmax, nmax_dev, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PC_RET(hipStreamSynchronize(st));
    o->v.P = P; o->v.n_total = total; o->v.n_max = nmax[0];
    // the size classes of this batch, for the dense dispatch (keyed by the batch's own `off` buffer, which lives as long as the object)
    ctx->hint_off = o->v.off; ctx->hint_P = P; ctx->hint_le256 = nmax[1]; ctx->hint_le272 = nmax[2];
    o->serial = gpc_child_register(ctx, o);
    return hipSuccess;
}

hipError_t pc_bucket_offsets(hipStream_t st, const uint32_t* skey, int n, int P, int32_t* off)
{
    hipLaunchKernelGGL(pc_bucket_offsets_kernel, dim3((P + 1 + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, st, skey, n, P, off);
    return hipGetLastError();
}

hipError_t pc_nmax(hipStream_t st, const int32_t* off, int P, int32_t* nmax)
{
    hipLaunchKernelGGL(pc_nmax_kernel, dim3(64), dim3(PC_THREADS), 0, st, off, P, nmax);
    return hipGetLastError();
}

namespace {

struct Scratch {                // per call, in the context's workspace
    PcVoxelTable T;
    int32_t *leaf_start, *nbr, *kcount, *owner, *cnt;
    double *py, *px0, *px1, *M, *cen;
    void* prim;
};

size_t carve_scratch(PcCarver& c, Scratch& s, size_t n, size_t pb, size_t prim_bytes)
{
    s.T.carve(c, n);
    s.owner = c.take<int32_t>(n);
    s.py = c.take<double>(n); s.px0 = c.take<double>(n); s.px1 = c.take<double>(n);
    s.leaf_start = c.take<int32_t>(pb + 1);
    s.nbr = c.take<int32_t>(27 * pb);
    s.kcount = c.take<int32_t>(pb);
    s.cnt = c.take<int32_t>(pb + 4);      // P + 1 counts | n_max | patches of <= 256 points | patches of <= 272 points
    s.M = c.take<double>(16 * pb);
    s.cen = c.take<double>(3 * pb);
    s.prim = c.take<char>(prim_bytes);
    return c.used;
}

}  // namespace

#define PC_HIP(call) PC_HIP_IN("gpc_project_cloud", call)

extern "C" {

// Safe in either order with gpc_ctx_destroy (the batch holds a reference on its context; hipFree synchronises the device).
// the caller holds ctx->mu (or the object was never published): the error paths of the cutters end here
void pc_patches_release(gpc_patches* o)
{
    if (!o) return;
    gpc_ctx* ctx = o->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    if (ctx && ctx->hint_off == o->v.off) ctx->hint_off = nullptr;
    if (ctx) gpc_child_unregister(ctx, o);
    if (o->block) (void)hipFree(o->block);
    delete o;
    if (ctx) gpc_ctx_unref(ctx);
}

void gpc_patches_destroy(gpc_patches* o)
{
    if (!o) return;
    gpc_ctx* ctx = o->ctx;
    if (!ctx) { pc_patches_release(o); return; }
    gpc_ctx_ref(ctx);                                  // the release may drop the last reference while the lock is held
    {
        std::lock_guard<std::mutex> lk(ctx->mu);       // dense_dispatch reads the size-class hint under the same lock
        pc_patches_release(o);
    }
    gpc_ctx_unref(ctx);
}

int gpc_project_cloud_dev(gpc_ctx* ctx, const gpc_point_xyzrgb* cloud, int n, double res, int sz, gpc_patches** out)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!out) return gpc_fail(ctx, GPC_EINVAL, "out is NULL");
    *out = nullptr;
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative point count");
    if (n > 0 && !cloud) return gpc_fail(ctx, GPC_EINVAL, "cloud is NULL");
    if (!(res > 0.0) || !(res < 1e300)) return gpc_fail(ctx, GPC_EINVAL, "res must be positive and finite");
    if (sz < 1 || sz > 1024) return gpc_fail(ctx, GPC_EINVAL, "sz must be in [1, 1024]");
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    hipStream_t st = ctx->stream;
    gpc_patches* o = new gpc_patches;
    o->ctx = ctx;
    gpc_ctx_ref(ctx);
    o->v.m = sz * sz;
    if (n == 0) {
        PC_HIP(hipMalloc(&o->block, 256));
        PC_HIP(hipMemsetAsync(o->block, 0, 256, st));
        PC_HIP(hipStreamSynchronize(st));
        o->v.off = static_cast<int32_t*>(o->block);
        o->serial = gpc_child_register(ctx, o);
        *out = o;
        return GPC_OK;
    }
    const size_t N = (size_t)n;

    // 1: bounds; the grid is anchored at the cloud's minimum corner
    uint32_t hb[8];
    if (int rc = pc_cloud_bounds(ctx, "gpc_project_cloud", cloud, n, hb)) { pc_patches_release(o); return rc; }
    PcGrid g;
    g.res = res;
    g.radius = std::sqrt(3.0f) / 2.0f * res;            // :194
    g.half = res / 2.0f;
    g.sz = sz;
    g.koff[0] = g.koff[1] = g.koff[2] = 0;
    double cells = 1.0;
    for (int a = 0; a < 3; ++a) {
        g.mn[a] = (double)pc_unordered(hb[a]);
        const double ext = std::floor(((double)pc_unordered(hb[3 + a]) - g.mn[a]) / res);
        if (!(ext < 2097152.0)) PC_FAIL(GPC_ERANGE, "more than 2^21 voxels of side res along an axis");
        g.kmax[a] = (int)ext;
        cells *= ext + 1.0;
    }
    g.bx = pc_bits_for(g.kmax[0]); g.by = pc_bits_for(g.kmax[1]); g.bz = pc_bits_for(g.kmax[2]);
    const size_t pb = cells < (double)n ? (size_t)cells : N;   // bound on the number of leaves

    // scratch
    size_t table_bytes = 0, scan2_bytes = 0;
    PC_HIP(pc_voxel_table_prim_bytes(ctx, g, N, &table_bytes));
    PC_HIP(rocprim::exclusive_scan(nullptr, scan2_bytes, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, pb + 1, rocprim::plus<int32_t>(), st));
    const size_t prim_bytes = std::max(table_bytes, scan2_bytes);
    Scratch S;
    {
        PcCarver measure(nullptr);
        if (int rc = gpc_ws_reserve(ctx, carve_scratch(measure, S, N, pb, prim_bytes))) { pc_patches_release(o); return rc; }
        PcCarver c(ctx->ws);
        carve_scratch(c, S, N, pb, prim_bytes);
    }

    // 2, 3: the voxel table, points in sorted order
    int32_t P = 0;
    PC_HIP(pc_voxel_table_build(ctx, g, cloud, n, S.T, S.prim, prim_bytes, &P));
    if ((long long)P * (long long)(sz * sz) > 0x7fffffffLL) PC_FAIL(GPC_ERANGE, "P * sz * sz exceeds 2^31-1");
    if ((size_t)P > pb) PC_FAIL(GPC_EHIP, "internal: %d leaves exceed the bound %zu", (int)P, pb);

    // the result: one block
    const size_t Pz = (size_t)P, m = (size_t)(sz * sz);
    PC_HIP(pc_patches_alloc(o, Pz, N, m));
    PcArgs A;
    memset(&A, 0, sizeof(A));
    A.g = g; A.n = n; A.P = P;
    uint64_t* leaf_key = const_cast<uint64_t*>(o->leaf_key);   // the leaf table outlives the call: it is written into the result
    o->grid = g;
    A.leaf_key = leaf_key; A.leaf_start = S.leaf_start; A.leaf_of = S.T.leaf_of; A.vals = S.T.vals; A.sp = S.T.sp;
    A.nbr = S.nbr; A.M = S.M; A.kcount = S.kcount; A.cen = S.cen; A.owner = S.owner; A.py = S.py; A.px0 = S.px0; A.px1 = S.px1;
    A.cnt = S.cnt; A.nmax = S.cnt + (P + 1);
    A.off = const_cast<int32_t*>(o->v.off); A.R = const_cast<double*>(o->v.rotations); A.mean = const_cast<double*>(o->v.means);
    A.rgb_mean = const_cast<double*>(o->v.rgb_means); A.W = const_cast<uint8_t*>(o->v.W);
    A.x0 = const_cast<double*>(o->v.x0); A.x1 = const_cast<double*>(o->v.x1); A.y = const_cast<double*>(o->v.y);
    A.rgb = const_cast<double*>(o->v.rgb); A.src = const_cast<int32_t*>(o->v.src);
    PC_HIP(hipMemsetAsync(S.cnt, 0, sizeof(int32_t) * (Pz + 4), st));
    PC_HIP(hipMemsetAsync(A.W, 0, Pz * m, st));
    PC_HIP(pc_voxel_table_leaves(ctx, n, S.T, P, leaf_key, S.leaf_start));
    // 4: frames
    const int lblk = (P + PC_WAVES - 1) / PC_WAVES;
    hipLaunchKernelGGL(pc_moment_kernel, dim3(lblk), dim3(PC_THREADS), 0, st, A);
    PC_HIP(hipGetLastError());
    hipLaunchKernelGGL(pc_frame_kernel, dim3((P + PC_FRAME_THREADS - 1) / PC_FRAME_THREADS), dim3(PC_FRAME_THREADS), 0, st, A);
    PC_HIP(hipGetLastError());
    // 5: ownership, offsets
    hipLaunchKernelGGL(pc_claim_kernel, dim3(lblk), dim3(PC_THREADS), 0, st, A);
    PC_HIP(hipGetLastError());
    size_t tb = prim_bytes;
    PC_HIP(rocprim::exclusive_scan(S.prim, tb, S.cnt, A.off, (int32_t)0, Pz + 1, rocprim::plus<int32_t>(), st));
    PC_HIP(pc_nmax(st, A.off, P, A.nmax));
    // 6: the patch batch (the colour planes' pitch is the total, read from off[P] on the device)
    hipLaunchKernelGGL(pc_emit_kernel, dim3(lblk), dim3(PC_THREADS), 0, st, A);
    PC_HIP(hipGetLastError());
    PC_HIP(pc_patches_publish(ctx, o, P, A.nmax));
    *out = o;
    return GPC_OK;
}

int gpc_project_cloud(gpc_ctx* ctx, const gpc_point_xyzrgb* cloud, int n, double res, int sz, gpc_patches** out)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!out) return gpc_fail(ctx, GPC_EINVAL, "out is NULL");
    *out = nullptr;
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative point count");
    if (n > 0 && !cloud) return gpc_fail(ctx, GPC_EINVAL, "cloud is NULL");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_project_cloud");
    const gpc_point_xyzrgb* d_cloud = st.up(cloud, (size_t)n);
    if (st.ok()) st.rc = gpc_project_cloud_dev(ctx, d_cloud, n, res, sz, out);
    return st.finish();
}

int gpc_patches_view_dev(const gpc_patches* p, gpc_patches_view* view)
{
    if (!p || !view) return GPC_EINVAL;
    *view = p->v;
    return GPC_OK;
}

int gpc_patches_fetch(const gpc_patches* p, int32_t* off, double* x0, double* x1, double* y, double* rgb, double* rotations,
                      double* means, double* rgb_means, uint8_t* W, int32_t* src)
{
    gpc_ctx* ctx = sp_live(p);
    if (!ctx) return GPC_EINVAL;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const gpc_patches_view& v = p->v;
    const size_t P = (size_t)v.P, N = (size_t)v.n_total;
    struct { void* dst; const void* src; size_t bytes; } cp[10] = {
        {off, v.off, 4 * (P + 1)}, {x0, v.x0, 8 * N}, {x1, v.x1, 8 * N}, {y, v.y, 8 * N}, {rgb, v.rgb, 24 * N},
        {rotations, v.rotations, 72 * P}, {means, v.means, 24 * P}, {rgb_means, v.rgb_means, 24 * P}, {W, v.W, P * (size_t)v.m},
        {src, v.src, 4 * N}};
    hipStream_t s = gpc_stream_of(ctx);
    for (auto& c : cp)
        if (c.dst && c.bytes) GPC_HIP(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, s));
    GPC_HIP(ctx, hipStreamSynchronize(s));
    return GPC_OK;
}

}  // extern "C"
