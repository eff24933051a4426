// distortion.hip -- what a user of a point-cloud codec reports: the distortion of one cloud against another.  For every point of cloud A
// the EXACT nearest neighbour in cloud B (ties to the lowest index of B), and from it the point-to-point error D1, the point-to-plane
// error D2 along the neighbour's normal and the colour error, as sums in an order no launch shape changes (gpc_cloud_distortion, one
// direction per call); and the plane normal the producer fitted to each leaf, scattered to the points the leaf owns
// (gpc_patches_normals), which is what makes D2 usable on a cloud this library cut.  The rule is in include/gpc.h; tests/distortion_ref.py
// restates it in NumPy with a brute-force scan, and the two agree by bits.
//
// The search runs on the cutters' voxel table (producer_internal.h):
//   1 ds_flag / scan / ds_compact   the valid records of B, stably compacted, with the map back to B's indices
//   2 pc_cloud_bounds, pc_voxel_table_build, pc_voxel_table_leaves over them: a grid of side `cell` anchored at B's minimum corner,
//     B's points sorted by voxel key (z, y, x), one contiguous segment per occupied voxel; ds_sidx: B's index per sorted position
//   3 ds_akeys + radix sort         A's points ordered by THEIR voxel in B's grid (clamped into it), so that the lanes of a wave walk the
//                                   same voxels and read the same segments of the sorted B
//   4 ds_search_kernel              a LANE per A point (DESIGN.md says why not a wave): Chebyshev rings r = 0, 1, .. of voxels around the
//                                   grid voxel nearest to the point; one binary search per (z, y) row of a ring's faces, the two x ends
//                                   of its interior rows; candidates compared by (d2, index of B).  Results scattered to A's order.
//   5 ds_sum0 / ds_sumk / ds_result the fixed-order sums: a wave per chunk of 4096 entries, lane = class i mod 64, ascending i, the
//                                   xor-shuffle tree 32 .. 1; the chunk sums again by the same rule until one is left.  Counts and maxima
//                                   ride in the same records: no atomics of any kind.
// Why the ring search is exact.  When rings 0 .. r are done, every voxel within Chebyshev distance r of the start voxel kc has been
// read.  A point q of B in any other voxel differs from kc by >= r + 1 voxels on some axis a, so |q_a - p_a| >= r cell + og_a, and on
// every other axis b |q_b - p_b| >= og_b, where og is how far p lies outside the grid's box per axis (0 inside):
//     d2(p, q) >= (r cell)^2 + sum og^2.
// The voxel coordinate floor((x - mn) / cell) is rounded, by less than 2^-31 of a voxel (two roundings of a quotient below 2^21 + 1); og
// carries the rounding of its three operations; the computed d2 that of its five.  The stop test therefore uses r - 2^-20 for r, takes
// 2^-50 (|p_a| + |mn_a| + the grid's extent) off every og_a, scales the bound by 1 - 2^-40, and stops only on a STRICT best < bound:
// an unseen point that ties with the best and has a lower index is still found.  The search also ends when the bound exceeds
// max_dist^2 (nothing unseen can count) and when the rings have covered the grid.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "producer_internal.h"   // (switches floating-point contraction off)

#define DS_CHUNK 4096            // entries per chunk of the fixed-order sums: 64 classes x 64 entries

namespace {

// what a chunk hands to the next level: the six sums (d1, d2, r, g, b, luma), the two maxima (d1, d2), the three counts
struct DsPartial {
    double s[6];
    double mx[2];
    long long c[3];
    long long pad;
};

struct DsArgs {
    PcGrid g;
    int na, P;
    double md2;                       // max_dist^2
    const gpc_point_xyzrgb *a, *b;    // the caller's clouds
    const int32_t* order;             // sorted position -> index of A
    const uint64_t* leaf_key;         // P occupied voxels of B's grid, ascending
    const int32_t* leaf_start;        // P + 1: their segments of sp
    const PcPoint* sp;                // B's valid points in voxel order
    const int32_t* sidx;              // ... and their indices in the caller's B
    const float* normals;             // nb x 3 or nullptr
    int32_t* nn;
    double *d2, *e2;                  // (never nullptr here: the caller's buffers or scratch)
};

__device__ static inline bool ds_finite3(float x, float y, float z)
{
    return fabsf(x) <= 3.4028234e38f && fabsf(y) <= 3.4028234e38f && fabsf(z) <= 3.4028234e38f;
}
__device__ static inline double ds_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

}  // namespace

// ---- 1: the valid records of B ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void ds_flag_kernel(const gpc_point_xyzrgb* b, int nb, int32_t* flag)
{
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= nb) return;
    const float4 p = *reinterpret_cast<const float4*>(&b[i]);
    flag[i] = ds_finite3(p.x, p.y, p.z) ? 1 : 0;
}

// scan = inclusive scan of flag: valid record i is record scan[i] - 1 of the compacted cloud (stable: ascending i)
__global__ __launch_bounds__(PC_THREADS) void ds_compact_kernel(const gpc_point_xyzrgb* b, int nb, const int32_t* flag, const int32_t* scan,
                                                                gpc_point_xyzrgb* bc, int32_t* bmap)
{
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= nb || !flag[i]) return;
    const int j = scan[i] - 1;
    const float4* src = reinterpret_cast<const float4*>(&b[i]);
    float4* dst = reinterpret_cast<float4*>(&bc[j]);
    dst[0] = src[0];
    dst[1] = src[1];
    bmap[j] = i;
}

// ---- 2: B's index per sorted position ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void ds_sidx_kernel(const int32_t* bmap, const int32_t* vals, int nbv, int32_t* sidx)
{
    const int s = blockIdx.x * PC_THREADS + threadIdx.x;
    if (s < nbv) sidx[s] = bmap[vals[s]];
}

// ---- 3: A's sort key: its voxel in B's grid, clamped into the grid; the invalid records behind every voxel --------------------------
__global__ __launch_bounds__(PC_THREADS) void ds_akeys_kernel(PcGrid g, const gpc_point_xyzrgb* a, int na, uint64_t* keys, int32_t* vals)
{
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= na) return;
    const float4 p = *reinterpret_cast<const float4*>(&a[i]);
    uint64_t key = 1ull << (g.bx + g.by + g.bz);
    if (ds_finite3(p.x, p.y, p.z)) {
        const float c[3] = {p.x, p.y, p.z};
        int k[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) k[ax] = (int)fmin(fmax(floor(((double)c[ax] - g.mn[ax]) / g.res), 0.0), (double)g.kmax[ax]);
        key = pc_pack(g, k[0], k[1], k[2]);
    }
    keys[i] = key;
    vals[i] = i;
}

// ---- 4: the search -------------------------------------------------------------------------------------------------------------------
namespace {
struct DsBest {
    double d2;
    int idx, s;       // index in the caller's B; sorted position
};
// the sorted positions [s0, s1) against p: the smaller d2 wins, then the lower index of B
__device__ static inline void ds_scan(const DsArgs& A, const double p[3], int s0, int s1, DsBest& best)
{
    for (int s = s0; s < s1; ++s) {
        const float4 q = *reinterpret_cast<const float4*>(&A.sp[s]);
        const double dx = p[0] - (double)q.x, dy = p[1] - (double)q.y, dz = p[2] - (double)q.z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const int idx = A.sidx[s];
        if (d2 < best.d2 || (d2 == best.d2 && idx < best.idx)) {
            best.d2 = d2;
            best.idx = idx;
            best.s = s;
        }
    }
}
// the voxels x0 .. x1 of row (y, z): neighbours in the table, and so are their segments
__device__ static inline void ds_row(const DsArgs& A, const double p[3], int x0, int x1, int y, int z, DsBest& best)
{
    const uint64_t key_lo = pc_pack(A.g, x0, y, z), key_hi = pc_pack(A.g, x1, y, z);
    const int L0 = pc_lower_bound(A.leaf_key, A.P, key_lo);
    int L1 = L0;
    while (L1 < A.P && A.leaf_key[L1] <= key_hi) ++L1;
    if (L1 > L0) ds_scan(A, p, A.leaf_start[L0], A.leaf_start[L1], best);
}
}  // namespace

__global__ __launch_bounds__(PC_THREADS) void ds_search_kernel(DsArgs A)
{
    const int t = blockIdx.x * PC_THREADS + threadIdx.x;
    if (t >= A.na) return;
    const int i = A.order[t];
    const PcGrid& g = A.g;
    const float4 pa = *reinterpret_cast<const float4*>(&A.a[i]);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    DsBest best = {inf, 0x7fffffff, -1};
    const double p[3] = {(double)pa.x, (double)pa.y, (double)pa.z};
    if (ds_finite3(pa.x, pa.y, pa.z)) {
        int kc[3], rmax = 0;
        double og2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double tt = floor((p[a] - g.mn[a]) / g.res), span = (double)(g.kmax[a] + 1) * g.res;
            double og = 0.0;
            if (tt < 0.0) og = g.mn[a] - p[a];
            else if (tt > (double)g.kmax[a]) og = p[a] - (g.mn[a] + span);
            og = fmax(og - 0x1p-50 * (fabs(p[a]) + fabs(g.mn[a]) + span), 0.0);
            og2 += og * og;
            kc[a] = (int)fmin(fmax(tt, 0.0), (double)g.kmax[a]);
            rmax = max(rmax, max(kc[a], g.kmax[a] - kc[a]));
        }
        for (int r = 0; r <= rmax; ++r) {
            const int xlo = kc[0] - r, xhi = kc[0] + r, ylo = kc[1] - r, yhi = kc[1] + r, zlo = kc[2] - r, zhi = kc[2] + r;
            const int xa = max(xlo, 0), xb = min(xhi, g.kmax[0]);
            for (int z = max(zlo, 0); z <= min(zhi, g.kmax[2]); ++z) {
                const bool zface = z == zlo || z == zhi;
                for (int y = max(ylo, 0); y <= min(yhi, g.kmax[1]); ++y) {
                    if (zface || y == ylo || y == yhi) {                 // a row of the ring's faces: all of it
                        ds_row(A, p, xa, xb, y, z, best);
                    } else {                                             // an interior row: its two x ends
                        if (xlo >= 0) ds_row(A, p, xlo, xlo, y, z, best);
                        if (xhi <= g.kmax[0]) ds_row(A, p, xhi, xhi, y, z, best);
                    }
                }
            }
            const double rr = fmax((double)r - 0x1p-20, 0.0) * g.res;
            const double bound = (rr * rr + og2) * (1.0 - 0x1p-40);
            if (best.d2 < bound || bound > A.md2) break;
        }
    }
    const bool matched = best.s >= 0 && best.d2 <= A.md2;
    double e2 = ds_nan();
    if (matched && A.normals) {
        const float* nf = A.normals + (size_t)best.idx * 3;
        const float n0 = nf[0], n1 = nf[1], n2 = nf[2];
        if (ds_finite3(n0, n1, n2)) {
            const float4 q = *reinterpret_cast<const float4*>(&A.sp[best.s]);
            const double dx = p[0] - (double)q.x, dy = p[1] - (double)q.y, dz = p[2] - (double)q.z;
            const double e = (dx * (double)n0 + dy * (double)n1) + dz * (double)n2;
            e2 = e * e;
        }
    }
    A.nn[i] = matched ? best.idx : -1;
    A.d2[i] = matched ? best.d2 : ds_nan();
    A.e2[i] = e2;
}

// B holds no valid record: nothing matches
__global__ __launch_bounds__(PC_THREADS) void ds_unmatched_kernel(int na, int32_t* nn, double* d2, double* e2)
{
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= na) return;
    nn[i] = -1;
    d2[i] = ds_nan();
    e2[i] = ds_nan();
}

// ---- 5: the sums ---------------------------------------------------------------------------------------------------------------------
namespace {
// the 64 class values of a chunk -> one, in every lane: the xor-shuffle tree 32, 16, .. 1
__device__ static inline void ds_tree(DsPartial& v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) v.s[k] = v.s[k] + __shfl_xor(v.s[k], d, 64);
#pragma unroll
        for (int k = 0; k < 2; ++k) v.mx[k] = fmax(v.mx[k], __shfl_xor(v.mx[k], d, 64));
#pragma unroll
        for (int k = 0; k < 3; ++k) v.c[k] = v.c[k] + __shfl_xor(v.c[k], d, 64);
    }
}
__device__ static inline void ds_clear(DsPartial& v)
{
#pragma unroll
    for (int k = 0; k < 6; ++k) v.s[k] = 0.0;
    v.mx[0] = v.mx[1] = 0.0;
    v.c[0] = v.c[1] = v.c[2] = 0;
    v.pad = 0;
}
}  // namespace

// level 0: a wave per chunk of 4096 A points; lane = class i mod 64, ascending i inside the class
__global__ __launch_bounds__(PC_THREADS) void ds_sum0_kernel(DsArgs A, int chunks, DsPartial* out)
{
    const int c = blockIdx.x * PC_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= chunks) return;
    DsPartial v;
    ds_clear(v);
    const long long base = (long long)c * DS_CHUNK;
    for (int j = 0; j < DS_CHUNK / 64; ++j) {
        const long long i = base + 64 * j + lane;
        if (i >= A.na) break;
        const gpc_point_xyzrgb* qa = &A.a[i];
        const float4 pa = *reinterpret_cast<const float4*>(qa);
        if (!ds_finite3(pa.x, pa.y, pa.z)) continue;
        v.c[0] += 1;
        const int nn = A.nn[i];
        if (nn < 0) continue;
        v.c[1] += 1;
        const double d2 = A.d2[i], e2 = A.e2[i];
        v.s[0] = v.s[0] + d2;
        v.mx[0] = fmax(v.mx[0], d2);
        if (e2 == e2) {
            v.c[2] += 1;
            v.s[1] = v.s[1] + e2;
            v.mx[1] = fmax(v.mx[1], e2);
        }
        const uint32_t ca = pc_rgb_of(qa), cb = pc_rgb_of(&A.b[nn]);      // r | g << 8 | b << 16
        const int dr = (int)(ca & 0xffu) - (int)(cb & 0xffu), dg = (int)((ca >> 8) & 0xffu) - (int)((cb >> 8) & 0xffu),
                  db = (int)((ca >> 16) & 0xffu) - (int)((cb >> 16) & 0xffu);
        v.s[2] = v.s[2] + (double)dr * (double)dr;
        v.s[3] = v.s[3] + (double)dg * (double)dg;
        v.s[4] = v.s[4] + (double)db * (double)db;
        const double lu = (0.2126 * (double)dr + 0.7152 * (double)dg) + 0.0722 * (double)db;
        v.s[5] = v.s[5] + lu * lu;
    }
    ds_tree(v);
    if (lane == 0) out[c] = v;
}

// level k: the same rule over the n records of the level below
__global__ __launch_bounds__(PC_THREADS) void ds_sumk_kernel(const DsPartial* in, int n, int chunks, DsPartial* out)
{
    const int c = blockIdx.x * PC_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= chunks) return;
    DsPartial v;
    ds_clear(v);
    const long long base = (long long)c * DS_CHUNK;
    for (int j = 0; j < DS_CHUNK / 64; ++j) {
        const long long i = base + 64 * j + lane;
        if (i >= n) break;
        const DsPartial w = in[i];
#pragma unroll
        for (int k = 0; k < 6; ++k) v.s[k] = v.s[k] + w.s[k];
#pragma unroll
        for (int k = 0; k < 2; ++k) v.mx[k] = fmax(v.mx[k], w.mx[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) v.c[k] = v.c[k] + w.c[k];
    }
    ds_tree(v);
    if (lane == 0) out[c] = v;
}

__global__ void ds_result_kernel(const DsPartial* top, gpc_distortion_result* res)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const DsPartial v = *top;
    gpc_distortion_result r;
    r.n_valid = v.c[0]; r.n_matched = v.c[1]; r.n_plane = v.c[2];
    r.sse_d1 = v.s[0]; r.max_d1 = v.mx[0];
    r.sse_d2 = v.s[1]; r.max_d2 = v.mx[1];
    r.sse_rgb[0] = v.s[2]; r.sse_rgb[1] = v.s[3]; r.sse_rgb[2] = v.s[4];
    r.sse_luma = v.s[5];
    *res = r;
}

// ---- gpc_patches_normals --------------------------------------------------------------------------------------------------------------
// flag[0] |= 1 where the batch names a point beyond n
__global__ __launch_bounds__(PC_THREADS) void ds_src_check_kernel(const int32_t* src, int n_total, int n, int32_t* flag)
{
    const int j = blockIdx.x * PC_THREADS + threadIdx.x;
    if (j >= n_total) return;
    const int i = src[j];
    if (i < 0 || i >= n) atomicOr(flag, 1);
}
__global__ __launch_bounds__(PC_THREADS) void ds_nan_fill_kernel(float* v, size_t count)
{
    const size_t i = (size_t)blockIdx.x * PC_THREADS + threadIdx.x;
    if (i < count) v[i] = __int_as_float(0x7fc00000);
}
// batch position j of leaf L (off[L] <= j < off[L + 1]) holds cloud point src[j]: it gets column 0 of R_L
__global__ __launch_bounds__(PC_THREADS) void ds_normals_kernel(const int32_t* off, const int32_t* src, const double* R, int P, int n_total, int n,
                                                                float* normals)
{
    const int j = blockIdx.x * PC_THREADS + threadIdx.x;
    if (j >= n_total) return;
    const int i = src[j];
    if (i < 0 || i >= n) return;
    int lo = 0, hi = P;                                       // the last L with off[L] <= j
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= j) lo = mid; else hi = mid;
    }
    const double* r = R + (size_t)lo * 9;
    float* o = normals + (size_t)i * 3;
    o[0] = (float)r[0]; o[1] = (float)r[1]; o[2] = (float)r[2];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
namespace {

struct DsScratch {                    // per call, in the context's workspace (its first 4096 bytes belong to pc_cloud_bounds)
    int32_t *flag, *scan, *bmap;      // nb
    gpc_point_xyzrgb* bc;             // nb: the valid records of B
    PcVoxelTable T;                   // nb
    uint64_t* leaf_key;               // nb
    int32_t *leaf_start, *sidx;       // nb + 1, nb
    uint64_t *ak0, *ak1;              // na: A's keys, sorted
    int32_t *av0, *av1;               // na: A's indices, in sorted order
    int32_t* nn;                      // na each, carved only where the caller passes nullptr
    double *d2, *e2;
    DsPartial* part;                  // every level of the sums
    void* prim;
};

size_t ds_levels(size_t n)            // records of every level of the sums over n entries
{
    size_t total = 0;
    do {
        n = (n + DS_CHUNK - 1) / DS_CHUNK;
        total += n;
    } while (n > 1);
    return total;
}

size_t ds_carve(PcCarver& c, DsScratch& s, size_t na, size_t nb, bool own_nn, bool own_d2, bool own_e2, size_t prim_bytes)
{
    (void)c.take<char>(4096);
    s.flag = c.take<int32_t>(nb); s.scan = c.take<int32_t>(nb); s.bmap = c.take<int32_t>(nb);
    s.bc = c.take<gpc_point_xyzrgb>(nb);
    s.T.carve(c, nb);
    s.leaf_key = c.take<uint64_t>(nb);
    s.leaf_start = c.take<int32_t>(nb + 1);
    s.sidx = c.take<int32_t>(nb);
    s.ak0 = c.take<uint64_t>(na); s.ak1 = c.take<uint64_t>(na);
    s.av0 = c.take<int32_t>(na); s.av1 = c.take<int32_t>(na);
    s.nn = own_nn ? c.take<int32_t>(na) : nullptr;
    s.d2 = own_d2 ? c.take<double>(na) : nullptr;
    s.e2 = own_e2 ? c.take<double>(na) : nullptr;
    s.part = c.take<DsPartial>(ds_levels(na));
    s.prim = c.take<char>(prim_bytes);                    // (last: a larger one moves nothing else)
    return c.used;
}

inline unsigned ds_blocks(size_t n) { return (unsigned)((n + PC_THREADS - 1) / PC_THREADS); }

// the library's cell: about four points of B per occupied voxel of a SURFACE that fills the two largest extents of B's box (a cloud that
// fills its volume gets emptier voxels and a few rings more), and never so small that an axis would need more than 2^20 voxels
double ds_auto_cell(const double ext[3], int nbv)
{
    double e[3] = {ext[0], ext[1], ext[2]};
    std::sort(e, e + 3);
    double cell = std::sqrt(4.0 * e[2] * e[1] / (double)nbv);
    if (!(cell > 0.0)) cell = e[2] > 0.0 ? 4.0 * e[2] / (double)nbv : 1.0;
    return std::max(cell, e[2] / 1048576.0);
}

}  // namespace

#define DS_HIP(call)                                                                                                               \
    do {                                                                                                                           \
        hipError_t e_ = (call);                                                                                                    \
        if (e_ != hipSuccess)                                                                                                      \
            return gpc_fail(ctx, e_ == hipErrorOutOfMemory ? GPC_ENOMEM : GPC_EHIP, "gpc_cloud_distortion: %s failed: %s", #call, \
                            hipGetErrorString(e_));                                                                                \
    } while (0)

extern "C" {

void gpc_default_params_distortion(gpc_distortion_params* p)
{
    if (!p) return;
    p->cell = 0.0;
    p->max_dist = INFINITY;
}

int gpc_cloud_distortion_dev(gpc_ctx* ctx, const gpc_point_xyzrgb* a, int na, const gpc_point_xyzrgb* b, int nb, const float* normals_b,
                             const gpc_distortion_params* params, int32_t* nn, double* d2, double* e2, gpc_distortion_result* result)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (na < 0 || nb < 0) return gpc_fail(ctx, GPC_EINVAL, "negative point count");
    if ((na > 0 && !a) || (nb > 0 && !b)) return gpc_fail(ctx, GPC_EINVAL, "a cloud is NULL");
    if (!result) return gpc_fail(ctx, GPC_EINVAL, "result is NULL");
    gpc_distortion_params prm;
    gpc_default_params_distortion(&prm);
    if (params) prm = *params;
    if (!(prm.cell >= 0.0) || !std::isfinite(prm.cell)) return gpc_fail(ctx, GPC_EINVAL, "cell must be finite and >= 0");
    if (!(prm.max_dist >= 0.0)) return gpc_fail(ctx, GPC_EINVAL, "max_dist must be >= 0");
    std::lock_guard<std::mutex> lk(ctx->mu);
    DS_HIP(hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    hipStream_t st = ctx->stream;
    if (na == 0) {
        DS_HIP(hipMemsetAsync(result, 0, sizeof(*result), st));
        return GPC_OK;
    }
    const size_t NA = (size_t)na, NB = (size_t)nb;

    // scratch.  The sort's temporary storage depends on the key bits, which depend on B's box: measured for the widest key first, and
    // once more when the box is known
    size_t asort_bytes = 0, scan_bytes = 0, table_bytes = 0;
    DS_HIP(rocprim::radix_sort_pairs(nullptr, asort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, NA, 0u,
                                     64u, st));
    PcGrid g;
    memset(&g, 0, sizeof(g));
    if (nb > 0) {
        DS_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, (int32_t*)nullptr, (int32_t*)nullptr, NB, rocprim::plus<int32_t>(), st));
        g.bx = g.by = g.bz = 21;
        DS_HIP(pc_voxel_table_prim_bytes(ctx, g, NB, &table_bytes));
    }
    size_t prim_bytes = std::max(asort_bytes, std::max(scan_bytes, table_bytes));
    DsScratch S;
    auto carve = [&]() -> int {
        PcCarver measure(nullptr);
        if (int rc = gpc_ws_reserve(ctx, ds_carve(measure, S, NA, NB, !nn, !d2, !e2, prim_bytes))) return rc;
        PcCarver c(ctx->ws);
        ds_carve(c, S, NA, NB, !nn, !d2, !e2, prim_bytes);
        return GPC_OK;
    };
    if (int rc = carve()) return rc;

    // 1: the valid records of B
    int32_t nbv = 0;
    auto compact = [&]() -> int {
        hipLaunchKernelGGL(ds_flag_kernel, dim3(ds_blocks(NB)), dim3(PC_THREADS), 0, st, b, nb, S.flag);
        DS_HIP(hipGetLastError());
        size_t tb = prim_bytes;
        DS_HIP(rocprim::inclusive_scan(S.prim, tb, S.flag, S.scan, NB, rocprim::plus<int32_t>(), st));
        hipLaunchKernelGGL(ds_compact_kernel, dim3(ds_blocks(NB)), dim3(PC_THREADS), 0, st, b, nb, S.flag, S.scan, S.bc, S.bmap);
        DS_HIP(hipGetLastError());
        DS_HIP(hipMemcpyAsync(&nbv, S.scan + (nb - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
        DS_HIP(hipStreamSynchronize(st));
        return GPC_OK;
    };
    if (nb > 0)
        if (int rc = compact()) return rc;

    DsArgs A;
    memset(&A, 0, sizeof(A));
    A.na = na;
    A.md2 = prm.max_dist * prm.max_dist;
    A.a = a; A.b = b; A.normals = normals_b;
    A.nn = nn ? nn : S.nn; A.d2 = d2 ? d2 : S.d2; A.e2 = e2 ? e2 : S.e2;

    if (nbv > 0) {
        // 2: the table over them, anchored at their minimum corner
        uint32_t hb[8];
        if (int rc = pc_cloud_bounds(ctx, "gpc_cloud_distortion", S.bc, nbv, hb)) return rc;
        double ext[3];
        for (int ax = 0; ax < 3; ++ax) {
            g.mn[ax] = (double)pc_unordered(hb[ax]);
            ext[ax] = (double)pc_unordered(hb[3 + ax]) - g.mn[ax];
        }
        int32_t P = 0;
        unsigned bits = 0;
        auto table = [&](double cell) -> int {               // B's points sorted by their voxel of side `cell`; P = occupied voxels
            g.res = cell;
            for (int ax = 0; ax < 3; ++ax) {
                const double k = std::floor(ext[ax] / g.res);
                if (!(k < 2097152.0)) return gpc_fail(ctx, GPC_ERANGE, "cell %g: more than 2^21 voxels along an axis of B's box", g.res);
                g.kmax[ax] = (int)k;
            }
            g.bx = pc_bits_for(g.kmax[0]); g.by = pc_bits_for(g.kmax[1]); g.bz = pc_bits_for(g.kmax[2]);
            bits = (unsigned)(g.bx + g.by + g.bz);
            DS_HIP(pc_voxel_table_prim_bytes(ctx, g, (size_t)nbv, &table_bytes));
            DS_HIP(rocprim::radix_sort_pairs(nullptr, asort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                                             NA, 0u, bits + 1u, st));
            if (std::max(asort_bytes, table_bytes) > prim_bytes) {
                prim_bytes = std::max(asort_bytes, table_bytes);
                const void* before = ctx->ws;
                if (int rc = carve()) return rc;
                if (ctx->ws != before)                       // the workspace moved: the compacted cloud went with the old one
                    if (int rc = compact()) return rc;
                A.nn = nn ? nn : S.nn; A.d2 = d2 ? d2 : S.d2; A.e2 = e2 ? e2 : S.e2;
            }
            DS_HIP(pc_voxel_table_build(ctx, g, S.bc, nbv, S.T, S.prim, prim_bytes, &P));
            if (P < 1 || P > nbv) return gpc_fail(ctx, GPC_EHIP, "gpc_cloud_distortion: internal: %d voxels of %d points", (int)P, (int)nbv);
            return GPC_OK;
        };
        if (prm.cell > 0.0) {
            if (int rc = table(prm.cell)) return rc;
        } else {
            // the library's choice: four points per voxel if B were a surface filling its box; a patchy or folded one crowds the voxels it
            // does occupy, and the table is then built once more, at the cell that the count of occupied voxels asks for
            const double c0 = ds_auto_cell(ext, nbv);
            if (int rc = table(c0)) return rc;
            const double crowd = (double)nbv / (double)P;
            if (crowd > 8.0)
                if (int rc = table(std::max(c0 * std::sqrt(4.0 / crowd), std::max(ext[0], std::max(ext[1], ext[2])) / 1048576.0))) return rc;
        }
        DS_HIP(pc_voxel_table_leaves(ctx, nbv, S.T, P, S.leaf_key, S.leaf_start));
        hipLaunchKernelGGL(ds_sidx_kernel, dim3(ds_blocks((size_t)nbv)), dim3(PC_THREADS), 0, st, S.bmap, S.T.vals, nbv, S.sidx);
        DS_HIP(hipGetLastError());
        // 3: A in the order of its voxels
        hipLaunchKernelGGL(ds_akeys_kernel, dim3(ds_blocks(NA)), dim3(PC_THREADS), 0, st, g, a, na, S.ak0, S.av0);
        DS_HIP(hipGetLastError());
        size_t tb = prim_bytes;
        DS_HIP(rocprim::radix_sort_pairs(S.prim, tb, S.ak0, S.ak1, S.av0, S.av1, NA, 0u, bits + 1u, st));
        // 4: the search
        A.g = g; A.P = P;
        A.order = S.av1; A.leaf_key = S.leaf_key; A.leaf_start = S.leaf_start; A.sp = S.T.sp; A.sidx = S.sidx;
        hipLaunchKernelGGL(ds_search_kernel, dim3(ds_blocks(NA)), dim3(PC_THREADS), 0, st, A);
        DS_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(ds_unmatched_kernel, dim3(ds_blocks(NA)), dim3(PC_THREADS), 0, st, na, A.nn, A.d2, A.e2);
        DS_HIP(hipGetLastError());
    }

    // 5: the sums, level by level
    DsPartial* level = S.part;
    int n = (int)((NA + DS_CHUNK - 1) / DS_CHUNK);
    hipLaunchKernelGGL(ds_sum0_kernel, dim3((unsigned)((n + PC_WAVES - 1) / PC_WAVES)), dim3(PC_THREADS), 0, st, A, n, level);
    DS_HIP(hipGetLastError());
    while (n > 1) {
        const int up = (n + DS_CHUNK - 1) / DS_CHUNK;
        hipLaunchKernelGGL(ds_sumk_kernel, dim3((unsigned)((up + PC_WAVES - 1) / PC_WAVES)), dim3(PC_THREADS), 0, st, level, n, up, level + n);
        DS_HIP(hipGetLastError());
        level += n;
        n = up;
    }
    hipLaunchKernelGGL(ds_result_kernel, dim3(1), dim3(64), 0, st, level, result);
    DS_HIP(hipGetLastError());
    return GPC_OK;
}

int gpc_cloud_distortion(gpc_ctx* ctx, const gpc_point_xyzrgb* a, int na, const gpc_point_xyzrgb* b, int nb, const float* normals_b,
                         const gpc_distortion_params* params, int32_t* nn, double* d2, double* e2, gpc_distortion_result* result)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (na < 0 || nb < 0) return gpc_fail(ctx, GPC_EINVAL, "negative point count");
    if ((na > 0 && !a) || (nb > 0 && !b)) return gpc_fail(ctx, GPC_EINVAL, "a cloud is NULL");
    if (!result) return gpc_fail(ctx, GPC_EINVAL, "result is NULL");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_cloud_distortion");
    const size_t NA = (size_t)na, NB = (size_t)nb;
    const gpc_point_xyzrgb* d_a = st.up(a, NA);
    const gpc_point_xyzrgb* d_b = st.up(b, NB);
    const float* d_nb = normals_b ? st.up(normals_b, 3 * NB) : nullptr;
    int32_t* d_nn = nn ? st.out<int32_t>(NA) : nullptr;
    double* d_d2 = d2 ? st.out<double>(NA) : nullptr;
    double* d_e2 = e2 ? st.out<double>(NA) : nullptr;
    gpc_distortion_result* d_res = st.out<gpc_distortion_result>(1);
    if (st.ok()) st.rc = gpc_cloud_distortion_dev(ctx, d_a, na, d_b, nb, d_nb, params, d_nn, d_d2, d_e2, d_res);
    st.down(nn, d_nn, NA);
    st.down(d2, d_d2, NA);
    st.down(e2, d_e2, NA);
    st.down(result, d_res, 1);
    return st.finish();
}

int gpc_patches_normals_dev(const gpc_patches* p, int n, float* normals)
{
    if (!p) return GPC_EINVAL;
    gpc_ctx* ctx = p->ctx;
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative point count");
    if (n > 0 && !normals) return gpc_fail(ctx, GPC_EINVAL, "normals is NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!gpc_child_listed(ctx, p)) return gpc_fail(ctx, GPC_EINVAL, "the batch is not a live object of its context");
    const int n_total = p->v.n_total, P = p->v.P;
    if (n_total > n) return gpc_fail(ctx, GPC_EINVAL, "the batch holds %d points, the cloud %d: it was cut from another cloud", n_total, n);
    if (n == 0) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    if (n_total > 0) {                                        // a src entry >= n is found out before anything is written
        if (int rc = gpc_ws_reserve(ctx, 256)) return rc;
        int32_t* flag = static_cast<int32_t*>(ctx->ws);
        int32_t bad = 0;
        GPC_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL(ds_src_check_kernel, dim3(ds_blocks((size_t)n_total)), dim3(PC_THREADS), 0, st, p->v.src, n_total, n, flag);
        GPC_HIP(ctx, hipGetLastError());
        GPC_HIP(ctx, hipMemcpyAsync(&bad, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        GPC_HIP(ctx, hipStreamSynchronize(st));
        if (bad) return gpc_fail(ctx, GPC_EINVAL, "the batch names a point beyond the cloud's %d: it was cut from another cloud", n);
    }
    hipLaunchKernelGGL(ds_nan_fill_kernel, dim3(ds_blocks(3 * (size_t)n)), dim3(PC_THREADS), 0, st, normals, 3 * (size_t)n);
    GPC_HIP(ctx, hipGetLastError());
    if (n_total > 0) {
        hipLaunchKernelGGL(ds_normals_kernel, dim3(ds_blocks((size_t)n_total)), dim3(PC_THREADS), 0, st, p->v.off, p->v.src, p->v.rotations, P,
                           n_total, n, normals);
        GPC_HIP(ctx, hipGetLastError());
    }
    return GPC_OK;
}

int gpc_patches_normals(const gpc_patches* p, int n, float* normals)
{
    if (!p) return GPC_EINVAL;
    gpc_ctx* ctx = p->ctx;
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative point count");
    if (n > 0 && !normals) return gpc_fail(ctx, GPC_EINVAL, "normals is NULL");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_patches_normals");
    float* d_n = st.out<float>(3 * (size_t)n);
    if (st.ok()) st.rc = gpc_patches_normals_dev(p, n, d_n);
    st.down(normals, d_n, 3 * (size_t)n);
    return st.finish();
}

}  // extern "C"
