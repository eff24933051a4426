// mapping.hip -- gp_mapping::insert_into_map (/root/reference/src/gp_mapping.cpp:37-152) on the GPU: a registered scan is cut against
// the leaf table of an existing model and a NEW gpc_patches comes out -- every old leaf, plus the voxels the scan opened -- whose batch
// holds the scan's points per leaf: what S[i] holds when train_processes (:293-343) runs.  The model is left untouched; the GP states
// follow through gpc_sparse_remap (sparse_api.hip).
//
// The reference walks old and new leaves in one interleaved order and lets each claim the points of its search sphere that nobody
// claimed before (occupied_indices).  As in producer.hip and registration.hip that walk is a per-point minimum: a point belongs to the
// FIRST leaf in (merged) leaf order that accepts it, out of the <= 27 leaves around its voxel.  Three kinds of leaf:
//   kept   an old leaf whose depth GP is not empty (:115): keeps R_i, mean_i, rgb_mean_i (transform_to_old, :213-243); window around the
//          stored mean (:227-228); depth as is, colours minus the stored colour mean (:237); W = old mask | cells hit now (:242)
//   fresh  a new leaf, or an old leaf with an empty depth GP, whose sphere holds >= min_nbr scan points (:121-137): the producer's
//          treatment on the scan's points -- frame of the sphere's moment matrix in the producer's hit order, origin at the voxel centre
//          (:266-267), depth-mean shift and colour mean over what it owns (transform_to_new, :245-291), W = cells hit now (:290)
//   idle   an old leaf with an empty depth GP and fewer than min_nbr scan points around it: old frame, old mask, no points
// A voxel that is new to the model becomes a leaf only if it is fresh (:126).  Leaf id = position in the merged sorted key table (the
// reference appends, :88-95); old_to_new is that monotone renumbering.
// Deviations from upstream: its to_be_added of a leaf below the threshold piles up across scans and is then paired with a mis-indexed
// last_inds (:261); here the threshold looks at the current scan only, which is the reference's behaviour for a leaf's first scan.
// train_classification (the ray-cast free mask, :154-211), which upstream runs between this and train_processes, is raycast.hip.
//
// The grid keeps the model's anchor mn and resolution; its whole-voxel origin shift koff and its extent kmax grow to cover the scan
// (producer_internal.h), so no old voxel centre moves.  Pipeline (integer / gather work, one stream, three reads of a few bytes):
//   1 pc_cloud_bounds       the scan's corners -> koff, kmax, key widths;  mp_rekey_kernel: the model's keys in the grown grid
//   2 pc_voxel_table_build, pc_voxel_table_leaves (the producer's stages, producer_internal.h): the scan's own voxel table, points in
//                           sorted order
//   3 mp_moment_kernel      one wave per scan voxel and per untrained old leaf: sphere count and moment matrix over the SCAN's points,
//                           in the producer's hit order (pc_sphere_moments)
//   4 mp_flag_kernel + scan which scan voxels become leaves;  mp_merge_kernel: merge of the two sorted key lists by rank (binary search)
//   5 mp_frame_kernel       a thread per merged leaf: class, frame (copied or pc_frame_of_moments), window origin
//   6 mp_claim_kernel       a thread per scan point: pc_first_accepting_leaf, the walk of the registration assignment, over the
//                           merged table, idle leaves skipped, window around the leaf's origin
//   7 bucket                stable radix sort of (owner, scan index): patch order, ascending scan index inside a patch; offsets by
//                           binary search in the sorted owners (pc_bucket_offsets; no atomics)
//   8 mp_means_kernel       one wave per leaf: depth sum in patch order (a serial chain, like the producer's), colour sums, the leaf's
//                           mean / rgb_mean, the mask it starts from;  mp_emit_kernel: a thread per owned point: the batch rows, W;
//                           pc_nmax and pc_patches_publish: the size classes, the view, the new object
// No floating-point atomics, no order left to the scheduler: the same inputs give the same bits.  Contraction is off (producer_internal.h)
// and every expression shared with the producer or the registration assignment is written in their association.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "producer_internal.h"   // (switches floating-point contraction off)
#include "sparse_internal.h"

enum { MP_IDLE = 0, MP_KEPT = 1, MP_FRESH = 2 };

struct MpArgs {
    PcGrid g0, g;                 // the model's grid, the result's
    int n, P0, U, P, min_nbr;     // scan points, old leaves, scan voxels, merged leaves
    const gpc_point_xyzrgb* cloud;
    const uint64_t* key0;         // model: leaf keys (in g0), basis sizes of the depth GPs (nullptr: every leaf trained), frames, masks
    const int32_t* bv;
    const double *R0, *mean0, *rgbm0;
    const uint8_t* W0;
    uint64_t* okey;               // P0: the model's keys in g
    const uint64_t* ukey;         // U: the scan's voxels;  ustart U + 1: their segments of sp
    const int32_t* ustart;
    const PcPoint* sp;
    double *Mu, *Mo;              // U x 16, P0 x 16 moment matrices
    int32_t *ku, *ko;             // U, P0 sphere counts
    int32_t *add, *arank;         // U + 1: scan voxel becomes a leaf; exclusive scan
    int32_t* o2n;                 // P0
    int32_t* from;                // P: old leaf id, or -1 - scan voxel
    uint64_t* mkey;               // P merged keys (in the result)
    int32_t* cls;                 // P
    double* org;                  // P x 3 window origin: stored mean (kept), voxel centre (fresh)
    double* shift;                // P: depth mean of a fresh leaf
    double* local;                // n x 3
    uint32_t *bkey, *skey;        // n: owner (P = nobody); sorted
    int32_t *bval, *sval;         // n: scan index; in bucket order
    int32_t* nmax;
    int32_t* off;                 // result
    double *R, *mean, *rgb_mean;
    uint8_t* W;
    double *x0, *x1, *y, *rgb;
    int32_t* src;
};

// ---- 1: the model's keys in the grown grid (a monotone map: the table stays sorted) ----------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void mp_rekey_kernel(MpArgs A)
{
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= A.P0) return;
    int k[3];
    pc_unpack(A.g0, A.key0[i], k);
    A.okey[i] = pc_pack(A.g, k[0] + (A.g.koff[0] - A.g0.koff[0]), k[1] + (A.g.koff[1] - A.g0.koff[1]), k[2] + (A.g.koff[2] - A.g0.koff[2]));
}

// ---- 3: sphere counts and moments over the scan's points -------------------------------------------------------------------------
// one wave per query voxel qkey[q]; skip_bv != nullptr: a query whose depth GP is not empty needs neither (kept leaf)
__global__ __launch_bounds__(PC_THREADS) void mp_moment_kernel(MpArgs A, const uint64_t* qkey, int nq, const int32_t* skip_bv, double* Mout,
                                                               int32_t* kout)
{
    __shared__ double prod[PC_WAVES][10 * PC_LROW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = blockIdx.x * PC_WAVES + w;
    if (q >= nq) return;                                      // whole waves leave; no block-level synchronisation below
    if (skip_bv && skip_bv[q] > 0) {
        if (lane == 0) kout[q] = 0;
        return;
    }
    const PcGrid& g = A.g;
    int k3[3];
    pc_unpack(g, qkey[q], k3);
    double center[3];
    pc_center(g, k3, center);
    int seg0 = 0, seg1 = 0;
    if (lane < 27) {
        const int nx = k3[0] + lane % 3 - 1, ny = k3[1] + (lane / 3) % 3 - 1, nz = k3[2] + lane / 9 - 1;
        int nb = -1;
        if (nx >= 0 && nx <= g.kmax[0] && ny >= 0 && ny <= g.kmax[1] && nz >= 0 && nz <= g.kmax[2])
            nb = pc_find_leaf(A.ukey, A.U, pc_pack(g, nx, ny, nz));
        if (nb >= 0) { seg0 = A.ustart[nb]; seg1 = A.ustart[nb + 1]; }
    }
    double M;
    int k;
    pc_sphere_moments(g, center, seg0, seg1, A.sp, prod[w], lane, M, k);
    if (lane < 16) Mout[(size_t)q * 16 + lane] = M;
    if (lane == 0) kout[q] = k;
}

// ---- 4: which scan voxels become leaves; the merge ---------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void mp_flag_kernel(MpArgs A)
{
    const int u = blockIdx.x * PC_THREADS + threadIdx.x;
    if (u > A.U) return;
    int f = 0;
    if (u < A.U) f = pc_find_leaf(A.okey, A.P0, A.ukey[u]) < 0 && A.ku[u] >= A.min_nbr;       // new to the model, :126
    A.add[u] = f;
}

// position in the merged table = own rank + the number of smaller keys of the other list
__global__ __launch_bounds__(PC_THREADS) void mp_merge_kernel(MpArgs A)
{
    const int t = blockIdx.x * PC_THREADS + threadIdx.x;
    if (t < A.P0) {
        const uint64_t key = A.okey[t];
        const int pos = t + A.arank[pc_lower_bound(A.ukey, A.U, key)];
        A.mkey[pos] = key;
        A.from[pos] = t;
        A.o2n[t] = pos;
    } else if (t < A.P0 + A.U) {
        const int u = t - A.P0;
        if (!A.add[u]) return;
        const uint64_t key = A.ukey[u];
        const int pos = A.arank[u] + pc_lower_bound(A.okey, A.P0, key);
        A.mkey[pos] = key;
        A.from[pos] = -1 - u;
    }
}

// ---- 5: class, frame, window origin ----------------------------------------------------------------------------------------------
#define MP_FRAME_THREADS 64

__global__ __launch_bounds__(MP_FRAME_THREADS) void mp_frame_kernel(MpArgs A)
{
    const int L = blockIdx.x * MP_FRAME_THREADS + threadIdx.x;
    if (L >= A.P) return;
    const int f = A.from[L];
    int cls;
    const double* M;
    int k;
    if (f >= 0) {
        const bool trained = !A.bv || A.bv[f] > 0;            // gps[..].size() > 0 (:115)
        k = A.ko[f];
        M = A.Mo + (size_t)f * 16;
        cls = trained ? MP_KEPT : (k >= A.min_nbr ? MP_FRESH : MP_IDLE);
    } else {
        k = A.ku[-1 - f];
        M = A.Mu + (size_t)(-1 - f) * 16;
        cls = MP_FRESH;
    }
    double R[9], org[3];
    if (cls == MP_FRESH) {
        pc_frame_of_moments(M, k, R);
        int k3[3];
        pc_unpack(A.g, A.mkey[L], k3);
        pc_center(A.g, k3, org);                              // :266-267
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = A.R0[(size_t)f * 9 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) org[i] = A.mean0[(size_t)f * 3 + i];      // :227-228
    }
    A.cls[L] = cls;
#pragma unroll
    for (int i = 0; i < 9; ++i) A.R[(size_t)L * 9 + i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) A.org[(size_t)L * 3 + i] = org[i];
}

// ---- 6: ownership ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void mp_claim_kernel(MpArgs A)
{
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= A.n) return;
    const float4 f = *reinterpret_cast<const float4*>(&A.cloud[i]);
    const double p[3] = {(double)f.x, (double)f.y, (double)f.z};
    int k[3];
    pc_voxel(A.g, f.x, f.y, f.z, k);                          // inside the grid: it was grown over the scan
    double q[3] = {0.0, 0.0, 0.0};
    const int32_t* cls = A.cls;
    const int owner = pc_first_accepting_leaf(A.g, A.mkey, A.P, p, k, A.R, A.org, [cls](int L) { return cls[L] == MP_IDLE; }, q);
    A.local[(size_t)i * 3] = q[0];
    A.local[(size_t)i * 3 + 1] = q[1];
    A.local[(size_t)i * 3 + 2] = q[2];
    A.bkey[i] = owner < 0 ? (uint32_t)A.P : (uint32_t)owner;
    A.bval[i] = i;
}

// ---- 8: means, masks, the batch ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void mp_means_kernel(MpArgs A)
{
    const int lane = threadIdx.x & 63;
    const int L = blockIdx.x * PC_WAVES + (threadIdx.x >> 6);
    if (L >= A.P) return;
    const PcGrid& g = A.g;
    const int cls = A.cls[L], f = A.from[L], m = g.sz * g.sz;
    uint8_t* W = A.W + (size_t)L * (size_t)m;
    const uint8_t* Wold = (f >= 0 && cls != MP_FRESH) ? A.W0 + (size_t)f * (size_t)m : nullptr;       // :242 | :290
    for (int c = lane; c < m; c += 64) W[c] = Wold ? Wold[c] : (uint8_t)0;
    double mean[3], cmean[3] = {0, 0, 0}, mnd = 0.0;
    if (cls == MP_FRESH) {
        const int s0 = A.off[L], s1 = A.off[L + 1], cnt = s1 - s0;
        int cs[3] = {0, 0, 0};
        for (int b0 = s0; b0 < s1; b0 += 64) {                // depth sum in patch order, colour sums (integers: any order)
            const int s = b0 + lane;
            double d = 0.0;
            if (s < s1) {
                const int i = A.sval[s];
                d = A.local[(size_t)i * 3];
                const uint32_t c = pc_rgb_of(&A.cloud[i]);
                cs[0] += (int)(c & 0xffu); cs[1] += (int)((c >> 8) & 0xffu); cs[2] += (int)((c >> 16) & 0xffu);
            }
            const int here = min(64, s1 - b0);
            for (int b = 0; b < here; ++b) mnd += pc_readlane_d(d, b);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
            for (int o = 32; o > 0; o >>= 1) cs[a] += __shfl_xor(cs[a], o);
#pragma unroll
        for (int a = 0; a < 3; ++a) mean[a] = A.org[(size_t)L * 3 + a];
        if (cnt > 0) {                                        // the producer's :101-107, :116; a leaf that owns nothing keeps its centre
            mnd /= (double)cnt;
#pragma unroll
            for (int a = 0; a < 3; ++a) cmean[a] = (double)cs[a] / (double)cnt;
            const double* R = A.R + (size_t)L * 9;
#pragma unroll
            for (int a = 0; a < 3; ++a) mean[a] += mnd * R[a];
        }
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mean[a] = A.mean0[(size_t)f * 3 + a];
            cmean[a] = A.rgbm0[(size_t)f * 3 + a];
        }
    }
    if (lane < 3) {
        A.mean[(size_t)L * 3 + lane] = lane == 0 ? mean[0] : (lane == 1 ? mean[1] : mean[2]);
        A.rgb_mean[(size_t)L * 3 + lane] = lane == 0 ? cmean[0] : (lane == 1 ? cmean[1] : cmean[2]);
    }
    if (lane == 0) A.shift[L] = mnd;
}

// a thread per owned point; bucket position = row of the batch.  W cells: plain byte stores of 1 (any order gives the same mask)
__global__ __launch_bounds__(PC_THREADS) void mp_emit_kernel(MpArgs A)
{
    const int s = blockIdx.x * PC_THREADS + threadIdx.x;
    if (s >= A.n) return;
    const uint32_t L = A.skey[s];
    if (L >= (uint32_t)A.P) return;
    const PcGrid& g = A.g;
    const size_t total = (size_t)A.off[A.P];
    const int i = A.sval[s];
    const double d = A.local[(size_t)i * 3], u = A.local[(size_t)i * 3 + 1], w = A.local[(size_t)i * 3 + 2];
    A.y[s] = A.cls[L] == MP_FRESH ? d - A.shift[L] : d;       // mean-removed (fresh) | as is (kept)
    A.x0[s] = u;
    A.x1[s] = w;
    A.src[s] = i;
    const uint32_t c = pc_rgb_of(&A.cloud[i]);
    const double* cm = A.rgb_mean + (size_t)L * 3;            // the leaf's own mean (fresh) | the stored one (kept, :237)
    A.rgb[s] = (double)(c & 0xffu) - cm[0];
    A.rgb[total + s] = (double)((c >> 8) & 0xffu) - cm[1];
    A.rgb[2 * total + s] = (double)((c >> 16) & 0xffu) - cm[2];
    A.W[(size_t)L * (size_t)(g.sz * g.sz) + (size_t)pc_mask_cell(g, u, w)] = 1;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
namespace {

struct MpScratch {
    PcVoxelTable T;
    uint64_t *okey, *ukey;
    int32_t *ustart, *ku, *ko, *add, *arank, *o2n, *from, *cls, *bval, *sval, *nmax;
    uint32_t *bkey, *skey;
    double *Mu, *Mo, *org, *shift, *local;
    void* prim;
};

// pl: bound on the number of merged leaves
size_t mp_carve(PcCarver& c, MpScratch& s, size_t n, size_t p0, size_t pl, size_t prim_bytes)
{
    s.T.carve(c, n);
    s.ukey = c.take<uint64_t>(n); s.ustart = c.take<int32_t>(n + 1);
    s.Mu = c.take<double>(16 * n); s.ku = c.take<int32_t>(n);
    s.add = c.take<int32_t>(n + 1); s.arank = c.take<int32_t>(n + 1);
    s.okey = c.take<uint64_t>(p0); s.Mo = c.take<double>(16 * p0); s.ko = c.take<int32_t>(p0); s.o2n = c.take<int32_t>(p0);
    s.from = c.take<int32_t>(pl); s.cls = c.take<int32_t>(pl); s.org = c.take<double>(3 * pl); s.shift = c.take<double>(pl);
    s.local = c.take<double>(3 * n);
    s.bkey = c.take<uint32_t>(n); s.skey = c.take<uint32_t>(n); s.bval = c.take<int32_t>(n); s.sval = c.take<int32_t>(n);
    s.nmax = c.take<int32_t>(4);
    s.prim = c.take<char>(prim_bytes);
    return c.used;
}

}  // namespace

#define MP_HIP(call) PC_HIP_IN("gpc_patches_insert_cloud", call)

extern "C" {

int gpc_patches_insert_cloud_dev(gpc_ctx* ctx, const gpc_patches* model, const gpc_sparse* depth, const gpc_point_xyzrgb* cloud, int n,
                                 int min_nbr, gpc_patches** out, int32_t* old_to_new)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!out) return gpc_fail(ctx, GPC_EINVAL, "out is NULL");
    *out = nullptr;
    if (!model) return gpc_fail(ctx, GPC_EINVAL, "model is NULL");
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative point count");
    if (n > 0 && !cloud) return gpc_fail(ctx, GPC_EINVAL, "cloud is NULL");
    if (min_nbr < 1) return gpc_fail(ctx, GPC_EINVAL, "min_nbr must be >= 1");
    std::lock_guard<std::mutex> lk(ctx->mu);
    // (an object of another context is not in this context's list: found out without touching it)
    if (!gpc_child_listed(ctx, model) || (depth && !gpc_child_listed(ctx, depth)))
        return gpc_fail(ctx, GPC_EINVAL, "model and depth must be live objects of this context");
    const int P0 = model->v.P;
    if (depth && (depth->ny != 1 || depth->P != P0))
        return gpc_fail(ctx, GPC_EINVAL, "depth must have ny == 1 and the model's P (%d), got ny %d, P %d", P0, depth->ny, depth->P);
    if (P0 == 0) return gpc_fail(ctx, GPC_EINVAL, "the model is empty: gpc_project_cloud cuts the first one");
    if (!old_to_new) return gpc_fail(ctx, GPC_EINVAL, "old_to_new is NULL");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    hipStream_t st = ctx->stream;
    const PcGrid g0 = model->grid;
    const int sz = g0.sz;
    const size_t N = (size_t)n, P0z = (size_t)P0, m = (size_t)(sz * sz);
    const int nblk = (n + PC_THREADS - 1) / PC_THREADS;
    gpc_patches* o = new gpc_patches;
    o->ctx = ctx;
    gpc_ctx_ref(ctx);
    o->v.m = sz * sz;

    // 1: the scan's corners; the grid grows over them by whole voxels
    PcGrid g = g0;
    if (n > 0) {
        uint32_t hb[8];
        if (int rc = pc_cloud_bounds(ctx, "gpc_patches_insert_cloud", cloud, n, hb)) { pc_patches_release(o); return rc; }
        for (int a = 0; a < 3; ++a) {
            // unshifted voxel coordinates of the scan's corners (floor((x - mn) / res) is monotone in x: the corners bound every point's)
            const double lo = std::floor(((double)pc_unordered(hb[a]) - g0.mn[a]) / g0.res);
            const double hi = std::floor(((double)pc_unordered(hb[3 + a]) - g0.mn[a]) / g0.res);
            const double koff = std::max((double)g0.koff[a], -lo);
            const double kmax = std::max((double)(g0.kmax[a] - g0.koff[a]), hi) + koff;
            if (!(kmax < 2097152.0)) PC_FAIL(GPC_ERANGE, "more than 2^21 voxels of side res along an axis");
            g.koff[a] = (int)koff;
            g.kmax[a] = (int)kmax;
        }
        g.bx = pc_bits_for(g.kmax[0]); g.by = pc_bits_for(g.kmax[1]); g.bz = pc_bits_for(g.kmax[2]);
    }

    // scratch
    size_t table_bytes = 0, scan2_bytes = 0, sort2_bytes = 0;
    const size_t Pbound = P0z + N;
    if (n > 0) {
        MP_HIP(pc_voxel_table_prim_bytes(ctx, g, N, &table_bytes));
        MP_HIP(rocprim::exclusive_scan(nullptr, scan2_bytes, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, N + 1, rocprim::plus<int32_t>(), st));
        MP_HIP(rocprim::radix_sort_pairs(nullptr, sort2_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, N,
                                         0u, (unsigned)pc_bits_for((int)std::min<size_t>(Pbound, 0x7fffffff)), st));
    }
    const size_t prim_bytes = std::max(table_bytes, std::max(sort2_bytes, scan2_bytes));
    MpScratch S;
    {
        PcCarver measure(nullptr);
        if (int rc = gpc_ws_reserve(ctx, mp_carve(measure, S, N, P0z, Pbound, prim_bytes))) { pc_patches_release(o); return rc; }
        PcCarver c(ctx->ws);
        mp_carve(c, S, N, P0z, Pbound, prim_bytes);
    }
    MpArgs A;
    memset(&A, 0, sizeof(A));
    A.g0 = g0; A.g = g; A.n = n; A.P0 = P0; A.min_nbr = min_nbr;
    A.cloud = cloud;
    A.key0 = model->leaf_key; A.bv = depth ? depth->b : nullptr;
    A.R0 = model->v.rotations; A.mean0 = model->v.means; A.rgbm0 = model->v.rgb_means; A.W0 = model->v.W;
    A.okey = S.okey; A.ukey = S.ukey; A.ustart = S.ustart; A.sp = S.T.sp;
    A.Mu = S.Mu; A.Mo = S.Mo; A.ku = S.ku; A.ko = S.ko; A.add = S.add; A.arank = S.arank; A.o2n = S.o2n; A.from = S.from; A.cls = S.cls;
    A.org = S.org; A.shift = S.shift; A.local = S.local;
    A.bkey = S.bkey; A.skey = S.skey; A.bval = S.bval; A.sval = S.sval; A.nmax = S.nmax;
    hipLaunchKernelGGL(mp_rekey_kernel, dim3((P0 + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, st, A);
    MP_HIP(hipGetLastError());

    // 2: the scan's voxel table
    int32_t U = 0;
    size_t tb;
    if (n > 0) {
        MP_HIP(pc_voxel_table_build(ctx, g, cloud, n, S.T, S.prim, prim_bytes, &U));
        if (U < 1 || U > n) PC_FAIL(GPC_EHIP, "internal: %d scan voxels of %d points", (int)U, n);
        MP_HIP(pc_voxel_table_leaves(ctx, n, S.T, U, S.ukey, S.ustart));
    }
    A.U = U;

    // 3: sphere counts and moments over the scan's points; 4: which voxels become leaves
    if (U > 0) {
        hipLaunchKernelGGL(mp_moment_kernel, dim3((U + PC_WAVES - 1) / PC_WAVES), dim3(PC_THREADS), 0, st, A, (const uint64_t*)S.ukey, (int)U,
                           (const int32_t*)nullptr, S.Mu, S.ku);
        MP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(mp_moment_kernel, dim3((P0 + PC_WAVES - 1) / PC_WAVES), dim3(PC_THREADS), 0, st, A, (const uint64_t*)S.okey, P0, A.bv,
                       S.Mo, S.ko);
    MP_HIP(hipGetLastError());
    hipLaunchKernelGGL(mp_flag_kernel, dim3((U + 1 + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, st, A);
    MP_HIP(hipGetLastError());
    int32_t nadd = 0;
    if (U > 0) {
        tb = prim_bytes;
        MP_HIP(rocprim::exclusive_scan(S.prim, tb, S.add, S.arank, (int32_t)0, (size_t)U + 1, rocprim::plus<int32_t>(), st));
        MP_HIP(hipMemcpyAsync(&nadd, S.arank + U, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    } else {
        MP_HIP(hipMemsetAsync(S.arank, 0, sizeof(int32_t), st));
    }
    MP_HIP(hipStreamSynchronize(st));
    if (nadd < 0 || nadd > U) PC_FAIL(GPC_EHIP, "internal: %d new leaves of %d scan voxels", (int)nadd, (int)U);
    const long long Pll = (long long)P0 + (long long)nadd;
    if (Pll * (long long)m > 0x7fffffffLL) PC_FAIL(GPC_ERANGE, "P * sz * sz exceeds 2^31-1");
    const int P = (int)Pll;
    const size_t Pz = (size_t)P;
    A.P = P;

    // the result: one block, laid out as the producer's
    MP_HIP(pc_patches_alloc(o, Pz, N, m));
    o->grid = g;
    A.mkey = const_cast<uint64_t*>(o->leaf_key);
    A.off = const_cast<int32_t*>(o->v.off); A.R = const_cast<double*>(o->v.rotations); A.mean = const_cast<double*>(o->v.means);
    A.rgb_mean = const_cast<double*>(o->v.rgb_means); A.W = const_cast<uint8_t*>(o->v.W);
    A.x0 = const_cast<double*>(o->v.x0); A.x1 = const_cast<double*>(o->v.x1); A.y = const_cast<double*>(o->v.y);
    A.rgb = const_cast<double*>(o->v.rgb); A.src = const_cast<int32_t*>(o->v.src);
    hipLaunchKernelGGL(mp_merge_kernel, dim3((P0 + U + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, st, A);
    MP_HIP(hipGetLastError());
    MP_HIP(hipMemcpyAsync(old_to_new, S.o2n, sizeof(int32_t) * P0z, hipMemcpyDeviceToHost, st));
    // 5: frames; 6: ownership; 7: buckets
    hipLaunchKernelGGL(mp_frame_kernel, dim3((P + MP_FRAME_THREADS - 1) / MP_FRAME_THREADS), dim3(MP_FRAME_THREADS), 0, st, A);
    MP_HIP(hipGetLastError());
    if (n > 0) {
        hipLaunchKernelGGL(mp_claim_kernel, dim3(nblk), dim3(PC_THREADS), 0, st, A);
        MP_HIP(hipGetLastError());
        tb = prim_bytes;
        MP_HIP(rocprim::radix_sort_pairs(S.prim, tb, S.bkey, S.skey, S.bval, S.sval, N, 0u, (unsigned)pc_bits_for(P), st));
        MP_HIP(pc_bucket_offsets(st, S.skey, n, P, A.off));
    } else {
        MP_HIP(hipMemsetAsync(A.off, 0, sizeof(int32_t) * (Pz + 1), st));
    }
    // 8: means and masks, then the batch rows
    const int lblk = (P + PC_WAVES - 1) / PC_WAVES;
    hipLaunchKernelGGL(mp_means_kernel, dim3(lblk), dim3(PC_THREADS), 0, st, A);
    MP_HIP(hipGetLastError());
    if (n > 0) {
        hipLaunchKernelGGL(mp_emit_kernel, dim3(nblk), dim3(PC_THREADS), 0, st, A);
        MP_HIP(hipGetLastError());
    }
    MP_HIP(hipMemsetAsync(S.nmax, 0, 4 * sizeof(int32_t), st));
    MP_HIP(pc_nmax(st, A.off, P, S.nmax));
    MP_HIP(pc_patches_publish(ctx, o, P, S.nmax));
    *out = o;
    return GPC_OK;
}

int gpc_patches_insert_cloud(gpc_ctx* ctx, const gpc_patches* model, const gpc_sparse* depth, const gpc_point_xyzrgb* cloud, int n,
                             int min_nbr, gpc_patches** out, int32_t* old_to_new)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (!out) return gpc_fail(ctx, GPC_EINVAL, "out is NULL");
    *out = nullptr;
    if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "negative point count");
    if (n > 0 && !cloud) return gpc_fail(ctx, GPC_EINVAL, "cloud is NULL");
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    GpcStaging st(ctx, "gpc_patches_insert_cloud");
    const gpc_point_xyzrgb* d_cloud = st.up(cloud, (size_t)n);
    if (st.ok()) st.rc = gpc_patches_insert_cloud_dev(ctx, model, depth, d_cloud, n, min_nbr, out, old_to_new);
    return st.finish();
}

}  // extern "C"
