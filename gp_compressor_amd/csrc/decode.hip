// decode.hip -- the read-out half of the codec in one pass: gpc_sparse_decode evaluates the depth and the colour GP of every trained leaf at
// the grid points whose cell holds data, and writes the reconstructed cloud as 32-byte records.  It replaces, for those points, the chain
// gpc_sparse_predict_dev (depth) -> gpc_sparse_predict_dev (colour) -> gpc_reproject_dev of gp_compressor::load_compressed
// (src/gp_compressor.cpp:298-380 of the reference), which evaluates all sz * sz points of a leaf and carries f* and C* through HBM; the
// mask is the producer's W, whose use upstream is commented out (:323-325), and / or the ray cast's cell labels.  The rule is stated in
// full in include/gpc.h.  Three stages on the context's stream, no atomics -- the same inputs give the same bytes:
//   count   a wave per leaf: the kept cells of its W / cells row (read coalesced; a count needs no transposition)
//   scan    one workgroup: exclusive scan of the P counts into the leaves' first records, the total into n_points
//   emit    a wave per leaf: alpha / BV of both GPs and the kept flags of the row staged in LDS once, then the grid in blocks of 64
//           points.  A lane tests its point; ballot + mbcnt rank the kept ones, which are appended in order to a queue of two blocks.
//           Whenever 64 are pending every lane evaluates one (b_depth + b_rgb kernel values, the frame, the clamp) and stores its
//           record at base[L] + running index; the rest is flushed after the last block.  Lanes are full at any fill, and the order is
//           ascending (L, p) by construction.
// The means are accumulated as sparse_predict_kernel / sparse_predict_small_kernel accumulate them (same expression, same order), the
// frame and the clamp are reproject_kernel's (explicit round-to-nearest operations): a record has the bits of that chain.
#include <algorithm>
#include <cmath>

#include "gpc_device.h"
#include "sparse_internal.h"

#define DC_COUNT_THREADS 256
#define DC_SCAN_THREADS 1024
#define DC_QUEUE 128              // two blocks of 64 pending points
#define DC_ROW_MAX 16384          // the kept flags of a leaf's row sit in LDS up to this m (sz <= 128); beyond it they are read where they are

struct DcGp {                     // one gpc_sparse as the kernel reads it
    const double *alpha, *BV;     // [P][ny][ld], [P][ld][2]
    const int32_t* b;
    int ld;
    double sf, c_exp;             // sigma_f^2, (double)(-0.5f) / l^2
};

struct DcArgs {
    int P, m, sz, capacity;
    int row_lds;                  // the kept flags of the row are staged in LDS (m <= DC_ROW_MAX)
    double res;
    const uint8_t *W, *cells;     // either may be nullptr
    DcGp depth, rgb;              // rgb.alpha == nullptr: no colour
    const double *R, *mean, *rgb_mean;
    const int32_t *cnt, *base;    // per leaf: kept points, first record
    gpc_point_xyzrgb* cloud;
    int32_t *leaf, *point;        // either may be nullptr
};

__device__ static inline bool dc_keep(const uint8_t* W, const uint8_t* cells, size_t at)
{
    bool k = true;
    if (W) k = W[at] != 0;
    if (cells) k = k && cells[at] != GPC_CELL_FREE;
    return k;
}

// ---- count: cnt[L] = kept points of leaf L (0 for a leaf without a depth basis) --------------------------------------------------------
__global__ __launch_bounds__(DC_COUNT_THREADS) void decode_count_kernel(int P, int m, const int32_t* b, const uint8_t* W, const uint8_t* cells,
                                                                         int32_t* cnt, int32_t* count_out)
{
    const int lane = threadIdx.x & 63, wpb = DC_COUNT_THREADS / 64;
    for (int L = blockIdx.x * wpb + (threadIdx.x >> 6); L < P; L += gridDim.x * wpb) {     // (wave-uniform)
        int n = 0;
        if (b[L] > 0) {
            if (!W && !cells) {
                n = m;
            } else {
                const size_t row = (size_t)L * (size_t)m;
                for (int c = lane; c < m; c += 64) n += dc_keep(W, cells, row + c) ? 1 : 0;
                for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
            }
        }
        if (lane == 0) {
            cnt[L] = n;
            if (count_out) count_out[L] = n;
        }
    }
}

// ---- scan: base[i] = sum_{j < i} cnt[j], total[0] = sum_j cnt[j].  Thread t holds the leaves [t per, (t + 1) per), per = ceil(P / 1024) ---
__global__ __launch_bounds__(DC_SCAN_THREADS) void decode_scan_kernel(int P, const int32_t* cnt, int32_t* base, int32_t* total)
{
    __shared__ int part[DC_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int per = (P + DC_SCAN_THREADS - 1) / DC_SCAN_THREADS;
    const int lo = min(P, tid * per), hi = min(P, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += cnt[i];
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < DC_SCAN_THREADS; o <<= 1) {      // inclusive Hillis-Steele scan
        const int v = (tid >= o) ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;                           // exclusive prefix of this thread's segment
    for (int i = lo; i < hi; ++i) {
        base[i] = run;
        run += cnt[i];
    }
    if (tid == DC_SCAN_THREADS - 1) total[0] = part[tid];
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------------------
struct DcLeaf {                   // what a wave holds of its leaf (wave-uniform)
    int bd, bc;                   // basis vectors in use: depth, colour
    const double *R, *mean, *cm;  // the frame in LDS: [9], [3], [3] (read by broadcast; in scalar registers the fifteen doubles spilled)
};

// the record of grid point p of the wave's leaf
__device__ static inline gpc_point_xyzrgb dc_record(const DcArgs& A, const DcLeaf& F, int p, const double* T, const double* bvd,
                                                    const double* ald, const double* bvc, const double* alc)
{
    const int gx = p % A.sz, gy = p / A.sz;
    const double q0 = A.res * (((double)gx + 0.5) / (double)A.sz - 0.5);     // dense_grid_points_kernel's expression
    const double q1 = A.res * (((double)gy + 0.5) / (double)A.sz - 0.5);
    // f = alpha^T k, as the predict kernels accumulate it (sparse_predict.hip)
    double f = 0.0;
    for (int i = 0; i < F.bd; ++i) {
        const double k = gpc_rbf_neg(A.depth.sf, A.depth.c_exp, q0, q1, bvd[2 * i], bvd[2 * i + 1], T);
        f += ald[i] * k;
    }
    double s[3] = {0.0, 0.0, 0.0};
    const int ldc = A.rgb.ld;
    for (int i = 0; i < F.bc; ++i) {
        const double k = gpc_rbf_neg(A.rgb.sf, A.rgb.c_exp, q0, q1, bvc[2 * i], bvc[2 * i + 1], T);
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += alc[c * ldc + i] * k;
    }
    gpc_point_xyzrgb r;
    float xyz[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                             // reproject_kernel's association
        const double v = __dadd_rn(__dadd_rn(__dmul_rn(F.R[i], f), __dmul_rn(F.R[i + 3], q0)), __dmul_rn(F.R[i + 6], q1));
        xyz[i] = (float)__dadd_rn(v, F.mean[i]);
    }
    r.x = xyz[0]; r.y = xyz[1]; r.z = xyz[2]; r.w = 1.0f;
    uint8_t rgb[3] = {0, 0, 0};
    if (A.rgb.alpha) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = rp_flatten(__dadd_rn(s[c], F.cm[c]));
    }
    r.r = rgb[0]; r.g = rgb[1]; r.b = rgb[2]; r.a = 255;
    r.pad[0] = r.pad[1] = r.pad[2] = 0.0f;
    return r;
}

// `n` queued points from the queue's head, one per lane, to the records first .. first + n - 1 (below the capacity)
__device__ static inline void dc_flush(const DcArgs& A, const DcLeaf& F, int L, const int* queue, int head, int n, int first, const double* T,
                                       const double* bvd, const double* ald, const double* bvc, const double* alc)
{
    const int lane = threadIdx.x;
    const int at = first + lane;
    if (lane < n && at < A.capacity) {
        const int p = queue[(head + lane) & (DC_QUEUE - 1)];
        A.cloud[at] = dc_record(A, F, p, T, bvd, ald, bvc, alc);
        if (A.leaf) A.leaf[at] = L;
        if (A.point) A.point[at] = p;
    }
}

__global__ __launch_bounds__(64) void decode_emit_kernel(DcArgs A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ldd = A.depth.ld, ldc = A.rgb.alpha ? A.rgb.ld : 0;
    double* T = reinterpret_cast<double*>(smem);   // 64
    double* bvd = T + GPC_EXP_TABLE_SIZE;          // [ldd][2]
    double* ald = bvd + 2 * ldd;                   // [ldd]
    double* bvc = ald + ldd;                       // [ldc][2]
    double* alc = bvc + 2 * ldc;                   // [3][ldc]
    double* frame = alc + 3 * ldc;                 // R [9], mean [3], rgb_mean [3], one spare
    int* queue = reinterpret_cast<int*>(frame + 16);                     // DC_QUEUE
    uint8_t* row = reinterpret_cast<uint8_t*>(queue + DC_QUEUE);         // m kept flags in the layout of W (A.row_lds only)
    const int lane = threadIdx.x;
    const int m = A.m, sz = A.sz;
    const bool masked = A.W || A.cells;
    gpc_exp_table_init(T);
    for (int L = blockIdx.x; L < A.P; L += gridDim.x) {
        const int n = __builtin_amdgcn_readfirstlane(A.cnt[L]);
        const int first = __builtin_amdgcn_readfirstlane(A.base[L]);
        if (n == 0 || first >= A.capacity) continue;                     // (wave-uniform, before any barrier)
        DcLeaf F;
        F.bd = min(__builtin_amdgcn_readfirstlane(A.depth.b[L]), ldd);
        F.bc = A.rgb.alpha ? min(__builtin_amdgcn_readfirstlane(A.rgb.b[L]), ldc) : 0;
        F.R = frame; F.mean = frame + 9; F.cm = frame + 12;
        const size_t rowg = (size_t)L * (size_t)m;
        __syncthreads();                                                 // (one wave: the previous leaf's reads are done)
        for (int i = lane; i < F.bd; i += 64) {
            bvd[2 * i] = A.depth.BV[((size_t)L * ldd + i) * 2];
            bvd[2 * i + 1] = A.depth.BV[((size_t)L * ldd + i) * 2 + 1];
            ald[i] = A.depth.alpha[(size_t)L * ldd + i];
        }
        for (int i = lane; i < F.bc; i += 64) {
            bvc[2 * i] = A.rgb.BV[((size_t)L * ldc + i) * 2];
            bvc[2 * i + 1] = A.rgb.BV[((size_t)L * ldc + i) * 2 + 1];
#pragma unroll
            for (int c = 0; c < 3; ++c) alc[c * ldc + i] = A.rgb.alpha[((size_t)L * 3 + c) * ldc + i];
        }
        if (lane < 9) frame[lane] = A.R[(size_t)L * 9 + lane];
        else if (lane < 12) frame[lane] = A.mean[(size_t)L * 3 + (lane - 9)];
        else if (lane < 15) frame[lane] = A.rgb.alpha ? A.rgb_mean[(size_t)L * 3 + (lane - 12)] : 0.0;
        if (masked && A.row_lds)
            for (int c = lane; c < m; c += 64) row[c] = dc_keep(A.W, A.cells, rowg + c) ? 1 : 0;     // coalesced
        __syncthreads();
        int head = 0, pend = 0, done = 0;                                // queue head, points pending, records written (wave-uniform)
        for (int p0 = 0; p0 < m; p0 += 64) {
            const int p = p0 + lane;
            bool keep = p < m;
            if (keep && masked) {
                const int c = sz * (p % sz) + p / sz;                    // the producer's cell, transposed against p
                keep = A.row_lds ? row[c] != 0 : dc_keep(A.W, A.cells, rowg + c);
            }
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
            if (keep) {
                const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                queue[(head + pend + rank) & (DC_QUEUE - 1)] = p;
            }
            pend += __popcll(bal);
            __syncthreads();
            if (pend >= 64) {
                dc_flush(A, F, L, queue, head, 64, first + done, T, bvd, ald, bvc, alc);
                head = (head + 64) & (DC_QUEUE - 1);
                pend -= 64;
                done += 64;
                __syncthreads();                                         // the slots just read are free for the next block
            }
        }
        if (pend > 0) dc_flush(A, F, L, queue, head, pend, first + done, T, bvd, ald, bvc, alc);
    }
}

// ------------------------------------------------------------------------------------------------ host side

static DcGp dc_gp_of(const gpc_sparse* g)
{
    DcGp G;
    G.alpha = g->alpha; G.BV = g->BV; G.b = g->b; G.ld = g->ld;
    G.sf = g->prm.sigmaf_sq;
    G.c_exp = (double)(-0.5f) / g->prm.l_sq;
    return G;
}

// what both entries check before they touch a buffer (the caller holds ctx->mu; ctx is depth's context and alive)
static int dc_check(gpc_ctx* ctx, const gpc_sparse* depth, const gpc_sparse* rgb, double res, int sz, const double* rotations,
                    const double* means, const double* rgb_means, int capacity, const void* cloud, const int32_t* n_points)
{
    // (an object of another context, or a destroyed one, is not in this context's list: found out without touching it)
    if (!gpc_child_listed(ctx, depth) || (rgb && !gpc_child_listed(ctx, rgb)))
        return gpc_fail(ctx, GPC_EINVAL, "depth and rgb must be live objects of one context");
    if (depth->ny != 1) return gpc_fail(ctx, GPC_EINVAL, "depth must have ny == 1, got %d", depth->ny);
    if (rgb && (rgb->ny != 3 || rgb->P != depth->P))
        return gpc_fail(ctx, GPC_EINVAL, "rgb must have ny == 3 and depth's P (%d), got ny %d, P %d", depth->P, rgb->ny, rgb->P);
    if (sz < 1) return gpc_fail(ctx, GPC_EINVAL, "sz must be at least 1");
    if (!std::isfinite(res)) return gpc_fail(ctx, GPC_EINVAL, "res is not finite");
    if (capacity < 0) return gpc_fail(ctx, GPC_EINVAL, "negative capacity");
    if (!n_points) return gpc_fail(ctx, GPC_EINVAL, "n_points is NULL");
    if (rgb && !rgb_means) return gpc_fail(ctx, GPC_EINVAL, "rgb needs rgb_means");
    if (depth->P > 0 && cloud && (!rotations || !means)) return gpc_fail(ctx, GPC_EINVAL, "rotations/means is NULL");
    if (depth->P > 0 && (long long)depth->P * (long long)sz * (long long)sz > 0x7fffffffLL)
        return gpc_fail(ctx, GPC_ERANGE, "P*m exceeds 2^31-1 points");
    return GPC_OK;
}

static size_t dc_emit_lds(int ldd, int ldc, int m, bool row_lds)
{
    return sizeof(double) * (size_t)(GPC_EXP_TABLE_SIZE + 3 * ldd + 5 * ldc + 16) + sizeof(int) * DC_QUEUE + (row_lds ? ((size_t)m + 15) & ~(size_t)15 : 0);
}

extern "C" {

int gpc_sparse_decode_dev(gpc_sparse* depth, gpc_sparse* rgb, double res, int sz, const uint8_t* W, const uint8_t* cells,
                          const double* rotations, const double* means, const double* rgb_means, int capacity, gpc_point_xyzrgb* cloud,
                          int32_t* leaf, int32_t* point, int32_t* count, int32_t* n_points)
{
    gpc_ctx* ctx = sp_live(depth);
    if (!ctx) return GPC_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = dc_check(ctx, depth, rgb, res, sz, rotations, means, rgb_means, capacity, cloud, n_points)) return rc;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    hipStream_t st = ctx->stream;
    const int P = depth->P;
    if (P == 0) {
        GPC_HIP(ctx, hipMemsetAsync(n_points, 0, sizeof(int32_t), st));
        return GPC_OK;
    }
    const int m = sz * sz;
    if (int rc = gpc_ws_reserve(ctx, sizeof(int32_t) * 2 * (size_t)P)) return rc;
    int32_t* cnt = static_cast<int32_t*>(ctx->ws);
    int32_t* base = cnt + P;
    const int wpb = DC_COUNT_THREADS / 64;
    hipLaunchKernelGGL(decode_count_kernel, dim3(std::min((P + wpb - 1) / wpb, ctx->num_cus * 8)), dim3(DC_COUNT_THREADS), 0, st, P, m,
                       depth->b, W, cells, cnt, count);
    GPC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(decode_scan_kernel, dim3(1), dim3(DC_SCAN_THREADS), 0, st, P, cnt, base, n_points);
    GPC_HIP(ctx, hipGetLastError());
    if (!cloud || capacity == 0) return GPC_OK;    // the sizing call
    DcArgs A;
    A.P = P; A.m = m; A.sz = sz; A.capacity = capacity;
    A.row_lds = m <= DC_ROW_MAX ? 1 : 0;
    A.res = res;
    A.W = W; A.cells = cells;
    A.depth = dc_gp_of(depth);
    if (rgb) A.rgb = dc_gp_of(rgb);
    else A.rgb = DcGp{nullptr, nullptr, nullptr, 0, 0.0, 0.0};
    A.R = rotations; A.mean = means; A.rgb_mean = rgb_means;
    A.cnt = cnt; A.base = base;
    A.cloud = cloud; A.leaf = leaf; A.point = point;
    const size_t lds = dc_emit_lds(A.depth.ld, rgb ? A.rgb.ld : 0, m, (W || cells) && A.row_lds);
    // (128 one-wave workgroups per CU: leaves differ in cost with their fill, and a finer deal evens that out -- measured on the C4-defaults batch
    // at 8 / 16 / 32 / 64 / 128 per CU, unmasked 0.58 / 0.64 / 0.56 / 0.52 / 0.51 ms, the masked legs alike: DESIGN 5.5a)
    hipLaunchKernelGGL(decode_emit_kernel, dim3(std::min(P, ctx->num_cus * 128)), dim3(64), lds, st, A);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}

int gpc_sparse_decode(gpc_sparse* depth, gpc_sparse* rgb, double res, int sz, const uint8_t* W, const uint8_t* cells, const double* rotations,
                      const double* means, const double* rgb_means, int capacity, gpc_point_xyzrgb* cloud, int32_t* leaf, int32_t* point,
                      int32_t* count, int32_t* n_points)
{
    gpc_ctx* ctx = sp_live(depth);
    if (!ctx) return GPC_EINVAL;
    size_t Pz = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (int rc = dc_check(ctx, depth, rgb, res, sz, rotations, means, rgb_means, capacity, cloud, n_points)) return rc;
        Pz = (size_t)depth->P;
    }
    if (Pz == 0) {
        *n_points = 0;
        return GPC_OK;
    }
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t Pm = Pz * (size_t)sz * (size_t)sz, cap = (size_t)capacity;
    GpcStaging st(ctx, "gpc_sparse_decode");
    const uint8_t* d_W = W ? st.up(W, Pm) : nullptr;
    const uint8_t* d_cells = cells ? st.up(cells, Pm) : nullptr;
    const double* d_R = (cloud && rotations) ? st.up(rotations, Pz * 9) : nullptr;
    const double* d_mu = (cloud && means) ? st.up(means, Pz * 3) : nullptr;
    const double* d_cm = rgb ? st.up(rgb_means, Pz * 3) : nullptr;
    gpc_point_xyzrgb* d_cloud = cloud ? st.out<gpc_point_xyzrgb>(cap) : nullptr;
    int32_t* d_leaf = (cloud && leaf) ? st.out<int32_t>(cap) : nullptr;
    int32_t* d_point = (cloud && point) ? st.out<int32_t>(cap) : nullptr;
    int32_t* d_count = count ? st.out<int32_t>(Pz) : nullptr;
    int32_t* d_n = st.out<int32_t>(1);
    if (st.ok())
        st.rc = gpc_sparse_decode_dev(depth, rgb, res, sz, d_W, d_cells, d_R, d_mu, d_cm, capacity, d_cloud, d_leaf, d_point, d_count, d_n);
    // the count first, then only that many records
    int32_t n = 0;
    st.down(&n, d_n, 1);
    st.sync();
    if (st.ok()) {
        const size_t w = (size_t)std::min(std::max(n, 0), capacity);
        st.down(cloud, d_cloud, w);
        st.down(leaf, d_leaf, w);
        st.down(point, d_point, w);
        st.down(count, d_count, Pz);
        st.sync();
    }
    const int rc = st.finish();
    if (rc == GPC_OK) *n_points = n;
    return rc;
}

}  // extern "C"
