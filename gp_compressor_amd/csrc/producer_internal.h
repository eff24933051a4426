// producer_internal.h -- the cloud cutter: what producer.hip (gpc_project_cloud), registration.hip (gpc_registration_*), mapping.hip
// (gpc_patches_insert_cloud), raycast.hip (gpc_patches_raycast), render.hip (gpc_patches_render) and distortion.hip
// (gpc_cloud_distortion) share.  Inline device pieces: the
// voxel grid of a patch batch and the key arithmetic of its leaf table, the search in that table, the per-point walk to the first leaf
// that accepts a point, a leaf's frame, mask cell and moment matrix, the ray / box test.  Declarations of what producer.hip defines
// once for every unit: the host stages that turn a cloud into a voxel table and a batch object, and the launchers of the bucket
// kernels (the library is built without relocatable device code: a kernel is launched from the unit that defines it).
#pragma once

#include <cmath>

#include "gpc_internal.h"

// These translation units are bit-exact against CPU restatements: floating-point contraction is off from here to their end, and
// every expression below is written in the association of oracle/gpc_oracle_producer.c.
#pragma clang fp contract(off)

struct PcGrid {
    double mn[3];       // minimum corner (the voxel grid's anchor)
    double res, radius, half;
    int kmax[3];        // largest voxel coordinate per axis
    int bx, by, bz;     // key = kz << (bx + by) | ky << bx | kx
    int sz;
    // whole-voxel shift of the origin (>= 0; 0 for a batch gpc_project_cloud cut): voxel k = floor((x - mn) / res) + koff.  A map that
    // grows below its first corner (mapping.hip) raises koff and keeps mn, so that no old voxel centre moves by rounding
    int koff[3];
};

__device__ static inline void pc_voxel(const PcGrid& g, float x, float y, float z, int k[3])
{
    k[0] = (int)floor(((double)x - g.mn[0]) / g.res) + g.koff[0];
    k[1] = (int)floor(((double)y - g.mn[1]) / g.res) + g.koff[1];
    k[2] = (int)floor(((double)z - g.mn[2]) / g.res) + g.koff[2];
}
__device__ static inline void pc_center(const PcGrid& g, const int k[3], double c[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = g.mn[a] + ((double)(k[a] - g.koff[a]) + 0.5) * g.res;
}
__host__ __device__ static inline uint64_t pc_pack(const PcGrid& g, int kx, int ky, int kz)
{
    return ((uint64_t)kz << (g.bx + g.by)) | ((uint64_t)ky << g.bx) | (uint64_t)kx;
}
__host__ __device__ static inline void pc_unpack(const PcGrid& g, uint64_t key, int k[3])
{
    k[0] = (int)(key & ((1ull << g.bx) - 1));
    k[1] = (int)((key >> g.bx) & ((1ull << g.by) - 1));
    k[2] = (int)(key >> (g.bx + g.by));
}

struct PcPoint {        // sorted-order record
    float x, y, z;
    uint32_t rgb;       // r | g << 8 | b << 16
};

// floats as unsigned integers of the same order (atomicMin / atomicMax on coordinates)
__device__ static inline uint32_t pc_ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ static inline float pc_unordered(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// first element >= key of the sorted a[0 .. n)
template <class T> __device__ static inline int pc_lower_bound(const T* a, int n, T key)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ static inline int pc_find_leaf(const uint64_t* leaf_key, int P, uint64_t key)
{
    const int lo = pc_lower_bound(leaf_key, P, key);
    return (lo < P && leaf_key[lo] == key) ? lo : -1;
}

// r | g << 8 | b << 16 of a record
__device__ static inline uint32_t pc_rgb_of(const gpc_point_xyzrgb* q)
{
    const uint32_t c = *reinterpret_cast<const uint32_t*>(&q->b);     // b | g << 8 | r << 16 | a << 24
    return ((c >> 16) & 0xffu) | (c & 0xff00u) | ((c & 0xffu) << 16);
}

// t = R^T e: e in the frame R (column-major: normal, u, v)
__device__ static inline void pc_to_frame(const double* R, const double e[3], double t[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = R[3 * a] * e[0] + R[3 * a + 1] * e[1] + R[3 * a + 2] * e[2];
}

// cell of the sz x sz mask that the in-plane coordinates (u, w) fall into (src/gp_compressor.cpp:90-92), clamped
__device__ static inline int pc_mask_cell(const PcGrid& g, double u, double w)
{
    int gx = (int)((double)g.sz * (u / g.res + 0.5)), gy = (int)((double)g.sz * (w / g.res + 0.5));
    gx = min(max(gx, 0), g.sz - 1);
    gy = min(max(gy, 0), g.sz - 1);
    return g.sz * gx + gy;
}

// slabs: does the ray o + t d meet the box [lo, hi) at some t >= 0?  tn, tf: where it enters and leaves
__device__ static inline bool pc_ray_box(const double lo[3], const double hi[3], const double o[3], const double d[3], double& tn, double& tf)
{
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    tn = -inf;
    tf = inf;
    bool meets = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (d[a] != 0.0) {
            const double t1 = (lo[a] - o[a]) / d[a], t2 = (hi[a] - o[a]) / d[a];
            tn = fmax(tn, fmin(t1, t2));
            tf = fmin(tf, fmax(t1, t2));
        } else if (!(lo[a] <= o[a] && o[a] < hi[a])) {
            meets = false;
        }
    }
    return meets && tn <= tf && tf >= 0.0;
}

// The per-point walk of registration and insertion: point p of voxel k (at most one voxel beyond the grid) belongs to the FIRST leaf in
// leaf order, out of the <= 27 around k, that skip(leaf) does not rule out, whose search sphere (around the voxel centre) holds p and
// whose +-half window, in the frame R[leaf] around origin[leaf], accepts it.  One binary search per (dz, dy) row: the <= 3 leaves of a row
// are neighbours in the sorted table.  Returns that leaf and q = R^T (p - origin), or -1 with q untouched.
template <class Skip>
__device__ static inline int pc_first_accepting_leaf(const PcGrid& g, const uint64_t* leaf_key, int P, const double p[3], const int k[3],
                                                     const double* R, const double* origin, Skip skip, double q[3])
{
    const double r2 = g.radius * g.radius;
    const int xlo = max(k[0] - 1, 0), xhi = min(k[0] + 1, g.kmax[0]);
    for (int j = 0; j < 9 && xlo <= xhi; ++j) {                             // rows (dz, dy) in ascending key order
        const int nz = k[2] + j / 3 - 1, ny = k[1] + j % 3 - 1;
        if (nz < 0 || nz > g.kmax[2] || ny < 0 || ny > g.kmax[1]) continue;
        const uint64_t key_lo = pc_pack(g, xlo, ny, nz), key_hi = pc_pack(g, xhi, ny, nz);
        for (int L = pc_lower_bound(leaf_key, P, key_lo); L < P; ++L) {     // the row's leaves are consecutive in the table
            const uint64_t key = leaf_key[L];
            if (key > key_hi) break;
            if (skip(L)) continue;
            int c3[3];
            pc_unpack(g, key, c3);
            double cen[3];
            pc_center(g, c3, cen);
            const double d[3] = {p[0] - cen[0], p[1] - cen[1], p[2] - cen[2]};
            if (!(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] <= r2)) continue;                  // radiusSearch
            const double* o = origin + (size_t)L * 3;
            const double e[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
            double t[3];
            pc_to_frame(R + (size_t)L * 9, e, t);
            if (t[1] > g.half || t[1] < -g.half || t[2] > g.half || t[2] < -g.half) continue;
            q[0] = t[0]; q[1] = t[1]; q[2] = t[2];
            return L;
        }
    }
    return -1;
}

__device__ static inline float pc_readlane_f(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ static inline double pc_readlane_d(double v, int lane)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}


// eigenvector of the smallest eigenvalue of the symmetric 4x4 matrix A: the cyclic Jacobi of orc_smallest_eigvec4
__device__ static inline void pc_smallest_eigvec4(double A[4][4], double v[4])
{
    double V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double offd = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) offd += A[p][q] * A[p][q];
        if (offd == 0.0) break;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double g = 100.0 * fabs(A[p][q]);       // negligible against both diagonal entries: drop it
                const bool drop = fabs(A[p][p]) + g == fabs(A[p][p]) && fabs(A[q][q]) + g == fabs(A[q][q]);
                if (A[p][q] != 0.0 && drop) A[p][q] = A[q][p] = 0.0;
                if (A[p][q] != 0.0) {
                    const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = c * akp - s * akq;
                        A[k][q] = s * akp + c * akq;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double apk = A[p][k], aqk = A[q][k];
                        A[p][k] = c * apk - s * aqk;
                        A[q][k] = s * apk + c * aqk;
                    }
                    A[p][q] = A[q][p] = 0.0;                  // the rotation annihilates this pair: make it exact
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double vkp = V[k][p], vkq = V[k][q];
                        V[k][p] = c * vkp - s * vkq;
                        V[k][q] = s * vkp + c * vkq;
                    }
                }
            }
        }
    }
    double best = A[0][0];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = V[k][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (A[i][i] < best) {
            best = A[i][i];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = V[k][i];
        }
}

__device__ static inline void pc_cross(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ static inline void pc_normalize(double a[3])
{
    const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (n > 0) { a[0] /= n; a[1] /= n; a[2] /= n; }
}

// compute_rotation (:29-64) from the 4x4 moment matrix M (row-major) of the k homogeneous points of a search sphere: R column-major
// (normal, u, v); fewer than 4 points give the identity (:31-34)
__device__ static inline void pc_frame_of_moments(const double* M, int k, double R[9])
{
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (k >= 4) {                                // :31-34
        double Mm[4][4], v[4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) Mm[a][b] = M[4 * a + b];
        pc_smallest_eigvec4(Mm, v);
        double normal[3] = {v[0], v[1], v[2]};
        pc_normalize(normal);
        const double x[3] = {1, 0, 0}, y[3] = {0, 1, 0}, z[3] = {0, 0, 1};
        double c1[3], c2[3];
        const double ax = fabs(normal[0]), ay = fabs(normal[1]), az = fabs(normal[2]);
        if (ax > ay && ax > az) {
            if (normal[0] < 0) { normal[0] = -normal[0]; normal[1] = -normal[1]; normal[2] = -normal[2]; }
            pc_cross(z, normal, c1);
        } else if (ay > ax && ay > az) {
            if (normal[1] < 0) { normal[0] = -normal[0]; normal[1] = -normal[1]; normal[2] = -normal[2]; }
            pc_cross(x, normal, c1);
        } else {
            if (normal[2] < 0) { normal[0] = -normal[0]; normal[1] = -normal[1]; normal[2] = -normal[2]; }
            pc_cross(y, normal, c1);
        }
        pc_normalize(c1);
        pc_cross(normal, c1, c2);
#pragma unroll
        for (int a = 0; a < 3; ++a) { R[a] = normal[a]; R[3 + a] = c1[a]; R[6 + a] = c2[a]; }
    }
}

#define PC_THREADS 256
#define PC_WAVES (PC_THREADS / 64)

#define PC_LROW 66         // LDS row pitch (doubles) of the product table: 64 hits + padding against bank conflicts

// One wave, one search sphere: lane j < 27 holds the sorted-order segment [seg0, seg1) of neighbour voxel (dz, dy, dx) = (j / 9, j / 3 % 3,
// j % 3) - 1.  The hits' exact products go to the wave's LDS table pr (10 rows of PC_LROW doubles) in hit order -- neighbour voxels in
// that order, ascending point index inside one: the oracle's accumulation order -- and lanes 0..15 add up entry (lane / 4, lane % 4) of
// the moment matrix; k = hits.
__device__ static inline void pc_sphere_moments(const PcGrid& g, const double center[3], int seg0, int seg1, const PcPoint* sp, double* pr,
                                                int lane, double& M, int& k)
{
    pr[9 * PC_LROW + lane] = 1.0;                             // the homogeneous coordinate's products
    const double r2 = g.radius * g.radius;
    // lanes 0..15: entry (ea, eb) of the moment matrix = product row of (min, max)
    const int ea = (lane >> 2) & 3, eb = lane & 3, lo = min(ea, eb), hi = max(ea, eb);
    const int row = (lo == 0 ? 0 : (lo == 1 ? 3 : (lo == 2 ? 5 : 6))) + hi;      // 0:0-3, 1:4-6, 2:7-8, 3:9
    const double* mine = pr + row * PC_LROW;
    M = 0.0;
    k = 0;
    for (int j = 0; j < 27; ++j) {
        const int s0 = __builtin_amdgcn_readlane(seg0, j), s1 = __builtin_amdgcn_readlane(seg1, j);
        for (int base = s0; base < s1; base += 64) {
            const int s = base + lane;
            double q0 = 0, q1 = 0, q2 = 0;
            bool in = false;
            if (s < s1) {
                const float4 p = *reinterpret_cast<const float4*>(&sp[s]);
                q0 = (double)p.x; q1 = (double)p.y; q2 = (double)p.z;
                const double ex = q0 - center[0], ey = q1 - center[1], ez = q2 - center[2];
                in = ex * ex + ey * ey + ez * ez <= r2;
            }
            const unsigned long long mask = __ballot(in);
            const int hits = __popcll(mask);
            if (in) {                                         // radiusSearch hit order = the oracle's accumulation order
                const int r = __popcll(mask & ((1ull << lane) - 1));
                pr[0 * PC_LROW + r] = q0 * q0; pr[1 * PC_LROW + r] = q0 * q1; pr[2 * PC_LROW + r] = q0 * q2; pr[3 * PC_LROW + r] = q0;
                pr[4 * PC_LROW + r] = q1 * q1; pr[5 * PC_LROW + r] = q1 * q2; pr[6 * PC_LROW + r] = q1;
                pr[7 * PC_LROW + r] = q2 * q2; pr[8 * PC_LROW + r] = q2;
            }
            __builtin_amdgcn_wave_barrier();                  // LDS is in order within a wave; keep the compiler in order too
#pragma unroll 8
            for (int r = 0; r < hits; ++r) M += mine[r];
            __builtin_amdgcn_wave_barrier();
            k += hits;
        }
    }
}

// bits of a key field that holds 0 .. kmax
static inline int pc_bits_for(int kmax)
{
    int b = 1;
    while ((1ll << b) <= (long long)kmax) ++b;
    return b;
}

// carves 256-byte aligned pieces out of one buffer; with base == nullptr it only measures
struct PcCarver {
    char* base;
    size_t used = 0;
    explicit PcCarver(void* b) : base(static_cast<char*>(b)) {}
    template <class T> T* take(size_t count)
    {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

struct gpc_patches {
    gpc_ctx* ctx = nullptr;
    gpc_patches_view v{};       // device pointers into `block`
    void* block = nullptr;      // one allocation holds every array of the batch
    // the voxel table the batch was cut with (gpc_registration assigns a scan's points to the same leaves): leaf id = patch id
    PcGrid grid{};
    const uint64_t* leaf_key = nullptr;   // P sorted unique voxel keys, in `block`
    uint64_t serial = 0;        // gpc_child_register
};

// ---- defined once in producer.hip, for every unit --------------------------------------------------------------------------------
// unregisters, frees and deletes a batch.  The caller holds ctx->mu (or the object was never published).
extern "C" void pc_patches_release(gpc_patches* o);

// The error paths of an entry that is building the batch `o` of context `ctx`: release it and fail.
#define PC_FAIL(...)                       \
    do {                                   \
        pc_patches_release(o);             \
        return gpc_fail(ctx, __VA_ARGS__); \
    } while (0)
#define PC_HIP_IN(entry, call)                                                                                                       \
    do {                                                                                                                             \
        hipError_t e_ = (call);                                                                                                      \
        if (e_ != hipSuccess)                                                                                                        \
            PC_FAIL(e_ == hipErrorOutOfMemory ? GPC_ENOMEM : GPC_EHIP, entry ": %s failed: %s", #call, hipGetErrorString(e_));        \
    } while (0)

// The host stages of a cutter, on ctx->stream; the caller holds ctx->mu.  Those that return hipError_t go into PC_HIP_IN.
// Bounds pass over n > 0 points, in the first 4096 bytes of the workspace: hb[0..2] = ordered min corner, hb[3..5] = ordered max corner
// (pc_unordered).  Refuses a non-finite coordinate (GPC_EINVAL).
int pc_cloud_bounds(gpc_ctx* ctx, const char* entry, const gpc_point_xyzrgb* cloud, int n, uint32_t hb[8]);

// scratch of the voxel table of n points: the caller carves it among its own and provides prim_bytes >= pc_voxel_table_prim_bytes
struct PcVoxelTable {
    uint64_t *k0, *keys;        // n: voxel keys in cloud order; sorted
    int32_t *v0, *vals;         // n: cloud index; in sorted order
    int32_t *head, *leaf_of;    // n: 1 where a voxel starts; leaf id per sorted position
    PcPoint* sp;                // n: the points in sorted order
    void carve(PcCarver& c, size_t n)
    {
        k0 = c.take<uint64_t>(n); keys = c.take<uint64_t>(n);
        v0 = c.take<int32_t>(n); vals = c.take<int32_t>(n);
        head = c.take<int32_t>(n); leaf_of = c.take<int32_t>(n);
        sp = c.take<PcPoint>(n);
    }
};
// rocPRIM's temporary storage for the sort and the scan of pc_voxel_table_build
hipError_t pc_voxel_table_prim_bytes(gpc_ctx* ctx, const PcGrid& g, size_t n, size_t* bytes);
// keys -> stable sort -> heads -> scan -> gather; *count = the number of occupied voxels, read back (the stream is idle on return)
hipError_t pc_voxel_table_build(gpc_ctx* ctx, const PcGrid& g, const gpc_point_xyzrgb* cloud, int n, const PcVoxelTable& T, void* prim,
                                size_t prim_bytes, int32_t* count);
// ... and, once the caller knows where they go: leaf_key[count] sorted unique keys, leaf_start[count + 1] their segments of T.sp
hipError_t pc_voxel_table_leaves(gpc_ctx* ctx, int n, const PcVoxelTable& T, int count, uint64_t* leaf_key, int32_t* leaf_start);

// the one layout of a batch's block: allocates o->block for P leaves of m cells and at most N points, sets o->v's pointers and o->leaf_key
hipError_t pc_patches_alloc(gpc_patches* o, size_t P, size_t N, size_t m);
// the tail of a cutter: reads off[P] and nmax_dev[0..2] (pc_nmax), fills the view, leaves the size classes with the context, registers o
hipError_t pc_patches_publish(gpc_ctx* ctx, gpc_patches* o, int P, const int32_t* nmax_dev);

// off[j] = first position of the sorted owners skey[0 .. n) that holds an owner >= j, j = 0 .. P: the exclusive scan of the per-leaf counts
// read off the sorted keys (no atomics); the unowned points (key P) sit behind off[P]
hipError_t pc_bucket_offsets(hipStream_t st, const uint32_t* skey, int n, int P, int32_t* off);
// nmax[0] = largest patch; nmax[1], nmax[2] = patches of <= 256 / <= 272 points: the size classes of the dense dispatch (dense_api.hip), which
// the host reads together with n_max and hands to it so that the class launches are sized exactly.  nmax[0..2] are zero on entry.
hipError_t pc_nmax(hipStream_t st, const int32_t* off, int P, int32_t* nmax);
