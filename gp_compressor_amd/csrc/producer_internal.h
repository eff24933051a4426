// producer_internal.h -- what producer.hip (gpc_project_cloud) shares with registration.hip (gpc_registration_*) and mapping.hip
// (gpc_patches_insert_cloud): the voxel grid of a patch batch, the key arithmetic of its leaf table, the plane frame of a search
// sphere's moment matrix, and the batch object itself.
#pragma once

#include <cmath>

#include "gpc_internal.h"

// Both translation units are bit-exact against CPU restatements: floating-point contraction is off from here to their end, and
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

__device__ static inline int pc_find_leaf(const uint64_t* leaf_key, int P, uint64_t key)
{
    int lo = 0, hi = P;                       // first element >= key
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (leaf_key[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < P && leaf_key[lo] == key) ? lo : -1;
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

// ---- the stages both cutters run: bounds, voxel keys, leaf table of the sorted keys, sorted-order copy (launch sites: producer.hip,
// mapping.hip)
// out[0..2] = ordered min, out[3..5] = ordered max, out[6] = 1 if a coordinate is not finite
static __global__ __launch_bounds__(PC_THREADS) void pc_bounds_kernel(const gpc_point_xyzrgb* cloud, int n, uint32_t* out)
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

static __global__ __launch_bounds__(PC_THREADS) void pc_keys_kernel(PcGrid g, const gpc_point_xyzrgb* cloud, int n, uint64_t* keys, int32_t* vals)
{
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= n) return;
    const float4 p = *reinterpret_cast<const float4*>(&cloud[i]);
    int k[3];
    pc_voxel(g, p.x, p.y, p.z, k);
    keys[i] = pc_pack(g, k[0], k[1], k[2]);
    vals[i] = i;
}

static __global__ __launch_bounds__(PC_THREADS) void pc_heads_kernel(const uint64_t* keys, int n, int32_t* head)
{
    const int s = blockIdx.x * PC_THREADS + threadIdx.x;
    if (s < n) head[s] = (s == 0 || keys[s] != keys[s - 1]) ? 1 : 0;
}

// leaf_of[s] holds the inclusive scan of head[] on entry (leaf id + 1) and the leaf id on exit
static __global__ __launch_bounds__(PC_THREADS) void pc_leaves_kernel(const uint64_t* keys, int n, int P, int32_t* leaf_of, uint64_t* leaf_key,
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

// points re-laid in sorted order
static __global__ __launch_bounds__(PC_THREADS) void pc_gather_kernel(const gpc_point_xyzrgb* cloud, const int32_t* vals, int n, PcPoint* sp)
{
    const int s = blockIdx.x * PC_THREADS + threadIdx.x;
    if (s >= n) return;
    const gpc_point_xyzrgb* q = &cloud[vals[s]];
    const float4 p = *reinterpret_cast<const float4*>(q);
    const uint32_t c = *reinterpret_cast<const uint32_t*>(&q->b);     // b | g << 8 | r << 16 | a << 24
    PcPoint o;
    o.x = p.x; o.y = p.y; o.z = p.z;
    o.rgb = ((c >> 16) & 0xffu) | (c & 0xff00u) | ((c & 0xffu) << 16);
    *reinterpret_cast<float4*>(&sp[s]) = *reinterpret_cast<const float4*>(&o);
}

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

// producer.hip: unregisters, frees and deletes a batch.  The caller holds ctx->mu (or the object was never published).
extern "C" void pc_patches_release(gpc_patches* o);
