// sparse_predict.hip -- what reads a trained batch of sparse GPs (state layout: sparse.hip): predict on a shared grid or on every
// patch's own points (/root/reference/src/sparse_gp.hpp:299-351, sparse_gp_field.hpp:268-320), the likelihoods and their derivatives
// of the registration inner loop, and the live part of train_parameters.  Each kernel family with its LDS size and launcher.
#include <algorithm>
#include <cstdlib>

#include "sparse_internal.h"

struct SpPredParams {
    gpc_params prm;
    double c_exp;
    int P, ny, ld, m, conf;
    int fast;   // LDS holds a second [ld][SP_PC] buffer: V = C K by sp_ck_chunk
    const double *xs0, *xs1;
    const double *alpha, *C, *BV;
    const int32_t* b;
    double *f_star, *sigma;
    int32_t* status_out;
    const int32_t* stat;
    // ragged form (gpc_sparse_predict_points): patch i predicts at ITS OWN points off[i] .. off[i+1]-1 of xs0/xs1 and writes rows
    // off[i] .. of the output planes (plane stride n_total) -- predict_measurements(f, X_i, sigma) as the reference's training-set
    // RMS block calls it (/root/reference/src/gp_compressor.cpp:303-315).  nullptr: the shared grid of load_compressed.
    const int32_t* off;
    int n_total;
    int small_max;   // patches with at most this many basis vectors are the business of sparse_predict_small_kernel (-1: none)
};

#define SP_PC 32   // grid points per chunk of the sigma path

// V = C K for a chunk of SP_PC = 32 points on the MFMA pipe: C (b x b, global, column-major) times K (b x 32, LDS).
// v_mfma_f64_16x16x4_f64 with M = 16 rows of C, N = 16 points, K = 4 columns of C per instruction: the A operand of lane l
// is C[i0 + (l & 15)][j0 + (l >> 4)] (one 8-byte global load per lane, 16 contiguous rows per column), the B operand is
// K[j0 + (l >> 4)][p0 + (l & 15)] (one conflict-free LDS read).  Wave w owns the row tiles w, w+4, w+8, w+12 for both point
// tiles (8 accumulators); the loads of the next K-step are issued before the MFMAs of the current one, unconditionally
// (clamped addresses, masked values).  The result goes to LDS as Vc[row][point].  1300 MFMAs per chunk at b = 200.
// (The first version had every (point, column-group) thread walk its own columns of C with one broadcast global load and one
// LDS read per FMA: 1 TFLOP/s; a register-tiled VALU version was LDS-latency-bound with one wave per SIMD: 2.5 TFLOP/s.)
typedef double sp_d4 __attribute__((ext_vector_type(4)));
#define SP_RT 4   // row tiles per wave (4 waves x 4 x 16 rows = 256 = GPC_MAX_BV)
__device__ static inline void sp_ck_chunk(const double* __restrict__ Cg, int ld, int b, const double* Kc, double* Vc)
{
    // (workgroup-uniform, and no barrier below.)  An empty basis has no product and no row to clamp an address to: min(i, b - 1) = -1
    // sent the unconditional prefetch to Cg[-1 - ld], in front of the patch's matrix and, for patch 0, in front of the allocation.
    if (b <= 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int nrt = (b + 15) >> 4;
    sp_d4 acc[SP_RT][2];
#pragma unroll
    for (int t = 0; t < SP_RT; ++t) acc[t][0] = acc[t][1] = sp_d4{0.0, 0.0, 0.0, 0.0};
    int rowc[SP_RT];       // clamped row of this lane in tile t
    bool rowok[SP_RT];
#pragma unroll
    for (int t = 0; t < SP_RT; ++t) {
        const int i = 16 * (wave + 4 * t) + lr;
        rowok[t] = i < b;
        rowc[t] = min(i, b - 1);
    }
    // Round 4: the A operands of SP_PF K-steps are in flight (a K-step is 8 MFMAs = 512 cycles of the pipe per wave; with one step of
    // look-ahead every step waited out most of a ~2000-cycle load: the sigma path of a 200-vector basis ran at 0.18 of the FP64 peak)
    constexpr int SP_PF = 4;
    double an[SP_PF][SP_RT];
#pragma unroll
    for (int u = 0; u < SP_PF; ++u) {
        const int jc = min(4 * u + lg, b - 1);
#pragma unroll
        for (int t = 0; t < SP_RT; ++t) an[u][t] = Cg[rowc[t] + (size_t)jc * ld];
    }
    for (int jb = 0; jb < b; jb += 4 * SP_PF) {
#pragma unroll
        for (int u = 0; u < SP_PF; ++u) {
            const int j0 = jb + 4 * u;
            if (j0 < b) {                                  // (wave-uniform)
                const bool jok = j0 + lg < b;
                double ac[SP_RT];
#pragma unroll
                for (int t = 0; t < SP_RT; ++t) ac[t] = (jok && rowok[t]) ? an[u][t] : 0.0;
                {
                    const int jn = min(j0 + 4 * SP_PF + lg, b - 1);
#pragma unroll
                    for (int t = 0; t < SP_RT; ++t) an[u][t] = Cg[rowc[t] + (size_t)jn * ld];
                }
                const int jl = min(j0 + lg, b - 1);
                const double b0 = jok ? Kc[jl * SP_PC + lr] : 0.0;
                const double b1 = jok ? Kc[jl * SP_PC + 16 + lr] : 0.0;
#pragma unroll
                for (int t = 0; t < SP_RT; ++t) {
                    if (wave + 4 * t < nrt) {     // wave-uniform
                        acc[t][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[t], b0, acc[t][0], 0, 0, 0);
                        acc[t][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[t], b1, acc[t][1], 0, 0, 0);
                    }
                }
            }
        }
    }
    // C/D layout: lane l, register r = V[i0 + (l >> 4) + 4 r][p0 + (l & 15)]
#pragma unroll
    for (int t = 0; t < SP_RT; ++t) {
        if (wave + 4 * t < nrt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * (wave + 4 * t) + lg + 4 * r;
                if (i < b) {
                    Vc[i * SP_PC + lr] = acc[t][0][r];
                    Vc[i * SP_PC + 16 + lr] = acc[t][1][r];
                }
            }
        }
    }
}

__global__ __launch_bounds__(SP_THREADS) void sparse_predict_kernel(SpPredParams A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int ld = A.ld, ny = A.ny;
    double* T = reinterpret_cast<double*>(smem);   // 64
    double* bv = T + 64;                           // 2*ld
    double* al = bv + 2 * ld;                      // ny*ld
    int* clamp = reinterpret_cast<int*>(al + 3 * ld);   // 2 doubles of room
    double* racc = al + 3 * ld + 2;                // [8][SP_PC]
    double* Kc = racc + 8 * SP_PC;                 // [ld][SP_PC]   (sigma path only; LDS is sized for it only then)
    double* Vc = Kc + (size_t)ld * SP_PC;          // [ld][SP_PC]   (A.fast only)
    gpc_exp_table_init(T);
    const double sf = A.prm.sigmaf_sq, s20 = A.prm.noise;

    for (int patch = blockIdx.x; patch < A.P; patch += gridDim.x) {
        const int b = A.b[patch];
        if (b <= A.small_max) continue;                 // (workgroup-uniform, before any barrier) sparse_predict_small_kernel took it
        const double* Cg = A.C + (size_t)patch * ld * ld;
        __syncthreads();
        for (int i = tid; i < b; i += SP_THREADS) {
            bv[2 * i] = A.BV[(size_t)patch * ld * 2 + 2 * i];
            bv[2 * i + 1] = A.BV[(size_t)patch * ld * 2 + 2 * i + 1];
            for (int c = 0; c < ny; ++c) al[c * ld + i] = A.alpha[((size_t)patch * ny + c) * ld + i];
        }
        if (tid == 0) *clamp = 0;
        __syncthreads();
        const int po = A.off ? A.off[patch] : 0;                           // first point of this patch in xs0 / xs1
        const int m = A.off ? A.off[patch + 1] - po : A.m;
        const size_t fstride = A.off ? (size_t)A.n_total : (size_t)m;     // distance between the output planes
        const double* xs0 = A.xs0 + po;
        const double* xs1 = A.xs1 + po;
        double* fs = A.off ? A.f_star + po : A.f_star + (size_t)patch * ny * m;
        // mean: f = alpha^T k (:329); b == 0 -> 0 (:321-327)
        for (int p = tid; p < m; p += SP_THREADS) {
            const double q0 = xs0[p], q1 = xs1[p];
            double s[3] = {0.0, 0.0, 0.0};
            for (int i = 0; i < b; ++i) {
                const double k = gpc_rbf_neg(sf, A.c_exp, q0, q1, bv[2 * i], bv[2 * i + 1], T);
                for (int c = 0; c < ny; ++c) s[c] += al[c * ld + i] * k;
            }
            for (int c = 0; c < ny; ++c) fs[(size_t)c * fstride + p] = s[c];
        }
        if (A.sigma) {
            double* sg = A.off ? A.sigma + po : A.sigma + (size_t)patch * m;
            for (int p0 = 0; p0 < m; p0 += SP_PC) {
                const int pc = min(SP_PC, m - p0);
                __syncthreads();
                for (int e = tid; e < b * SP_PC; e += SP_THREADS) {
                    const int pp = e & (SP_PC - 1), i = e / SP_PC;
                    Kc[i * SP_PC + pp] = (pp < pc) ? gpc_rbf_neg(sf, A.c_exp, xs0[p0 + pp], xs1[p0 + pp], bv[2 * i], bv[2 * i + 1], T) : 0.0;
                }
                __syncthreads();
                if (A.fast) {
                    sp_ck_chunk(Cg, ld, b, Kc, Vc);
                    __syncthreads();
                }
                const int pp = tid & (SP_PC - 1), ig = tid / SP_PC;   // 8 row groups
                double acc = 0.0;
                for (int j = ig; j < b; j += SP_THREADS / SP_PC) {
                    // (C k)_j  (:330; C is symmetric)
                    double t = 0.0;
                    if (A.fast) t = Vc[j * SP_PC + pp];
                    else
                        for (int i = 0; i < b; ++i) t += Kc[i * SP_PC + pp] * Cg[i + (size_t)j * ld];
                    acc += t * Kc[j * SP_PC + pp];
                }
                racc[ig * SP_PC + pp] = acc;
                __syncthreads();
                if (tid < pc) {
                    const double kstar = sp_kstar(sf, xs0[p0 + tid], xs1[p0 + tid]);   // (:316)
                    double kCk = 0.0;
                    for (int q = 0; q < SP_THREADS / SP_PC; ++q) kCk += racc[q * SP_PC + tid];
                    double sigma = (b == 0) ? kstar + s20 : s20 + kstar + kCk;
                    if (sigma < 0) { sigma = 0; *clamp = 1; }                 // :334-337
                    if (A.conf) {
                        sigma /= kstar + s20;
                        sigma = (double)100.0f * ((double)1.0f - sigma);    // :340-345
                    } else {
                        sigma = sqrt(sigma);
                    }
                    sg[p0 + tid] = sigma;
                }
            }
        }
        __syncthreads();
        if (tid == 0 && A.status_out) {
            int st = A.stat[patch];
            if (st == GPC_STATUS_OK && *clamp) st = GPC_STATUS_SIGMA_CLAMPED;
            A.status_out[patch] = st;
        }
    }
}

// ---- predict with a SMALL basis: one wave per patch, a lane per grid point (round 4) ------------------------------------------------
// At the reference's default hyper-parameters a patch keeps ~13 basis vectors (8 .. 41 over a batch), and predict_measurements ALWAYS
// computes sigma = sqrt(s20 + k* + k^T C k) (/root/reference/src/sparse_gp.hpp:299-351; the caller drops it, src/gp_compressor.cpp:333-334).
// sparse_predict_kernel is shaped for a basis of 100 .. 200 -- a 256-thread workgroup per patch, chunks of 32 points, K and V = C K
// through LDS, the MFMA pipe, five barriers per chunk -- and at b = 13 its sigma path took 4.3 ms for 32768 patches (the mean 0.5 ms):
// 1.2 TFLOP/s on 6 GFLOP.  Here a lane owns a grid point: its b kernel values stay in registers (BM = 16 or 32 of them, zero beyond b),
// C sits in LDS zero-padded to BM x BM and is read by broadcast, the mean and k^T C k are register FMAs -- no barrier, no reduction, no
// second evaluation of k.  Mean: the same operations in the same order as sparse_predict_kernel (bit-identical); sigma: t_j = sum_i
// C_ij k_i, then sum_j t_j k_j, a summation order of its own, held by the tolerance against the oracle.  Patches with more than BM
// vectors are left to sparse_predict_kernel (SpPredParams::small_max), patches within the other instance's range to that one.
template <int BM>
__global__ __launch_bounds__(64) void sparse_predict_small_kernel(SpPredParams A, int b_lo)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* T = reinterpret_cast<double*>(smem);   // 64
    double* Cl = T + 64;                           // [BM][BM] column-major, zero-padded
    double* al = Cl + BM * BM;                     // [3][BM]
    double* bv = al + 3 * BM;                      // [BM][2]
    const int lane = threadIdx.x;
    const int ld = A.ld, ny = A.ny;
    gpc_exp_table_init(T);
    const double sf = A.prm.sigmaf_sq, s20 = A.prm.noise;
    for (int patch = blockIdx.x; patch < A.P; patch += gridDim.x) {
        const int b = __builtin_amdgcn_readfirstlane(A.b[patch]);
        if (b < b_lo || b > BM) continue;
        __builtin_amdgcn_wave_barrier();           // (one wave: LDS instructions execute in order; the compiler must keep them so)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const double* Cg = A.C + (size_t)patch * ld * ld;
        for (int e = lane; e < BM * BM; e += 64) {
            const int i = e % BM, j = e / BM;
            Cl[e] = (i < b && j < b) ? Cg[i + (size_t)j * ld] : 0.0;
        }
        if (lane < BM) {
            const bool in = lane < b;
            bv[2 * lane] = in ? A.BV[(size_t)patch * ld * 2 + 2 * lane] : 0.0;
            bv[2 * lane + 1] = in ? A.BV[(size_t)patch * ld * 2 + 2 * lane + 1] : 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) al[c * BM + lane] = (in && c < ny) ? A.alpha[((size_t)patch * ny + c) * ld + lane] : 0.0;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int po = A.off ? A.off[patch] : 0;
        const int m = A.off ? A.off[patch + 1] - po : A.m;
        const size_t fstride = A.off ? (size_t)A.n_total : (size_t)m;
        const double* xs0 = A.xs0 + po;
        const double* xs1 = A.xs1 + po;
        double* fs = A.off ? A.f_star + po : A.f_star + (size_t)patch * ny * m;
        double* sg = A.sigma ? (A.off ? A.sigma + po : A.sigma + (size_t)patch * m) : nullptr;
        bool clamped = false;
        // (the lane's grid coordinates are loaded per iteration, on purpose: holding a shared grid in registers -- 28 VGPRs, two waves per
        // SIMD less -- measured 1.24 against 1.12 ms for the sigma-predict of the defaults batch, staging it in LDS once per wave 1.30)
        double nq0 = 0.0, nq1 = 0.0;             // the NEXT 64 points' coordinates are requested before this block's arithmetic
        if (lane < m) { nq0 = xs0[lane]; nq1 = xs1[lane]; }
        for (int p = lane; p < m; p += 64) {
            const double q0 = nq0, q1 = nq1;
            if (p + 64 < m) { nq0 = xs0[p + 64]; nq1 = xs1[p + 64]; }
            double k[BM];
            double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < BM; ++i) {
                k[i] = 0.0;
                if (i < b) {                                    // (wave-uniform)
                    k[i] = gpc_rbf_neg(sf, A.c_exp, q0, q1, bv[2 * i], bv[2 * i + 1], T);
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (c < ny) s[c] += al[c * BM + i] * k[i];   // f = alpha^T k (:329), in sparse_predict_kernel's order
                }
            }
            for (int c = 0; c < ny; ++c) fs[(size_t)c * fstride + p] = s[c];
            if (sg) {
                double kCk = 0.0;
#pragma unroll
                for (int j = 0; j < BM; ++j) {
                    if (j < b) {                                // (wave-uniform)
                        double t = 0.0;
#pragma unroll
                        for (int i = 0; i < BM; ++i) t += k[i] * Cl[i + BM * j];     // (C k)_j (:330; rows beyond b are zero)
                        kCk += t * k[j];
                    }
                }
                // (:316; the point's coordinates are read again here: kept live from the top of the loop they cost a wave per SIMD)
                const double kstar = sp_kstar(sf, xs0[p], xs1[p]);
                double sigma = (b == 0) ? kstar + s20 : s20 + kstar + kCk;
                if (sigma < 0) { sigma = 0; clamped = true; }                 // :334-337
                if (A.conf) {
                    sigma /= kstar + s20;
                    sigma = (double)100.0f * ((double)1.0f - sigma);    // :340-345
                } else {
                    sigma = sqrt(sigma);
                }
                sg[p] = sigma;
            }
        }
        const bool any_clamp = __builtin_amdgcn_ballot_w64(clamped) != 0;
        if (lane == 0 && A.status_out) {
            int st = A.stat[patch];
            if (st == GPC_STATUS_OK && any_clamp) st = GPC_STATUS_SIGMA_CLAMPED;
            A.status_out[patch] = st;
        }
    }
}

// ---- registration inner loop: likelihoods and their derivatives on ragged point sets ----
// sparse_gp::compute_likelihoods -> likelihood (/root/reference/src/sparse_gp.hpp:387-427) and compute_derivatives ->
// likelihood_dx (:463-508) with rbf_kernel::kernel_dx (src/rbf_kernel.cpp:33-41); field variants
// src/sparse_gp_field.hpp:322-392.  Per point: k (b), v = C k (the O(b^2) part), then
//   sigma = s20 + k^T v + k**,  off = y - alpha^T k,  sigma_dx = 2 k_dx^T v,  k_dx row j = -(p0/p1) (x - BV_j) exp(..) = -(x - BV_j) k_j / p1
//   l = exp(-|off|^2 / (2 sigma)) / sqrt((2 pi)^ny sigma)
//   dX = exppart * (-sigma_dx + 2 (k_dx^T alpha) off + sigma_dx / sigma |off|^2),  exppart = exp(-|off|^2/(2 sigma)) / (2 sigma^1.5)
// Same work distribution as the sigma path of sparse_predict_kernel: chunks of SP_PC points, thread = (point, one of 8
// row groups of C), partial sums reduced through LDS.
struct SpLikParams {
    gpc_params prm;
    double c_exp;
    int P, ny, ld, n_total;
    int fast;   // LDS holds a second [ld][SP_PC] buffer: V = C K by sp_ck_chunk
    const int32_t* off;
    const double *x0, *x1, *y;
    const double *alpha, *C, *BV;
    const int32_t* b;
    double *dX, *l;
    double* raw;   // train_sigmaf pass (prm.sigmaf_sq == 1): per point e^T C e, alpha^T e, sum_j |x - BV_j|^2 e_j alpha_j
};
#define SP_NQ 12   // partial sums per thread: kCk, 2 x (k_dx^T v), ny x mu, 2 x ny x (k_dx^T alpha)

__global__ __launch_bounds__(SP_THREADS) void sparse_likelihood_kernel(SpLikParams A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int ld = A.ld, ny = A.ny;
    double* T = reinterpret_cast<double*>(smem);   // 64
    double* bv = T + 64;                           // 2*ld
    double* al = bv + 2 * ld;                      // 3*ld
    double* racc = al + 3 * ld;                    // [SP_NQ][8][SP_PC]
    double* Kc = racc + SP_NQ * 8 * SP_PC;         // [ld][SP_PC]
    double* Vc = Kc + (size_t)ld * SP_PC;          // [ld][SP_PC]   (A.fast only)
    gpc_exp_table_init(T);
    const double sf = A.prm.sigmaf_sq, s20 = A.prm.noise, inv_l = 1.0 / A.prm.l_sq;

    for (int patch = blockIdx.x; patch < A.P; patch += gridDim.x) {
        const int b = A.b[patch];
        const int o = A.off[patch], n = A.off[patch + 1] - o;
        const double* Cg = A.C + (size_t)patch * ld * ld;
        __syncthreads();
        for (int i = tid; i < b; i += SP_THREADS) {
            bv[2 * i] = A.BV[(size_t)patch * ld * 2 + 2 * i];
            bv[2 * i + 1] = A.BV[(size_t)patch * ld * 2 + 2 * i + 1];
            for (int c = 0; c < ny; ++c) al[c * ld + i] = A.alpha[((size_t)patch * ny + c) * ld + i];
        }
        for (int p0 = 0; p0 < n; p0 += SP_PC) {
            const int pc = min(SP_PC, n - p0);
            __syncthreads();
            for (int e = tid; e < b * SP_PC; e += SP_THREADS) {
                const int pp = e & (SP_PC - 1), i = e / SP_PC;
                Kc[i * SP_PC + pp] = (pp < pc) ? gpc_rbf_neg(sf, A.c_exp, A.x0[o + p0 + pp], A.x1[o + p0 + pp], bv[2 * i], bv[2 * i + 1], T) : 0.0;
            }
            __syncthreads();
            if (A.fast) {
                sp_ck_chunk(Cg, ld, b, Kc, Vc);
                __syncthreads();
            }
            const int pp = tid & (SP_PC - 1), ig = tid / SP_PC;   // 8 row groups
            const bool live = pp < pc;
            const double q0 = live ? A.x0[o + p0 + pp] : 0.0, q1 = live ? A.x1[o + p0 + pp] : 0.0;
            double acc[SP_NQ];
#pragma unroll
            for (int q = 0; q < SP_NQ; ++q) acc[q] = 0.0;
            for (int j = ig; j < b; j += SP_THREADS / SP_PC) {
                double t = 0.0;                                   // v_j = (C k)_j, C symmetric
                if (A.fast) t = Vc[j * SP_PC + pp];
                else
                    for (int i = 0; i < b; ++i) t += Kc[i * SP_PC + pp] * Cg[i + (size_t)j * ld];
                const double kj = Kc[j * SP_PC + pp];
                const double g0 = -(q0 - bv[2 * j]) * kj * inv_l, g1 = -(q1 - bv[2 * j + 1]) * kj * inv_l;   // k_dx row j
                acc[0] += t * kj;
                acc[1] += g0 * t;
                acc[2] += g1 * t;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c < ny) {
                        const double a = al[c * ld + j];
                        acc[3 + c] += a * kj;
                        acc[6 + c] += g0 * a;
                        acc[9 + c] += g1 * a;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < SP_NQ; ++q) racc[(q * 8 + ig) * SP_PC + pp] = acc[q];
            __syncthreads();
            if (tid < pc) {
                double r[SP_NQ];
#pragma unroll
                for (int q = 0; q < SP_NQ; ++q) {
                    double s_ = 0.0;
                    for (int w = 0; w < SP_THREADS / SP_PC; ++w) s_ += racc[(q * 8 + w) * SP_PC + tid];
                    r[q] = s_;
                }
                const double kstar = sp_kstar(sf, A.x0[o + p0 + tid], A.x1[o + p0 + tid]);
                double offv[3] = {0.0, 0.0, 0.0}, sq = 0.0;
                for (int c = 0; c < ny; ++c) {
                    offv[c] = A.y[(size_t)c * A.n_total + o + p0 + tid] - r[3 + c];
                    sq += offv[c] * offv[c];
                }
                if (A.l) {
                    const double sigma = s20 + kstar + r[0];                                    // :420-425
                    const double two_pi = (double)2.0f * 3.14159265358979323846;
                    const double norm = (ny == 1) ? two_pi * sigma : two_pi * two_pi * two_pi * sigma;
                    A.l[o + p0 + tid] = (double)1.0f / sqrt(norm) * exp((double)(-0.5f) / sigma * sq);
                }
                if (A.dX) {
                    const double sigma = s20 + r[0] + kstar;                                    // :485
                    const double sqrtsigma = sqrt(sigma);
                    const double exppart = (double)0.5f / (sigma * sqrtsigma) * exp((double)(-0.5f) / sigma * sq);
                    double* d = A.dX + (size_t)(o + p0 + tid) * 3;
                    for (int dd = 0; dd < 2; ++dd) {
                        const double sigma_dx = (double)2.0f * r[1 + dd];
                        double ko = 0.0;
                        for (int c = 0; c < ny; ++c) ko += r[6 + 3 * dd + c] * offv[c];
                        d[1 + dd] = exppart * (-sigma_dx + (double)2.0f * ko + sigma_dx / sigma * sq);
                    }
                    d[0] = (ny == 1) ? (double)(-1.0f) / (sigma * sqrtsigma) * offv[0] * exppart : 0.0;   // field: dx(0) = 0
                }
                if (A.raw) {
                    const double u0 = A.x0[o + p0 + tid], u1 = A.x1[o + p0 + tid];
                    double h = 0.0;
                    for (int j = 0; j < b; ++j) {
                        const double d0 = u0 - bv[2 * j], d1 = u1 - bv[2 * j + 1];
                        h += (d0 * d0 + d1 * d1) * Kc[j * SP_PC + tid] * al[j];
                    }
                    double* w = A.raw + (size_t)(o + p0 + tid) * 3;
                    w[0] = r[0]; w[1] = r[3]; w[2] = h;
                }
            }
        }
    }
}

// ---- row f4: the live part of sparse_gp::train_parameters (src/sparse_gp.hpp:586-640) ---------------------------------
// The inner do-loop holds the state (alpha, C, BV) fixed and moves only kernel.param()(0) = sigma_f^2 = p, and every
// quantity it evaluates is a polynomial in p over per-point sums that do not depend on p:
//     k = p e,   alpha^T k = p a_i,   k_dtheta(:,0)^T alpha = a_i,   k_dtheta(:,1)^T alpha = p 0.5f/p1^2 h_i,   k^T C k = p^2 q_i
// with e_j = exp(-0.5f/p1 |x_i - BV_j|^2), a_i = alpha^T e, h_i = sum_j |x_i - BV_j|^2 e_j alpha_j, q_i = e^T C e.  The O(n b^2)
// sums come from one pass of sparse_likelihood_kernel (MFMA C K) with sigma_f^2 = 1; the <= 102 iterations are then O(n)
// each and run here, one wave per patch.
struct SpTrainParams {
    int P, max_counter;
    double sf, l_sq, s20, step;
    const int32_t *off, *b;
    const double *raw, *y;
    double *p0, *ls, *delta;
    int32_t* iters;
};

__device__ static inline double sp_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);    // the same bits in every lane
    return v;
}

__global__ __launch_bounds__(SP_THREADS) void sparse_train_kernel(SpTrainParams A)
{
    const int lane = threadIdx.x & 63;
    const int patch = blockIdx.x * (SP_THREADS / 64) + (threadIdx.x >> 6);
    if (patch >= A.P) return;
    const int o = A.off[patch], n = A.off[patch + 1] - o;
    double p = A.sf, d0 = 0.0, d1 = 0.0;
    int iters = 0;
    if (A.b[patch] >= 20) {                                        // "if (first && BV.cols() < 20) return;"  (:609-611)
        const double logsqrt2pi = (double)0.5f * log((double)2.0f * 3.14159265358979323846);
        const double hc = (double)0.5f / (A.l_sq * A.l_sq);
        const double* raw = A.raw + (size_t)o * 3;
        const double* y = A.y + o;
        int counter = 0;
        do {
            d0 = d1 = 0.0;
            for (int i = lane; i < n; i += 64) {                   // likelihood_dtheta (:510-519), summed over the points (:619-623)
                const double a = raw[3 * i + 1], h = raw[3 * i + 2];
                const double r = p * a - y[i];
                d0 += r * a;
                d1 += r * (p * hc * h);
            }
            d0 = sp_wave_sum(d0);
            d1 = sp_wave_sum(d1);
            p += A.step * d0;                                      // :624
            double ls = 0.0;
            for (int i = lane; i < n; i += 64) {                   // log_likelihood (:356-385) with the updated parameter
                const double q = raw[3 * i], a = raw[3 * i + 1];
                const double mu = p * a, sigma = A.s20 + p + p * p * q;
                const double cent2 = (y[i] - mu) * (y[i] - mu);
                ls += -logsqrt2pi - (double)0.5f * log(sigma) - (double)0.5f * cent2 / sigma;
            }
            ls = sp_wave_sum(ls);
            if (lane == 0) A.ls[(size_t)patch * (A.max_counter + 2) + counter] = ls;
            iters = counter + 1;
            if (counter > A.max_counter) break;                    // :630-633
            ++counter;
        } while (sqrt(d0 * d0 + d1 * d1) > (double)1e-2f);         // :636 (a NaN gradient ends the loop as well)
    }
    if (lane == 0) {
        A.p0[patch] = p;
        A.iters[patch] = iters;
        A.delta[2 * patch] = d0;
        A.delta[2 * patch + 1] = d1;
    }
}

// ------------------------------------------------------------------------------------------------ host side

static size_t sp_lik_lds(int ld, bool fast)
{
    return sizeof(double) * (size_t)(64 + 5 * ld + SP_NQ * 8 * SP_PC + (size_t)ld * SP_PC * (fast ? 2 : 1));
}
static size_t sp_pred_lds(int ld, bool sigma, bool fast)
{
    return sizeof(double) * (size_t)(64 + 5 * ld + (sigma ? (size_t)ld * SP_PC * (fast ? 2 : 1) : 0) + 8 * SP_PC + 2);
}

// The predict launches: the two instances of the small-basis kernel (b <= 16, 17 .. 32) and sparse_predict_kernel for the rest (it skips what
// they took: A.small_max).  The three work on disjoint patches, and at the reference's defaults each is a short launch that ends in a tail of a few
// long patches: they run SIDE BY SIDE on the context's stream and its two copy streams (forked and joined with events; the streams exist since
// gpc_ctx_create).
int sp_predict_launch(gpc_sparse* g, int m, const int32_t* off, int n_total, const double* xs0, const double* xs1, double* f_star,
                      double* sigma, int conf, int32_t* status, int max_blocks)
{
    gpc_ctx* ctx = g->ctx;
    SpPredParams A;
    A.prm = g->prm;
    A.c_exp = (double)(-0.5f) / g->prm.l_sq;
    A.P = g->P; A.ny = g->ny; A.ld = g->ld; A.m = m; A.conf = conf;
    A.xs0 = xs0; A.xs1 = xs1; A.alpha = g->alpha; A.C = g->C; A.BV = g->BV; A.b = g->b;
    A.f_star = f_star; A.sigma = sigma; A.status_out = status; A.stat = g->stat;
    A.off = off; A.n_total = n_total;
    A.fast = (sigma != nullptr && sp_pred_lds(g->ld, true, true) <= 160u * 1024u) ? 1 : 0;
    const size_t lds = sp_pred_lds(g->ld, sigma != nullptr, A.fast != 0);
    // per call: the attribute is per device, and a process may hold contexts on several GPUs (idempotent, host-side only)
    GPC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(sparse_predict_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    int per_cu = (int)((160u * 1024u) / lds);
    per_cu = per_cu > max_blocks ? max_blocks : (per_cu < 1 ? 1 : per_cu);
    const int grid = std::min(g->P, ctx->num_cus * per_cu);
    A.small_max = -1;
    hipStream_t main_s = ctx->stream;
    if (getenv("GPC_SPARSE_NO_SMALL_PREDICT") || A.ld < 1) {
        hipLaunchKernelGGL(sparse_predict_kernel, dim3(grid), dim3(SP_THREADS), lds, main_s, A);
        GPC_HIP(ctx, hipGetLastError());
        return GPC_OK;
    }
    // (with sigma only: measured at the reference's defaults, 32768 patches -- sigma-predict 1.14 -> 0.84 ms; the mean-only launches are too
    // short to pay for the fork and join, 0.23 -> 0.28 ms)
    const bool fork = ctx->s_in && ctx->s_out && A.sigma != nullptr;
    hipStream_t s32 = fork ? ctx->s_in : main_s, sreg = fork ? ctx->s_out : main_s;
    // (the third launch goes to the context's OWN stream: the legacy default stream does not overlap its kernels with another stream's, and
    // a caller's stream may share a hardware queue with s_in or s_out -- dense_host.hip, dense_host; own_stream, s_in and s_out never do)
    hipStream_t s16 = (fork && ctx->own_stream) ? ctx->own_stream : main_s;
    if (fork) {
        GPC_HIP(ctx, hipEventRecord(ctx->ev[0][GPC_EV_SPARSE_FORK], main_s));
        GPC_HIP(ctx, hipStreamWaitEvent(s32, ctx->ev[0][GPC_EV_SPARSE_FORK], 0));
        GPC_HIP(ctx, hipStreamWaitEvent(sreg, ctx->ev[0][GPC_EV_SPARSE_FORK], 0));
        if (s16 != main_s) GPC_HIP(ctx, hipStreamWaitEvent(s16, ctx->ev[0][GPC_EV_SPARSE_FORK], 0));
    }
    const int waves = std::min(A.P, ctx->num_cus * 16);
    const size_t l16 = sizeof(double) * (size_t)(64 + 16 * 16 + 5 * 16), l32 = sizeof(double) * (size_t)(64 + 32 * 32 + 5 * 32);
    A.small_max = 32;
    // (the regular kernel first: its few patches are the longest)
    hipLaunchKernelGGL(sparse_predict_kernel, dim3(grid), dim3(SP_THREADS), lds, sreg, A);
    GPC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL((sparse_predict_small_kernel<32>), dim3(std::min(A.P, ctx->num_cus * 12)), dim3(64), l32, s32, A, 17);
    GPC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL((sparse_predict_small_kernel<16>), dim3(waves), dim3(64), l16, s16, A, 0);
    GPC_HIP(ctx, hipGetLastError());
    if (fork) {
        GPC_HIP(ctx, hipEventRecord(ctx->ev[1][GPC_EV_SPARSE_FORK], s32));
        GPC_HIP(ctx, hipEventRecord(ctx->ev[2][GPC_EV_SPARSE_FORK], sreg));
        GPC_HIP(ctx, hipStreamWaitEvent(main_s, ctx->ev[1][GPC_EV_SPARSE_FORK], 0));
        GPC_HIP(ctx, hipStreamWaitEvent(main_s, ctx->ev[2][GPC_EV_SPARSE_FORK], 0));
        if (s16 != main_s) {
            GPC_HIP(ctx, hipEventRecord(ctx->ev[1][GPC_EV_SPARSE_OWN], s16));
            GPC_HIP(ctx, hipStreamWaitEvent(main_s, ctx->ev[1][GPC_EV_SPARSE_OWN], 0));
        }
    }
    return GPC_OK;
}

int sp_likelihood_launch(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y,
                         double* dX, double* l, double* raw)
{
    gpc_ctx* ctx = sp_live(g);
    if (!ctx) return GPC_EINVAL;
    SpLikParams A;
    A.prm = g->prm;
    A.raw = raw;
    if (raw) A.prm.sigmaf_sq = 1.0;
    A.c_exp = (double)(-0.5f) / g->prm.l_sq;
    A.P = g->P; A.ny = g->ny; A.ld = g->ld; A.n_total = n_total;
    A.off = off; A.x0 = x0; A.x1 = x1; A.y = y;
    A.alpha = g->alpha; A.C = g->C; A.BV = g->BV; A.b = g->b;
    A.dX = dX; A.l = l;
    A.fast = (sp_lik_lds(g->ld, true) <= 160u * 1024u) ? 1 : 0;
    const size_t lds = sp_lik_lds(g->ld, A.fast != 0);
    // per call: the attribute is per device, and a process may hold contexts on several GPUs (idempotent, host-side only)
    GPC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(sparse_likelihood_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    int per_cu = (int)((160u * 1024u) / lds);
    per_cu = per_cu > 4 ? 4 : (per_cu < 1 ? 1 : per_cu);
    int grid = std::min(g->P, ctx->num_cus * per_cu);
    hipLaunchKernelGGL(sparse_likelihood_kernel, dim3(grid), dim3(SP_THREADS), lds, ctx->stream, A);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}

int sp_train_launch(gpc_sparse* g, const int32_t* off, const double* y, const double* raw, double step, int max_counter, double* p0,
                    int32_t* iters, double* ls, double* delta)
{
    gpc_ctx* ctx = g->ctx;
    SpTrainParams T;
    T.P = g->P; T.max_counter = max_counter;
    T.sf = g->prm.sigmaf_sq; T.l_sq = g->prm.l_sq; T.s20 = g->prm.noise; T.step = step;
    T.off = off; T.b = g->b; T.raw = raw; T.y = y;
    T.p0 = p0; T.ls = ls; T.delta = delta; T.iters = iters;
    const int wpb = SP_THREADS / 64;
    hipLaunchKernelGGL(sparse_train_kernel, dim3((g->P + wpb - 1) / wpb), dim3(SP_THREADS), 0, ctx->stream, T);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}
