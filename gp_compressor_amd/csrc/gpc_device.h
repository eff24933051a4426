// gpc_device.h -- device-side helpers shared by the dense and sparse kernels (gfx950, wave64).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#define GPC_WAVE 64

// ---------------------------------------------------------------------------------------------------------
// exp() for the RBF kernel.  Table-driven (Tang): x = (64 e + j) ln2/64 + r, |r| <= ln2/128,
// exp(x) = 2^e * T[j] * (1 + p(r)), p of degree 5 (truncation r^6/720 < 3.5e-17).  Max error ~1 ulp, which is
// the same class as glibc's exp the reference calls (src/rbf_kernel.cpp:17); parity is stated as a tolerance.
// The table (64 doubles = 512 B) is staged into LDS once per workgroup by gpc_exp_table_init().
// Compiles for host as well so that the CPU test-suite can check its accuracy without a GPU.
// ---------------------------------------------------------------------------------------------------------
#define GPC_EXP_TABLE_SIZE 64

// one copy per translation unit (no -fgpu-rdc); 512 B
static __constant__ double c_gpc_exp_table[GPC_EXP_TABLE_SIZE] = {
#include "gpc_exp_table.inc"
};
static const double h_gpc_exp_table[GPC_EXP_TABLE_SIZE] = {
#include "gpc_exp_table.inc"
};

__host__ __device__ static inline double gpc_exp_tbl(double x, const double* __restrict__ T)
{
    const double INV_LN2_64 = 92.332482616893656768;        // 64 / ln 2
    const double LN2_64_HI = 0x1.62e42fef80000p-7;           // ln2/64 rounded to 34 bits: n * hi is exact for |n| < 2^19
    const double LN2_64_LO = 0x1.1cf79abc9e3b4p-42;          // ln2/64 - hi
    // clamp: outside [-760, 720] the result is 0 / inf anyway; keeps the int conversion in range. NaN falls through.
    double xc = x < -760.0 ? -760.0 : (x > 720.0 ? 720.0 : x);
    double nd = __builtin_rint(xc * INV_LN2_64);
    int n = (int)nd;
    double r = __builtin_fma(-nd, LN2_64_HI, xc);
    r = __builtin_fma(-nd, LN2_64_LO, r);
    int j = n & (GPC_EXP_TABLE_SIZE - 1);
    int e = n >> 6;
    double p = __builtin_fma(r, 1.0 / 120.0, 1.0 / 24.0);
    p = __builtin_fma(r, p, 1.0 / 6.0);
    p = __builtin_fma(r, p, 0.5);
    double r2 = r * r;
    p = __builtin_fma(r2, p, r);          // r + r^2 (1/2 + r/6 + r^2/24 + r^3/120)
    double t = T[j];
    double v = __builtin_fma(t, p, t);
#if defined(__HIP_DEVICE_COMPILE__)
    v = __builtin_amdgcn_ldexp(v, e);     // v_ldexp_f64: correct gradual underflow / overflow to inf
#else
    v = __builtin_ldexp(v, e);
#endif
    return (x != x) ? x : v;
}

// exp(x) for x <= 0 (the RBF exponent): same algorithm without the upper clamp and the NaN select (a NaN argument
// still comes out as NaN: r and therefore p are NaN).
__device__ static inline double gpc_exp_neg(double x, const double* __restrict__ T)
{
    const double INV_LN2_64 = 92.332482616893656768;
    const double LN2_64_HI = 0x1.62e42fef80000p-7;
    const double LN2_64_LO = 0x1.1cf79abc9e3b4p-42;
    const double xc = x < -760.0 ? -760.0 : x;
    const double nd = __builtin_rint(xc * INV_LN2_64);
    const int n = (int)nd;
    double r = __builtin_fma(-nd, LN2_64_HI, xc);
    r = __builtin_fma(-nd, LN2_64_LO, r);
    double p = __builtin_fma(r, 1.0 / 120.0, 1.0 / 24.0);
    p = __builtin_fma(r, p, 1.0 / 6.0);
    p = __builtin_fma(r, p, 0.5);
    p = __builtin_fma(r * r, p, r);
    const double t = T[n & (GPC_EXP_TABLE_SIZE - 1)];
    return __builtin_amdgcn_ldexp(__builtin_fma(t, p, t), n >> 6);
}

// exp(x) for -2^-5 <= x <= 0: the degree-7 Taylor polynomial, no table and no range reduction (truncation
// x^8/8! <= 2.3e-17 relative, i.e. below half an ulp; measured <= 1 ulp vs libm, tests/test_capi_cpu.py).  This is the
// regime of a GP patch model whose length scale exceeds the patch (c d^2 = -d^2 / (2 l^2) is tiny): a third of the
// instructions of the table-driven path and no LDS access.  Callers prove the argument range from a bound on the patch
// extent (dense_mfma.hip) and fall back to gpc_exp_neg otherwise.
#define GPC_EXP_SMALL_MAX 0.03125
__host__ __device__ static inline double gpc_exp_small(double x)
{
    double p = __builtin_fma(x, 1.0 / 5040.0, 1.0 / 720.0);
    p = __builtin_fma(x, p, 1.0 / 120.0);
    p = __builtin_fma(x, p, 1.0 / 24.0);
    p = __builtin_fma(x, p, 1.0 / 6.0);
    p = __builtin_fma(x, p, 0.5);
    p = __builtin_fma(x, p, 1.0);
    return __builtin_fma(x, p, 1.0);
}

// exp(-t) for 0 <= t <= 2^-5 (DEG 7) / 0 <= t <= 2^-8 (DEG 5): Taylor polynomials with literal coefficients (truncation t^8/8! <= 2.3e-17,
// t^6/6! <= 4.9e-18: below a tenth of an ulp of the result, which is ~1).  Callers hold coordinates pre-scaled by sqrt(-c), so that the
// squared distance IS t: distance (4 operations) + 5 or 7 FMAs per kernel value, no multiplication by c (one-wave dense kernel, round 4).
#define GPC_EXP_TINY_MAX 0.00390625
template <int DEG>
__host__ __device__ static inline double gpc_expm_poly(double t)
{
    double p;
    if (DEG == 7) {
        p = __builtin_fma(t, -1.0 / 5040.0, 1.0 / 720.0);
        p = __builtin_fma(t, p, -1.0 / 120.0);
        p = __builtin_fma(t, p, 1.0 / 24.0);
    } else {
        p = __builtin_fma(t, -1.0 / 120.0, 1.0 / 24.0);
    }
    p = __builtin_fma(t, p, -1.0 / 6.0);
    p = __builtin_fma(t, p, 0.5);
    p = __builtin_fma(t, p, -1.0);
    return __builtin_fma(t, p, 1.0);
}

__device__ static inline void gpc_exp_table_init(double* T_lds)
{
    for (int i = threadIdx.x; i < GPC_EXP_TABLE_SIZE; i += blockDim.x) T_lds[i] = c_gpc_exp_table[i];
}

// RBF / squared-exponential kernel.  c = (double)(-0.5f) / l_sq is formed on the host exactly like the reference
// evaluates `-0.5f / p(1)` (src/rbf_kernel.cpp:17, src/gaussian_process.cpp:49); sf = sigma_f^2.
__device__ static inline double gpc_rbf(double sf, double c, double xi0, double xi1, double xj0, double xj1, const double* T)
{
    double d0 = xi0 - xj0, d1 = xi1 - xj1;
    double sq = __builtin_fma(d0, d0, d1 * d1);   // explicit: left to the compiler, WHICH product is fused differs from one inlining context to the next
    return sf * gpc_exp_tbl(c * sq, T);
}

// same with the x <= 0 exponential (c < 0 because l_sq > 0 is checked by the API)
__device__ static inline double gpc_rbf_neg(double sf, double c, double xi0, double xi1, double xj0, double xj1, const double* T)
{
    double d0 = xi0 - xj0, d1 = xi1 - xj1;
    double sq = __builtin_fma(d0, d0, d1 * d1);   // explicit: left to the compiler, WHICH product is fused differs from one inlining context to the next
    return sf * gpc_exp_neg(c * sq, T);
}

// k(x*, x*) of the predictive variance (gaussian_process::predict_measurements, src/gaussian_process.cpp:40): sf exp(c |x* - x*|^2) is sf
// for a finite x* (x - x = +0 and exp(0) is exactly 1: finite data keeps its bits) and NaN when a coordinate is NaN or +-inf (x - x = NaN),
// as the reference's own evaluation gives it.  No select, three operations per prediction point (sp_kstar is the sparse path's twin).
__device__ static inline double gpc_kss(double sf, double x0, double x1) { return sf + ((x0 - x0) + (x1 - x1)); }

__device__ static inline double gpc_rbf_small(double sf, double c, double xi0, double xi1, double xj0, double xj1)
{
    double d0 = xi0 - xj0, d1 = xi1 - xj1;
    double sq = __builtin_fma(d0, d0, d1 * d1);   // explicit: left to the compiler, WHICH product is fused differs from one inlining context to the next
    return sf * gpc_exp_small(c * sq);
}

// ---------------------------------------------------------------------------------------------------------
// flatten_colors (src/gp_compressor.cpp:251-265) of one value, shared by reproject.hip and render.hip:
// x.cast<short>() as the x86-64 reference binary evaluates it (cvttsd2si, then truncation to 16 bits), then the clamp
// ---------------------------------------------------------------------------------------------------------
__device__ static inline uint8_t rp_flatten(double x)
{
    if (x != x || __builtin_isinf(x)) return 255;
    const int w = (x >= 2147483648.0 || x < -2147483648.0) ? (int)0x80000000 : (int)x;     // (int)x truncates toward zero
    const int v = (int)(short)(unsigned short)(unsigned)w;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---------------------------------------------------------------------------------------------------------
// The scalar quantiser of the bit-packed model (include/gpc.h, gpc_sparse_quantize_rd): one definition for the search kernel, the decoder
// kernel and the host (gpc_test_quantize_host).  An array v[0..b) of finite doubles at width w in 1..16:
//     lo = the largest float <= min v, hi = the smallest float >= max v      (they do not depend on w)
//     step = (hi - lo) / (2^w - 1);   q_i = step > 0 ? clamp(rint((v_i - lo) / step), 0, 2^w - 1) : 0;   v'_i = lo + q_i * step
// Every operation is rounded once (contraction off inside these bodies), so that tests/quantize_ref.py reproduces the bits.
// ---------------------------------------------------------------------------------------------------------
__host__ __device__ static inline float gpc_q_lo(double vmin)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2float_rd(vmin);
#else
    const float f = (float)vmin;
    return (double)f > vmin ? __builtin_nextafterf(f, -__builtin_inff()) : f;
#endif
}

__host__ __device__ static inline float gpc_q_hi(double vmax)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2float_ru(vmax);
#else
    const float f = (float)vmax;
    return (double)f < vmax ? __builtin_nextafterf(f, __builtin_inff()) : f;
#endif
}

__host__ __device__ static inline double gpc_q_step(float lo, float hi, int w)
{
#pragma clang fp contract(off)
    return ((double)hi - (double)lo) / (double)((1 << w) - 1);
}

__host__ __device__ static inline uint16_t gpc_q_code(double v, float lo, double step, int w)
{
#pragma clang fp contract(off)
    if (!(step > 0.0)) return 0;
    const double qmax = (double)((1 << w) - 1);
    const double r = __builtin_rint((v - (double)lo) / step);      // round-half-even
    return (uint16_t)(!(r > 0.0) ? 0.0 : (r > qmax ? qmax : r));
}

__host__ __device__ static inline double gpc_q_value(uint16_t q, float lo, double step)
{
#pragma clang fp contract(off)
    const double t = (double)q * step;
    return (double)lo + t;
}

// ---------------------------------------------------------------------------------------------------------
// The allocation rule of the byte budget (include/gpc.h, gpc_rate_allocate): one definition for the kernels (rate_alloc.hip) and the host
// (gpc_test_rate_allocate_host).  Row r offers k = 0 .. kmax removals; the cost of an option at the multiplier lambda is
//     c(k) = w e(k) + (rate(k) == 0 ? 0.0 : lambda (double)rate(k)),     rate(k) = unit (kmax - k)  (int64)
// with the product and the sum rounded once each (contraction off).  The choice is the largest k that attains the minimum over the options
// whose cost is not NaN (0 for a row whose c(0) is NaN): gpc_ra_take is that order, so a sequential scan and any reduction tree agree.
// ---------------------------------------------------------------------------------------------------------
#define GPC_RA_UNDECIDED 0
#define GPC_RA_INFEASIBLE 1    // S(+inf) < need
#define GPC_RA_FREE 2          // S(0) >= need
#define GPC_RA_BISECT 3

// which multiplier an evaluation sweep uses, and which total of the state it adds to
#define GPC_RA_AT_INF 0
#define GPC_RA_AT_ZERO 1
#define GPC_RA_AT_MID 2
#define GPC_RA_AT_HI 3         // the final multiplier: k_hi
#define GPC_RA_AT_LO 4         // the bracket's lower end (refinement; else the final multiplier again): k_lo

// the bracket and the totals of one call (device memory in the _dev entry: no sweep's launch depends on a value read back)
struct gpc_ra_state {
    unsigned long long lo, hi;          // bit patterns of the bracket's ends
    long long need;
    long long s[5];                     // S at the multiplier of each GPC_RA_AT_*; s[GPC_RA_AT_MID] is cleared after every sweep
    long long saved_ref;                // the saving of the refined choice
    int mode, refine;
    int switched_ref, switched_all;     // rows with k != k_lo under the refined choice / under k_hi
    int fallback;                       // the refined choice missed `need`: k = k_hi
};

__host__ __device__ static inline double gpc_ra_from_bits(unsigned long long b)
{
    double v;
    __builtin_memcpy(&v, &b, sizeof v);
    return v;
}

__host__ __device__ static inline int gpc_ra_kmax(int kmax, int ld) { return kmax < 0 ? 0 : (kmax > ld ? ld : kmax); }
__host__ __device__ static inline int gpc_ra_unit(const int32_t* unit, int unit_all, int r)
{
    const int u = unit ? unit[r] : unit_all;
    return u < 1 ? 1 : u;
}

__host__ __device__ static inline double gpc_ra_cost(double w, double e, long long rate, double lambda)
{
#pragma clang fp contract(off)
    const double D = w * e;
    const double t = rate == 0 ? 0.0 : lambda * (double)rate;
    return D + t;
}

// does option (c, k) replace the best so far (cb, kb)?  kb < 0: there is none yet.  c is not NaN.
__host__ __device__ static inline bool gpc_ra_take(double c, int k, double cb, int kb)
{
    return kb < 0 || c < cb || (c == cb && k > kb);
}

// the row's choice by the sequential scan (the host twin; the kernel strides the options over a wave and merges with gpc_ra_take)
__host__ __device__ static inline int gpc_ra_choice(int kmax, double d0, const double* d, double w, int unit, double lambda)
{
    const double c0 = gpc_ra_cost(w, d0, (long long)unit * kmax, lambda);
    if (c0 != c0) return 0;
    double cb = c0;
    int kb = 0;
    for (int k = 1; k <= kmax; ++k) {
        const double c = gpc_ra_cost(w, d[k - 1], (long long)unit * (kmax - k), lambda);
        if (c == c && gpc_ra_take(c, k, cb, kb)) { cb = c; kb = k; }
    }
    return kb;
}

__host__ __device__ static inline void gpc_ra_init(gpc_ra_state* s, long long need, int refine)
{
    s->lo = 0ull;                       // bits(0.0)
    s->hi = 0x7ff0000000000000ull;      // bits(+inf)
    s->need = need;
    for (int i = 0; i < 5; ++i) s->s[i] = 0;
    s->saved_ref = 0;
    s->mode = GPC_RA_UNDECIDED;
    s->refine = refine != 0;
    s->switched_ref = s->switched_all = s->fallback = 0;
}

// is the sweep `at` still to be done, and at which multiplier?
__host__ __device__ static inline bool gpc_ra_sweep(const gpc_ra_state* s, int at, double* lambda)
{
    const double inf = gpc_ra_from_bits(0x7ff0000000000000ull);
    switch (at) {
    case GPC_RA_AT_INF: *lambda = inf; return true;
    case GPC_RA_AT_ZERO: *lambda = 0.0; return true;
    case GPC_RA_AT_MID:
        if (s->mode != GPC_RA_BISECT || s->hi - s->lo <= 1ull) return false;
        *lambda = gpc_ra_from_bits(s->lo + (s->hi - s->lo) / 2ull);
        return true;
    default: {
        const double fin = s->mode == GPC_RA_INFEASIBLE ? inf : (s->mode == GPC_RA_FREE ? 0.0 : gpc_ra_from_bits(s->hi));
        *lambda = (at == GPC_RA_AT_LO && s->mode == GPC_RA_BISECT && s->refine) ? gpc_ra_from_bits(s->lo) : fin;
        return true;
    }
    }
}

// after the two end points: which case is it?
__host__ __device__ static inline void gpc_ra_decide(gpc_ra_state* s)
{
    s->mode = s->s[GPC_RA_AT_INF] < s->need ? GPC_RA_INFEASIBLE : (s->s[GPC_RA_AT_ZERO] >= s->need ? GPC_RA_FREE : GPC_RA_BISECT);
}

// after a sweep at mid: move one end (a no-op once the bracket has closed, or outside the bisection)
__host__ __device__ static inline void gpc_ra_update(gpc_ra_state* s)
{
    if (s->mode == GPC_RA_BISECT && s->hi - s->lo > 1ull) {
        const unsigned long long mid = s->lo + (s->hi - s->lo) / 2ull;
        if (s->s[GPC_RA_AT_MID] >= s->need) s->hi = mid;
        else s->lo = mid;
    }
    s->s[GPC_RA_AT_MID] = 0;
}

// the row's final count from the exclusive scan E of unit (k_hi - k_lo), started at S(lo)
__host__ __device__ static inline int gpc_ra_pick(long long E, long long need, int k_hi, int k_lo) { return E < need ? k_hi : k_lo; }

// ---------------------------------------------------------------------------------------------------------
// wave / block reductions
// ---------------------------------------------------------------------------------------------------------
__device__ static inline double gpc_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum through LDS scratch (>= blockDim.x/64 doubles); every thread gets the result
__device__ static inline double gpc_block_sum(double v, double* scratch)
{
    v = gpc_wave_sum(v);
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[w] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += scratch[i];
    return s;
}

// ---------------------------------------------------------------------------------------------------------
// Noise functors: the duck-typed Noise contract of the reference, q = dx_ln(y, x, sigma_x) = d/dx ln P(y|x) and
// r = dx2_ln(y, x, sigma_x) = d2/dx2 ln P(y|x)   (/root/reference/src/gaussian_noise.h:7-10, src/probit_noise.h).
// One definition for every kernel that needs them (sparse add, the dense IRLS loop, gpc_noise_eval).
// ---------------------------------------------------------------------------------------------------------
#define GPC_NOISE_GAUSSIAN 0
#define GPC_NOISE_PROBIT_REF 1   // probit_noise as written: "Phi"(z) = erf(z) / (2.0f*sqrt(2.0f))   (src/probit_noise.cpp:15,26)
#define GPC_NOISE_PROBIT_STD 2   // the fix: Phi(z) = (1 + erf(z / sqrt 2)) / 2, a CDF; everything else as upstream

// gaussian_noise::dx_ln / dx2_ln   (/root/reference/src/gaussian_noise.cpp:9-18)
__device__ static inline void gpc_gaussian_q_r(double s20, double y, double x, double sigma_x, double* q, double* r)
{
    *q = (y - x) / (s20 + sigma_x);
    *r = (double)(-1.0f) / (s20 + sigma_x);
}

// probit_noise::dx_ln / dx2_ln   (/root/reference/src/probit_noise.cpp:11-31), operation for operation.  `2.0f*sqrt(2.0f)`
// is a float product upstream (the sqrt(float) overload), checked against the compiled reference object in
// tests/golden/noise_ref.json; exp(-z*z/2) and sqrt(2.0f*M_PI) are double.  model == GPC_NOISE_PROBIT_STD swaps the
// one expression that is wrong upstream (ef) and keeps the rest.
// ef: the functor's "Phi"(z).  With model == GPC_NOISE_PROBIT_STD it is the probability P(y | x) at z = y x / sqrt(s20 + sigma_x) --
// what the occupancy read-out reports at sigma_x = the latent predictive variance (dense_variance.hip).
__device__ static inline double gpc_probit_ef(int model, double z)
{
    return (model == GPC_NOISE_PROBIT_STD) ? 0.5 * erfc(-z * 0.70710678118654752440) : erf(z) / (double)(2.0f * 1.41421354f);
}

__device__ static inline void gpc_probit_q_r(int model, double s20, double y, double x, double sigma_x, double* q, double* r)
{
    const double sigma2 = s20 + sigma_x;
    const double sigma = sqrt(sigma2);
    const double z = y * x / sigma;
    const double ef = gpc_probit_ef(model, z);
    const double efprim = exp(-z * z / 2.0) / sqrt(2.0 * 3.14159265358979323846);
    *q = y / sigma * efprim / ef;                                 // :17
    const double efprimprim = -z * efprim;                        // :28
    const double first = efprim / ef;                             // :29
    *r = (efprimprim / ef - first * first) / sigma2;              // :30
}

// ---- the evidence read-outs (dense_evidence.hip, and the generic kernel's own in dense_generic.hip): the one order of their sums ------
// the 64 lanes' values in one fixed order; every lane gets the sum
__device__ static __forceinline__ double ev_wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
#define EV_HALF_LOG_2PI 0.91893853320467274178   // 0.5 log(2 pi)
