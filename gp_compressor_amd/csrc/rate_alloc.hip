// rate_alloc.hip -- rate control to a byte budget: how many removals each row (one GP of one leaf) takes so that a number of bytes is saved
// at the smallest total weighted error (include/gpc.h, gpc_rate_allocate).  The rule itself -- cost, tie order, bracket -- is in gpc_device.h,
// shared with the host twin at the end of this file.  The _dev entry enqueues a fixed sequence and reads nothing back: the two end points,
// 63 sweeps at the bracket's middle (no-ops once it has closed), k_hi and k_lo, the scan of the marginal rows, the write-out.
#include "gpc_internal.h"
#include "gpc_device.h"

#include <algorithm>

namespace {

constexpr int RA_BLOCK = 256;                   // threads of every kernel here: 4 rows per workgroup in a sweep, one scan tile of 256 rows
constexpr int RA_WAVES = RA_BLOCK / GPC_WAVE;

struct ra_rows {
    int R, ld;
    const int32_t* kmax;
    const double *d0, *d, *w;
    double w_all;
    const int32_t* unit;
    int unit_all;
};

__global__ void ra_init_kernel(gpc_ra_state* st, long long need, int refine) { gpc_ra_init(st, need, refine); }
// step 0: after the two end points; step 1: after a sweep at the middle
__global__ void ra_step_kernel(gpc_ra_state* st, int step)
{
    if (step == 0) gpc_ra_decide(st);
    else gpc_ra_update(st);
}

// One wave per row, lanes striding the options; the arg-min through a fixed xor tree (gpc_ra_take is a total order on distinct k, so every
// lane ends with the same pair); the wave's unit * k, summed over its rows, goes into the state's int64 total with one atomic.
__global__ __launch_bounds__(RA_BLOCK) void ra_eval_kernel(ra_rows a, gpc_ra_state* st, int at, int32_t* __restrict__ kout)
{
    double lambda;
    if (!gpc_ra_sweep(st, at, &lambda)) return;
    const int lane = threadIdx.x & (GPC_WAVE - 1), wave = threadIdx.x >> 6;
    long long total = 0;
    for (long long r = (long long)blockIdx.x * RA_WAVES + wave; r < a.R; r += (long long)gridDim.x * RA_WAVES) {
        const int km = gpc_ra_kmax(a.kmax[r], a.ld), u = gpc_ra_unit(a.unit, a.unit_all, (int)r);
        const double wr = a.w ? a.w[r] : a.w_all, e0 = a.d0[r];
        const double* dr = a.d + (size_t)r * (size_t)a.ld;
        double cb = 0.0;
        int kb = -1;
        for (int k = lane; k <= km; k += GPC_WAVE) {
            const double c = gpc_ra_cost(wr, k == 0 ? e0 : dr[k - 1], (long long)u * (km - k), lambda);
            if (c == c && gpc_ra_take(c, k, cb, kb)) { cb = c; kb = k; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double co = __shfl_xor(cb, o, GPC_WAVE);
            const int ko = __shfl_xor(kb, o, GPC_WAVE);
            if (ko >= 0 && gpc_ra_take(co, ko, cb, kb)) { cb = co; kb = ko; }
        }
        const double c0 = gpc_ra_cost(wr, e0, (long long)u * km, lambda);
        const int choice = (c0 != c0 || kb < 0) ? 0 : kb;      // a NaN c(0): the row is fixed
        if (lane == 0 && kout) kout[r] = choice;
        total += (long long)u * choice;
    }
    // one atomic per workgroup: a single word takes well under a hundred atomics per microsecond, which would bound a sweep of thousands of waves
    __shared__ long long part[RA_WAVES];
    if (lane == 0) part[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long sum = 0;
        for (int i = 0; i < RA_WAVES; ++i) sum += part[i];
        if (sum != 0) atomicAdd((unsigned long long*)&st->s[at], (unsigned long long)sum);
    }
}

// inclusive scan of one int64 per thread over the workgroup; *total gets the workgroup's sum.  lds: RA_WAVES entries.
__device__ static inline long long ra_block_scan(long long v, long long* lds, long long* total)
{
    const int lane = threadIdx.x & (GPC_WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < GPC_WAVE; o <<= 1) {
        const long long t = __shfl_up(v, o, GPC_WAVE);
        if (lane >= o) v += t;
    }
    __syncthreads();                    // the previous use of lds is over
    if (lane == GPC_WAVE - 1) lds[wave] = v;
    __syncthreads();
    long long before = 0, all = 0;
    for (int i = 0; i < RA_WAVES; ++i) {
        if (i < wave) before += lds[i];
        all += lds[i];
    }
    *total = all;
    return v + before;
}

__device__ static inline long long ra_delta(const ra_rows& a, const int32_t* khi, const int32_t* klo, long long r)
{
    return r < a.R ? (long long)gpc_ra_unit(a.unit, a.unit_all, (int)r) * (khi[r] - klo[r]) : 0;
}

// the refinement's exclusive scan over rows, in three launches: the sum of every tile of RA_BLOCK rows, ...
__global__ __launch_bounds__(RA_BLOCK) void ra_tile_sum_kernel(ra_rows a, const int32_t* __restrict__ khi, const int32_t* __restrict__ klo,
                                                              long long* __restrict__ tile, int ntiles)
{
    __shared__ long long lds[RA_WAVES];
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        long long sum;
        (void)ra_block_scan(ra_delta(a, khi, klo, (long long)t * RA_BLOCK + threadIdx.x), lds, &sum);
        if (threadIdx.x == 0) tile[t] = sum;
    }
}

// ... the exclusive scan of the tile sums in place, by one workgroup with a carry, ...
__global__ __launch_bounds__(RA_BLOCK) void ra_tile_scan_kernel(long long* __restrict__ tile, int ntiles)
{
    __shared__ long long lds[RA_WAVES];
    long long carry = 0;
    for (int base = 0; base < ntiles; base += RA_BLOCK) {
        const int t = base + (int)threadIdx.x;
        const long long v = t < ntiles ? tile[t] : 0;
        long long sum;
        const long long incl = ra_block_scan(v, lds, &sum);
        if (t < ntiles) tile[t] = carry + incl - v;
        carry += sum;
    }
}

// ... and the scan inside every tile, started at S(lo) + the tile's offset: E_r, the row's count, the refined choice's saving and the number
// of rows it moves off k_lo (and that k_hi would)
__global__ __launch_bounds__(RA_BLOCK) void ra_pick_kernel(ra_rows a, const int32_t* __restrict__ khi, const int32_t* __restrict__ klo,
                                                          const long long* __restrict__ tile, int ntiles, gpc_ra_state* st,
                                                          int32_t* __restrict__ kref)
{
    __shared__ long long lds[RA_WAVES];
    const long long need = st->need, s_lo = st->s[GPC_RA_AT_LO];
    long long saved = 0, sw_ref = 0, sw_all = 0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long r = (long long)t * RA_BLOCK + threadIdx.x;
        const long long v = ra_delta(a, khi, klo, r);
        long long sum;
        const long long incl = ra_block_scan(v, lds, &sum);
        if (r < a.R) {
            const int k = gpc_ra_pick(s_lo + tile[t] + (incl - v), need, khi[r], klo[r]);
            kref[r] = k;
            saved += (long long)gpc_ra_unit(a.unit, a.unit_all, (int)r) * k;
            sw_ref += k != klo[r];
            sw_all += khi[r] != klo[r];
        }
    }
    long long tot;
    (void)ra_block_scan(saved, lds, &tot);
    if (threadIdx.x == 0 && tot != 0) atomicAdd((unsigned long long*)&st->saved_ref, (unsigned long long)tot);
    (void)ra_block_scan(sw_ref, lds, &tot);
    if (threadIdx.x == 0 && tot != 0) atomicAdd(&st->switched_ref, (int)tot);
    (void)ra_block_scan(sw_all, lds, &tot);
    if (threadIdx.x == 0 && tot != 0) atomicAdd(&st->switched_all, (int)tot);
}

// what both the kernel and the host twin report once the totals are in
__host__ __device__ static inline void ra_finish(gpc_ra_state* st, gpc_rate_result* res)
{
    st->fallback = st->saved_ref < st->need;      // (with exact sums only the infeasible case, where k_lo = k_hi anyway)
    if (!res) return;
    double lambda;
    (void)gpc_ra_sweep(st, GPC_RA_AT_HI, &lambda);
    res->lambda = lambda;
    res->saved = st->fallback ? st->s[GPC_RA_AT_HI] : st->saved_ref;
    res->max_saving = st->s[GPC_RA_AT_INF];
    res->feasible = st->mode != GPC_RA_INFEASIBLE;
    res->switched_rows = st->fallback ? st->switched_all : st->switched_ref;
}

__host__ __device__ static inline int ra_target(int count, int k) { return count - k < 1 ? 1 : count - k; }

__global__ void ra_finish_kernel(gpc_ra_state* st, gpc_rate_result* res) { ra_finish(st, res); }

__global__ __launch_bounds__(RA_BLOCK) void ra_write_kernel(int R, const gpc_ra_state* st, const int32_t* __restrict__ khi,
                                                           const int32_t* __restrict__ kref, const int32_t* __restrict__ count,
                                                           int32_t* __restrict__ k, int32_t* __restrict__ target)
{
    const int32_t* src = st->fallback ? khi : kref;
    for (long long r = (long long)blockIdx.x * RA_BLOCK + threadIdx.x; r < R; r += (long long)gridDim.x * RA_BLOCK) {
        const int kr = src[r];
        if (k) k[r] = kr;
        if (target) target[r] = ra_target(count[r], kr);
    }
}

size_t ra_align(size_t b) { return (b + 255) & ~(size_t)255; }

// what every entry refuses before it looks at a row (include/gpc.h); ctx may be nullptr (the host twin)
int ra_check(gpc_ctx* ctx, int R, int ld, const int32_t* kmax, const double* d0, const double* d, const double* w, double w_all,
             const int32_t* unit, int unit_all, const int32_t* count, const int32_t* target)
{
    if (R < 0) return gpc_fail(ctx, GPC_EINVAL, "rate_allocate: R = %d is negative", R);
    if (ld < 1) return gpc_fail(ctx, GPC_EINVAL, "rate_allocate: ld = %d, must be >= 1", ld);
    if (R > 0 && (!kmax || !d0 || !d)) return gpc_fail(ctx, GPC_EINVAL, "rate_allocate: kmax/d0/d is NULL");
    if (!w && !(w_all >= 0.0)) return gpc_fail(ctx, GPC_EINVAL, "rate_allocate: w_all must be >= 0, got %g", w_all);
    if (!unit && unit_all < 1) return gpc_fail(ctx, GPC_EINVAL, "rate_allocate: unit_all = %d, must be >= 1", unit_all);
    if (target && !count) return gpc_fail(ctx, GPC_EINVAL, "rate_allocate: target needs count");
    return GPC_OK;
}

}  // namespace

extern "C" {

int gpc_rate_allocate_dev(gpc_ctx* ctx, int R, int ld, const int32_t* kmax, const double* d0, const double* d, const double* w, double w_all,
                          const int32_t* unit, int unit_all, int64_t need, int refine, const int32_t* count, int32_t* k, int32_t* target,
                          gpc_rate_result* result)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (int rc = ra_check(ctx, R, ld, kmax, d0, d, w, w_all, unit, unit_all, count, target)) return rc;
    if (R == 0) return GPC_OK;
    // (test hook) GPC_ALLOC_BLOCKS caps the workgroups per launch: the grid-stride wrap and the multi-block scan at a small R
    const char* cap_env = getenv("GPC_ALLOC_BLOCKS");
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcp = gpc_debug_poison_lds(ctx)) return rcp;
    int cap = ctx->num_cus * 2;         // a sweep is a few MB: two workgroups per CU stride the rows, and the totals cost few atomics
    if (cap_env && atoi(cap_env) >= 1) cap = atoi(cap_env);
    const int ntiles = (R + RA_BLOCK - 1) / RA_BLOCK;
    const int g_eval = (int)std::min<long long>(((long long)R + RA_WAVES - 1) / RA_WAVES, cap), g_tile = std::min(ntiles, cap);
    const size_t o_state = 0, o_khi = ra_align(sizeof(gpc_ra_state)), o_klo = o_khi + ra_align((size_t)R * 4), o_kref = o_klo + ra_align((size_t)R * 4),
                 o_tile = o_kref + ra_align((size_t)R * 4), bytes = o_tile + ra_align((size_t)ntiles * 8);
    if (int rc = gpc_ws_reserve(ctx, bytes)) return rc;
    char* ws = static_cast<char*>(ctx->ws);
    gpc_ra_state* st = reinterpret_cast<gpc_ra_state*>(ws + o_state);
    int32_t *khi = reinterpret_cast<int32_t*>(ws + o_khi), *klo = reinterpret_cast<int32_t*>(ws + o_klo), *kref = reinterpret_cast<int32_t*>(ws + o_kref);
    long long* tile = reinterpret_cast<long long*>(ws + o_tile);
    const ra_rows a = {R, ld, kmax, d0, d, w, w_all, unit, unit_all};
    hipStream_t s = ctx->stream;
    ra_init_kernel<<<1, 1, 0, s>>>(st, (long long)need, refine);
    ra_eval_kernel<<<g_eval, RA_BLOCK, 0, s>>>(a, st, GPC_RA_AT_INF, nullptr);
    ra_eval_kernel<<<g_eval, RA_BLOCK, 0, s>>>(a, st, GPC_RA_AT_ZERO, nullptr);
    ra_step_kernel<<<1, 1, 0, s>>>(st, 0);
    for (int i = 0; i < 63; ++i) {
        ra_eval_kernel<<<g_eval, RA_BLOCK, 0, s>>>(a, st, GPC_RA_AT_MID, nullptr);
        ra_step_kernel<<<1, 1, 0, s>>>(st, 1);
    }
    ra_eval_kernel<<<g_eval, RA_BLOCK, 0, s>>>(a, st, GPC_RA_AT_HI, khi);
    ra_eval_kernel<<<g_eval, RA_BLOCK, 0, s>>>(a, st, GPC_RA_AT_LO, klo);
    ra_tile_sum_kernel<<<g_tile, RA_BLOCK, 0, s>>>(a, khi, klo, tile, ntiles);
    ra_tile_scan_kernel<<<1, RA_BLOCK, 0, s>>>(tile, ntiles);
    ra_pick_kernel<<<g_tile, RA_BLOCK, 0, s>>>(a, khi, klo, tile, ntiles, st, kref);
    ra_finish_kernel<<<1, 1, 0, s>>>(st, result);
    if (k || target) ra_write_kernel<<<g_tile, RA_BLOCK, 0, s>>>(R, st, khi, kref, count, k, target);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}

int gpc_rate_allocate(gpc_ctx* ctx, int R, int ld, const int32_t* kmax, const double* d0, const double* d, const double* w, double w_all,
                      const int32_t* unit, int unit_all, int64_t need, int refine, const int32_t* count, int32_t* k, int32_t* target,
                      gpc_rate_result* result)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (int rc = ra_check(ctx, R, ld, kmax, d0, d, w, w_all, unit, unit_all, count, target)) return rc;
    if (R == 0) return GPC_OK;
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)R;
    GpcStaging st(ctx, "gpc_rate_allocate");
    const int32_t* d_kmax = st.up(kmax, n);
    const double *d_d0 = st.up(d0, n), *d_d = st.up(d, n * (size_t)ld);
    const double* d_w = w ? st.up(w, n) : nullptr;
    const int32_t* d_unit = unit ? st.up(unit, n) : nullptr;
    const int32_t* d_count = count ? st.up(count, n) : nullptr;
    int32_t* d_k = k ? st.out<int32_t>(n) : nullptr;
    int32_t* d_target = target ? st.out<int32_t>(n) : nullptr;
    gpc_rate_result* d_res = result ? st.out<gpc_rate_result>(1) : nullptr;
    if (st.ok())
        st.rc = gpc_rate_allocate_dev(ctx, R, ld, d_kmax, d_d0, d_d, d_w, w_all, d_unit, unit_all, need, refine, d_count, d_k, d_target, d_res);
    st.down(k, d_k, n);
    st.down(target, d_target, n);
    st.down(result, d_res, 1);
    return st.finish();
}

// The same rule from the same source on the CPU (no context, no device): the sequence of gpc_rate_allocate_dev, one row after the other.
int gpc_test_rate_allocate_host(int R, int ld, const int32_t* kmax, const double* d0, const double* d, const double* w, double w_all,
                                const int32_t* unit, int unit_all, int64_t need, int refine, const int32_t* count, int32_t* k, int32_t* target,
                                gpc_rate_result* result)
{
    if (int rc = ra_check(nullptr, R, ld, kmax, d0, d, w, w_all, unit, unit_all, count, target)) return rc;
    if (R == 0) return GPC_OK;
    gpc_ra_state st;
    std::vector<int32_t> khi((size_t)R), klo((size_t)R), kref((size_t)R);
    auto sweep = [&](int at, int32_t* kout) {
        double lambda;
        if (!gpc_ra_sweep(&st, at, &lambda)) return;
        for (int r = 0; r < R; ++r) {
            const int km = gpc_ra_kmax(kmax[r], ld), u = gpc_ra_unit(unit, unit_all, r);
            const int c = gpc_ra_choice(km, d0[r], d + (size_t)r * (size_t)ld, w ? w[r] : w_all, u, lambda);
            if (kout) kout[r] = c;
            st.s[at] += (long long)u * c;
        }
    };
    gpc_ra_init(&st, (long long)need, refine);
    sweep(GPC_RA_AT_INF, nullptr);
    sweep(GPC_RA_AT_ZERO, nullptr);
    gpc_ra_decide(&st);
    for (int i = 0; i < 63; ++i) {
        sweep(GPC_RA_AT_MID, nullptr);
        gpc_ra_update(&st);
    }
    sweep(GPC_RA_AT_HI, khi.data());
    sweep(GPC_RA_AT_LO, klo.data());
    long long E = st.s[GPC_RA_AT_LO];
    for (int r = 0; r < R; ++r) {
        const int u = gpc_ra_unit(unit, unit_all, r);
        kref[r] = gpc_ra_pick(E, st.need, khi[r], klo[r]);
        E += (long long)u * (khi[r] - klo[r]);
        st.saved_ref += (long long)u * kref[r];
        st.switched_ref += kref[r] != klo[r];
        st.switched_all += khi[r] != klo[r];
    }
    ra_finish(&st, result);
    for (int r = 0; r < R; ++r) {
        const int kr = st.fallback ? khi[r] : kref[r];
        if (k) k[r] = kr;
        if (target) target[r] = ra_target(count[r], kr);
    }
    return GPC_OK;
}

}  // extern "C"
