// sparse_scatter.hip -- gpc_sparse_predict_scattered_dev: the read-out of a gpc_sparse at (patch id, point) pairs in ARBITRARY order (the
// hits of a render are that).  Every other read-out entry wants its points bucketed by patch (`off`); this one makes the buckets on the
// device and runs the same kernels on them, so its result is the bucketed entry's bit for bit:
//   keys     key = patch[i], or P for a skipped entry (patch[i] outside [0, P)); value = i
//   sort     rocprim::radix_sort_pairs over the ceil(log2(P + 1)) bits that hold 0 .. P; stable: ascending i inside a bucket
//   offsets  a thread per p in 0 .. P: off[p] = lower_bound(sorted keys, p), at most bits(n) + 1 halvings; off[P] = the valid entries,
//            which never leave the device
//   gather   x0, x1 through `stride` into bucket order
//   predict  sp_predict_launch on (off, plane stride n): the kernels touch rows below off[P] only
//   scatter  f and sigma back to entry order, NaN for the skipped entries
// A thread per entry, plain vector stores, no atomics: the same inputs give the same bits.  All scratch is carved from the context's
// workspace, which sp_predict_launch does not use; its fork onto the context's side streams starts behind an event recorded on this
// stream after the gather and joins this stream before the scatter, so the scratch is ordered across it.
#include <rocprim/device/device_radix_sort.hpp>

#include "producer_internal.h"   // PcCarver, pc_bits_for, PC_THREADS
#include "sparse_internal.h"

__global__ __launch_bounds__(PC_THREADS) void sp_scatter_keys_kernel(int n, int P, const int32_t* __restrict__ patch, uint32_t* __restrict__ key,
                                                                     int32_t* __restrict__ val)
{
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t p = patch[i];
    key[i] = (p < 0 || p >= P) ? (uint32_t)P : (uint32_t)p;
    val[i] = i;
}

// off[p] = the first sorted position whose key is >= p
__global__ __launch_bounds__(PC_THREADS) void sp_scatter_offsets_kernel(int n, int P, const uint32_t* __restrict__ skey, int32_t* __restrict__ off)
{
    const int p = blockIdx.x * PC_THREADS + threadIdx.x;
    if (p > P) return;
    int lo = 0, hi = n;                                       // the answer is in [lo, hi]
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (skey[mid] < (uint32_t)p) lo = mid + 1;
        else hi = mid;
    }
    off[p] = lo;
}

__global__ __launch_bounds__(PC_THREADS) void sp_scatter_gather_kernel(int n, const int32_t* __restrict__ sval, const double* __restrict__ x0,
                                                                       const double* __restrict__ x1, size_t stride, double* __restrict__ g0,
                                                                       double* __restrict__ g1)
{
    const int r = blockIdx.x * PC_THREADS + threadIdx.x;
    if (r >= n) return;
    const size_t i = (size_t)sval[r];                         // (the skipped entries, at the end, are gathered too and read by nobody)
    g0[r] = x0[i * stride];
    g1[r] = x1[i * stride];
}

// sorted position r holds entry sval[r]; it was predicted iff its key is a patch.  skey == nullptr: no patch at all (P == 0), every entry
// r is skipped.  fb / f, sb / s: bucket order in, entry order out, either pair nullptr.
__global__ __launch_bounds__(PC_THREADS) void sp_scatter_back_kernel(int n, int P, int ny, const uint32_t* __restrict__ skey,
                                                                     const int32_t* __restrict__ sval, const double* __restrict__ fb,
                                                                     const double* __restrict__ sb, double* __restrict__ f, double* __restrict__ s)
{
    const int r = blockIdx.x * PC_THREADS + threadIdx.x;
    if (r >= n) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool valid = skey && skey[r] < (uint32_t)P;
    const size_t i = skey ? (size_t)sval[r] : (size_t)r;
    if (f)
        for (int c = 0; c < ny; ++c) f[(size_t)c * (size_t)n + i] = valid ? fb[(size_t)c * (size_t)n + (size_t)r] : nan;
    if (s) s[i] = valid ? sb[r] : nan;
}

int sp_scatter_launch(gpc_sparse* g, int n, const int32_t* patch, const double* x0, const double* x1, int stride, double* f, double* sigma,
                      int conf, int32_t* status)
{
    gpc_ctx* ctx = g->ctx;
    hipStream_t st = ctx->stream;
    const int P = g->P, ny = g->ny;
    const size_t nz = (size_t)n;
    const unsigned blocks = (unsigned)((nz + PC_THREADS - 1) / PC_THREADS);
    if (n == 0 && !status) return GPC_OK;                    // (with status the empty batch is still reported on)
    if (P == 0) {                                             // every entry is skipped
        if (n > 0 && (f || sigma)) {
            hipLaunchKernelGGL(sp_scatter_back_kernel, dim3(blocks), dim3(PC_THREADS), 0, st, n, 0, ny, (const uint32_t*)nullptr,
                               (const int32_t*)nullptr, (const double*)nullptr, (const double*)nullptr, f, sigma);
            GPC_HIP(ctx, hipGetLastError());
        }
        return GPC_OK;
    }
    const unsigned key_bits = (unsigned)pc_bits_for(P);       // the key P must fit
    size_t sort_bytes = 0;
    if (n > 0)
        GPC_HIP(ctx, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                                               nz, 0u, key_bits, st));
    uint32_t *key = nullptr, *skey = nullptr;
    int32_t *val = nullptr, *sval = nullptr, *off = nullptr;
    double *g0 = nullptr, *g1 = nullptr, *fb = nullptr, *sb = nullptr;
    void* prim = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        PcCarver c(pass ? ctx->ws : nullptr);
        off = c.take<int32_t>((size_t)P + 1);
        key = c.take<uint32_t>(nz); skey = c.take<uint32_t>(nz);
        val = c.take<int32_t>(nz); sval = c.take<int32_t>(nz);
        g0 = c.take<double>(nz); g1 = c.take<double>(nz);
        fb = c.take<double>((size_t)ny * nz + 1);             // (the predict kernels take a mean plane, wanted or not)
        sb = sigma ? c.take<double>(nz + 1) : nullptr;
        prim = c.take<char>(sort_bytes);
        if (!pass) {
            const int rc = gpc_ws_reserve(ctx, c.used);
            if (rc != GPC_OK) return rc;
        }
    }
    if (n > 0) {
        hipLaunchKernelGGL(sp_scatter_keys_kernel, dim3(blocks), dim3(PC_THREADS), 0, st, n, P, patch, key, val);
        GPC_HIP(ctx, hipGetLastError());
        GPC_HIP(ctx, rocprim::radix_sort_pairs(prim, sort_bytes, key, skey, val, sval, nz, 0u, key_bits, st));
    }
    hipLaunchKernelGGL(sp_scatter_offsets_kernel, dim3((unsigned)((size_t)P / PC_THREADS + 1)), dim3(PC_THREADS), 0, st, n, P, skey, off);
    GPC_HIP(ctx, hipGetLastError());
    if (n > 0) {
        hipLaunchKernelGGL(sp_scatter_gather_kernel, dim3(blocks), dim3(PC_THREADS), 0, st, n, sval, x0, x1, (size_t)stride, g0, g1);
        GPC_HIP(ctx, hipGetLastError());
    }
    if (int rc = sp_predict_launch(g, 0, off, n, g0, g1, fb, sb, conf, status, 4)) return rc;
    if (n > 0 && (f || sigma)) {
        hipLaunchKernelGGL(sp_scatter_back_kernel, dim3(blocks), dim3(PC_THREADS), 0, st, n, P, ny, skey, sval, fb, sb, f, sigma);
        GPC_HIP(ctx, hipGetLastError());
    }
    return GPC_OK;
}
