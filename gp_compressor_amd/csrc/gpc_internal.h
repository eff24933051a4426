// gpc_internal.h -- shared host-side definitions of libgpc_hip.so (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdlib>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gpc.h"

// A Cholesky pivot <= GPC_PIVOT_RTOL * (sigma_f^2 + noise) is reported as GPC_STATUS_NOT_SPD.  Eigen::LLT tests
// `pivot <= 0` (and the reference never looks at the result, /root/reference/src/gaussian_process.cpp:22); with a
// kernel + noise >= 0 Gram matrix a non-positive pivot can only come from cancellation, where the sign of the
// 1e-19 residue is an accident of the summation order.  A relative threshold makes the report deterministic.
#define GPC_PIVOT_RTOL 1e-14

struct gpc_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;  // created with the context
    hipStream_t stream = nullptr;      // stream in use (own_stream or the caller's)
    int num_cus = 256;
    // grow-only device workspace (K / L factors of the generic dense kernel, variance scratch, grid tables)
    void* ws = nullptr;
    size_t ws_bytes = 0;
    int32_t* tickets = nullptr;        // 64 counters (allocated on first use): patches handed out one at a time where their cost varies (dense_mfma_big.hip)
    // host-pointer entries (dense_host.hip, dense_host): a grow-only device arena for the batch, pinned staging buffers for
    // pageable caller memory, and two copy streams so that the upload of chunk c+1 and the download of chunk c-1 run on the
    // SDMA engines while the kernel works on chunk c
    void* io = nullptr;
    size_t io_bytes = 0;
    void* pin_in = nullptr;
    size_t pin_in_bytes = 0;
    void* pin_out = nullptr;
    size_t pin_out_bytes = 0;
    hipStream_t s_in = nullptr, s_out = nullptr, s_c2 = nullptr;   // copy-in, copy-out, second compute stream
    bool pipe_active = false;          // a two-stream host-pointer call is in flight on own_stream / s_c2 (under mu): see gpc_ws_reserve
    unsigned foreign_gen = 0;          // ... and the number of calls of other threads that touched the workspace meanwhile
    hipEvent_t ev[3][16] = {};         // [.][slot]: slots 0 .. 7 are the chunks of the host-pointer pipeline, the others are named in GpcEvSlot
    std::mutex host_mu;                // one host-pointer call at a time per context (they share the arena)
    // size classes of the last batch gpc_project_cloud produced on this context (its `off` buffer, how many of its P patches have
    // <= 256 / <= 272 points): lets the dense dispatch size its class launches exactly instead of P workgroups each
    const int32_t* hint_off = nullptr;
    int hint_P = 0, hint_le256 = 0, hint_le272 = 0;
    std::mutex mu;
    char err[512] = {0};
    const char* last_dense_kernel = "";
    // Ownership (include/gpc.h): every object created from the context (gpc_sparse, gpc_patches) holds one reference.
    // gpc_ctx_destroy releases the device resources and the caller's reference; the struct itself lives until the last
    // child has been destroyed, so a child destroyed AFTER its context finds a `dead` context instead of freed memory.
    std::atomic<int> refs{1};
    std::atomic<bool> dead{false};
    // the live gpc_patches / gpc_sparse objects of this context (address, serial number; under mu): an object that REFERS to others
    // without owning them (gpc_registration) asks here whether they still exist before it touches them
    std::vector<std::pair<const void*, uint64_t>> children;
    uint64_t next_serial = 1;
};

// gpc_ctx::ev[.][slot] above the eight chunk slots
enum GpcEvSlot {
    GPC_EV_PIPE_ORDER = 10,     // the host-pointer pipeline against other threads' calls (gpc_ws_reserve, gpc_pipe_chunk_order)
    GPC_EV_SPARSE_OWN = 12,     // [1]: the sparse predict fork's launch on own_stream joins the caller's stream
    GPC_EV_CLASS_FORK = 13,     // fork and join of the dense size-class launches
    GPC_EV_SPARSE_FORK = 14,    // fork and join of the sparse predict launches
    GPC_EV_ARENA = 15,          // the host-pointer arena against the caller's stream, and the pipeline's compute streams joining it
};

static inline void gpc_ctx_ref(gpc_ctx* ctx) { ctx->refs.fetch_add(1, std::memory_order_relaxed); }
static inline void gpc_ctx_unref(gpc_ctx* ctx)
{
    if (ctx->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete ctx;
}

// Caller holds ctx->mu.  The serial number tells an object from a later one at the same address.
static inline uint64_t gpc_child_register(gpc_ctx* ctx, const void* obj)
{
    ctx->children.emplace_back(obj, ctx->next_serial);
    return ctx->next_serial++;
}
static inline void gpc_child_unregister(gpc_ctx* ctx, const void* obj)
{
    for (size_t i = 0; i < ctx->children.size(); ++i)
        if (ctx->children[i].first == obj) {
            ctx->children.erase(ctx->children.begin() + (long)i);
            return;
        }
}
// Is obj a live object of THIS context?  (An object of another context is not in the list: found out without touching it.)
static inline bool gpc_child_listed(const gpc_ctx* ctx, const void* obj)
{
    for (const auto& c : ctx->children)
        if (c.first == obj) return true;
    return false;
}
static inline bool gpc_child_alive(const gpc_ctx* ctx, const void* obj, uint64_t serial)
{
    for (const auto& c : ctx->children)
        if (c.first == obj) return c.second == serial;
    return false;
}

static inline int gpc_fail(gpc_ctx* ctx, int code, const char* fmt, ...)
{
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define GPC_HIP(ctx, call)                                                                              \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return gpc_fail((ctx), e_ == hipErrorOutOfMemory ? GPC_ENOMEM : GPC_EHIP, "%s failed: %s",  \
                            #call, hipGetErrorString(e_));                                              \
    } while (0)

// The context's stream as the caller configured it, for code that does NOT hold ctx->mu: gpc_ctx_set_stream on another thread writes
// ctx->stream under the lock, so a bare read may race with it.
static inline hipStream_t gpc_stream_of(gpc_ctx* ctx)
{
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ctx->stream;
}

// Checks a host `off` array of P patches (off[0] == 0, non-decreasing) and reports the largest patch and the number of points
// (either may be nullptr).
static inline int gpc_check_host_off(gpc_ctx* ctx, int P, const int32_t* off, int* n_max, int* n_total)
{
    if (P > 0 && off[0] != 0) return gpc_fail(ctx, GPC_EINVAL, "off[0] must be 0");
    int mx = 0;
    for (int i = 0; i < P; ++i) {
        const int n = off[i + 1] - off[i];
        if (n < 0) return gpc_fail(ctx, GPC_EINVAL, "off must be non-decreasing (patch %d)", i);
        mx = n > mx ? n : mx;
    }
    if (n_max) *n_max = mx;
    if (n_total) *n_total = P > 0 ? off[P] : 0;
    return GPC_OK;
}

// Device staging of a host-pointer entry point: the entry validates its arguments, then reads as a list of up() / out(), the
// call of its _dev twin (`if (st.ok()) st.rc = ..._dev(...)`), a list of down() and `return st.finish()`.  The first failing HIP
// call is remembered and every later call is a no-op (up / out then return nullptr).  finish() -- and the destructor, on an
// early return -- synchronises the stream BEFORE it frees the buffers, so the entry is synchronous for its caller and no copy or
// kernel in flight loses its memory.  Sizes are element counts.  The entry does not hold ctx->mu (the _dev twin takes it).
struct GpcStaging {
    gpc_ctx* ctx;
    const char* entry;   // for the error text
    hipStream_t stream;
    hipError_t err = hipSuccess;
    int rc = GPC_OK;     // what the _dev twin returned
    std::vector<void*> bufs;
    bool live = true;    // until release()

    GpcStaging(gpc_ctx* c, const char* name, hipStream_t s) : ctx(c), entry(name), stream(s) {}
    GpcStaging(gpc_ctx* c, const char* name) : GpcStaging(c, name, gpc_stream_of(c)) {}
    GpcStaging(const GpcStaging&) = delete;
    GpcStaging& operator=(const GpcStaging&) = delete;
    ~GpcStaging() { release(); }

    bool ok() const { return err == hipSuccess && rc == GPC_OK; }
    // device buffer of n elements (at least 8 bytes), optionally zeroed
    template <class T> T* out(size_t n, bool zero = false)
    {
        if (!ok()) return nullptr;
        void* d = nullptr;
        const size_t bytes = n * sizeof(T) > 8 ? n * sizeof(T) : 8;
        if ((err = hipMalloc(&d, bytes)) != hipSuccess) return nullptr;
        bufs.push_back(d);
        if (zero) err = hipMemsetAsync(d, 0, bytes, stream);
        return static_cast<T*>(d);
    }
    // ... filled from n host elements (no copy when h is nullptr or n == 0)
    template <class T> T* up(const T* h, size_t n)
    {
        T* d = out<T>(n);
        if (d && h && n) err = hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, stream);
        return d;
    }
    // n elements back to the host (skipped when h is nullptr or n == 0, and after a failure)
    template <class T> void down(T* h, const T* d, size_t n)
    {
        if (ok() && h && n) err = hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, stream);
    }
    // what has been downloaded so far is in host memory when this returns
    void sync()
    {
        if (ok()) err = hipStreamSynchronize(stream);
    }
    void release()
    {
        if (!live) return;
        live = false;
        const hipError_t e = hipStreamSynchronize(stream);
        if (err == hipSuccess) err = e;
        for (void* d : bufs) (void)hipFree(d);
    }
    // the _dev twin's code if it failed (with its own error text), else the staging's
    int finish()
    {
        release();
        if (rc != GPC_OK) return rc;
        if (err != hipSuccess) return gpc_fail(ctx, err == hipErrorOutOfMemory ? GPC_ENOMEM : GPC_EHIP, "%s: %s", entry, hipGetErrorString(err));
        return GPC_OK;
    }
};

// grow-only workspace; sets the error on failure.  Caller holds ctx->mu.  `stream` is the stream of the call in hand: a grow synchronises
// it before the old block goes and clears the new one on it.  `pipe_chunk`: the caller is a chunk of the two-stream host-pointer pipeline.
static inline int gpc_ws_reserve(gpc_ctx* ctx, hipStream_t stream, bool pipe_chunk, size_t bytes)
{
    // "Thread-safe per context" (include/gpc.h) while a two-stream host-pointer call is in flight: its chunk kernels use the workspace from
    // the context's two compute streams, which the stream of ANOTHER thread's call (not a chunk of the pipeline) is not
    // ordered against.  Every user of the workspace comes through here first: that call goes behind the chunks already enqueued; the
    // chunks enqueued after it go behind the context's stream in turn (gpc_pipe_chunk_order).
    if (ctx->pipe_active && !pipe_chunk && !getenv("GPC_NO_PIPE_ORDER")) {   // (the switch: what the test of this looks like without it)
        ++ctx->foreign_gen;
        GPC_HIP(ctx, hipEventRecord(ctx->ev[0][GPC_EV_PIPE_ORDER], ctx->own_stream));
        GPC_HIP(ctx, hipEventRecord(ctx->ev[1][GPC_EV_PIPE_ORDER], ctx->s_c2));
        GPC_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev[0][GPC_EV_PIPE_ORDER], 0));
        GPC_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev[1][GPC_EV_PIPE_ORDER], 0));
    }
    if (bytes <= ctx->ws_bytes) return GPC_OK;
    // The new block is allocated BEFORE the old one is released: a request the device cannot serve leaves the context with the
    // workspace it had.  Only when old + new do not fit side by side is the old one given up first.
    void* nw = nullptr;
    // (diagnostic: GPC_WS_FAIL_ABOVE=<bytes> makes every larger request fail like an exhausted device -- the test of the fallbacks)
    const char* lim = getenv("GPC_WS_FAIL_ABOVE");
    if (lim && bytes > (size_t)atoll(lim)) return gpc_fail(ctx, GPC_ENOMEM, "workspace allocation failed (GPC_WS_FAIL_ABOVE)");
    hipError_t e = hipMalloc(&nw, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (!ctx->ws) return gpc_fail(ctx, GPC_ENOMEM, "workspace allocation failed");
        GPC_HIP(ctx, hipStreamSynchronize(stream));
        const size_t old_bytes = ctx->ws_bytes;
        GPC_HIP(ctx, hipFree(ctx->ws));
        ctx->ws = nullptr;
        ctx->ws_bytes = 0;
        e = hipMalloc(&nw, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            // put back what was there, so that later (smaller) calls find the context as it was
            if (hipMalloc(&ctx->ws, old_bytes) == hipSuccess) {
                ctx->ws_bytes = old_bytes;
                (void)hipMemsetAsync(ctx->ws, getenv("GPC_POISON_LDS") ? 0xFF : 0, old_bytes, stream);
            } else {
                (void)hipGetLastError();
                ctx->ws = nullptr;
            }
            return gpc_fail(ctx, GPC_ENOMEM, "workspace allocation failed");
        }
    } else if (ctx->ws) {
        // the previous workspace may still be in use by work enqueued on the stream
        GPC_HIP(ctx, hipStreamSynchronize(stream));
        GPC_HIP(ctx, hipFree(ctx->ws));
    }
    ctx->ws = nw;
    ctx->ws_bytes = bytes;
    // recycled device memory holds arbitrary bit patterns; the kernels write every workspace element before they use it,
    // but their (clamped, unconditional) prefetches may touch elements they never consume: keep those reads free of
    // signalling patterns and the results independent of what ran before
    GPC_HIP(ctx, hipMemsetAsync(ctx->ws, getenv("GPC_POISON_LDS") ? 0xFF : 0, bytes, stream));   // diagnostic runs: NaN instead of zero
    return GPC_OK;
}
// ... for a call on the context's own stream that uses the whole workspace (every caller outside the dense path)
static inline int gpc_ws_reserve(gpc_ctx* ctx, size_t bytes) { return gpc_ws_reserve(ctx, ctx->stream, false, bytes); }
// The other half of that ordering, for a chunk of the pipeline about to launch on `stream` (in the ctx->mu critical section of its launches:
// no foreign call can slip in between).  If a call of another thread touched the workspace since this compute stream's last chunk
// (*seen_gen: gpc_ctx::foreign_gen as the stream last saw it), the chunk goes behind the context's stream as it stands now: that call may
// use -- or re-grow and clear -- the region this chunk is about to write.
static inline int gpc_pipe_chunk_order(gpc_ctx* ctx, hipStream_t stream, unsigned* seen_gen)
{
    if (*seen_gen == ctx->foreign_gen) return GPC_OK;
    *seen_gen = ctx->foreign_gen;
    if (ctx->stream == stream) return GPC_OK;
    GPC_HIP(ctx, hipEventRecord(ctx->ev[2][GPC_EV_PIPE_ORDER], ctx->stream));
    GPC_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev[2][GPC_EV_PIPE_ORDER], 0));
    return GPC_OK;
}

// Diagnostic (GPC_POISON_LDS=1): before every kernel family runs, fill the LDS of every CU with NaN.  LDS keeps what the
// previous kernel left there, so a read of a word the current kernel never wrote is otherwise a coin toss; with the poison it
// is a NaN in the output and a failing test.  Enqueued on the context's stream; a no-op unless the variable is set.
extern "C" int gpc_debug_poison_lds(gpc_ctx* ctx);
