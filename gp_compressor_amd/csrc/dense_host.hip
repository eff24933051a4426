// dense_host.hip -- host-pointer entries of the dense path: H2D, kernels, D2H, synchronous for the caller and pipelined inside.
#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <thread>
#include <vector>

#include "dense_internal.h"

// Copy with several threads: staging pageable caller memory through pinned buffers is a CPU memcpy, and one core moves
// ~10 GB/s where PCIe 5 moves 50.  A small pool owned by the process (created at the first host-pointer call on pageable
// memory, joined at exit) splits every copy into one slice per thread.
namespace {
class CopyPool {
public:
    static CopyPool& get()
    {
        static CopyPool p;
        return p;
    }
    void copy(void* dst, const void* src, size_t bytes)
    {
        if (bytes < (1u << 20) || th_.empty()) { std::memcpy(dst, src, bytes); return; }
        // One request at a time: the pool is process-wide while the callers' lock (ctx->host_mu) is per context, so two threads on
        // two contexts do get here together; the request fields below are shared with the workers.
        std::lock_guard<std::mutex> call(call_mu_);
        std::unique_lock<std::mutex> lk(m_);
        dst_ = (char*)dst; src_ = (const char*)src; bytes_ = bytes;
        remaining_ = (int)th_.size();
        ++gen_;
        lk.unlock();
        cv_.notify_all();
        slice(0);                                   // the caller takes slice 0
        lk.lock();
        done_.wait(lk, [&] { return remaining_ == 0; });
    }
private:
    CopyPool()
    {
        unsigned hc = std::thread::hardware_concurrency();
        const int n = (int)std::min(4u, hc > 2 ? hc / 2 : 1u);      // measured on the 16-CPU share of a 1-GPU box: 4 threads 4.35 ms per C2 call, 8: 6.6, 12: 4.4
        parts_ = n;
        for (int t = 1; t < n; ++t) th_.emplace_back([this, t] { run(t); });
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
            ++gen_;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void slice(int t)
    {
        const size_t per = ((bytes_ / parts_) + 63) & ~(size_t)63;
        const size_t lo = std::min(bytes_, per * t), hi = (t == parts_ - 1) ? bytes_ : std::min(bytes_, per * (t + 1));
        if (lo < hi) std::memcpy(dst_ + lo, src_ + lo, hi - lo);
    }
    void run(int t)
    {
        unsigned long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(m_);
            cv_.wait(lk, [&] { return gen_ != seen; });
            seen = gen_;
            if (stop_) return;
            lk.unlock();
            slice(t);
            lk.lock();
            if (--remaining_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_, call_mu_;
    std::condition_variable cv_, done_;
    char* dst_ = nullptr;
    const char* src_ = nullptr;
    size_t bytes_ = 0;
    int parts_ = 1, remaining_ = 0;
    unsigned long gen_ = 0;
    bool stop_ = false;
};
}  // namespace
static void par_memcpy(void* dst, const void* src, size_t bytes) { CopyPool::get().copy(dst, src, bytes); }
extern "C" void gpc_test_par_memcpy(void* dst, const void* src, size_t bytes) { par_memcpy(dst, src, bytes); }   // host-only test hook

static bool is_pinned(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

static int grow(gpc_ctx* ctx, void** p, size_t* have, size_t need, bool pinned)
{
    if (need <= *have) return GPC_OK;
    if (*p) {
        GPC_HIP(ctx, hipDeviceSynchronize());
        if (pinned) GPC_HIP(ctx, hipHostFree(*p)); else GPC_HIP(ctx, hipFree(*p));
        *p = nullptr;
        *have = 0;
    }
    need = (need + (need >> 2) + 4095) & ~(size_t)4095;           // 25 % head-room: ragged batches of one cloud vary a little
    if (pinned) GPC_HIP(ctx, hipHostMalloc(p, need, hipHostMallocDefault)); else GPC_HIP(ctx, hipMalloc(p, need));
    *have = need;
    return GPC_OK;
}

// Host-pointer entry of the dense path: H2D, kernel, D2H, synchronous for the caller -- but pipelined inside.  The batch is cut
// into up to four chunks of whole patches; chunk c+1 goes up (copy stream, SDMA engine) and chunk c-1 comes down (second copy
// stream) while the kernel runs on chunk c.  Pinned caller memory (gpc_host_alloc) is transferred in place; pageable memory is
// staged through the context's pinned buffers by a threaded memcpy, which overlaps the GPU work of the previous chunk as well.
// (Copies issued from pageable memory run as blit kernels that queue behind a compute kernel filling every CU: with those,
// chunking overlaps nothing -- measured in round 1.)
static int dense_host(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off,
                      const double* x0, const double* x1, const double* y, int ny,
                      int m, const double* xs0, const double* xs1, double res, int sz, bool grid,
                      double* f_star, double* v_star, double* alpha_out, int32_t* status)
{
    if (!ctx || ctx->dead.load()) return GPC_EINVAL;
    if (P < 0) return gpc_fail(ctx, GPC_EINVAL, "negative size");
    if (P > 0 && !off) return gpc_fail(ctx, GPC_EINVAL, "off is NULL");
    int n_max = 0, n_total = 0;
    int rc = gpc_check_host_off(ctx, P, off, &n_max, &n_total);
    if (rc != GPC_OK) return rc;
    rc = dense_check(ctx, params, P, off, n_max, n_total, x0, x1, y, ny, m, f_star);
    if (rc != GPC_OK) return rc;
    if (!grid && m > 0 && (!xs0 || !xs1)) return gpc_fail(ctx, GPC_EINVAL, "xs0/xs1 is NULL");
    if (P == 0) return GPC_OK;
    std::lock_guard<std::mutex> hlk(ctx->host_mu);
    GPC_HIP(ctx, hipSetDevice(ctx->device));
    const bool want_v = !grid && params->want_variance && v_star;
    const size_t N = (size_t)n_total;
    // (chunks of at least 1024 patches: below four patches per CU the dense dispatch leaves the one-wave-per-patch kernel)
    const DenseSwitches sw = dense_switches_read();
    int C = sw.host_no_pipeline ? 1 : P >= 4096 ? 4 : P >= 2048 ? 2 : 1;
    // Round 4: when the one-wave kernel takes the chunks, the kernels of consecutive chunks run on TWO streams, each in its own half of
    // the workspace (one factor slot per patch of a chunk), so that a chunk's draining workgroups and the next chunk's first ones share
    // the chip -- a chunk of 1024 .. 2048 patches is a single round of resident workgroups, i.e. all ramp and tail -- and the batch goes
    // through in EIGHT chunks: the first upload and the last download, which nothing overlaps, halve.  GPC_HOST_ONE_STREAM=1: as before.
    bool two = false;
    size_t half = 0;
    unsigned seen_gen[2] = {0, 0};      // gpc_ctx::foreign_gen as the two compute streams last saw it (dense_dispatch)
    struct PipeFlag {           // gpc_ctx::pipe_active for the duration of a two-stream call, whichever way it ends
        gpc_ctx* c;
        bool on;
        ~PipeFlag()
        {
            if (!on) return;
            std::lock_guard<std::mutex> lk(c->mu);
            c->pipe_active = false;
        }
    } pipe{ctx, false};
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        // the facts of a chunk (n_total: an upper bound of a chunk's -- the variance path keeps one weight per point in its half)
        DenseFacts chunk{(P + 7) / 8, n_max, n_total, ny, m, want_v, !grid && xs0, false, ctx->num_cus, false};
        // (measured on the C2 batch, same box: 1.95 against 2.12 ms per call, 4.2 against 3.87 M patches/s PCIe-inclusive; at 128 points per
        // patch the kernel is a third of the call and eight chunks only add transfers' fixed costs -- 1.09 against 0.96 ms -- hence n_max > 160)
        // EVERY chunk must go to the one-wave kernel: the halves are sized for its factor slots, and a chunk that reserved more (small
        // patches with the variance wanted go to the register kernel and its factor export) would move the workspace under the other
        // stream's chunk
        bool all_w1 = C == 4 && P >= 8192 && n_max > 160 && !alpha_out && !sw.host_one_stream && ctx->own_stream != nullptr;
        for (int c = 0; c < 8 && all_w1; ++c) {
            const int p0 = (int)((long long)P * c / 8), p1 = (int)((long long)P * (c + 1) / 8);
            DenseFacts fc = chunk;
            fc.P = p1 - p0;
            fc.n_max = 1;
            for (int i = p0; i < p1; ++i) fc.n_max = std::max(fc.n_max, off[i + 1] - off[i]);
            all_w1 = dense_route(fc, sw).kind == DENSE_ONE_WAVE;
        }
        if (all_w1) {
            // the halves: the one-wave kernel's workspace for the largest chunk ((P + 7) / 8 patches of up to n_max points)
            half = (dense_w1_ws_bytes(chunk, dense_route(chunk, sw), nullptr) + 255) & ~(size_t)255;
            if (gpc_ws_reserve(ctx, 2 * half) == GPC_OK) {
                two = true;
                C = 8;
                pipe.on = ctx->pipe_active = true;                 // (calls of other threads on this context: see gpc_ws_reserve)
                seen_gen[0] = seen_gen[1] = ctx->foreign_gen;
            } else {
                (void)hipGetLastError();
            }
        }
    }
    // device arena: [off chunks | x0 | x1 | y planes per chunk | xs0 xs1 | f | v | alpha | status]
    auto al256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t b_off = al256(sizeof(int32_t) * (size_t)(P + C)), b_x = al256(8 * N), b_y = al256(8 * N * ny), b_xs = al256(8 * (size_t)m),
                 b_f = al256(8 * (size_t)P * ny * m), b_v = want_v ? al256(8 * (size_t)P * m) : 0, b_al = alpha_out ? al256(8 * N * ny) : 0,
                 b_st = al256(sizeof(int32_t) * (size_t)P);
    if ((rc = grow(ctx, &ctx->io, &ctx->io_bytes, b_off + 2 * b_x + b_y + 2 * b_xs + b_f + b_v + b_al + b_st, false))) return rc;
    char* d = static_cast<char*>(ctx->io);
    int32_t* d_off = (int32_t*)d; d += b_off;
    double* d_x0 = (double*)d; d += b_x;
    double* d_x1 = (double*)d; d += b_x;
    double* d_y = (double*)d; d += b_y;
    double* d_xs0 = (double*)d; d += b_xs;
    double* d_xs1 = (double*)d; d += b_xs;
    double* d_f = (double*)d; d += b_f;
    double* d_v = (double*)d; d += b_v;
    double* d_al = (double*)d; d += b_al;
    int32_t* d_st = (int32_t*)d;
    // pinned staging: inputs [off chunks | x0 | x1 | y] and outputs [f | v | alpha | status] -- only what is pageable on the caller's side
    const bool pin_x = is_pinned(x0) && is_pinned(x1) && is_pinned(y), pin_f = (m == 0 || is_pinned(f_star)) && (!want_v || is_pinned(v_star));
    if ((rc = grow(ctx, &ctx->pin_in, &ctx->pin_in_bytes, b_off + (pin_x ? 0 : 2 * b_x + b_y), true))) return rc;
    if ((rc = grow(ctx, &ctx->pin_out, &ctx->pin_out_bytes, b_st + (pin_f ? 0 : b_f + b_v), true))) return rc;
    char* hp = static_cast<char*>(ctx->pin_in);
    int32_t* h_off = (int32_t*)hp; hp += b_off;
    double* h_x0 = (double*)hp; hp += pin_x ? 0 : b_x;
    double* h_x1 = (double*)hp; hp += pin_x ? 0 : b_x;
    double* h_y = (double*)hp;
    char* ho = static_cast<char*>(ctx->pin_out);
    int32_t* h_st = (int32_t*)ho; ho += b_st;
    double* h_f = (double*)ho; ho += pin_f ? 0 : b_f;
    double* h_v = (double*)ho;
    hipStream_t sc = gpc_stream_of(ctx), si = ctx->s_in, so = ctx->s_out;
    // the arena may still be read by work a previous call left on the compute stream
    GPC_HIP(ctx, hipEventRecord(ctx->ev[0][GPC_EV_ARENA], sc));
    GPC_HIP(ctx, hipStreamWaitEvent(si, ctx->ev[0][GPC_EV_ARENA], 0));
    if (!grid && m) {
        GPC_HIP(ctx, hipMemcpyAsync(d_xs0, xs0, 8 * (size_t)m, hipMemcpyHostToDevice, si));
        GPC_HIP(ctx, hipMemcpyAsync(d_xs1, xs1, 8 * (size_t)m, hipMemcpyHostToDevice, si));
    }
    int p_lo[9];
    for (int c = 0; c <= C; ++c) p_lo[c] = (int)((long long)P * c / C);
    const hipStream_t sc_main = sc;
    // Both compute streams of the two-stream mode are the context's own (the call is synchronous for the caller anyway; its stream is
    // ordered in front of and behind them with events).  Two reasons, both measured: the legacy default stream does not overlap its
    // kernels with another stream's (2.49 against 1.98 ms per C2 call), and HIP deals streams onto its four hardware queues in creation
    // order, so a caller's stream made before the context can share a queue with s_c2 and serialise the pair (2.46 against 2.0 ms with
    // the bench on a torch side stream) -- own_stream, s_in, s_out and s_c2 are created back to back and never share one.
    const hipStream_t sc_a = two ? ctx->own_stream : sc_main;
    int fail = GPC_OK;
    for (int c = 0; c < C && fail == GPC_OK; ++c) {
        const int p0 = p_lo[c], Pc = p_lo[c + 1] - p0;
        const size_t r0 = (size_t)off[p0], Nc = (size_t)off[p0 + Pc] - r0;
        int32_t* ho_c = h_off + p0 + c;                                   // chunk c owns Pc + 1 entries
        int nmax_c = 0;
        for (int i = 0; i <= Pc; ++i) ho_c[i] = off[p0 + i] - off[p0];
        for (int i = 0; i < Pc; ++i) nmax_c = std::max(nmax_c, ho_c[i + 1] - ho_c[i]);
        int32_t* d_off_c = d_off + p0 + c;
        GPC_HIP(ctx, hipMemcpyAsync(d_off_c, ho_c, sizeof(int32_t) * (size_t)(Pc + 1), hipMemcpyHostToDevice, si));
        // chunk-local layout on the device: x0 | x1 | ny planes of Nc (the kernel's plane stride is the chunk's n_total)
        double* dx0 = d_x0 + r0; double* dx1 = d_x1 + r0; double* dy = d_y + r0 * ny;
        if (Nc) {
            const double *sx0 = x0 + r0, *sx1 = x1 + r0;
            if (!pin_x) {
                par_memcpy(h_x0 + r0, sx0, 8 * Nc);
                par_memcpy(h_x1 + r0, sx1, 8 * Nc);
                sx0 = h_x0 + r0; sx1 = h_x1 + r0;
            }
            GPC_HIP(ctx, hipMemcpyAsync(dx0, sx0, 8 * Nc, hipMemcpyHostToDevice, si));
            GPC_HIP(ctx, hipMemcpyAsync(dx1, sx1, 8 * Nc, hipMemcpyHostToDevice, si));
            for (int q = 0; q < ny; ++q) {
                const double* sy = y + (size_t)q * N + r0;
                if (!pin_x) { par_memcpy(h_y + r0 * ny + q * Nc, sy, 8 * Nc); sy = h_y + r0 * ny + q * Nc; }
                GPC_HIP(ctx, hipMemcpyAsync(dy + q * Nc, sy, 8 * Nc, hipMemcpyHostToDevice, si));
            }
        }
        GPC_HIP(ctx, hipEventRecord(ctx->ev[0][c], si));
        sc = (two && (c & 1)) ? ctx->s_c2 : sc_a;                        // this chunk's compute stream
        if (two && (c == 1 || (c == 0 && sc_a != sc_main))) {              // a stream of ours starts behind whatever the caller's stream carried
            GPC_HIP(ctx, hipStreamWaitEvent(sc, ctx->ev[0][GPC_EV_ARENA], 0));
            if (!grid && m && c == 1) GPC_HIP(ctx, hipStreamWaitEvent(sc, ctx->ev[0][0], 0));   // (xs0 / xs1 went up in front of chunk 0)
        }
        GPC_HIP(ctx, hipStreamWaitEvent(sc, ctx->ev[0][c], 0));
        double* df = d_f + (size_t)p0 * ny * m;
        DenseArgs a = dense_args(params, Pc, d_off_c, nmax_c, (int)Nc, dx0, dx1, dy, ny, m, df, alpha_out ? d_al + r0 * ny : nullptr, d_st + p0);
        if (grid) {
            a.prm.want_variance = 0;
            a.grid_res = res; a.grid_sz = sz;
        } else {
            a.xs0 = d_xs0; a.xs1 = d_xs1;
            a.v_star = want_v ? d_v + (size_t)p0 * m : nullptr;
        }
        {   // on the chunk's compute stream and, in the two-stream mode, in its half of the workspace
            const DenseSite site{sc, (two && (c & 1)) ? half : 0, two ? half : 0};
            std::lock_guard<std::mutex> lk(ctx->mu);
            rc = dense_dispatch(ctx, a, site, two ? &seen_gen[c & 1] : nullptr);
        }
        if (rc != GPC_OK) { fail = rc; break; }
        GPC_HIP(ctx, hipEventRecord(ctx->ev[1][c], sc));
        GPC_HIP(ctx, hipStreamWaitEvent(so, ctx->ev[1][c], 0));
        if (m) GPC_HIP(ctx, hipMemcpyAsync(pin_f ? (void*)(f_star + (size_t)p0 * ny * m) : (void*)(h_f + (size_t)p0 * ny * m), df,
                                           8 * (size_t)Pc * ny * m, hipMemcpyDeviceToHost, so));
        if (want_v && m) GPC_HIP(ctx, hipMemcpyAsync(pin_f ? (void*)(v_star + (size_t)p0 * m) : (void*)(h_v + (size_t)p0 * m), d_v + (size_t)p0 * m,
                                                     8 * (size_t)Pc * m, hipMemcpyDeviceToHost, so));
        GPC_HIP(ctx, hipMemcpyAsync(h_st + p0, d_st + p0, sizeof(int32_t) * (size_t)Pc, hipMemcpyDeviceToHost, so));
        GPC_HIP(ctx, hipEventRecord(ctx->ev[2][c], so));
    }
    if (fail != GPC_OK) {
        (void)hipStreamSynchronize(si); (void)hipStreamSynchronize(sc_main); (void)hipStreamSynchronize(so);
        if (two) { (void)hipStreamSynchronize(ctx->s_c2); (void)hipStreamSynchronize(sc_a); }
        return fail;
    }
    // alpha has chunk-local planes on the device ([ny][Nc] per chunk): gathered plane by plane at the end (rarely requested)
    for (int c = 0; c < C; ++c) {
        const int p0 = p_lo[c], Pc = p_lo[c + 1] - p0;
        GPC_HIP(ctx, hipEventSynchronize(ctx->ev[2][c]));
        if (!pin_f && m) par_memcpy(f_star + (size_t)p0 * ny * m, h_f + (size_t)p0 * ny * m, 8 * (size_t)Pc * ny * m);
        if (!pin_f && want_v && m) par_memcpy(v_star + (size_t)p0 * m, h_v + (size_t)p0 * m, 8 * (size_t)Pc * m);
        if (status) std::memcpy(status + p0, h_st + p0, sizeof(int32_t) * (size_t)Pc);
    }
    if (alpha_out && N) {
        for (int c = 0; c < C; ++c) {
            const int p0 = p_lo[c], Pc = p_lo[c + 1] - p0;
            const size_t r0 = (size_t)off[p0], Nc = (size_t)off[p0 + Pc] - r0;
            for (int q = 0; q < ny && Nc; ++q)
                GPC_HIP(ctx, hipMemcpyAsync(alpha_out + (size_t)q * N + r0, d_al + r0 * ny + q * Nc, 8 * Nc, hipMemcpyDeviceToHost, so));
        }
        GPC_HIP(ctx, hipStreamSynchronize(so));
    }
    if (two) {
        // the caller's stream is ordered behind our compute streams (the next _dev call on the context may reuse the workspace)
        GPC_HIP(ctx, hipEventRecord(ctx->ev[1][GPC_EV_ARENA], ctx->s_c2));
        GPC_HIP(ctx, hipStreamWaitEvent(sc_main, ctx->ev[1][GPC_EV_ARENA], 0));
        if (sc_a != sc_main) {
            GPC_HIP(ctx, hipEventRecord(ctx->ev[2][GPC_EV_ARENA], sc_a));
            GPC_HIP(ctx, hipStreamWaitEvent(sc_main, ctx->ev[2][GPC_EV_ARENA], 0));
        }
    }
    GPC_HIP(ctx, hipStreamSynchronize(sc_main));
    return GPC_OK;
}

extern "C" {

int gpc_dense_fit_predict(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off,
                          const double* x0, const double* x1, const double* y, int ny,
                          int m, const double* xs0, const double* xs1,
                          double* f_star, double* v_star, double* alpha_out, int32_t* status)
{
    return dense_host(ctx, params, P, off, x0, x1, y, ny, m, xs0, xs1, 0.0, 0, false, f_star, v_star, alpha_out, status);
}

int gpc_dense_fit_predict_grid(gpc_ctx* ctx, const gpc_params* params, int P, const int32_t* off,
                               const double* x0, const double* x1, const double* y, int ny,
                               double res, int sz, double* f_star, double* alpha_out, int32_t* status)
{
    if (ctx && (sz < 0 || sz > 1024)) return gpc_fail(ctx, GPC_EINVAL, "sz out of range");
    return dense_host(ctx, params, P, off, x0, x1, y, ny, sz * sz, nullptr, nullptr, res, sz, true, f_star, nullptr,
                      alpha_out, status);
}

}  // extern "C"
