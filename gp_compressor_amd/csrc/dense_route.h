// dense_route.h -- which kernel a dense batch runs on, as a value: the environment switches of the dense path (DenseSwitches), what
// the rule looks at (DenseFacts) and what it answers (DenseRoute: the kernel, the shape its launcher needs, the name
// gpc_last_dense_kernel reports).  dense_route() is the whole rule and nothing else; dense_dispatch (dense_api.hip) and the host
// pipeline (dense_host.hip) ask it, the launchers execute what it says.  Host-only, plain C++17 without HIP types: a CPU build can
// include it, and gpc_test_dense_route exercises it without a GPU.
#pragma once

#include <cstdlib>

#include "../../include/gpc.h"

// Every switch is read once per entry-point call (tests flip them between calls on one context).
struct DenseSwitches {
    bool force_generic, force_big;      // diagnostics: the generic / the tiled kernel for everything it can run
    bool no_w1, no_w1_512, w2;          // without the one-wave kernel / its 512-point instance; the tiled kernel's two-wave shape at 193 .. 256 points
    bool w1_min_p_set;
    int w1_min_p;                       // the one-wave kernel's smallest batch (default: four patches per CU)
    int w1_slots;                       // its factor slots per launch, 0: DENSE_W1_MAX_SLOTS
    bool no_split, no_nt17, no_hint;    // the size-class split of a ragged batch, its 257 .. 272-point class, the host-side class sizes
    bool big_no_w2, big_no_w4;          // the tiled kernel without its two-wave / its four-wave 512-point shape
    int var_w4;                         // the variance kernel's four-wave form: -1 by its own rule, 0 never, 1 always
    bool host_no_pipeline, host_one_stream;   // host-pointer entries: one chunk / never the two-stream mode
};

static inline DenseSwitches dense_switches_read()
{
    DenseSwitches s{};
    s.force_generic = getenv("GPC_FORCE_GENERIC") != nullptr;
    s.force_big = getenv("GPC_FORCE_BIG") != nullptr;
    s.no_w1 = getenv("GPC_NO_W1") != nullptr;
    s.no_w1_512 = getenv("GPC_NO_W1_512") != nullptr;
    s.w2 = getenv("GPC_W2") != nullptr;
    const char* mp = getenv("GPC_W1_MIN_P");
    s.w1_min_p_set = mp != nullptr;
    s.w1_min_p = mp ? atoi(mp) : 0;
    const char* sl = getenv("GPC_W1_SLOTS");
    s.w1_slots = sl && atoi(sl) > 0 ? atoi(sl) : 0;
    s.no_split = getenv("GPC_NO_SPLIT") != nullptr;
    s.no_nt17 = getenv("GPC_NO_NT17") != nullptr;
    s.no_hint = getenv("GPC_NO_HINT") != nullptr;
    s.big_no_w2 = getenv("GPC_BIG_NO_W2") != nullptr;
    s.big_no_w4 = getenv("GPC_BIG_NO_W4") != nullptr;
    const char* vw = getenv("GPC_VAR_W4");
    s.var_w4 = vw ? (atoi(vw) != 0 ? 1 : 0) : -1;
    s.host_no_pipeline = getenv("GPC_HOST_NO_PIPELINE") != nullptr;
    s.host_one_stream = getenv("GPC_HOST_ONE_STREAM") != nullptr;
    return s;
}

struct DenseFacts {
    int P, n_max, n_total, ny, m;
    bool variance;      // V* is computed (the caller asked for it AND want_variance is set)
    bool pointwise;     // X* given point by point; false: the grid form
    bool alpha_out;     // the weights are wanted
    int num_cus;
    bool irls;          // the Newton / IRLS loop of the probit likelihood
};

enum DenseKind {
    DENSE_NO_ROUTE = -1,   // the one-wave kernel's workspace was refused and nothing else computes the variance at this size
    DENSE_NOTHING = 0,     // no patch, or neither a prediction nor the weights wanted
    DENSE_ONE_WAVE,        // dense_mfma_w1.hip
    DENSE_REGISTER,        // dense_mfma.hip
    DENSE_TILED,           // dense_mfma_big.hip
    DENSE_GENERIC,         // dense_generic.hip
    DENSE_SPLIT            // three size classes on the register and the tiled kernel
};

#define DENSE_W1_MAX_SLOTS 8192

struct DenseRoute {
    DenseKind kind;
    const char* name;             // what gpc_last_dense_kernel reports
    int w1_npad, w1_slots;        // one-wave: 256 or 512 points; at most this many patches (= factor slots) per launch
    int nt;                       // register: 4 / 8 / 12 / 16 / 17 tiles
    bool export_factor;           //           ... and the factor exported for the variance kernel (also: the IRLS instances of the tiled kernel)
    int waves, npad, per_cu;      // tiled (and the split's third class): the instance and how many workgroups a CU holds
    bool nt17, need_big;          // split: with the 257 .. 272-point class; with patches beyond its last register class
    int var_w4;                   // DenseSwitches::var_w4, for the variance launcher
};

static inline DenseRoute dense_route_register(int n_max, bool variance, int var_w4)
{
    static const char* const names[2][5] = {
        {"dense_mfma_nt4", "dense_mfma_nt8", "dense_mfma_nt12", "dense_mfma_nt16", "dense_mfma_nt17"},
        {"dense_mfma_nt4 + dense_variance", "dense_mfma_nt8 + dense_variance", "dense_mfma_nt12 + dense_variance",
         "dense_mfma_nt16 + dense_variance", ""}};
    const int i = n_max <= 64 ? 0 : n_max <= 128 ? 1 : n_max <= 192 ? 2 : n_max <= 256 ? 3 : 4;
    DenseRoute r{};
    r.kind = DENSE_REGISTER;
    r.nt = i < 4 ? 4 * (i + 1) : 17;
    r.export_factor = variance;
    r.name = names[variance][i];
    r.var_w4 = var_w4;
    return r;
}

// <8 waves, 1024 points, 2 rows per pass, 2 waves/SIMD>: 103 KB of LDS, one workgroup per CU: 256 < n <= 1024.
// <4 waves, 256 points, 2 rows per pass, 2 waves/SIMD>: 37 KB of LDS, two workgroups = two patches per CU: the cross-check
// shape for n <= 256 (GPC_FORCE_BIG=1).  (A 1-row, <= 128-VGPR variant with FOUR patches per CU was measured slower, 2.45 M
// against 2.68 M patches/s on C2: each workgroup runs 2.2x longer -- the shape is bound by the factor stream, not by latency.)
static inline DenseRoute dense_route_tiled(const DenseFacts& f, const DenseSwitches& s)
{
    DenseRoute r{};
    r.kind = DENSE_TILED;
    r.var_w4 = s.var_w4;
    const bool depth = f.ny == 1;
    // depth plane, n <= 256: TWO waves per workgroup (the chain wave + one worker) and FOUR workgroups per CU (40 KB of LDS each)
    if (f.n_max <= 256 && depth && !f.variance && !s.big_no_w2) { r.waves = 2; r.npad = 256; r.per_cu = 4; }
    else if (f.n_max <= 256) { r.waves = 4; r.npad = 256; r.per_cu = 2; }
    // (the two-wave shape at 512 points, three workgroups per CU at 50 KB of LDS: 16.0 ms on C3 against 12.2 -- six waves per CU, and
    // one worker cannot carry a step's 28 row passes)
    // depth plane only, up to 512 points: four waves, two patches per CU (62 KB of LDS each).  Measured on the producer's own batches
    // (273 .. 324 points): GP phase 3.29 against 3.42 ms.  At n = 512 (C3) the 8-wave shape used to win, 13.2 against 13.4 ms -- both
    // chain waves sat on SIMD 0, which then idled; with the second workgroup's chain on SIMD 2 (HW_ID wave slot, see the kernel) the
    // two-workgroup shape wins, 12.23 against 12.63 ms on the same box (round 3)
    else if (f.n_max <= 512 && depth && !s.big_no_w4) { r.waves = 4; r.npad = 512; r.per_cu = 2; }
    else { r.waves = 8; r.npad = 1024; r.per_cu = 1; }
    if (f.irls) {
        // The IRLS instances: four waves for n <= 256, eight beyond.  Their grid has always been sized with the plain shape's
        // workgroups per CU (above); the patches are handed out by ticket, so that only decides how many workgroups queue.
        if (f.n_max <= 256) { r.waves = 4; r.npad = 256; } else { r.waves = 8; r.npad = 1024; }
        r.name = r.waves == 4 ? "dense_mfma_big_w4_irls" : "dense_mfma_big_irls";
        // with the latent variance (or the occupancy probability) wanted: the same instances with the export on -- one slot per patch,
        // which keeps the factor of the last solve -- and the row-scaled variance kernel behind them, at every n <= 1024
        if (f.variance) {
            r.export_factor = true;
            r.name = r.waves == 4 ? "dense_mfma_big_w4_irls + dense_variance_big" : "dense_mfma_big_irls + dense_variance_big";
        }
    } else {
        r.name = r.waves == 2 ? "dense_mfma_big_w2" : r.npad == 256 ? "dense_mfma_big_w4"       // (beyond 256 points the shape is not part of the name)
                 : f.variance ? "dense_mfma_big + dense_variance_big" : "dense_mfma_big";
    }
    return r;
}

// The sub-route of a split's class: 0: n <= 256 and 1: 257 .. 272 points on the register kernel, 2: the rest on the tiled kernel.
static inline DenseRoute dense_route_class(const DenseRoute& split, int which)
{
    if (which < 2) return dense_route_register(which ? 17 * 16 : 256, false, split.var_w4);
    DenseRoute r = split;
    r.kind = DENSE_TILED;
    return r;
}

// The rule.  `w1_refused`: the route of a batch whose one-wave workspace the device could not serve.
static inline DenseRoute dense_route(const DenseFacts& f_in, const DenseSwitches& s, bool w1_refused = false)
{
    DenseFacts f = f_in;
    DenseRoute none{};
    none.kind = DENSE_NOTHING;
    none.name = "";
    if (f.P == 0 || (!f.irls && f.m == 0 && !f.alpha_out)) return none;
    if (f.n_max < 1) f.n_max = 1;
    if (f.irls) return dense_route_tiled(f, s);
    const int n = f.n_max;
    const bool v = f.variance, depth = f.ny == 1, ny_ok = f.ny == 1 || f.ny == 3;
    if (!s.force_generic && !s.force_big && ny_ok) {
        const bool no_split = f.P == 1 || s.no_split;
        // Depth plane, a batch large enough to fill the chip: ONE wave per patch, eight patches per CU (dense_mfma_w1.hip) -- no hand-over
        // between waves at all.  Measured against the register-resident kernel at 8192 patches: 256 points 1.72 against 2.57 ms,
        // 192: 0.98 / 1.70, 128: 0.48 / 1.06, 64: 0.20 / 0.62; at 512 patches the two are level, below that the register kernel's eight
        // waves per patch win on latency (64 patches x 192 points: 0.066 against 0.134 ms) -- hence the batch-size rule (GPC_W1_MIN_P
        // overrides it).  The variance goes this way for 193 .. 256 points, where its solve kernel is the <16> shape, with point-wise X*
        // only (the variance entry has no grid form); the 512-point instance's slots are not the layout the variance kernels read.
        // (round 4: the 512-point instance takes the depth plane of batches whose largest patch has 257 .. 512 points -- C3, and the ragged
        // batches of a cloud cut for 256-point patches, which the size-class split used to deal to three kernels; GPC_NO_W1_512=1: as before)
        const int min_p = s.w1_min_p_set ? s.w1_min_p : 4 * f.num_cus;
        const bool w1_can = depth && (v ? n <= 256 && n > 192 && f.pointwise : n <= 512);
        if (w1_can && f.P >= min_p && f.P > 1 && !s.no_w1 && !(n > 256 && s.no_w1_512)) {
            if (!w1_refused) {
                DenseRoute r{};
                r.kind = DENSE_ONE_WAVE;
                r.w1_npad = n <= 256 ? 256 : 512;
                r.w1_slots = s.w1_slots ? s.w1_slots : DENSE_W1_MAX_SLOTS;
                r.var_w4 = s.var_w4;
                r.name = v ? "dense_mfma_w1 + dense_variance" : n <= 256 ? "dense_mfma_w1" : "dense_mfma_w1_512";
                return r;
            }
            // refused: the register-resident kernel needs no workspace at all -- but its variance path does
            if (v) { none.kind = DENSE_NO_ROUTE; return none; }
        }
        // (GPC_W2=1: the two-wave shape of the tiled kernel, round 3's first headline kernel, kept as a cross-check)
        if (n > 192 && n <= 256 && depth && !v && f.P > 1 && s.w2) return dense_route_tiled(f, s);
        // one shape of the register kernel for the whole batch: n <= 256 for depth and colour, n <= 272 for the depth plane alone
        // (NT = 17); the variance path exports the factor of the n <= 256 shapes only
        if (n <= 256 || (no_split && n <= 17 * 16 && depth && !v && !s.no_nt17)) return dense_route_register(n, v, s.var_w4);
        // Ragged batches whose largest patch exceeds the register kernel's 256 points are sorted into size classes on the device.
        // (a batch whose patches all have n_max points -- P n_max == n_total: every n_i <= n_max and they add up to n_total -- has one
        // size class and the host knows it: no classification, no empty class launches waiting for a CU beside the tiled kernel)
        const bool uniform = (long long)f.P * n == (long long)f.n_total;
        if (!v && n <= GPC_MAX_POINTS && !no_split && !(uniform && n > 17 * 16)) {
            DenseRoute r = dense_route_tiled(f, s);
            r.kind = DENSE_SPLIT;
            r.nt17 = depth && !s.no_nt17;
            r.need_big = !(r.nt17 && n <= 17 * 16);
            r.name = !r.need_big ? "dense_mfma_nt16 + dense_mfma_nt17" : r.nt17 ? "dense_mfma_nt16 + dense_mfma_nt17 + dense_mfma_big"
                                                                                 : "dense_mfma_nt16 + dense_mfma_big";
            return r;
        }
    }
    // the tiled kernel: 256 < n <= 1024 (with the variance: point-wise X* only); GPC_FORCE_BIG: whatever it can run, as a diagnostic
    const bool big_can = n > 256 && n <= 1024 && (!v || f.pointwise) && ny_ok;
    if ((big_can || (s.force_big && n <= 1024 && !v)) && !s.force_generic) return dense_route_tiled(f, s);
    DenseRoute r{};
    r.kind = DENSE_GENERIC;
    r.name = "dense_generic";
    return r;
}
