// gp_compressor.cpp -- host-side mirror of /root/reference/src/gp_compressor.cpp on top of the C-ABI (include/gpc.h).
#include "gp_compressor.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <stdexcept>
#include <tuple>
#include <unordered_map>

namespace gpc {

double rbf_kernel::kernel_function(const double xi[2], const double xj[2]) const
{
    const double d0 = xi[0] - xj[0], d1 = xi[1] - xj[1];
    return p_[0] * std::exp(-0.5f / p_[1] * (d0 * d0 + d1 * d1));   // src/rbf_kernel.cpp:17
}

namespace {

struct VoxelKey {
    int x, y, z;
    bool operator==(const VoxelKey& o) const { return x == o.x && y == o.y && z == o.z; }
    bool operator<(const VoxelKey& o) const { return std::tie(z, y, x) < std::tie(o.z, o.y, o.x); }
};
struct VoxelHash {
    size_t operator()(const VoxelKey& k) const
    {
        return (size_t)k.x * 73856093u ^ (size_t)k.y * 19349663u ^ (size_t)k.z * 83492791u;
    }
};

// eigenvector of the smallest eigenvalue of a symmetric 4x4 matrix (cyclic Jacobi): the last right singular vector of
// the k x 4 homogeneous point matrix, which is what JacobiSVD(...).matrixV().col(3) gives (src/gp_compressor.cpp:35-36)
void smallest_eigvec4(double A[4][4], double v[4])
{
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 64; ++sweep) {
        double offd = 0;
        for (int p = 0; p < 4; ++p)
            for (int q = p + 1; q < 4; ++q) offd += A[p][q] * A[p][q];
        if (offd == 0.0) break;
        for (int p = 0; p < 4; ++p) {
            for (int q = p + 1; q < 4; ++q) {
                if (A[p][q] == 0.0) continue;
                const double g = 100.0 * std::fabs(A[p][q]);     // negligible against both diagonal entries: drop it
                if (std::fabs(A[p][p]) + g == std::fabs(A[p][p]) && std::fabs(A[q][q]) + g == std::fabs(A[q][q])) {
                    A[p][q] = A[q][p] = 0.0;
                    continue;
                }
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                A[p][q] = A[q][p] = 0.0;                       // the rotation annihilates this pair: make it exact
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
        }
    }
    int best = 0;
    for (int i = 1; i < 4; ++i)
        if (A[i][i] < A[best][best]) best = i;
    for (int k = 0; k < 4; ++k) v[k] = V[k][best];
}

void cross(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
void normalize(double a[3])
{
    const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (n > 0) { a[0] /= n; a[1] /= n; a[2] /= n; }
}

void check(int rc, gpc_ctx* ctx, const char* what)
{
    if (rc != GPC_OK) throw std::runtime_error(std::string(what) + ": " + (ctx ? gpc_last_error(ctx) : "gpc error") +
                                               " (code " + std::to_string(rc) + ")");
}

// Device memory of one context, owned: allocated (and optionally filled from a host vector) in the constructor, freed in the destructor
// (gpc_dev_free synchronises the context's stream first).  Whatever throws, nothing allocated through it leaks.
class dev_buf {
    gpc_ctx* ctx_ = nullptr;
    void* p_ = nullptr;
public:
    dev_buf() = default;
    dev_buf(gpc_ctx* c, size_t bytes) : ctx_(c) { check(gpc_dev_malloc(c, bytes, &p_), c, "gpc_dev_malloc"); }
    template <class T> dev_buf(gpc_ctx* c, const std::vector<T>& h) : dev_buf(c, sizeof(T) * h.size())   // delegating: a failed upload frees
    {
        check(gpc_dev_memcpy(c, p_, h.data(), sizeof(T) * h.size(), GPC_COPY_H2D), c, "gpc_dev_memcpy (upload)");
    }
    dev_buf(dev_buf&& o) noexcept : ctx_(o.ctx_), p_(o.release<void>()) {}
    dev_buf& operator=(dev_buf&& o) noexcept { std::swap(ctx_, o.ctx_); std::swap(p_, o.p_); return *this; }
    ~dev_buf() { if (p_) (void)gpc_dev_free(ctx_, p_); }
    template <class T> T* as() const { return static_cast<T*>(p_); }
    template <class T> T* release() { T* q = as<T>(); p_ = nullptr; return q; }   // the caller owns it from here
    void download(void* h, size_t bytes) const { check(gpc_dev_memcpy(ctx_, h, p_, bytes, GPC_COPY_D2H), ctx_, "gpc_dev_memcpy (download)"); }
};

// Declared AFTER the buffers of a sharded scope, so that it runs before them, on the normal and on the throwing path: no buffer of any
// device is freed before every shard context has been synchronised -- a peer may still be reading it in the exchange.
struct sync_shards {
    const std::vector<gpc_ctx*>& ctxs;
    ~sync_shards() { for (gpc_ctx* c : ctxs) (void)gpc_ctx_synchronize(c); }
};

// The RCCL group bracket: a group left open would swallow every later collective of the process, so the destructor ends it.
class rccl_group {
    gpc_ctx* ctx_;
    bool open_ = false;
public:
    explicit rccl_group(gpc_ctx* c) : ctx_(c) { check(gpc_group_start(), c, "gpc_group_start"); open_ = true; }
    void end() { open_ = false; check(gpc_group_end(), ctx_, "gpc_group_end"); }
    ~rccl_group() { if (open_) (void)gpc_group_end(); }
};

// ---- the shard layout: pure host code (reached without a GPU through gpc_host_shard / gpc_host_shard_scatter) ------------------------
// what the two sharded flows hand gpc_partition_patches as the cost model: 0 = dense (n^3), > 0 = sparse (n min(n, capacity)^2)
int sparse_cost(const gpc_params& depth) { return depth.capacity > 0 ? depth.capacity : 1; }

// slot -> patch table, world * S entries with S = ceil(P / world), -1 = padding
std::vector<int32_t> deal_patches(const patch_batch& b, int world, int cost)
{
    if (world <= 0) throw std::invalid_argument("deal_patches: world must be positive");
    const int P = b.patches();
    std::vector<int32_t> slots((size_t)((P + world - 1) / world) * world, -1);
    if (P > 0) check(gpc_partition_patches(P, b.off.data(), world, cost, slots.data()), nullptr, "gpc_partition_patches");
    return slots;
}

struct shard_batch {
    std::vector<int32_t> off, pd, pc;       // off: S + 1; pd / pc: the insertion orders of the local points (empty when none were given)
    std::vector<double> x0, x1, y, rgb;     // rgb: three planes with the LOCAL stride off[S]
    int n_max = 0;
};

// The slots of device r as a local CSR batch: slot q holds the rows of patch slots[r * S + q], a padding slot is an empty patch.
// perm_d / perm_c (patch order, may be null) hold patch-local indices, so they travel with their patch unchanged.
shard_batch cut_shard(const patch_batch& b, const std::vector<int32_t>& slots, int world, int r, const int32_t* perm_d = nullptr,
                      const int32_t* perm_c = nullptr)
{
    const size_t S = slots.size() / world, N = b.x0.size();
    const int32_t* mine = slots.data() + r * S;
    shard_batch s;
    s.off.assign(S + 1, 0);
    for (size_t q = 0; q < S; ++q) {
        const int p = mine[q];
        const int n = p >= 0 ? b.off[p + 1] - b.off[p] : 0;
        s.off[q + 1] = s.off[q] + n;
        s.n_max = std::max(s.n_max, n);
    }
    const size_t Nl = (size_t)s.off[S];
    s.x0.resize(Nl); s.x1.resize(Nl); s.y.resize(Nl); s.rgb.resize(3 * Nl);
    if (perm_d) s.pd.resize(Nl);
    if (perm_c) s.pc.resize(Nl);
    for (size_t q = 0; q < S; ++q) {
        const int p = mine[q];
        if (p < 0) continue;
        const size_t o = (size_t)b.off[p], n = (size_t)(b.off[p + 1] - b.off[p]), lo = (size_t)s.off[q];
        std::copy_n(b.x0.data() + o, n, s.x0.data() + lo);
        std::copy_n(b.x1.data() + o, n, s.x1.data() + lo);
        std::copy_n(b.y.data() + o, n, s.y.data() + lo);
        for (int a = 0; a < 3; ++a) std::copy_n(b.rgb.data() + a * N + o, n, s.rgb.data() + a * Nl + lo);
        if (perm_d) std::copy_n(perm_d + o, n, s.pd.data() + lo);
        if (perm_c) std::copy_n(perm_c + o, n, s.pc.data() + lo);
    }
    return s;
}

// a per-slot array of device r into patch order; padding slots write nothing
void scatter_slots(const std::vector<int32_t>& slots, int world, int r, const int32_t* per_slot, int32_t* per_patch)
{
    const size_t S = slots.size() / world;
    for (size_t q = 0; q < S; ++q) {
        const int p = slots[r * S + q];
        if (p >= 0) per_patch[p] = per_slot[q];
    }
}

// ---- the device side of a shard ------------------------------------------------------------------------------------------------------
struct dev_shard {
    shard_batch h;
    dev_buf off, x0, x1, y, rgb, pd, pc, st;     // st: one status word per slot; pd / pc stay 8 spare bytes without insertion orders
    dev_shard(gpc_ctx* c, shard_batch&& b)
        : h(std::move(b)), off(c, h.off), x0(c, h.x0), x1(c, h.x1), y(c, h.y), rgb(c, h.rgb), pd(c, h.pd), pc(c, h.pc),
          st(c, sizeof(int32_t) * (h.off.size() - 1)) {}
};

void fetch_status(const std::vector<dev_shard>& sh, const std::vector<int32_t>& slots, std::vector<int32_t>& status)
{
    const int world = (int)sh.size();
    std::vector<int32_t> st(slots.size() / world);
    for (int r = 0; r < world; ++r) {
        sh[r].st.download(st.data(), sizeof(int32_t) * st.size());
        scatter_slots(slots, world, r, st.data(), status.data());
    }
}

// The one exchange.  lf / lc: per device the depth [S][m] and colour [S][3m] grids of its slots, already enqueued.  The partition goes to
// the communicators, ONE bracket holds the all-gather of both (one fused exchange), device 0 un-permutes to patch order and the host
// gets f* [P][m] and c* [P][3m].
void gather_grids(const std::vector<gpc_ctx*>& ctx, const std::vector<gpc_comm*>& comm, const std::vector<int32_t>& slots, int P, int m,
                  const std::vector<dev_buf>& lf, const std::vector<dev_buf>& lc, std::vector<double>& f_star, std::vector<double>& c_star)
{
    const int world = (int)ctx.size();
    const size_t row = sizeof(double) * (size_t)m;
    std::vector<dev_buf> gf, gc;
    for (gpc_ctx* c : ctx) {
        gf.emplace_back(c, slots.size() * row);
        gc.emplace_back(c, slots.size() * 3 * row);
    }
    dev_buf f(ctx[0], P * row), c(ctx[0], P * 3 * row);
    sync_shards sync{ctx};
    for (int r = 0; r < world; ++r) check(gpc_comm_set_partition(comm[r], P, slots.data()), ctx[r], "gpc_comm_set_partition");
    rccl_group group(ctx[0]);
    for (int r = 0; r < world; ++r) {
        check(gpc_allgather_fstar_dev(comm[r], m, lf[r].as<const double>(), gf[r].as<double>(), nullptr), ctx[r], "all-gather f*");
        check(gpc_allgather_fstar_dev(comm[r], 3 * m, lc[r].as<const double>(), gc[r].as<double>(), nullptr), ctx[r], "all-gather c*");
    }
    group.end();
    check(gpc_unpermute_fstar_dev(comm[0], m, gf[0].as<const double>(), f.as<double>()), ctx[0], "un-permute f*");
    check(gpc_unpermute_fstar_dev(comm[0], 3 * m, gc[0].as<const double>(), c.as<double>()), ctx[0], "un-permute c*");
    f_star.assign((size_t)P * m, 0.0);
    c_star.assign((size_t)P * 3 * m, 0.0);
    f.download(f_star.data(), P * row);
    c.download(c_star.data(), P * 3 * row);
}

pointcloud to_cloud(const std::vector<gpc_point_xyzrgb>& recs)
{
    pointcloud out(recs.size());
    for (size_t q = 0; q < recs.size(); ++q) out[q] = point{recs[q].x, recs[q].y, recs[q].z, recs[q].r, recs[q].g, recs[q].b};
    return out;
}

}  // namespace

gp_compressor::gp_compressor(double res, int sz, int device)
    : rng([] { return std::rand(); }), res_(res), sz_(sz), model_(gp_model::sparse), device_(device)
{
    gpc_default_params_sparse(&depth_params, 1);
    gpc_default_params_sparse(&rgb_params, 3);
    gpc_default_params_dense(&dense_params);
}

gp_compressor::gp_compressor(const pointcloud& ncloud, double res, int sz, gp_model model, int device) : gp_compressor(res, sz, device)
{
    cloud_ = ncloud;
    model_ = model;
}

void gp_compressor::release_device()
{
    if (dev_patches_) { gpc_patches_destroy(dev_patches_); dev_patches_ = nullptr; }
    drop_dense_grids();
}

void gp_compressor::drop_dense_grids()
{
    if (ctx_) {
        if (d_dense_f_) (void)gpc_dev_free(ctx_, d_dense_f_);
        if (d_dense_c_) (void)gpc_dev_free(ctx_, d_dense_c_);
    }
    d_dense_f_ = d_dense_c_ = nullptr;
}

void gp_compressor::set_devices(const std::vector<int>& devices)
{
    if (!devices.empty() && (!dense_cand_depth_.empty() || !dense_cand_rgb_.empty()))
        throw std::runtime_error("set_devices: dense candidates are set; per-leaf selection runs in the single-device flows only "
                                 "(set_dense_candidates({}, {}) first)");
    for (gpc_sparse* q : shard_gps_) if (q) gpc_sparse_destroy(q);
    for (gpc_sparse* q : shard_rgb_) if (q) gpc_sparse_destroy(q);
    shard_gps_.clear();
    shard_rgb_.clear();
    shard_slots_.clear();
    for (gpc_comm* c : shard_comm_) gpc_comm_destroy(c);
    for (gpc_ctx* c : shard_ctx_) gpc_ctx_destroy(c);
    shard_comm_.clear();
    shard_ctx_.clear();
    devices_ = devices;
}

// one context per device and the communicators of the one exchange
void gp_compressor::init_shards()
{
    if (!shard_ctx_.empty()) return;
    const int world = (int)devices_.size();
    // built into locals and committed to the members only when every context and communicator exists: a failure half-way
    // leaves the object in its single-device state, never with null handles that a later call would pass on
    std::vector<gpc_ctx*> ctxs(world, nullptr);
    std::vector<gpc_comm*> comms(world, nullptr);
    try {
        for (int r = 0; r < world; ++r) check(gpc_ctx_create(&ctxs[r], devices_[r]), nullptr, "gpc_ctx_create (shard)");
        check(gpc_comm_create_all(world, ctxs.data(), comms.data()), ctxs[0], "gpc_comm_create_all");
    } catch (...) {
        for (gpc_comm* c : comms) if (c) gpc_comm_destroy(c);
        for (gpc_ctx* c : ctxs) if (c) gpc_ctx_destroy(c);
        throw;
    }
    shard_ctx_.swap(ctxs);
    shard_comm_.swap(comms);
}

// The sparse model over several GPUs (BASELINE configs[3]; the reference keeps adding to trained GPs,
// /root/reference/src/gp_mapping.cpp:338-339): gpc_partition_patches with the sparse cost model deals the patches ONCE, the
// depth and colour GPs of a device's slots are created there and stay there.  perm_d / perm_c: the insertion orders in
// patch order, as train_processes() drew them.
void gp_compressor::train_sparse_sharded(const std::vector<int32_t>& perm_d, const std::vector<int32_t>& perm_c)
{
    const int world = (int)devices_.size();
    init_shards();
    if (shard_slots_.empty()) {
        // built in locals and committed to the members only when every create has succeeded (as init_shards() does): a create that
        // throws midway must not leave shard_slots_ filled beside half-created GPs
        std::vector<int32_t> slots = deal_patches(batch_, world, sparse_cost(depth_params));
        const int S = (int)slots.size() / world;
        std::vector<gpc_sparse*> gps(world, nullptr), rgb(world, nullptr);
        try {
            for (int r = 0; r < world; ++r) {
                check(gpc_sparse_create(shard_ctx_[r], &depth_params, S, 1, &gps[r]), shard_ctx_[r], "gpc_sparse_create(depth, shard)");
                check(gpc_sparse_create(shard_ctx_[r], &rgb_params, S, 3, &rgb[r]), shard_ctx_[r], "gpc_sparse_create(rgb, shard)");
            }
        } catch (...) {
            for (int r = 0; r < world; ++r) {
                if (gps[r]) gpc_sparse_destroy(gps[r]);
                if (rgb[r]) gpc_sparse_destroy(rgb[r]);
            }
            throw;
        }
        shard_slots_.swap(slots);
        shard_gps_.swap(gps);
        shard_rgb_.swap(rgb);
    }
    std::vector<dev_shard> sh;
    sync_shards sync{shard_ctx_};
    for (int r = 0; r < world; ++r) sh.emplace_back(shard_ctx_[r], cut_shard(batch_, shard_slots_, world, r, perm_d.data(), perm_c.data()));
    // the add calls only enqueue: the devices run side by side
    for (int r = 0; r < world; ++r) {
        const dev_shard& s = sh[r];
        check(gpc_sparse_add_dev(shard_gps_[r], s.off.as<int32_t>(), s.h.n_max, s.h.off.back(), s.x0.as<double>(), s.x1.as<double>(),
                                 s.y.as<double>(), s.pd.as<int32_t>(), s.st.as<int32_t>()), shard_ctx_[r], "gpc_sparse_add_dev (shard, depth)");
        check(gpc_sparse_add_dev(shard_rgb_[r], s.off.as<int32_t>(), s.h.n_max, s.h.off.back(), s.x0.as<double>(), s.x1.as<double>(),
                                 s.rgb.as<double>(), s.pc.as<int32_t>(), s.st.as<int32_t>()), shard_ctx_[r], "gpc_sparse_add_dev (shard, rgb)");
    }
    fetch_status(sh, shard_slots_, status_);
}

// basis sizes of the sharded sparse model, slot by slot into patch order
std::vector<int32_t> gp_compressor::shard_basis_sizes() const
{
    const int world = (int)devices_.size();
    std::vector<int32_t> bv(batch_.patches(), 0), sz_slot(shard_slots_.size() / world);
    for (int r = 0; r < world; ++r) {
        check(gpc_sparse_sizes(shard_gps_[r], sz_slot.data()), shard_ctx_[r], "gpc_sparse_sizes (shard)");
        scatter_slots(shard_slots_, world, r, sz_slot.data(), bv.data());
    }
    return bv;
}

// load_compressed() of the sharded sparse model: every device predicts the grids of its slots, ONE grouped all-gather of the depth and
// the colour grids reassembles them on device 0 in patch order.
void gp_compressor::predict_sparse_sharded(const std::vector<double>& xs0, const std::vector<double>& xs1, std::vector<double>& f_star,
                                           std::vector<double>& c_star)
{
    const int world = (int)devices_.size();
    const size_t grid = sizeof(double) * xs0.size() * (shard_slots_.size() / world);     // the depth grids of one device's slots
    std::vector<dev_buf> d_xs0, d_xs1, lf, lc;
    sync_shards sync{shard_ctx_};
    for (gpc_ctx* c : shard_ctx_) {
        d_xs0.emplace_back(c, xs0);
        d_xs1.emplace_back(c, xs1);
        lf.emplace_back(c, grid);
        lc.emplace_back(c, 3 * grid);
    }
    for (int r = 0; r < world; ++r) {
        check(gpc_sparse_predict_dev(shard_gps_[r], (int)xs0.size(), d_xs0[r].as<double>(), d_xs1[r].as<double>(), lf[r].as<double>(), nullptr, 0,
                                     nullptr), shard_ctx_[r], "gpc_sparse_predict_dev (shard, depth)");
        check(gpc_sparse_predict_dev(shard_rgb_[r], (int)xs0.size(), d_xs0[r].as<double>(), d_xs1[r].as<double>(), lc[r].as<double>(), nullptr, 0,
                                     nullptr), shard_ctx_[r], "gpc_sparse_predict_dev (shard, rgb)");
    }
    gather_grids(shard_ctx_, shard_comm_, shard_slots_, batch_.patches(), (int)xs0.size(), lf, lc, f_star, c_star);
}

// The dense model over several GPUs: the batched form of "patches shard embarrassingly, one all-gather reassembles the
// decompressed cloud" (BASELINE north_star; patches are independent, src/gp_compressor.cpp:146-163).
void gp_compressor::train_dense_sharded()
{
    const int m = sz_ * sz_, world = (int)devices_.size();
    init_shards();
    const std::vector<int32_t> slots = deal_patches(batch_, world, 0);
    const int S = (int)slots.size() / world;
    std::vector<dev_shard> sh;
    std::vector<dev_buf> lf, lc;
    sync_shards sync{shard_ctx_};
    for (int r = 0; r < world; ++r) {
        sh.emplace_back(shard_ctx_[r], cut_shard(batch_, slots, world, r));
        lf.emplace_back(shard_ctx_[r], sizeof(double) * (size_t)S * m);
        lc.emplace_back(shard_ctx_[r], sizeof(double) * (size_t)S * 3 * m);
    }
    // every device fits + predicts its slots: the launches only enqueue, so the devices run concurrently
    for (int r = 0; r < world; ++r) {
        const dev_shard& s = sh[r];
        gpc_ctx* c = shard_ctx_[r];
        check(gpc_dense_fit_predict_grid_dev(c, &dense_params, S, s.off.as<int32_t>(), s.h.n_max, s.h.off.back(), s.x0.as<double>(),
                                             s.x1.as<double>(), s.y.as<double>(), 1, res_, sz_, lf[r].as<double>(), nullptr,
                                             s.st.as<int32_t>()), c, "gpc_dense_fit_predict_grid_dev (shard, depth)");
        check(gpc_dense_fit_predict_grid_dev(c, &dense_params, S, s.off.as<int32_t>(), s.h.n_max, s.h.off.back(), s.x0.as<double>(),
                                             s.x1.as<double>(), s.rgb.as<double>(), 3, res_, sz_, lc[r].as<double>(), nullptr, nullptr),
              c, "gpc_dense_fit_predict_grid_dev (shard, rgb)");
    }
    // device 0 hands the grids to the host flow (load_compressed reprojects them)
    gather_grids(shard_ctx_, shard_comm_, slots, batch_.patches(), m, lf, lc, dense_f_, dense_c_);
    fetch_status(sh, slots, status_);
}

gp_compressor::~gp_compressor()
{
    set_devices({});          // the shard GPs, communicators and contexts
    release_device();
    if (gps_) gpc_sparse_destroy(gps_);
    if (rgb_gps_) gpc_sparse_destroy(rgb_gps_);
    if (ctx_) gpc_ctx_destroy(ctx_);
}

// src/gp_compressor.cpp:21-27
void gp_compressor::save_compressed(const std::string& /*name: ignored by the reference too*/)
{
    if (gpu_producer && devices_.empty()) project_cloud_device(); else project_cloud();
    train_processes();
}

// project_cloud() on the GPU: upload the cloud as pcl::PointXYZRGB records, fetch the batch
void gp_compressor::project_cloud_device()
{
    if (!ctx_) check(gpc_ctx_create(&ctx_, device_), nullptr, "gpc_ctx_create");
    std::vector<gpc_point_xyzrgb> rec(cloud_.size());
    for (size_t i = 0; i < cloud_.size(); ++i) {
        const point& p = cloud_[i];
        rec[i] = gpc_point_xyzrgb{p.x, p.y, p.z, 1.0f, p.b, p.g, p.r, 255, {0.0f, 0.0f, 0.0f}};
    }
    release_device();
    gpc_patches* pt = nullptr;
    check(gpc_project_cloud(ctx_, rec.data(), (int)rec.size(), res_, sz_, &pt), ctx_, "gpc_project_cloud");
    gpc_patches_view v;
    gpc_patches_view_dev(pt, &v);
    batch_ = patch_batch();
    const size_t P = (size_t)v.P, N = (size_t)v.n_total;
    batch_.off.assign(P + 1, 0);
    batch_.x0.resize(N); batch_.x1.resize(N); batch_.y.resize(N); batch_.rgb.resize(3 * N);
    batch_.rotations.resize(P); batch_.means.resize(P); batch_.rgb_means.resize(P);
    batch_.W.resize(P * (size_t)v.m);
    const int rc = gpc_patches_fetch(pt, batch_.off.data(), batch_.x0.data(), batch_.x1.data(), batch_.y.data(), batch_.rgb.data(),
                                     P ? batch_.rotations[0].data() : nullptr, P ? batch_.means[0].data() : nullptr,
                                     P ? batch_.rgb_means[0].data() : nullptr, batch_.W.data(), nullptr);
    if (rc != GPC_OK) gpc_patches_destroy(pt); else dev_patches_ = pt;     // the batch stays on the device for train_processes()
    check(rc, ctx_, "gpc_patches_fetch");
    projected_ = true;
}

// src/gp_compressor.cpp:29-64
void gp_compressor::compute_rotation(double R[9], const std::vector<double>& pts4, int k) const
{
    auto setcol = [&](int c, const double v[3]) { R[3 * c] = v[0]; R[3 * c + 1] = v[1]; R[3 * c + 2] = v[2]; };
    if (k < 4) {
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        std::memcpy(R, I, sizeof(I));
        return;
    }
    double M[4][4] = {};
    for (int p = 0; p < k; ++p)
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) M[a][b] += pts4[4 * p + a] * pts4[4 * p + b];
    double v[4];
    smallest_eigvec4(M, v);
    double normal[3] = {v[0], v[1], v[2]};
    normalize(normal);
    const double x[3] = {1, 0, 0}, y[3] = {0, 1, 0}, z[3] = {0, 0, 1};
    double c1[3];
    const double ax = std::fabs(normal[0]), ay = std::fabs(normal[1]), az = std::fabs(normal[2]);
    if (ax > ay && ax > az) {            // pointing in x dir
        if (normal[0] < 0) { normal[0] = -normal[0]; normal[1] = -normal[1]; normal[2] = -normal[2]; }
        cross(z, normal, c1);
    } else if (ay > ax && ay > az) {     // pointing in y dir
        if (normal[1] < 0) { normal[0] = -normal[0]; normal[1] = -normal[1]; normal[2] = -normal[2]; }
        cross(x, normal, c1);
    } else {                             // pointing in z dir
        if (normal[2] < 0) { normal[0] = -normal[0]; normal[1] = -normal[1]; normal[2] = -normal[2]; }
        cross(y, normal, c1);
    }
    normalize(c1);
    double c2[3];
    cross(normal, c1, c2);
    setcol(0, normal);
    setcol(1, c1);
    setcol(2, c2);
}

// src/gp_compressor.cpp:177-249 with project_points (:66-118) inlined per leaf
void gp_compressor::project_cloud()
{
    release_device();
    batch_ = patch_batch();
    batch_.off.push_back(0);
    const size_t npts = cloud_.size();
    if (npts == 0) { projected_ = true; return; }
    // voxel hash of side res, anchored at the cloud's minimum corner
    double mn[3] = {cloud_[0].x, cloud_[0].y, cloud_[0].z};
    for (const point& p : cloud_) {
        mn[0] = std::min<double>(mn[0], p.x);
        mn[1] = std::min<double>(mn[1], p.y);
        mn[2] = std::min<double>(mn[2], p.z);
    }
    auto key_of = [&](const point& p) {
        return VoxelKey{(int)std::floor((p.x - mn[0]) / res_), (int)std::floor((p.y - mn[1]) / res_),
                        (int)std::floor((p.z - mn[2]) / res_)};
    };
    std::unordered_map<VoxelKey, std::vector<int>, VoxelHash> grid;
    for (size_t i = 0; i < npts; ++i) grid[key_of(cloud_[i])].push_back((int)i);
    std::vector<VoxelKey> leaves;
    leaves.reserve(grid.size());
    for (auto& kv : grid) leaves.push_back(kv.first);
    std::sort(leaves.begin(), leaves.end());   // deterministic leaf order (the octree's depth-first order is PCL's)

    const double radius = std::sqrt(3.0f) / 2.0f * res_;   // :194, sphere encompassing the voxel
    std::vector<char> occupied(npts, 0);                   // occupied_indices (:200): exclusive point ownership
    std::vector<int> index_search;
    std::vector<double> pts4, cols;
    const int m = sz_ * sz_;
    for (const VoxelKey& key : leaves) {
        const double center[3] = {mn[0] + (key.x + 0.5) * res_, mn[1] + (key.y + 0.5) * res_, mn[2] + (key.z + 0.5) * res_};
        // radiusSearch(center, radius) (:220): radius < res, so the 27 neighbouring voxels cover the sphere
        index_search.clear();
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    auto it = grid.find(VoxelKey{key.x + dx, key.y + dy, key.z + dz});
                    if (it == grid.end()) continue;
                    for (int idx : it->second) {
                        const point& p = cloud_[idx];
                        const double ex = p.x - center[0], ey = p.y - center[1], ez = p.z - center[2];
                        if (ex * ex + ey * ey + ez * ez <= radius * radius) index_search.push_back(idx);
                    }
                }
        // hit order = patch point order: neighbour voxels in (dz, dy, dx) order, ascending index inside a voxel (PCL's is its
        // octree traversal order); the GPU producer and the oracle walk the same order, so all three agree bit for bit
        std::array<double, 9> R{};
        std::array<double, 3> mid{center[0], center[1], center[2]}, cmean{0, 0, 0};
        const int k = (int)index_search.size();
        pts4.assign(4 * (size_t)k, 1.0);
        cols.assign(3 * (size_t)k, 0.0);
        for (int q = 0; q < k; ++q) {
            const point& p = cloud_[index_search[q]];
            pts4[4 * q] = p.x; pts4[4 * q + 1] = p.y; pts4[4 * q + 2] = p.z;
            cols[3 * q] = p.r; cols[3 * q + 1] = p.g; cols[3 * q + 2] = p.b;
        }
        compute_rotation(R.data(), pts4, k);
        // project_points (:66-118)
        const size_t first = batch_.x0.size();
        std::vector<uint8_t> W(m, 0);
        double mnd = 0;
        std::vector<std::array<double, 3>> colours;
        for (int q = 0; q < k; ++q) {
            const int gi = index_search[q];
            if (occupied[gi]) continue;                                         // :81-83
            const double d[3] = {pts4[4 * q] - mid[0], pts4[4 * q + 1] - mid[1], pts4[4 * q + 2] - mid[2]};
            double pt[3];
            for (int a = 0; a < 3; ++a) pt[a] = R[3 * a] * d[0] + R[3 * a + 1] * d[1] + R[3 * a + 2] * d[2];   // R^T d
            if (pt[1] > res_ / 2.0f || pt[1] < -res_ / 2.0f || pt[2] > res_ / 2.0f || pt[2] < -res_ / 2.0f) continue;   // :85-87
            mnd += pt[0];
            occupied[gi] = 1;
            int gx = (int)((double)sz_ * (pt[1] / res_ + 0.5f)), gy = (int)((double)sz_ * (pt[2] / res_ + 0.5f));     // :90-92
            gx = std::min(std::max(gx, 0), sz_ - 1);
            gy = std::min(std::max(gy, 0), sz_ - 1);
            W[sz_ * gx + gy] = 1;
            batch_.y.push_back(pt[0]);
            batch_.x0.push_back(pt[1]);
            batch_.x1.push_back(pt[2]);
            colours.push_back({cols[3 * q], cols[3 * q + 1], cols[3 * q + 2]});
            for (int a = 0; a < 3; ++a) cmean[a] += cols[3 * q + a];
        }
        const size_t cnt = batch_.x0.size() - first;
        if (cnt > 0) {
            mnd /= (double)cnt;                                                 // :101-107
            for (int a = 0; a < 3; ++a) cmean[a] /= (double)cnt;
            for (size_t q = first; q < batch_.y.size(); ++q) batch_.y[q] -= mnd;
            for (int a = 0; a < 3; ++a) mid[a] += mnd * R[a];                   // center += mn*R.col(0)  (:116)
        }
        // colours are appended plane-wise after the loop (3 planes of N); keep them per patch for now
        for (auto& c : colours)
            for (int a = 0; a < 3; ++a) batch_.rgb.push_back(c[a] - cmean[a]);   // temporary AoS, re-packed below
        batch_.off.push_back((int32_t)batch_.x0.size());
        batch_.rotations.push_back(R);
        batch_.means.push_back(mid);
        batch_.rgb_means.push_back(cmean);
        batch_.W.insert(batch_.W.end(), W.begin(), W.end());
    }
    // AoS colours -> 3 planes of N (Eigen column-major n x 3, per the C-ABI layout)
    const size_t N = batch_.x0.size();
    std::vector<double> planes(3 * N);
    for (size_t q = 0; q < N; ++q)
        for (int a = 0; a < 3; ++a) planes[a * N + q] = batch_.rgb[3 * q + a];
    batch_.rgb.swap(planes);
    projected_ = true;
}

// sparse_gp::shuffle (src/sparse_gp.hpp:43-56): ind[i] <-> ind[rand() % i] for i = n-1 .. 1
void gp_compressor::shuffle(std::vector<int32_t>& perm, int n)
{
    const size_t base = perm.size();
    for (int i = 0; i < n; ++i) perm.push_back(i);
    for (int i = n - 1; i > 0; --i) {
        const int r = rng() % i;
        std::swap(perm[base + i], perm[base + r]);
    }
}

static const char* const dense_candidates_sharded =
    "dense candidates and set_devices() do not combine: gpc_dense_select runs every candidate on the device that holds the patch, and the "
    "sharded flow balances its partition for one fit per patch -- clear one of the two";

void gp_compressor::set_dense_candidates(const std::vector<gpc_hyper>& depth, const std::vector<gpc_hyper>& rgb)
{
    if ((!depth.empty() || !rgb.empty()) && !devices_.empty()) throw std::runtime_error(dense_candidates_sharded);
    dense_cand_depth_ = depth;
    dense_cand_rgb_ = rgb;
}

void gp_compressor::dense_plane(bool on_device, const std::vector<gpc_hyper>& cand, const int32_t* off, int n_max, int n_total,
                                const double* x0, const double* x1, const double* y, int ny, double* grid, int32_t* status, int32_t* best,
                                double* ev, const char* what)
{
    const int P = batch_.patches(), H = (int)cand.size();
    const std::string tag = std::string(H ? (on_device ? "gpc_dense_select_dev(" : "gpc_dense_select(")
                                          : (on_device ? "gpc_dense_fit_predict_grid_dev(" : "gpc_dense_fit_predict_grid(")) + what + ")";
    int rc;
    if (H == 0)
        rc = on_device ? gpc_dense_fit_predict_grid_dev(ctx_, &dense_params, P, off, n_max, n_total, x0, x1, y, ny, res_, sz_, grid, nullptr, status)
                       : gpc_dense_fit_predict_grid(ctx_, &dense_params, P, off, x0, x1, y, ny, res_, sz_, grid, nullptr, status);
    else
        rc = on_device ? gpc_dense_select_dev(ctx_, &dense_params, H, cand.data(), P, off, n_max, n_total, x0, x1, y, ny, 0, nullptr, nullptr,
                                              res_, sz_, grid, nullptr, nullptr, ev, best, nullptr, status)
                       : gpc_dense_select(ctx_, &dense_params, H, cand.data(), P, off, x0, x1, y, ny, 0, nullptr, nullptr, res_, sz_, grid,
                                          nullptr, nullptr, ev, best, nullptr, status);
    check(rc, ctx_, tag.c_str());
}

// src/gp_compressor.cpp:121-175, batched
void gp_compressor::train_processes()
{
    if (!projected_) project_cloud();
    const int P = batch_.patches();
    if (P == 0) { trained_ = true; return; }
    if (!ctx_) check(gpc_ctx_create(&ctx_, device_), nullptr, "gpc_ctx_create");
    const int m = sz_ * sz_;
    status_.assign(P, 0);
    gpc_patches_view dv{};
    const bool on_device = dev_patches_ != nullptr;
    if (on_device) gpc_patches_view_dev(dev_patches_, &dv);
    if (model_ == gp_model::dense) {
        const bool sel_d = !dense_cand_depth_.empty(), sel_c = !dense_cand_rgb_.empty();
        if ((sel_d || sel_c) && !devices_.empty()) throw std::runtime_error(dense_candidates_sharded);
        dense_best_depth_.clear();
        dense_best_rgb_.clear();
        dense_ev_depth_.clear();
        if (sel_d) { dense_best_depth_.assign(P, -1); dense_ev_depth_.assign(P, 0.0); }
        if (sel_c) dense_best_rgb_.assign(P, -1);
        if (on_device) {
            // depth and colour grids predicted straight from the device batch; they stay in HBM for load_compressed()
            drop_dense_grids();
            dev_buf f(ctx_, sizeof(double) * (size_t)P * m), c(ctx_, sizeof(double) * (size_t)P * 3 * m), st(ctx_, sizeof(int32_t) * (size_t)P);
            dev_buf bd, bc, ev;
            if (sel_d) { bd = dev_buf(ctx_, sizeof(int32_t) * (size_t)P); ev = dev_buf(ctx_, sizeof(double) * (size_t)P); }
            if (sel_c) bc = dev_buf(ctx_, sizeof(int32_t) * (size_t)P);
            dense_plane(true, dense_cand_depth_, dv.off, dv.n_max, dv.n_total, dv.x0, dv.x1, dv.y, 1, f.as<double>(), st.as<int32_t>(),
                        bd.as<int32_t>(), ev.as<double>(), "depth");
            dense_plane(true, dense_cand_rgb_, dv.off, dv.n_max, dv.n_total, dv.x0, dv.x1, dv.rgb, 3, c.as<double>(), st.as<int32_t>(),
                        bc.as<int32_t>(), nullptr, "rgb");
            st.download(status_.data(), sizeof(int32_t) * (size_t)P);
            if (sel_d) { bd.download(dense_best_depth_.data(), sizeof(int32_t) * (size_t)P); ev.download(dense_ev_depth_.data(), sizeof(double) * (size_t)P); }
            if (sel_c) bc.download(dense_best_rgb_.data(), sizeof(int32_t) * (size_t)P);
            d_dense_f_ = f.release<double>();         // kept only once both grids exist
            d_dense_c_ = c.release<double>();
        } else if (!devices_.empty()) {
            train_dense_sharded();
        } else {
            dense_f_.assign((size_t)P * m, 0.0);
            dense_c_.assign((size_t)P * 3 * m, 0.0);
            dense_plane(false, dense_cand_depth_, batch_.off.data(), 0, 0, batch_.x0.data(), batch_.x1.data(), batch_.y.data(), 1,
                        dense_f_.data(), status_.data(), dense_best_depth_.data(), dense_ev_depth_.data(), "depth");
            dense_plane(false, dense_cand_rgb_, batch_.off.data(), 0, 0, batch_.x0.data(), batch_.x1.data(), batch_.rgb.data(), 3,
                        dense_c_.data(), status_.data(), dense_best_rgb_.data(), nullptr, "rgb");
        }
        mean_added_ = 0;
        max_added_ = 0;
        for (int i = 0; i < P; ++i) {
            const int n = batch_.off[i + 1] - batch_.off[i];
            mean_added_ += n;
            max_added_ = std::max(max_added_, n);
        }
        mean_added_ /= P;
        trained_ = true;
        return;
    }
    const bool sharded = !devices_.empty();
    if (!sharded) {
        if (!gps_) check(gpc_sparse_create(ctx_, &depth_params, P, 1, &gps_), ctx_, "gpc_sparse_create(depth)");
        if (!rgb_gps_) check(gpc_sparse_create(ctx_, &rgb_params, P, 3, &rgb_gps_), ctx_, "gpc_sparse_create(rgb)");
    }
    // the reference shuffles inside gps[i].add_measurements and again inside RGB_gps[i].add_measurements, patch by
    // patch (:162-163): draw the two orders in that interleaving
    std::vector<int32_t> perm_d, perm_c;
    for (int i = 0; i < P; ++i) {
        const int n = batch_.off[i + 1] - batch_.off[i];
        shuffle(perm_d, n);
        shuffle(perm_c, n);
    }
    if (sharded) {
        train_sparse_sharded(perm_d, perm_c);
    } else if (on_device) {
        // the points are already in HBM: only the two insertion orders go up
        dev_buf pd(ctx_, perm_d), pc(ctx_, perm_c), st(ctx_, sizeof(int32_t) * (size_t)P);
        check(gpc_sparse_add_dev(gps_, dv.off, dv.n_max, dv.n_total, dv.x0, dv.x1, dv.y, pd.as<int32_t>(), st.as<int32_t>()),
              ctx_, "gpc_sparse_add_dev(depth)");
        check(gpc_sparse_add_dev(rgb_gps_, dv.off, dv.n_max, dv.n_total, dv.x0, dv.x1, dv.rgb, pc.as<int32_t>(), st.as<int32_t>()),
              ctx_, "gpc_sparse_add_dev(rgb)");
        st.download(status_.data(), sizeof(int32_t) * (size_t)P);
    } else {
        check(gpc_sparse_add(gps_, batch_.off.data(), batch_.x0.data(), batch_.x1.data(), batch_.y.data(), perm_d.data(),
                             status_.data()), ctx_, "gpc_sparse_add(depth)");
        check(gpc_sparse_add(rgb_gps_, batch_.off.data(), batch_.x0.data(), batch_.x1.data(), batch_.rgb.data(), perm_c.data(),
                             status_.data()), ctx_, "gpc_sparse_add(rgb)");
    }
    std::vector<int32_t> bv(P, 0);
    if (sharded) bv = shard_basis_sizes();
    else check(gpc_sparse_sizes(gps_, bv.data()), ctx_, "gpc_sparse_sizes");
    double mean = 0, added = 0;                  // "Mean added" / "Max added" (:164-168, 173-174)
    int maxm = 0;
    for (int i = 0; i < P; ++i) {
        if (batch_.off[i + 1] == batch_.off[i]) continue;
        mean = (added * mean + bv[i]) / (added + 1);
        maxm = std::max(maxm, (int)bv[i]);
        added += 1;
    }
    mean_added_ = mean;
    max_added_ = maxm;
    trained_ = true;
}

// src/gp_compressor.cpp:251-265 (x.cast<short>() as on x86-64, see oracle/gpc_oracle.c)
void gp_compressor::flatten_colors(uint8_t out[3], const double c[3])
{
    for (int i = 0; i < 3; ++i) {
        const double x = c[i];
        int v;
        if (std::isnan(x) || std::isinf(x)) {
            v = 255;
        } else {
            const int32_t w = (x >= 2147483648.0 || x < -2147483648.0) ? INT32_MIN : (int32_t)x;
            v = (int16_t)(uint16_t)(uint32_t)w;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
        }
        out[i] = (uint8_t)v;
    }
}

// src/gp_compressor.cpp:267-386
pointcloud gp_compressor::load_compressed()
{
    const int P = batch_.patches();
    const int m = sz_ * sz_;
    if (!trained_ || P == 0) return {};
    std::vector<double> xs0(m), xs1(m);
    int pcount = 0;
    for (int y = 0; y < sz_; ++y)                     // :320-331, y outer / x inner
        for (int x = 0; x < sz_; ++x) {
            xs0[pcount] = res_ * (((double)x + 0.5f) / (double)sz_ - 0.5f);
            xs1[pcount] = res_ * (((double)y + 0.5f) / (double)sz_ - 0.5f);
            ++pcount;
        }
    if (dev_patches_) {
        // predict (sparse) and reproject on the device; the records are the only download
        gpc_patches_view dv{};
        gpc_patches_view_dev(dev_patches_, &dv);
        std::vector<int32_t> bvh(P, 1);
        if (model_ == gp_model::dense) for (int i = 0; i < P; ++i) bvh[i] = batch_.off[i + 1] - batch_.off[i];
        else check(gpc_sparse_sizes(gps_, bvh.data()), ctx_, "gpc_sparse_sizes");
        dev_buf d_xs0(ctx_, xs0), d_xs1(ctx_, xs1), d_bv(ctx_, bvh), d_rec(ctx_, sizeof(gpc_point_xyzrgb) * (size_t)P * m), d_n(ctx_, 4);
        dev_buf d_f, d_c;                             // sparse model: the grids predicted now; the dense model kept its own from training
        const double *f = d_dense_f_, *c = d_dense_c_;
        if (model_ != gp_model::dense) {
            d_f = dev_buf(ctx_, sizeof(double) * (size_t)P * m);
            d_c = dev_buf(ctx_, sizeof(double) * (size_t)P * 3 * m);
            f = d_f.as<double>();
            c = d_c.as<double>();
            check(gpc_sparse_predict_dev(gps_, m, d_xs0.as<double>(), d_xs1.as<double>(), d_f.as<double>(), nullptr, 0, nullptr),
                  ctx_, "gpc_sparse_predict_dev(depth)");
            check(gpc_sparse_predict_dev(rgb_gps_, m, d_xs0.as<double>(), d_xs1.as<double>(), d_c.as<double>(), nullptr, 0, nullptr),
                  ctx_, "gpc_sparse_predict_dev(rgb)");
        }
        check(gpc_reproject_dev(ctx_, P, m, d_bv.as<int32_t>(), d_xs0.as<double>(), d_xs1.as<double>(), f, c, dv.rotations, dv.means,
                                dv.rgb_means, d_rec.as<gpc_point_xyzrgb>(), d_n.as<int32_t>()), ctx_, "gpc_reproject_dev");
        int32_t npts = 0;
        d_n.download(&npts, 4);
        std::vector<gpc_point_xyzrgb> recs((size_t)std::max(npts, 0));
        d_rec.download(recs.data(), sizeof(gpc_point_xyzrgb) * recs.size());
        return to_cloud(recs);
    }
    std::vector<double> f_star, c_star;
    std::vector<int32_t> bv(P, 1);
    if (model_ == gp_model::dense) {
        f_star = dense_f_;
        c_star = dense_c_;
        for (int i = 0; i < P; ++i) bv[i] = batch_.off[i + 1] - batch_.off[i];
    } else if (!devices_.empty()) {
        predict_sparse_sharded(xs0, xs1, f_star, c_star);
        bv = shard_basis_sizes();
    } else {
        f_star.assign((size_t)P * m, 0.0);
        c_star.assign((size_t)P * 3 * m, 0.0);
        check(gpc_sparse_sizes(gps_, bv.data()), ctx_, "gpc_sparse_sizes");
        // the caller discards V_star (:333-334), so sigma is not requested
        check(gpc_sparse_predict(gps_, m, xs0.data(), xs1.data(), f_star.data(), nullptr, 0, nullptr), ctx_, "gpc_sparse_predict(depth)");
        check(gpc_sparse_predict(rgb_gps_, m, xs0.data(), xs1.data(), c_star.data(), nullptr, 0, nullptr), ctx_, "gpc_sparse_predict(rgb)");
    }
    // reprojection + colour clamp (:335-373) fused on the GPU: the predicted grids become pcl::PointXYZRGB records
    std::vector<double> R((size_t)P * 9), mu((size_t)P * 3), cm((size_t)P * 3);
    for (int i = 0; i < P; ++i) {
        std::memcpy(&R[(size_t)i * 9], batch_.rotations[i].data(), 9 * sizeof(double));
        std::memcpy(&mu[(size_t)i * 3], batch_.means[i].data(), 3 * sizeof(double));
        std::memcpy(&cm[(size_t)i * 3], batch_.rgb_means[i].data(), 3 * sizeof(double));
    }
    std::vector<gpc_point_xyzrgb> recs((size_t)P * m);
    int32_t npts = 0;
    check(gpc_reproject(ctx_, P, m, bv.data(), xs0.data(), xs1.data(), f_star.data(), c_star.data(), R.data(), mu.data(), cm.data(),
                        recs.data(), &npts), ctx_, "gpc_reproject");
    recs.resize((size_t)npts);
    return to_cloud(recs);
}

// load_compressed() in one pass and only where the leaf holds data: gpc_sparse_decode under the occupancy mask W that project_points built
// for this purpose (:90-92, :117; its use at :323-325 is commented out upstream).  The records are those load_compressed() gives for the
// grid points whose cell of W is set, in the same order.  A model read from a file carries no W and decodes every point.
pointcloud gp_compressor::load_compressed_masked()
{
    if (model_ == gp_model::dense) throw std::runtime_error("load_compressed_masked: the sparse model only (the dense model keeps grids, not GP states)");
    if (!devices_.empty()) throw std::runtime_error("load_compressed_masked: the single-device flow only (the sharded states live on their devices)");
    const int P = batch_.patches();
    if (!trained_ || P == 0) return {};
    int32_t npts = 0;
    std::vector<gpc_point_xyzrgb> recs;
    if (dev_patches_) {
        // the batch is in HBM: a sizing call, then exactly that many records, which are the only download
        gpc_patches_view dv{};
        gpc_patches_view_dev(dev_patches_, &dv);
        dev_buf d_n(ctx_, 4);
        check(gpc_sparse_decode_dev(gps_, rgb_gps_, res_, sz_, dv.W, nullptr, dv.rotations, dv.means, dv.rgb_means, 0, nullptr, nullptr, nullptr,
                                    nullptr, d_n.as<int32_t>()), ctx_, "gpc_sparse_decode_dev (sizing)");
        d_n.download(&npts, 4);
        recs.resize((size_t)std::max(npts, 0));
        if (recs.empty()) return {};
        dev_buf d_rec(ctx_, sizeof(gpc_point_xyzrgb) * recs.size());
        check(gpc_sparse_decode_dev(gps_, rgb_gps_, res_, sz_, dv.W, nullptr, dv.rotations, dv.means, dv.rgb_means, npts,
                                    d_rec.as<gpc_point_xyzrgb>(), nullptr, nullptr, nullptr, d_n.as<int32_t>()), ctx_, "gpc_sparse_decode_dev");
        d_rec.download(recs.data(), sizeof(gpc_point_xyzrgb) * recs.size());
        return to_cloud(recs);
    }
    std::vector<double> R((size_t)P * 9), mu((size_t)P * 3), cm((size_t)P * 3);
    for (int i = 0; i < P; ++i) {
        std::memcpy(&R[(size_t)i * 9], batch_.rotations[i].data(), 9 * sizeof(double));
        std::memcpy(&mu[(size_t)i * 3], batch_.means[i].data(), 3 * sizeof(double));
        std::memcpy(&cm[(size_t)i * 3], batch_.rgb_means[i].data(), 3 * sizeof(double));
    }
    const uint8_t* W = batch_.W.size() == (size_t)P * sz_ * sz_ ? batch_.W.data() : nullptr;
    check(gpc_sparse_decode(gps_, rgb_gps_, res_, sz_, W, nullptr, R.data(), mu.data(), cm.data(), 0, nullptr, nullptr, nullptr, nullptr, &npts),
          ctx_, "gpc_sparse_decode (sizing)");
    recs.resize((size_t)std::max(npts, 0));
    if (recs.empty()) return {};
    check(gpc_sparse_decode(gps_, rgb_gps_, res_, sz_, W, nullptr, R.data(), mu.data(), cm.data(), npts, recs.data(), nullptr, nullptr, nullptr,
                            &npts), ctx_, "gpc_sparse_decode");
    return to_cloud(recs);
}

// The decoded cloud against the input cloud, both directions, through gpc_cloud_distortion; D2 along the producer's plane normals, which
// only the original side has.
distortion_stats gp_compressor::distortion(const pointcloud& decoded, double peak)
{
    if (!devices_.empty()) throw std::runtime_error("distortion: the single-device flow only");
    if (cloud_.empty()) throw std::runtime_error("distortion: the object holds no input cloud (a model read from a file does not)");
    if (!ctx_) check(gpc_ctx_create(&ctx_, device_), nullptr, "gpc_ctx_create");
    auto records = [](const pointcloud& c) {
        std::vector<gpc_point_xyzrgb> rec(c.size());
        for (size_t i = 0; i < c.size(); ++i) rec[i] = gpc_point_xyzrgb{c[i].x, c[i].y, c[i].z, 1.0f, c[i].b, c[i].g, c[i].r, 255, {0.0f, 0.0f, 0.0f}};
        return rec;
    };
    const std::vector<gpc_point_xyzrgb> orig = records(cloud_), dec = records(decoded);
    const int n = (int)orig.size(), nd = (int)dec.size();
    std::vector<float> normals(3 * orig.size());
    if (dev_patches_) {
        check(gpc_patches_normals(dev_patches_, n, normals.data()), ctx_, "gpc_patches_normals");
    } else {
        gpc_patches* cut = nullptr;
        check(gpc_project_cloud(ctx_, orig.data(), n, res_, sz_, &cut), ctx_, "gpc_project_cloud");
        const int rc = gpc_patches_normals(cut, n, normals.data());
        gpc_patches_destroy(cut);
        check(rc, ctx_, "gpc_patches_normals");
    }
    gpc_distortion_result r[2];
    check(gpc_cloud_distortion(ctx_, dec.data(), nd, orig.data(), n, normals.data(), nullptr, nullptr, nullptr, nullptr, &r[0]), ctx_,
          "gpc_cloud_distortion (decoded -> original)");
    check(gpc_cloud_distortion(ctx_, orig.data(), n, dec.data(), nd, nullptr, nullptr, nullptr, nullptr, nullptr, &r[1]), ctx_,
          "gpc_cloud_distortion (original -> decoded)");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    auto psnr = [&](double sse, long long count, double pk) {
        if (!(count > 0) || sse != sse) return nan;
        if (sse == 0) return std::numeric_limits<double>::infinity();
        return 10.0 * std::log10(pk * pk * (double)count / sse);
    };
    // both means, and the PSNR of the direction with the larger one
    auto metric = [&](const double sse[2], const long long count[2], double pk, double mse[2]) {
        int worst = -1;
        for (int d = 0; d < 2; ++d) {
            mse[d] = count[d] > 0 ? sse[d] / (double)count[d] : nan;
            if (mse[d] == mse[d] && (worst < 0 || mse[d] > mse[worst])) worst = d;
        }
        return worst < 0 ? nan : psnr(sse[worst], count[worst], pk);
    };
    distortion_stats s{};
    long long matched[2], plane[2];
    for (int d = 0; d < 2; ++d) {
        s.n_valid[d] = r[d].n_valid;
        matched[d] = s.n_matched[d] = r[d].n_matched;
        plane[d] = s.n_plane[d] = r[d].n_plane;
    }
    const double d1[2] = {r[0].sse_d1, r[1].sse_d1}, d2[2] = {r[0].sse_d2, r[1].sse_d2}, lu[2] = {r[0].sse_luma, r[1].sse_luma};
    s.psnr_d1 = metric(d1, matched, peak, s.mse_d1);
    s.psnr_d2 = metric(d2, plane, peak, s.mse_d2);
    s.psnr_luma = metric(lu, matched, 255.0, s.mse_luma);
    for (int c = 0; c < 3; ++c) {
        const double sc[2] = {r[0].sse_rgb[c], r[1].sse_rgb[c]};
        double mse[2];
        s.psnr_rgb[c] = metric(sc, matched, 255.0, mse);
        s.mse_rgb[0][c] = mse[0];
        s.mse_rgb[1][c] = mse[1];
    }
    return s;
}

// ---- model file (row f3) ---------------------------------------------------------------------------------------------
// little-endian; header: "GPCM", u32 version = 1, f64 res, i32 sz, i32 P, gpc_params depth, gpc_params rgb (raw structs, with their
// size in front); per patch: f64 R[9], mean[3], rgb_mean[3]; i32 b_depth, b_rgb; f64 BV_depth[b][2], alpha_depth[b],
// BV_rgb[b'][2], alpha_rgb[3][b'].
// version = 2 (save_model_quantized): the same header; per patch after b_depth, b_rgb: u8 w_depth, w_rgb; then per GP (depth, ny = 1; colour,
// ny = 3): w == 0: the raw doubles of version 1; w > 0: f32 (lo, hi) x (ny + 2) in the order BV column 0, BV column 1, the alpha planes, then
// the w-bit codes of BV0[0..b), BV1[0..b), alpha plane 0[0..b), .. packed LSB-first (code k holds bits k w .. (k + 1) w - 1 of the stream, bit
// j of the stream is bit j % 8 of byte j / 8), zero-padded to a whole byte per GP.  The values are v = lo + code * (hi - lo) / (2^w - 1)
// (include/gpc.h, gpc_sparse_quantize_rd).
namespace {
struct file_closer { void operator()(FILE* f) const { if (f) std::fclose(f); } };
template <class T> void wr(FILE* f, const T* p, size_t n) { if (n && std::fwrite(p, sizeof(T), n, f) != n) throw std::runtime_error("model file: write failed"); }
template <class T> void rd(FILE* f, T* p, size_t n) { if (n && std::fread(p, sizeof(T), n, f) != n) throw std::runtime_error("model file: truncated"); }

// one GP's codes as a bit stream, LSB-first
struct bit_packer {
    std::vector<uint8_t> bytes;
    uint64_t acc = 0;
    int held = 0;
    void put(uint32_t code, int w)
    {
        acc |= (uint64_t)(code & ((1u << w) - 1u)) << held;
        held += w;
        for (; held >= 8; held -= 8, acc >>= 8) bytes.push_back((uint8_t)(acc & 0xff));
    }
    void pad()
    {
        if (held > 0) bytes.push_back((uint8_t)(acc & 0xff));
        acc = 0;
        held = 0;
    }
};
struct bit_reader {
    const uint8_t* bytes;
    size_t pos = 0;
    uint64_t acc = 0;
    int held = 0;
    uint16_t get(int w)
    {
        for (; held < w; held += 8) acc |= (uint64_t)bytes[pos++] << held;
        const uint16_t code = (uint16_t)(acc & ((1u << w) - 1u));
        acc >>= w;
        held -= w;
        return code;
    }
};
size_t packed_bytes(int b, int ny, int w) { return ((size_t)b * (size_t)(ny + 2) * (size_t)w + 7) / 8; }

// what gpc_sparse_quantize_rd leaves of one GP, with the raw state beside it for the leaves that escape
struct quantized_gp {
    int ny = 1, ld = 0;
    std::vector<int32_t> b, bits;
    std::vector<uint16_t> qa, qb;       // [P][ny][ld], [P][ld][2]
    std::vector<float> range;           // [P][ny + 2][2]
    std::vector<double> alpha, bv;      // [P][ny][ld], [P][ld][2]
};

// the GP of patch i as version 2 stores it
void write_gp_v2(FILE* f, const quantized_gp& q, int i)
{
    const int ny = q.ny, ld = q.ld, b = q.b[i], w = q.bits[i];
    const double* bv = &q.bv[(size_t)i * ld * 2];
    if (w == 0) {
        wr(f, bv, (size_t)2 * b);
        for (int c = 0; c < ny; ++c) wr(f, &q.alpha[((size_t)i * ny + c) * ld], (size_t)b);
        return;
    }
    wr(f, &q.range[(size_t)i * (ny + 2) * 2], (size_t)(ny + 2) * 2);
    bit_packer pk;
    pk.bytes.reserve(packed_bytes(b, ny, w));
    for (int col = 0; col < 2; ++col)
        for (int k = 0; k < b; ++k) pk.put(q.qb[((size_t)i * ld + k) * 2 + col], w);
    for (int c = 0; c < ny; ++c)
        for (int k = 0; k < b; ++k) pk.put(q.qa[((size_t)i * ny + c) * ld + k], w);
    pk.pad();
    wr(f, pk.bytes.data(), pk.bytes.size());
}

// ... and read back: a raw leaf into alpha / bv, a quantised one into range / qa / qb
void read_gp_v2(FILE* f, quantized_gp& q, int i)
{
    const int ny = q.ny, ld = q.ld, b = q.b[i], w = q.bits[i];
    if (w == 0) {
        rd(f, &q.bv[(size_t)i * ld * 2], (size_t)2 * b);
        for (int c = 0; c < ny; ++c) rd(f, &q.alpha[((size_t)i * ny + c) * ld], (size_t)b);
        return;
    }
    rd(f, &q.range[(size_t)i * (ny + 2) * 2], (size_t)(ny + 2) * 2);
    std::vector<uint8_t> bytes(packed_bytes(b, ny, w));
    rd(f, bytes.data(), bytes.size());
    bit_reader br{bytes.data()};
    for (int col = 0; col < 2; ++col)
        for (int k = 0; k < b; ++k) q.qb[((size_t)i * ld + k) * 2 + col] = br.get(w);
    for (int c = 0; c < ny; ++c)
        for (int k = 0; k < b; ++k) q.qa[((size_t)i * ny + c) * ld + k] = br.get(w);
}

void size_gp(quantized_gp& q, int P, int ny, int ld)
{
    q.ny = ny; q.ld = ld;
    q.b.assign(P, 0);
    q.bits.assign(P, 0);
    q.qa.assign((size_t)P * ny * ld, 0);
    q.qb.assign((size_t)P * ld * 2, 0);
    q.range.assign((size_t)P * (ny + 2) * 2, 0.0f);
    q.alpha.assign((size_t)P * ny * ld, 0.0);
    q.bv.assign((size_t)P * ld * 2, 0.0);
}
}  // namespace

size_t gp_compressor::save_model(const std::string& path)
{
    if (model_ != gp_model::sparse) throw std::runtime_error("save_model: the sparse model only");
    if (!devices_.empty()) throw std::runtime_error("save_model: the single-device flow only (the sharded states live on their devices)");
    if (!trained_) { project_cloud(); train_processes(); }
    const int P = batch_.patches();
    std::unique_ptr<FILE, file_closer> f(std::fopen(path.c_str(), "wb"));
    if (!f) throw std::runtime_error("save_model: cannot open " + path);
    const uint32_t version = 1, psz = (uint32_t)sizeof(gpc_params);
    wr(f.get(), "GPCM", 4);
    wr(f.get(), &version, 1);
    wr(f.get(), &res_, 1);
    const int32_t hdr[2] = {sz_, P};
    wr(f.get(), hdr, 2);
    wr(f.get(), &psz, 1);
    wr(f.get(), &depth_params, 1);
    wr(f.get(), &rgb_params, 1);
    if (P > 0) {
        const int ldd = gpc_sparse_ld(gps_), ldc = gpc_sparse_ld(rgb_gps_);
        std::vector<int32_t> bd(P), bc(P);
        check(gpc_sparse_sizes(gps_, bd.data()), ctx_, "gpc_sparse_sizes");
        check(gpc_sparse_sizes(rgb_gps_, bc.data()), ctx_, "gpc_sparse_sizes");
        std::vector<double> ad((size_t)P * ldd), bvd((size_t)P * ldd * 2), ac((size_t)P * 3 * ldc), bvc((size_t)P * ldc * 2);
        check(gpc_sparse_get_state(gps_, ad.data(), nullptr, nullptr, bvd.data()), ctx_, "gpc_sparse_get_state");
        check(gpc_sparse_get_state(rgb_gps_, ac.data(), nullptr, nullptr, bvc.data()), ctx_, "gpc_sparse_get_state");
        for (int i = 0; i < P; ++i) {
            wr(f.get(), batch_.rotations[i].data(), 9);
            wr(f.get(), batch_.means[i].data(), 3);
            wr(f.get(), batch_.rgb_means[i].data(), 3);
            const int32_t b2[2] = {bd[i], bc[i]};
            wr(f.get(), b2, 2);
            wr(f.get(), &bvd[(size_t)i * ldd * 2], (size_t)2 * bd[i]);
            wr(f.get(), &ad[(size_t)i * ldd], (size_t)bd[i]);
            wr(f.get(), &bvc[(size_t)i * ldc * 2], (size_t)2 * bc[i]);
            for (int c = 0; c < 3; ++c) wr(f.get(), &ac[((size_t)i * 3 + c) * ldc], (size_t)bc[i]);
        }
    }
    const long pos = std::ftell(f.get());
    return pos < 0 ? 0 : (size_t)pos;
}

size_t gp_compressor::save_model_quantized(const std::string& path, double max_mse_depth, double max_mse_rgb, int bits_min, int bits_max)
{
    if (model_ != gp_model::sparse) throw std::runtime_error("save_model_quantized: the sparse model only");
    if (!devices_.empty())
        throw std::runtime_error("save_model_quantized: the single-device flow only (the sharded states live on their devices)");
    if (loaded_)
        throw std::runtime_error("save_model_quantized: a loaded model has no training points; quantise the trained object");
    if (!trained_) { project_cloud(); train_processes(); }
    const int P = batch_.patches();
    quantized_gp qd, qc;
    if (P > 0) {
        size_gp(qd, P, 1, gpc_sparse_ld(gps_));
        size_gp(qc, P, 3, gpc_sparse_ld(rgb_gps_));
        const double* ys[2] = {batch_.y.data(), batch_.rgb.data()};
        const double bound[2] = {max_mse_depth, max_mse_rgb};
        gpc_sparse* gp[2] = {gps_, rgb_gps_};
        quantized_gp* q[2] = {&qd, &qc};
        for (int k = 0; k < 2; ++k) {
            check(gpc_sparse_sizes(gp[k], q[k]->b.data()), ctx_, "gpc_sparse_sizes");
            check(gpc_sparse_get_state(gp[k], q[k]->alpha.data(), nullptr, nullptr, q[k]->bv.data()), ctx_, "gpc_sparse_get_state");
            check(gpc_sparse_quantize_rd(gp[k], batch_.off.data(), batch_.x0.data(), batch_.x1.data(), ys[k], bits_min, bits_max, bound[k], nullptr,
                                         q[k]->bits.data(), q[k]->qa.data(), q[k]->qb.data(), q[k]->range.data(), nullptr, nullptr, nullptr,
                                         nullptr),
                  ctx_, k == 0 ? "gpc_sparse_quantize_rd(depth)" : "gpc_sparse_quantize_rd(rgb)");
            // a leaf whose quantised form (ranges + codes) would not be smaller than its raw doubles -- one vector -- stays raw
            for (int i = 0; i < P; ++i) {
                const size_t na = (size_t)q[k]->ny + 2, b = (size_t)q[k]->b[i];
                if (q[k]->bits[i] > 0 && 8 * na + packed_bytes((int)b, q[k]->ny, q[k]->bits[i]) >= 8 * b * na) q[k]->bits[i] = 0;
            }
        }
    }
    std::unique_ptr<FILE, file_closer> f(std::fopen(path.c_str(), "wb"));
    if (!f) throw std::runtime_error("save_model_quantized: cannot open " + path);
    const uint32_t version = 2, psz = (uint32_t)sizeof(gpc_params);
    wr(f.get(), "GPCM", 4);
    wr(f.get(), &version, 1);
    wr(f.get(), &res_, 1);
    const int32_t hdr[2] = {sz_, P};
    wr(f.get(), hdr, 2);
    wr(f.get(), &psz, 1);
    wr(f.get(), &depth_params, 1);
    wr(f.get(), &rgb_params, 1);
    for (int i = 0; i < P; ++i) {
        wr(f.get(), batch_.rotations[i].data(), 9);
        wr(f.get(), batch_.means[i].data(), 3);
        wr(f.get(), batch_.rgb_means[i].data(), 3);
        const int32_t b2[2] = {qd.b[i], qc.b[i]};
        wr(f.get(), b2, 2);
        const uint8_t w2[2] = {(uint8_t)qd.bits[i], (uint8_t)qc.bits[i]};
        wr(f.get(), w2, 2);
        write_gp_v2(f.get(), qd, i);
        write_gp_v2(f.get(), qc, i);
    }
    const long pos = std::ftell(f.get());
    return pos < 0 ? 0 : (size_t)pos;
}

gp_compressor* gp_compressor::load_model(const std::string& path, int device)
{
    std::unique_ptr<FILE, file_closer> f(std::fopen(path.c_str(), "rb"));
    if (!f) throw std::runtime_error("load_model: cannot open " + path);
    char magic[4];
    uint32_t version = 0, psz = 0;
    double res = 0;
    int32_t hdr[2] = {0, 0};
    rd(f.get(), magic, 4);
    rd(f.get(), &version, 1);
    if (std::memcmp(magic, "GPCM", 4) != 0 || (version != 1 && version != 2)) throw std::runtime_error("load_model: not a GPCM v1 or v2 file");
    rd(f.get(), &res, 1);
    rd(f.get(), hdr, 2);
    rd(f.get(), &psz, 1);
    if (psz != sizeof(gpc_params) || hdr[0] <= 0 || hdr[1] < 0) throw std::runtime_error("load_model: bad header");
    std::unique_ptr<gp_compressor> g(new gp_compressor(res, hdr[0], device));
    rd(f.get(), &g->depth_params, 1);
    rd(f.get(), &g->rgb_params, 1);
    const int P = hdr[1];
    g->batch_.off.assign((size_t)P + 1, 0);
    g->batch_.rotations.resize(P);
    g->batch_.means.resize(P);
    g->batch_.rgb_means.resize(P);
    g->projected_ = true;
    if (P > 0) {
        check(gpc_ctx_create(&g->ctx_, device), nullptr, "gpc_ctx_create");
        check(gpc_sparse_create(g->ctx_, &g->depth_params, P, 1, &g->gps_), g->ctx_, "gpc_sparse_create(depth)");
        check(gpc_sparse_create(g->ctx_, &g->rgb_params, P, 3, &g->rgb_gps_), g->ctx_, "gpc_sparse_create(rgb)");
        const int ldd = gpc_sparse_ld(g->gps_), ldc = gpc_sparse_ld(g->rgb_gps_);
        quantized_gp qd, qc;                 // (version 1: every width 0, every leaf raw)
        size_gp(qd, P, 1, ldd);
        size_gp(qc, P, 3, ldc);
        bool any_quantized = false;
        for (int i = 0; i < P; ++i) {
            rd(f.get(), g->batch_.rotations[i].data(), 9);
            rd(f.get(), g->batch_.means[i].data(), 3);
            rd(f.get(), g->batch_.rgb_means[i].data(), 3);
            int32_t b2[2];
            rd(f.get(), b2, 2);
            if (b2[0] < 0 || b2[0] > ldd || b2[1] < 0 || b2[1] > ldc) throw std::runtime_error("load_model: basis-vector count out of range");
            uint8_t w2[2] = {0, 0};
            if (version == 2) rd(f.get(), w2, 2);
            if (w2[0] > 16 || w2[1] > 16) throw std::runtime_error("load_model: code width out of range");
            qd.b[i] = b2[0];
            qc.b[i] = b2[1];
            qd.bits[i] = w2[0];
            qc.bits[i] = w2[1];
            any_quantized = any_quantized || w2[0] || w2[1];
            read_gp_v2(f.get(), qd, i);
            read_gp_v2(f.get(), qc, i);
        }
        // the raw leaves (a quantised one: zeros for now), then the decoder over the quantised ones
        check(gpc_sparse_set_state(g->gps_, qd.b.data(), qd.alpha.data(), nullptr, nullptr, qd.bv.data()), g->ctx_, "gpc_sparse_set_state(depth)");
        check(gpc_sparse_set_state(g->rgb_gps_, qc.b.data(), qc.alpha.data(), nullptr, nullptr, qc.bv.data()), g->ctx_, "gpc_sparse_set_state(rgb)");
        if (any_quantized) {
            check(gpc_sparse_dequantize(g->gps_, qd.b.data(), qd.bits.data(), qd.qa.data(), qd.qb.data(), qd.range.data()), g->ctx_,
                  "gpc_sparse_dequantize(depth)");
            check(gpc_sparse_dequantize(g->rgb_gps_, qc.b.data(), qc.bits.data(), qc.qa.data(), qc.qb.data(), qc.range.data()), g->ctx_,
                  "gpc_sparse_dequantize(rgb)");
        }
    }
    g->trained_ = true;
    g->loaded_ = true;
    return g.release();
}

std::array<long long, 2> gp_compressor::prune(int keep_depth, int keep_rgb, double tol_depth, double tol_rgb)
{
    if (model_ != gp_model::sparse) throw std::runtime_error("prune: the sparse model only");
    if (!devices_.empty()) throw std::runtime_error("prune: the single-device flow only (the sharded states live on their devices)");
    if (loaded_) throw std::runtime_error("prune: a loaded model holds (BV, alpha) only; prune the trained object before save_model");
    if (!trained_) { project_cloud(); train_processes(); }
    const int P = batch_.patches();
    std::array<long long, 2> total = {0, 0};
    if (P <= 0) return total;
    std::vector<int32_t> rd_((size_t)P), rc_((size_t)P);
    check(gpc_sparse_prune(gps_, keep_depth, nullptr, tol_depth, rd_.data(), nullptr, nullptr, nullptr), ctx_, "gpc_sparse_prune(depth)");
    check(gpc_sparse_prune(rgb_gps_, keep_rgb, nullptr, tol_rgb, rc_.data(), nullptr, nullptr, nullptr), ctx_, "gpc_sparse_prune(rgb)");
    for (int i = 0; i < P; ++i) { total[0] += rd_[i]; total[1] += rc_[i]; }
    return total;
}

std::array<long long, 2> gp_compressor::prune_to_error(double max_mse_depth, double max_mse_rgb, int keep_depth, int keep_rgb)
{
    if (model_ != gp_model::sparse) throw std::runtime_error("prune_to_error: the sparse model only");
    if (!devices_.empty()) throw std::runtime_error("prune_to_error: the single-device flow only (the sharded states live on their devices)");
    if (loaded_) throw std::runtime_error("prune_to_error: a loaded model holds (BV, alpha) only; prune the trained object before save_model");
    if (!trained_) { project_cloud(); train_processes(); }
    const int P = batch_.patches();
    std::array<long long, 2> total = {0, 0};
    if (P <= 0) return total;
    std::vector<int32_t> rd_((size_t)P), rc_((size_t)P);
    check(gpc_sparse_prune_rd(gps_, batch_.off.data(), batch_.x0.data(), batch_.x1.data(), batch_.y.data(), keep_depth, nullptr, max_mse_depth,
                              nullptr, rd_.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
          ctx_, "gpc_sparse_prune_rd(depth)");
    check(gpc_sparse_prune_rd(rgb_gps_, batch_.off.data(), batch_.x0.data(), batch_.x1.data(), batch_.rgb.data(), keep_rgb, nullptr, max_mse_rgb,
                              nullptr, rc_.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
          ctx_, "gpc_sparse_prune_rd(rgb)");
    for (int i = 0; i < P; ++i) { total[0] += rd_[i]; total[1] += rc_[i]; }
    return total;
}

size_t gp_compressor::model_bytes() const
{
    if (model_ != gp_model::sparse) throw std::runtime_error("model_bytes: the sparse model only");
    if (!devices_.empty()) throw std::runtime_error("model_bytes: the single-device flow only (the sharded states live on their devices)");
    if (!trained_) throw std::runtime_error("model_bytes: the object is not trained yet");
    const int P = batch_.patches();
    size_t bytes = 4 + sizeof(uint32_t) + sizeof(double) + 2 * sizeof(int32_t) + sizeof(uint32_t) + 2 * sizeof(gpc_params);
    if (P <= 0) return bytes;
    std::vector<int32_t> bd((size_t)P), bc((size_t)P);
    check(gpc_sparse_sizes(gps_, bd.data()), ctx_, "gpc_sparse_sizes");
    check(gpc_sparse_sizes(rgb_gps_, bc.data()), ctx_, "gpc_sparse_sizes");
    for (int i = 0; i < P; ++i) bytes += 15 * sizeof(double) + 2 * sizeof(int32_t) + (size_t)24 * bd[i] + (size_t)40 * bc[i];
    return bytes;
}

std::array<long long, 2> gp_compressor::prune_to_bytes(size_t budget_bytes, double w_depth, double w_rgb)
{
    if (model_ != gp_model::sparse) throw std::runtime_error("prune_to_bytes: the sparse model only");
    if (!devices_.empty()) throw std::runtime_error("prune_to_bytes: the single-device flow only (the sharded states live on their devices)");
    if (loaded_) throw std::runtime_error("prune_to_bytes: a loaded model holds (BV, alpha) only; prune the trained object before save_model");
    if (!(w_depth >= 0.0) || !(w_rgb >= 0.0)) throw std::runtime_error("prune_to_bytes: the weights must be >= 0 (0: normalise)");
    if (!trained_) { project_cloud(); train_processes(); }
    const int P = batch_.patches();
    std::array<long long, 2> total = {0, 0};
    const size_t now = model_bytes();
    if (P <= 0) {
        if (budget_bytes < now) throw std::runtime_error("prune_to_bytes: the budget is below the floor of " + std::to_string(now) + " bytes");
        return total;
    }
    const long long need = (long long)now - (long long)budget_bytes;
    gpc_sparse* const gp[2] = {gps_, rgb_gps_};
    const double* const ys[2] = {batch_.y.data(), batch_.rgb.data()};
    const int ny[2] = {1, 3}, unit_of[2] = {24, 40}, ldg[2] = {gpc_sparse_ld(gps_), gpc_sparse_ld(rgb_gps_)};
    const double wg[2] = {w_depth, w_rgb};
    const int ld = std::max(ldg[0], ldg[1]);
    const size_t R = (size_t)2 * P;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<int32_t> kmax(R, 0), unit(R), count(R), k(R), target(R), ident((size_t)P);
    std::vector<double> d0(R, nan), d(R * (size_t)ld, nan), w(R);
    for (int i = 0; i < P; ++i) ident[i] = i;
    for (int g = 0; g < 2; ++g) {
        // the curves: every removal of the chain with its error, on a copy
        gpc_sparse* cp = nullptr;
        check(gpc_sparse_remap(gp[g], P, ident.data(), &cp), ctx_, "gpc_sparse_remap");
        std::vector<double> mse((size_t)P * ldg[g], nan);
        const int rc = gpc_sparse_prune_rd(cp, batch_.off.data(), batch_.x0.data(), batch_.x1.data(), ys[g], 1, nullptr,
                                           std::numeric_limits<double>::infinity(), nullptr, &kmax[(size_t)g * P], nullptr, nullptr, mse.data(),
                                           &d0[(size_t)g * P], nullptr, nullptr);
        gpc_sparse_destroy(cp);
        check(rc, ctx_, "gpc_sparse_prune_rd (curves)");
        check(gpc_sparse_sizes(gp[g], &count[(size_t)g * P]), ctx_, "gpc_sparse_sizes");
        double sum = 0.0;                       // sum_p n_p ny mse0_p in ascending leaf order
        for (int i = 0; i < P; ++i) {
            const size_t r = (size_t)g * P + i;
            std::memcpy(&d[r * ld], &mse[(size_t)i * ldg[g]], sizeof(double) * ldg[g]);
            unit[r] = unit_of[g];
            const double n = (double)(batch_.off[i + 1] - batch_.off[i]);
            if (n > 0 && std::isfinite(d0[r])) sum += n * (double)ny[g] * d0[r];
        }
        const double scale = wg[g] != 0.0 ? wg[g] : ((sum > 0.0 && std::isfinite(sum)) ? 1.0 / sum : 1.0);
        for (int i = 0; i < P; ++i) w[(size_t)g * P + i] = scale * (double)(batch_.off[i + 1] - batch_.off[i]) * (double)ny[g];
    }
    gpc_rate_result res = {};
    check(gpc_rate_allocate(ctx_, (int)R, ld, kmax.data(), d0.data(), d.data(), w.data(), 0.0, unit.data(), 0, (int64_t)need, 1, count.data(),
                            k.data(), target.data(), &res),
          ctx_, "gpc_rate_allocate");
    if (!res.feasible)
        throw std::runtime_error("prune_to_bytes: a budget of " + std::to_string(budget_bytes) + " bytes is below the floor of " +
                                 std::to_string((long long)now - (long long)res.max_saving) + " bytes (the model holds " + std::to_string(now) + ")");
    std::vector<int32_t> removed(R);
    for (int g = 0; g < 2; ++g)
        check(gpc_sparse_prune(gp[g], 0, &target[(size_t)g * P], 0.0, &removed[(size_t)g * P], nullptr, nullptr, nullptr), ctx_, "gpc_sparse_prune");
    for (int g = 0; g < 2; ++g)
        for (int i = 0; i < P; ++i) total[g] += removed[(size_t)g * P + i];
    return total;
}

}  // namespace gpc

// ---- C doors for the Python test-suite -----------------------------------------------------------------------------
namespace {
int fail(const std::exception& e, char* err, int errlen)
{
    if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", e.what());
    return -1;
}
// out_xyz / out_rgb hold up to capacity_pts points: the count, or -2 when the cloud does not fit
int put_cloud(const gpc::pointcloud& c, float* out_xyz, uint8_t* out_rgb, int capacity_pts)
{
    if ((int)c.size() > capacity_pts) return -2;
    for (size_t i = 0; i < c.size(); ++i) {
        out_xyz[3 * i] = c[i].x; out_xyz[3 * i + 1] = c[i].y; out_xyz[3 * i + 2] = c[i].z;
        out_rgb[3 * i] = c[i].r; out_rgb[3 * i + 1] = c[i].g; out_rgb[3 * i + 2] = c[i].b;
    }
    return (int)c.size();
}
// the slot table of a `world`-device run as the dense (sparse == 0) or the sparse flow deals it
std::vector<int32_t> table_of(const gpc::gp_compressor* g, int world, int sparse)
{
    return gpc::deal_patches(g->patches(), world, sparse ? gpc::sparse_cost(g->depth_params) : 0);
}
template <class T> void put(const std::vector<T>& v, T* out) { if (out && !v.empty()) std::memcpy(out, v.data(), sizeof(T) * v.size()); }
}  // namespace

extern "C" {

// host-only: cut and project the patches of a cloud (no GPU needed).  Returns an opaque handle.
void* gpc_host_create(const float* xyz, const uint8_t* rgb, int n, double res, int sz, int model, int device)
{
    gpc::pointcloud c((size_t)n);
    for (int i = 0; i < n; ++i) c[i] = gpc::point{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
    return new gpc::gp_compressor(c, res, sz, model == 1 ? gpc::gp_model::dense : gpc::gp_model::sparse, device);
}
void gpc_host_destroy(void* h) { delete static_cast<gpc::gp_compressor*>(h); }
void gpc_host_seed(void* h, unsigned seed)
{
    // deterministic stand-in for libc rand(): a 31-bit LCG owned by the object
    auto* g = static_cast<gpc::gp_compressor*>(h);
    auto state = std::make_shared<uint64_t>(seed);
    g->rng = [state]() -> int {
        *state = (*state * 6364136223846793005ULL + 1442695040888963407ULL);
        return (int)((*state >> 33) & 0x7fffffff);
    };
}
void gpc_host_set_sparse_kernel(void* h, double sigmaf_sq, double l_sq, double s20_depth, double s20_rgb, int capacity)
{
    auto* g = static_cast<gpc::gp_compressor*>(h);
    g->depth_params.sigmaf_sq = g->rgb_params.sigmaf_sq = sigmaf_sq;
    g->depth_params.l_sq = g->rgb_params.l_sq = l_sq;
    g->depth_params.noise = s20_depth;
    g->rgb_params.noise = s20_rgb;
    g->depth_params.capacity = g->rgb_params.capacity = capacity;
}
// rgb_params.ref_field_delete_bug (the class's default is the reference's multiply, 1): 0 lets the colour field delete as its derivation
// says, which is what pruning colour below a few vectors needs (include/gpc.h, gpc_sparse_prune).  Before training.
void gpc_host_set_field_delete_bug(void* h, int on)
{
    static_cast<gpc::gp_compressor*>(h)->rgb_params.ref_field_delete_bug = on ? 1 : 0;
}
int gpc_host_project(void* h)
{
    try { static_cast<gpc::gp_compressor*>(h)->project_cloud(); return 0; } catch (...) { return -1; }
}
int gpc_host_project_device(void* h, char* err, int errlen)
{
    try { static_cast<gpc::gp_compressor*>(h)->project_cloud_device(); return 0; }
    catch (const std::exception& e) { return fail(e, err, errlen); }
}
int gpc_host_set_devices(void* h, const int* devices, int n, char* err, int errlen)
{
    try { static_cast<gpc::gp_compressor*>(h)->set_devices(std::vector<int>(devices, devices + (n > 0 ? n : 0))); return 0; }
    catch (const std::exception& e) { return fail(e, err, errlen); }
}
// candidates as (sigmaf_sq, l_sq, noise) triples, nd for the depth plane and nc for the colour planes (0: that plane keeps dense_params)
int gpc_host_set_dense_candidates(void* h, const double* depth, int nd, const double* rgb, int nc, char* err, int errlen)
{
    try {
        std::vector<gpc_hyper> d, c;
        for (int i = 0; i < nd; ++i) d.push_back(gpc_hyper{depth[3 * i], depth[3 * i + 1], depth[3 * i + 2]});
        for (int i = 0; i < nc; ++i) c.push_back(gpc_hyper{rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]});
        static_cast<gpc::gp_compressor*>(h)->set_dense_candidates(d, c);
        return 0;
    } catch (const std::exception& e) { return fail(e, err, errlen); }
}
// which: 0 dense_best_depth, 1 dense_best_rgb; returns the length (0 without candidates); out may be NULL to ask for it
int gpc_host_dense_best(void* h, int which, int32_t* out)
{
    const auto* g = static_cast<gpc::gp_compressor*>(h);
    const std::vector<int32_t>& v = which ? g->dense_best_rgb() : g->dense_best_depth();
    if (out && !v.empty()) std::memcpy(out, v.data(), sizeof(int32_t) * v.size());
    return (int)v.size();
}
const char* gpc_host_last_dense_kernel(void* h) { return static_cast<gpc::gp_compressor*>(h)->last_dense_kernel(); }
int gpc_host_dense_evidence_depth(void* h, double* out)
{
    const std::vector<double>& v = static_cast<gpc::gp_compressor*>(h)->dense_evidence_depth();
    if (out && !v.empty()) std::memcpy(out, v.data(), sizeof(double) * v.size());
    return (int)v.size();
}
void gpc_host_set_gpu_producer(void* h, int on) { static_cast<gpc::gp_compressor*>(h)->gpu_producer = on != 0; }
int gpc_host_patch_count(void* h) { return static_cast<gpc::gp_compressor*>(h)->patches().patches(); }
int gpc_host_point_count(void* h) { return (int)static_cast<gpc::gp_compressor*>(h)->patches().x0.size(); }
// copies the batch: off[P+1], x0/x1/y[N], rgb[3N], R[9P], mean[3P], rgb_mean[3P]
void gpc_host_get_batch(void* h, int32_t* off, double* x0, double* x1, double* y, double* rgb, double* R, double* mean,
                        double* rgb_mean)
{
    const gpc::patch_batch& b = static_cast<gpc::gp_compressor*>(h)->patches();
    std::memcpy(off, b.off.data(), sizeof(int32_t) * b.off.size());
    const size_t N = b.x0.size(), P = (size_t)b.patches();
    std::memcpy(x0, b.x0.data(), 8 * N);
    std::memcpy(x1, b.x1.data(), 8 * N);
    std::memcpy(y, b.y.data(), 8 * N);
    std::memcpy(rgb, b.rgb.data(), 8 * 3 * N);
    for (size_t i = 0; i < P; ++i) {
        std::memcpy(R + 9 * i, b.rotations[i].data(), 72);
        std::memcpy(mean + 3 * i, b.means[i].data(), 24);
        std::memcpy(rgb_mean + 3 * i, b.rgb_means[i].data(), 24);
    }
}
// GPU: save_compressed + load_compressed.  out_xyz / out_rgb hold up to P*sz*sz points; returns the count or < 0.
void gpc_host_get_mask(void* h, uint8_t* W)
{
    const auto& b = static_cast<gpc::gp_compressor*>(h)->patches();
    if (!b.W.empty()) std::memcpy(W, b.W.data(), b.W.size());
}

int gpc_host_roundtrip(void* h, float* out_xyz, uint8_t* out_rgb, int capacity_pts, double* mean_added, int* max_added,
                       char* err, int errlen)
{
    auto* g = static_cast<gpc::gp_compressor*>(h);
    try {
        g->save_compressed("unused");
        const int n = put_cloud(g->load_compressed(), out_xyz, out_rgb, capacity_pts);
        if (mean_added) *mean_added = g->mean_added();
        if (max_added) *max_added = g->max_added();
        return n;
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}

// model file: write the trained sparse model / reconstruct a cloud from a file alone.  Return bytes / point count, < 0 on error.
long long gpc_host_save_model(void* h, const char* path, char* err, int errlen)
{
    try {
        return (long long)static_cast<gpc::gp_compressor*>(h)->save_model(path);
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}
// the bit-packed model file: gp_compressor::save_model_quantized (trains first if needed).  Returns bytes, < 0 on error.
long long gpc_host_save_model_quantized(void* h, const char* path, double max_mse_depth, double max_mse_rgb, int bits_min, int bits_max,
                                        char* err, int errlen)
{
    try {
        return (long long)static_cast<gpc::gp_compressor*>(h)->save_model_quantized(path, max_mse_depth, max_mse_rgb, bits_min, bits_max);
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}
// rate control: gp_compressor::prune (trains first if needed); removed[2] = vectors removed {depth, colour}.  Returns 0, or < 0 on error.
int gpc_host_prune(void* h, int keep_depth, int keep_rgb, double tol_depth, double tol_rgb, long long removed[2], char* err, int errlen)
{
    try {
        const auto r = static_cast<gpc::gp_compressor*>(h)->prune(keep_depth, keep_rgb, tol_depth, tol_rgb);
        if (removed) { removed[0] = r[0]; removed[1] = r[1]; }
        return 0;
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}
// rate control against a distortion bound: gp_compressor::prune_to_error (trains first if needed); removed[2] as above.  0, or < 0 on error.
int gpc_host_prune_to_error(void* h, double max_mse_depth, double max_mse_rgb, int keep_depth, int keep_rgb, long long removed[2], char* err,
                            int errlen)
{
    try {
        const auto r = static_cast<gpc::gp_compressor*>(h)->prune_to_error(max_mse_depth, max_mse_rgb, keep_depth, keep_rgb);
        if (removed) { removed[0] = r[0]; removed[1] = r[1]; }
        return 0;
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}
// the exact size of the file save_model would write now: gp_compressor::model_bytes.  Bytes, or < 0 on error.
long long gpc_host_model_bytes(void* h, char* err, int errlen)
{
    try {
        return (long long)static_cast<gpc::gp_compressor*>(h)->model_bytes();
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}
// rate control to a byte budget: gp_compressor::prune_to_bytes (trains first if needed); removed[2] as above.  0, or < 0 on error.
int gpc_host_prune_to_bytes(void* h, long long budget_bytes, double w_depth, double w_rgb, long long removed[2], char* err, int errlen)
{
    try {
        if (budget_bytes < 0) throw std::runtime_error("prune_to_bytes: a negative budget");
        const auto r = static_cast<gpc::gp_compressor*>(h)->prune_to_bytes((size_t)budget_bytes, w_depth, w_rgb);
        if (removed) { removed[0] = r[0]; removed[1] = r[1]; }
        return 0;
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}
// load_compressed() of the object as it stands (trained, possibly pruned): the point count or < 0
int gpc_host_load_compressed(void* h, float* out_xyz, uint8_t* out_rgb, int capacity_pts, char* err, int errlen)
{
    try {
        return put_cloud(static_cast<gpc::gp_compressor*>(h)->load_compressed(), out_xyz, out_rgb, capacity_pts);
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}
// load_compressed_masked() of the object as it stands: the point count or < 0
int gpc_host_load_compressed_masked(void* h, float* out_xyz, uint8_t* out_rgb, int capacity_pts, char* err, int errlen)
{
    try {
        return put_cloud(static_cast<gpc::gp_compressor*>(h)->load_compressed_masked(), out_xyz, out_rgb, capacity_pts);
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}
// gp_compressor::distortion of the cloud (xyz, rgb; n points) against the object's input cloud.  out[24]: n_valid[2], n_matched[2],
// n_plane[2] (as doubles), mse_d1[2], mse_d2[2], mse_rgb[2][3], mse_luma[2], psnr_d1, psnr_d2, psnr_rgb[3], psnr_luma.  0, or < 0 on error.
int gpc_host_distortion(void* h, const float* xyz, const uint8_t* rgb, int n, double peak, double* out, char* err, int errlen)
{
    try {
        gpc::pointcloud c((size_t)(n > 0 ? n : 0));
        for (size_t i = 0; i < c.size(); ++i) c[i] = gpc::point{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
        const gpc::distortion_stats s = static_cast<gpc::gp_compressor*>(h)->distortion(c, peak);
        int k = 0;
        for (int d = 0; d < 2; ++d) out[k++] = (double)s.n_valid[d];
        for (int d = 0; d < 2; ++d) out[k++] = (double)s.n_matched[d];
        for (int d = 0; d < 2; ++d) out[k++] = (double)s.n_plane[d];
        for (int d = 0; d < 2; ++d) out[k++] = s.mse_d1[d];
        for (int d = 0; d < 2; ++d) out[k++] = s.mse_d2[d];
        for (int d = 0; d < 2; ++d)
            for (int ch = 0; ch < 3; ++ch) out[k++] = s.mse_rgb[d][ch];
        for (int d = 0; d < 2; ++d) out[k++] = s.mse_luma[d];
        out[k++] = s.psnr_d1;
        out[k++] = s.psnr_d2;
        for (int ch = 0; ch < 3; ++ch) out[k++] = s.psnr_rgb[ch];
        out[k++] = s.psnr_luma;
        return 0;
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}
int gpc_host_decompress_file(const char* path, int device, float* out_xyz, uint8_t* out_rgb, int capacity_pts, char* err, int errlen)
{
    try {
        std::unique_ptr<gpc::gp_compressor> g(gpc::gp_compressor::load_model(path, device));
        return put_cloud(g->load_compressed(), out_xyz, out_rgb, capacity_pts);
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}

// ---- the shard layout of the multi-GPU flows, host code only: no context is created, no device touched -------------------------------
// Device r of a `world`-device run over the projected cloud (sparse != 0: the sparse flow's table).  sizes = {S, local points, n_max};
// every array may be NULL (the first call asks for the sizes): slots [S], off [S + 1], x0 / x1 / y [Nl], rgb [3][Nl], and pd / pc [Nl] when
// the insertion orders perm_d / perm_c [N] (patch order) are given.  Returns 0, or -1 with the reason in err.
int gpc_host_shard(void* h, int world, int sparse, int r, const int32_t* perm_d, const int32_t* perm_c, int32_t sizes[3], int32_t* slots,
                   int32_t* off, double* x0, double* x1, double* y, double* rgb, int32_t* pd, int32_t* pc, char* err, int errlen)
{
    try {
        const auto* g = static_cast<gpc::gp_compressor*>(h);
        const std::vector<int32_t> table = table_of(g, world, sparse);
        if (r < 0 || r >= world) throw std::invalid_argument("gpc_host_shard: no such device");
        const gpc::shard_batch s = gpc::cut_shard(g->patches(), table, world, r, perm_d, perm_c);
        const size_t S = s.off.size() - 1;
        sizes[0] = (int32_t)S; sizes[1] = s.off[S]; sizes[2] = s.n_max;
        if (slots) std::copy_n(table.data() + r * S, S, slots);
        put(s.off, off); put(s.x0, x0); put(s.x1, x1); put(s.y, y); put(s.rgb, rgb); put(s.pd, pd); put(s.pc, pc);
        return 0;
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}
// per_slot [S] of device r into per_patch [P], as the flows scatter status words and basis sizes
int gpc_host_shard_scatter(void* h, int world, int sparse, int r, const int32_t* per_slot, int32_t* per_patch, char* err, int errlen)
{
    try {
        const std::vector<int32_t> table = table_of(static_cast<gpc::gp_compressor*>(h), world, sparse);
        if (r < 0 || r >= world) throw std::invalid_argument("gpc_host_shard_scatter: no such device");
        gpc::scatter_slots(table, world, r, per_slot, per_patch);
        return 0;
    } catch (const std::exception& e) {
        return fail(e, err, errlen);
    }
}

}  // extern "C"
