// gp_compressor.hpp -- host-side C++ mirror of the reference's class surface for the hot path.
//
// Same names, argument meaning and flow as /root/reference/src/gp_compressor.{h,cpp}: a cloud goes in, octree-leaf
// patches are cut and projected into their plane frames on the host (project_cloud / compute_rotation /
// project_points, src/gp_compressor.cpp:29-118,177-249), the per-patch GP loops (train_processes :121-175 and the
// patch loop of load_compressed :298-380) run BATCHED on the GPU through the C-ABI of include/gpc.h, and the
// predicted grids are re-projected to a coloured cloud (:335-373).  PCL and Eigen are not used: the spatial index is
// a plain voxel hash of side `res` (enough to feed the hot path; the octree itself is out of scope, SURVEY section 2
// row 9) and the 4x4 plane fit is a Jacobi eigen-solve.
#pragma once

#include <array>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/gpc.h"

namespace gpc {

// pcl::PointXYZRGB, the fields the path touches (src/gp_compressor.h:20)
struct point {
    float x, y, z;
    uint8_t r, g, b;
};
using pointcloud = std::vector<point>;

// Duck-typed functors of the reference, host versions (what the kernels evaluate on the device).
class rbf_kernel {   // src/rbf_kernel.h:7-25
    double p_[2];
public:
    explicit rbf_kernel(double sigmaf_sq = 100e-0f, double l_sq = 1 * 1) : p_{sigmaf_sq, l_sq} {}
    int param_size() const { return 2; }
    const double* param() const { return p_; }
    double kernel_function(const double xi[2], const double xj[2]) const;   // src/rbf_kernel.cpp:15-18
};
class gaussian_noise {   // src/gaussian_noise.h:4-11
public:
    double s20;
    explicit gaussian_noise(double s20_) : s20(s20_) {}
    double dx_ln(double y, double x, double sigma_x) const { return (y - x) / (s20 + sigma_x); }
    double dx2_ln(double, double, double sigma_x) const { return -1.0f / (s20 + sigma_x); }
};

enum class gp_model {
    sparse,   // sparse_gp<rbf_kernel, gaussian_noise> + sparse_gp_field<rbf_kernel, gaussian_noise_3d>: what the reference runs
    dense     // gaussian_process (src/gaussian_process.h), the batched-Cholesky model of the north star
};

// The patch batch project_cloud() hands to the GPU: exactly the X, y, C of src/gp_compressor.cpp:146-155, batched.
struct patch_batch {
    std::vector<int32_t> off;            // P + 1
    std::vector<double> x0, x1;          // patch-frame coordinates pt(1), pt(2)
    std::vector<double> y;               // depth pt(0), mean-removed
    std::vector<double> rgb;             // 3 planes of N, mean-removed colours
    std::vector<std::array<double, 9>> rotations;   // R_i, column-major (columns = normal, u, v)
    std::vector<std::array<double, 3>> means;       // patch centres after the mean-depth shift (:116)
    std::vector<std::array<double, 3>> rgb_means;
    std::vector<uint8_t> W;              // sz*sz occupancy mask per patch (:117)
    int patches() const { return (int)off.size() - 1; }
};

// What gp_compressor::distortion reports.  Index 0: decoded -> original, 1: original -> decoded.  A mean over no point is NaN.
struct distortion_stats {
    long long n_valid[2], n_matched[2], n_plane[2];       // gpc_distortion_result's counts per direction
    double mse_d1[2], mse_d2[2], mse_rgb[2][3], mse_luma[2];
    // 10 log10(peak^2 count / sse) of the direction with the LARGER mean square error (NaN ignored); +inf at sse == 0.  The peak is the
    // caller's for d1 and d2 and 255 for the colours.
    double psnr_d1, psnr_d2, psnr_rgb[3], psnr_luma;
};

class gp_compressor {
public:
    // gp_compressor(pointcloud::ConstPtr ncloud, double res = 0.1f, int sz = 10)   src/gp_compressor.h:65
    gp_compressor(const pointcloud& ncloud, double res = 0.1f, int sz = 10, gp_model model = gp_model::sparse,
                  int device = 0);
    ~gp_compressor();
    gp_compressor(const gp_compressor&) = delete;
    gp_compressor& operator=(const gp_compressor&) = delete;

    void save_compressed(const std::string& name);   // src/gp_compressor.cpp:21-27 (name unused upstream as well)
    pointcloud load_compressed();                    // src/gp_compressor.cpp:267-386
    // load_compressed() restricted to the grid points whose cell of the occupancy mask W holds data (the use of W the reference
    // comments out, :323-325), in one pass on the GPU (gpc_sparse_decode): the same records in the same order, without the GP's
    // extrapolation into the empty part of a leaf's window.  Sparse model, single-device flow; anything else throws.  A model read
    // from a file stores no W and decodes every point.
    pointcloud load_compressed_masked();
    // The distortion of a decoded cloud against the object's own input cloud, in both directions (gpc_cloud_distortion: the exact nearest
    // neighbour, D1, D2, colour).  D2 uses the plane normals of the projected batch (gpc_patches_normals), which exist on the ORIGINAL
    // side only: mse_d2[1] is NaN.  Either model; the single-device flow, and an object that has its input cloud (a loaded model has
    // none); anything else throws.  The object is not modified: where the batch was cut on the host, the same batch is cut on the device for
    // the normals alone and dropped.
    distortion_stats distortion(const pointcloud& decoded, double peak);

    // The wire format the reference never wrote (save_compressed ignores `name`): per patch the
    // frame (R_i, mean_i, RGB mean) and the two sparse GPs as (BV, alpha) -- all the decompressor's mean prediction needs.
    // C and Q are not stored: a loaded model reconstructs the same cloud bit for bit, but cannot be trained further.
    // Sparse model only.  Returns the number of bytes written.
    size_t save_model(const std::string& path);
    static gp_compressor* load_model(const std::string& path, int device = 0);
    // Rate control: prune every patch's depth GP to keep_depth and its colour GP to keep_rgb basis vectors, then on while the lowest
    // score |alpha_i|^2 / (Q_ii + C_ii) is below tol_depth / tol_rgb (gpc_sparse_prune: the reference's capacity deletion,
    // src/sparse_gp.hpp:206-223, continued).  In place; trains first if needed.  save_model() then writes the smaller model (24 bytes
    // less per depth vector, 40 per colour vector; same file format).  Sparse model, single-device flow, and an object that was
    // trained here (a loaded model has no C and Q); anything else throws.  Returns the vectors removed {depth, colour}.
    std::array<long long, 2> prune(int keep_depth, int keep_rgb, double tol_depth = 0.0, double tol_rgb = 0.0);
    // Rate control against a distortion bound: every patch's depth / colour GP sheds vectors by the same rule while the mean square error
    // on the patch's own training points stays within max_mse_depth / max_mse_rgb, and never below keep_depth / keep_rgb vectors
    // (gpc_sparse_prune_rd on the projected batch; it stops at the first removal that would exceed the bound).  Same preconditions and
    // exceptions as prune(); save_model() then writes the smaller model.  Returns the vectors removed {depth, colour}.
    std::array<long long, 2> prune_to_error(double max_mse_depth, double max_mse_rgb, int keep_depth = 1, int keep_rgb = 1);
    // Rate control by precision: the model file with every leaf's (BV, alpha) stored at the fewest bits per coefficient, one width per
    // GP and leaf in bits_min .. bits_max, whose mean square error on the leaf's own training points stays within max_mse_depth /
    // max_mse_rgb (gpc_sparse_quantize_rd on the projected batch; the first accepted width wins).  Writes GPCM version 2: per GP the
    // width, ny + 2 float ranges and the bit-packed codes; a leaf no width fits (or that would not be smaller) is stored raw as in version 1.  The
    // object itself is not modified; load_model() reads both versions.  Trains first if needed.  Same preconditions and exceptions as
    // prune_to_error(); an argument gpc_sparse_quantize_rd refuses throws.  Returns the number of bytes written.
    size_t save_model_quantized(const std::string& path, double max_mse_depth, double max_mse_rgb, int bits_min = 1, int bits_max = 16);
    // The exact size of the file save_model() would write for the object as it stands: the header, per leaf 15 doubles and 2 int32, and
    // 24 bytes per depth vector, 40 per colour vector.  A trained (or loaded) sparse model of the single-device flow; anything else throws.
    size_t model_bytes() const;
    // Rate control to a byte budget: make the model fit in budget_bytes and spend the bytes where they buy the most.  need =
    // model_bytes() - budget_bytes; every leaf's two rate-distortion curves on its own training points (gpc_sparse_prune_rd without a
    // bound, on copies); ONE allocation over the 2 P rows, depth then colour (gpc_rate_allocate: it minimises the sum of weight x n_p x ny x
    // mse_p); then both GPs are pruned in place to the allocated counts.  w_depth / w_rgb = 0 normalises that GP's rows by 1 / sum_p n_p ny
    // mse0_p, so that the objective is the sum of the two relative total errors.  Same preconditions and exceptions as prune_to_error(); a
    // budget below what the removals can reach throws, its message naming the floor, and leaves the object untouched.  save_model() then
    // writes at most budget_bytes.  Returns the vectors removed {depth, colour}.
    std::array<long long, 2> prune_to_bytes(size_t budget_bytes, double w_depth = 0, double w_rgb = 0);

    // host-only part, usable without a GPU
    void project_cloud();                            // src/gp_compressor.cpp:177-249
    // the same batch, bit for bit, cut on the GPU (gpc_project_cloud); what save_compressed()
    // uses unless gpu_producer is cleared
    void project_cloud_device();
    bool gpu_producer = true;
    const patch_batch& patches() const { return batch_; }
    // statistics the reference prints ("Mean added" / "Max added", :173-174)
    double mean_added() const { return mean_added_; }
    int max_added() const { return max_added_; }
    // Multi-GPU: the reference is one process, so one process drives the GPUs of the node -- one gpc_ctx per
    // device, gpc_partition_patches (longest-processing-time) deals the patches, every device fits + predicts its slots and ONE
    // RCCL all-gather (gpc_comm_create_all + gpc_group bracket) reassembles the grids.  Host-cut patches (save_compressed() then
    // runs project_cloud() on the host); an empty list returns to the single-device flow.  Dense model: fit + predict per device
    // at training time.  Sparse model (what the reference runs): the partition is drawn with the sparse cost model and the two GPs
    // of a patch live on ITS device from train_processes() to load_compressed() (fixed affinity: the state never moves), which
    // predicts per device and gathers the grids once.
    void set_devices(const std::vector<int>& devices);
    // Dense model: per-leaf hyper-parameter selection by the log marginal likelihood (gpc_dense_select, include/gpc.h).  With candidates
    // set for a plane, train_processes() fits every leaf under each of them -- sigmaf_sq, l_sq and noise over dense_params -- and keeps
    // the grid of the one with the largest evidence (the colour plane decides by the sum over its three channels); an empty vector
    // leaves that plane at dense_params, and with both empty nothing changes.  Single-device flows only: the sharded flow deals
    // patches to devices that each would have to run every candidate, so candidates together with set_devices() throw.
    void set_dense_candidates(const std::vector<gpc_hyper>& depth, const std::vector<gpc_hyper>& rgb);
    // per leaf, after train_processes(): the winning candidate of the plane (-1: none was eligible; empty without candidates) and the
    // winner's log marginal likelihood of the depth plane
    const std::vector<int32_t>& dense_best_depth() const { return dense_best_depth_; }
    const std::vector<int32_t>& dense_best_rgb() const { return dense_best_rgb_; }
    const std::vector<double>& dense_evidence_depth() const { return dense_ev_depth_; }
    // name of the kernels the last dense call of this object's context ran ("" before any): gpc_last_dense_kernel
    const char* last_dense_kernel() const { return ctx_ ? gpc_last_dense_kernel(ctx_) : ""; }
    // insertion-order source; default std::rand like sparse_gp::shuffle (src/sparse_gp.hpp:43-56)
    std::function<int()> rng;
    // hyper-parameters (defaults = the reference's compile-time constants)
    gpc_params depth_params, rgb_params, dense_params;

protected:
    void compute_rotation(double R[9], const std::vector<double>& pts4, int k) const;   // :29-64
    void train_processes();                                                            // :121-175
    static void flatten_colors(uint8_t out[3], const double c[3]);                      // :251-265
    void shuffle(std::vector<int32_t>& perm, int n);

    gp_compressor(double res, int sz, int device);   // empty shell for load_model
    pointcloud cloud_;
    double res_;
    int sz_;
    gp_model model_;
    int device_;
    patch_batch batch_;
    bool projected_ = false, trained_ = false;
    bool loaded_ = false;                     // load_model: (BV, alpha) only
    gpc_ctx* ctx_ = nullptr;
    gpc_sparse* gps_ = nullptr;
    gpc_sparse* rgb_gps_ = nullptr;
    std::vector<double> dense_f_, dense_c_;   // dense model: grids predicted at training time (fit + predict are fused)
    // device-resident flow (project_cloud_device): the batch stays in HBM, the GP kernels and the reprojection read it
    // there, and only `off`, the insertion orders and the final cloud cross PCIe
    gpc_patches* dev_patches_ = nullptr;
    double *d_dense_f_ = nullptr, *d_dense_c_ = nullptr;
    void release_device();
    void drop_dense_grids();
    void train_dense_sharded();
    std::vector<gpc_hyper> dense_cand_depth_, dense_cand_rgb_;     // set_dense_candidates()
    std::vector<int32_t> dense_best_depth_, dense_best_rgb_;
    std::vector<double> dense_ev_depth_;
    // one plane of the dense model on the whole batch, device or host pointers throughout: gpc_dense_select[_dev] in the grid form when
    // the plane has candidates (best [P] and, when ev != nullptr, the winner's log_ev [P][ny] are written), else the plain grid entry
    void dense_plane(bool on_device, const std::vector<gpc_hyper>& cand, const int32_t* off, int n_max, int n_total, const double* x0,
                     const double* x1, const double* y, int ny, double* grid, int32_t* status, int32_t* best, double* ev, const char* what);
    void init_shards();
    void train_sparse_sharded(const std::vector<int32_t>& perm_d, const std::vector<int32_t>& perm_c);
    void predict_sparse_sharded(const std::vector<double>& xs0, const std::vector<double>& xs1, std::vector<double>& f_star,
                                std::vector<double>& c_star);
    std::vector<int32_t> shard_basis_sizes() const;
    std::vector<gpc_sparse*> shard_gps_, shard_rgb_;   // sparse model, sharded: the GPs of a device's slots
    std::vector<int32_t> shard_slots_;                 // world * S: slot -> patch (-1 padding), from gpc_partition_patches
    std::vector<int> devices_;                // set_devices(): non-empty = the sharded flow
    std::vector<gpc_ctx*> shard_ctx_;         // one per device (shard_ctx_[0] is its own context, not ctx_)
    std::vector<gpc_comm*> shard_comm_;
    std::vector<int32_t> status_;
    double mean_added_ = 0.0;
    int max_added_ = 0;
};

}  // namespace gpc
