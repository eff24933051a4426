"""ctypes door onto the host-side C++ mirror of the reference classes (gp_compressor_amd/host -> libgpc_host.so).
Used by the tests; a C++ caller includes gp_compressor_amd/host/gp_compressor.hpp directly."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libgpc_host.so")
_lib = None


def build():
    from . import build as b
    b.build()
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host")])


def load():
    global _lib
    if _lib is None:
        try:
            import torch  # noqa: F401  (see capi.load: torch's libamdhip64 must be mapped first)
        except ImportError:
            pass
        if not os.path.exists(LIB):
            build()
        L = C.CDLL(LIB)
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        L.gpc_host_create.restype = vp
        L.gpc_host_create.argtypes = [vp, vp, i, d, i, i, i]
        L.gpc_host_destroy.argtypes = [vp]
        L.gpc_host_seed.argtypes = [vp, C.c_uint]
        L.gpc_host_set_sparse_kernel.argtypes = [vp, d, d, d, d, i]
        L.gpc_host_set_field_delete_bug.argtypes = [vp, i]
        L.gpc_host_project.argtypes = [vp]
        L.gpc_host_project_device.argtypes = [vp, vp, i]
        L.gpc_host_set_gpu_producer.argtypes = [vp, i]
        L.gpc_host_set_devices.argtypes = [vp, vp, i, vp, i]
        L.gpc_host_set_dense_candidates.argtypes = [vp, vp, i, vp, i, vp, i]
        L.gpc_host_dense_best.argtypes = [vp, i, vp]
        L.gpc_host_dense_evidence_depth.argtypes = [vp, vp]
        L.gpc_host_last_dense_kernel.restype = C.c_char_p
        L.gpc_host_last_dense_kernel.argtypes = [vp]
        L.gpc_host_patch_count.argtypes = [vp]
        L.gpc_host_point_count.argtypes = [vp]
        L.gpc_host_get_batch.argtypes = [vp] * 9
        L.gpc_host_get_mask.argtypes = [vp, vp]
        L.gpc_host_roundtrip.argtypes = [vp, vp, vp, i, vp, vp, vp, i]
        L.gpc_host_save_model.restype = C.c_longlong
        L.gpc_host_save_model.argtypes = [vp, C.c_char_p, vp, i]
        L.gpc_host_save_model_quantized.restype = C.c_longlong
        L.gpc_host_save_model_quantized.argtypes = [vp, C.c_char_p, d, d, i, i, vp, i]
        L.gpc_host_decompress_file.argtypes = [C.c_char_p, i, vp, vp, i, vp, i]
        L.gpc_host_prune.argtypes = [vp, i, i, d, d, vp, vp, i]
        L.gpc_host_prune_to_error.argtypes = [vp, d, d, i, i, vp, vp, i]
        L.gpc_host_model_bytes.restype = C.c_longlong
        L.gpc_host_model_bytes.argtypes = [vp, vp, i]
        L.gpc_host_prune_to_bytes.argtypes = [vp, C.c_longlong, d, d, vp, vp, i]
        L.gpc_host_load_compressed.argtypes = [vp, vp, vp, i, vp, i]
        L.gpc_host_load_compressed_masked.argtypes = [vp, vp, vp, i, vp, i]
        L.gpc_host_distortion.argtypes = [vp, vp, vp, i, d, vp, vp, i]
        L.gpc_host_shard.argtypes = [vp, i, i, i] + [vp] * 12 + [i]
        L.gpc_host_shard_scatter.argtypes = [vp, i, i, i, vp, vp, vp, i]
        _lib = L
    return _lib


class GpCompressor:
    """gp_compressor(cloud, res, sz): save_compressed() / load_compressed() (src/gp_compressor.h:65-67)."""

    def __init__(self, xyz, rgb, res=0.1, sz=10, model="sparse", device=0, seed=None):
        self.L = load()
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        self.rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        self.sz = sz
        self.h = self.L.gpc_host_create(self.xyz.ctypes.data, self.rgb.ctypes.data, len(self.xyz), float(res), int(sz),
                                        1 if model == "dense" else 0, device)
        if seed is not None:
            self.L.gpc_host_seed(self.h, seed)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.gpc_host_destroy(self.h)
            self.h = None

    def set_gpu_producer(self, on):
        """save_compressed(): cut the patches on the GPU and keep the whole round trip on the device (default), or on the host"""
        self.L.gpc_host_set_gpu_producer(self.h, int(bool(on)))

    def set_devices(self, devices):
        """multi-GPU mode of the dense model: one process drives these devices (gp_compressor::set_devices); [] switches it off"""
        d = np.ascontiguousarray(devices, dtype=np.int32)
        err = C.create_string_buffer(512)
        if self.L.gpc_host_set_devices(self.h, d.ctypes.data if len(d) else None, len(d), C.addressof(err), 512) != 0:
            raise RuntimeError(f"set_devices failed: {err.value.decode()}")

    def set_dense_candidates(self, depth=(), rgb=()):
        """dense model: per-leaf hyper-parameter selection by the log marginal likelihood (gp_compressor::set_dense_candidates);
        depth, rgb: (sigmaf_sq, l_sq, noise) triples, an empty list leaves that plane at dense_params.  Before training."""
        d = np.ascontiguousarray(depth, dtype=np.float64).reshape(-1, 3)
        c = np.ascontiguousarray(rgb, dtype=np.float64).reshape(-1, 3)
        err = C.create_string_buffer(512)
        if self.L.gpc_host_set_dense_candidates(self.h, d.ctypes.data if len(d) else None, len(d), c.ctypes.data if len(c) else None, len(c),
                                                C.addressof(err), 512) != 0:
            raise RuntimeError(f"set_dense_candidates failed: {err.value.decode()}")

    def _dense_best(self, which):
        out = np.zeros(self.L.gpc_host_dense_best(self.h, which, None), dtype=np.int32)
        self.L.gpc_host_dense_best(self.h, which, out.ctypes.data if len(out) else None)
        return out

    def dense_best_depth(self):
        """per leaf, after training with depth candidates: the winner's index (-1: no candidate eligible); empty without candidates"""
        return self._dense_best(0)

    def dense_best_rgb(self):
        return self._dense_best(1)

    def last_dense_kernel(self):
        """the kernels the object's last dense call ran (gpc_last_dense_kernel of its context)"""
        return self.L.gpc_host_last_dense_kernel(self.h).decode()

    def dense_evidence_depth(self):
        """per leaf, after training with depth candidates: the winner's log marginal likelihood"""
        out = np.zeros(self.L.gpc_host_dense_evidence_depth(self.h, None), dtype=np.float64)
        self.L.gpc_host_dense_evidence_depth(self.h, out.ctypes.data if len(out) else None)
        return out

    def set_sparse_kernel(self, sigmaf_sq, l_sq, s20_depth, s20_rgb, capacity):
        self.L.gpc_host_set_sparse_kernel(self.h, sigmaf_sq, l_sq, s20_depth, s20_rgb, capacity)

    def set_field_delete_bug(self, on):
        """ref_field_delete_bug of the colour GP (default 1, the reference's multiply); 0: the field deletes as its derivation says, which
        pruning colour deeply needs.  Before training."""
        self.L.gpc_host_set_field_delete_bug(self.h, int(bool(on)))

    def project_cloud(self, device=False):
        """project_cloud() on the host, or (device=True) the same batch cut on the GPU"""
        if device:
            err = C.create_string_buffer(512)
            if self.L.gpc_host_project_device(self.h, C.addressof(err), 512) != 0:
                raise RuntimeError(f"project_cloud_device failed: {err.value.decode()}")
        else:
            assert self.L.gpc_host_project(self.h) == 0
        P, N = self.L.gpc_host_patch_count(self.h), self.L.gpc_host_point_count(self.h)
        off = np.zeros(P + 1, dtype=np.int32)
        x0, x1, y = np.zeros(N), np.zeros(N), np.zeros(N)
        rgb = np.zeros((3, N))
        R, mean, cm = np.zeros((P, 9)), np.zeros((P, 3)), np.zeros((P, 3))
        self.L.gpc_host_get_batch(self.h, *[a.ctypes.data for a in (off, x0, x1, y, rgb, R, mean, cm)])
        W = np.zeros((P, self.sz * self.sz), dtype=np.uint8)
        self.L.gpc_host_get_mask(self.h, W.ctypes.data)
        return dict(off=off, x0=x0, x1=x1, y=y, rgb=rgb, R=R.reshape(P, 3, 3).transpose(0, 2, 1).copy(), mean=mean, rgb_mean=cm, W=W)

    def roundtrip(self):
        """save_compressed("...") then load_compressed(): returns (xyz float32 (M,3), rgb uint8 (M,3), mean_added, max_added)."""
        assert self.L.gpc_host_project(self.h) == 0
        cap = self.L.gpc_host_patch_count(self.h) * self.sz * self.sz
        oxyz = np.zeros((max(cap, 1), 3), dtype=np.float32)
        orgb = np.zeros((max(cap, 1), 3), dtype=np.uint8)
        mean_added = C.c_double(0)
        max_added = C.c_int(0)
        err = C.create_string_buffer(512)
        n = self.L.gpc_host_roundtrip(self.h, oxyz.ctypes.data, orgb.ctypes.data, cap, C.addressof(mean_added),
                                      C.addressof(max_added), C.addressof(err), 512)
        if n < 0:
            raise RuntimeError(f"gp_compressor round trip failed ({n}): {err.value.decode()}")
        return oxyz[:n], orgb[:n], mean_added.value, max_added.value

    def shard(self, world, r, sparse=False, perm_d=None, perm_c=None):
        """the local batch the multi-GPU flows cut for device r of `world` (host code only; after project_cloud()): slots (S,), off (S + 1,),
        n_max, x0 / x1 / y (Nl,), rgb (3, Nl) and, when the insertion orders are given in patch order, pd / pc (Nl,)"""
        perms = [None if p is None else np.ascontiguousarray(p, dtype=np.int32) for p in (perm_d, perm_c)]
        head = [self.h, world, int(bool(sparse)), r] + [None if p is None else p.ctypes.data for p in perms]
        sizes = np.zeros(3, dtype=np.int32)
        err = C.create_string_buffer(512)
        if self.L.gpc_host_shard(*head, sizes.ctypes.data, *[None] * 9, C.addressof(err), 512) != 0:
            raise RuntimeError(f"gpc_host_shard failed: {err.value.decode()}")
        S, Nl, n_max = (int(v) for v in sizes)
        out = dict(slots=np.zeros(S, np.int32), off=np.zeros(S + 1, np.int32), x0=np.zeros(Nl), x1=np.zeros(Nl), y=np.zeros(Nl),
                   rgb=np.zeros((3, Nl)), pd=np.zeros(0 if perms[0] is None else Nl, np.int32), pc=np.zeros(0 if perms[1] is None else Nl, np.int32))
        if self.L.gpc_host_shard(*head, sizes.ctypes.data, *[a.ctypes.data for a in out.values()], C.addressof(err), 512) != 0:
            raise RuntimeError(f"gpc_host_shard failed: {err.value.decode()}")
        return dict(out, n_max=n_max)

    def shard_scatter(self, world, r, per_slot, per_patch, sparse=False):
        """scatter device r's per-slot int32 array into the patch-ordered int32 array per_patch (in place), skipping padding slots"""
        per_slot = np.ascontiguousarray(per_slot, dtype=np.int32)
        assert per_patch.dtype == np.int32 and per_patch.flags.c_contiguous
        err = C.create_string_buffer(512)
        if self.L.gpc_host_shard_scatter(self.h, world, int(bool(sparse)), r, per_slot.ctypes.data, per_patch.ctypes.data, C.addressof(err), 512) != 0:
            raise RuntimeError(f"gpc_host_shard_scatter failed: {err.value.decode()}")


    def save_model(self, path):
        """write the trained sparse model (frames + (BV, alpha) per patch); returns the file size in bytes"""
        err = C.create_string_buffer(512)
        n = self.L.gpc_host_save_model(self.h, os.fsencode(path), C.addressof(err), 512)
        if n < 0:
            raise RuntimeError(f"save_model failed: {err.value.decode()}")
        return int(n)

    def save_model_quantized(self, path, max_mse_depth, max_mse_rgb, bits_min=1, bits_max=16):
        """gp_compressor::save_model_quantized: the model file (GPCM version 2) with every leaf's (BV, alpha) at the fewest bits per
        coefficient in bits_min .. bits_max whose mean square error on the leaf's own training points stays within max_mse_depth /
        max_mse_rgb; a leaf no width fits is stored raw.  The object is not modified (trains first if needed).  Returns the file size."""
        err = C.create_string_buffer(512)
        n = self.L.gpc_host_save_model_quantized(self.h, os.fsencode(path), float(max_mse_depth), float(max_mse_rgb), int(bits_min),
                                                 int(bits_max), C.addressof(err), 512)
        if n < 0:
            raise RuntimeError(f"save_model_quantized failed: {err.value.decode()}")
        return int(n)

    def prune(self, keep_depth, keep_rgb, tol_depth=0.0, tol_rgb=0.0):
        """gp_compressor::prune: every patch's depth / colour GP down to keep_depth / keep_rgb basis vectors, then on while the lowest
        score is below the tolerance; in place (trains first if needed).  Returns (removed_depth, removed_rgb), summed over the patches."""
        err = C.create_string_buffer(512)
        rm = np.zeros(2, dtype=np.int64)
        if self.L.gpc_host_prune(self.h, int(keep_depth), int(keep_rgb), float(tol_depth), float(tol_rgb), rm.ctypes.data,
                                 C.addressof(err), 512) != 0:
            raise RuntimeError(f"prune failed: {err.value.decode()}")
        return int(rm[0]), int(rm[1])

    def prune_to_error(self, max_mse_depth, max_mse_rgb, keep_depth=1, keep_rgb=1):
        """gp_compressor::prune_to_error: every patch's depth / colour GP sheds vectors while the mean square error on its own training
        points stays within max_mse_depth / max_mse_rgb, never below keep_depth / keep_rgb vectors; in place (trains first if needed).
        Returns (removed_depth, removed_rgb), summed over the patches."""
        err = C.create_string_buffer(512)
        rm = np.zeros(2, dtype=np.int64)
        if self.L.gpc_host_prune_to_error(self.h, float(max_mse_depth), float(max_mse_rgb), int(keep_depth), int(keep_rgb), rm.ctypes.data,
                                          C.addressof(err), 512) != 0:
            raise RuntimeError(f"prune_to_error failed: {err.value.decode()}")
        return int(rm[0]), int(rm[1])

    def model_bytes(self):
        """gp_compressor::model_bytes: the exact size of the file save_model would write for the trained object as it stands"""
        err = C.create_string_buffer(512)
        n = self.L.gpc_host_model_bytes(self.h, C.addressof(err), 512)
        if n < 0:
            raise RuntimeError(f"model_bytes failed: {err.value.decode()}")
        return int(n)

    def prune_to_bytes(self, budget_bytes, w_depth=0.0, w_rgb=0.0):
        """gp_compressor::prune_to_bytes: make the model fit in budget_bytes by one joint allocation of removals over every leaf's
        depth and colour GP (a weight of 0 normalises that GP's errors by their total); in place (trains first if needed).  An
        infeasible budget raises, naming the floor, and leaves the object as it was.  Returns (removed_depth, removed_rgb)."""
        err = C.create_string_buffer(512)
        rm = np.zeros(2, dtype=np.int64)
        if self.L.gpc_host_prune_to_bytes(self.h, int(budget_bytes), float(w_depth), float(w_rgb), rm.ctypes.data, C.addressof(err),
                                          512) != 0:
            raise RuntimeError(f"prune_to_bytes failed: {err.value.decode()}")
        return int(rm[0]), int(rm[1])

    def load_compressed(self, masked=False):
        """load_compressed() of the object as it stands (trained, possibly pruned): (xyz float32 (M,3), rgb uint8 (M,3)).  masked:
        load_compressed_masked(), only the grid points whose cell of the occupancy mask W holds data (sparse model, one device)."""
        cap = self.L.gpc_host_patch_count(self.h) * self.sz * self.sz
        oxyz = np.zeros((max(cap, 1), 3), dtype=np.float32)
        orgb = np.zeros((max(cap, 1), 3), dtype=np.uint8)
        err = C.create_string_buffer(512)
        entry = self.L.gpc_host_load_compressed_masked if masked else self.L.gpc_host_load_compressed
        n = entry(self.h, oxyz.ctypes.data, orgb.ctypes.data, cap, C.addressof(err), 512)
        if n < 0:
            raise RuntimeError(f"load_compressed failed ({n}): {err.value.decode()}")
        return oxyz[:n], orgb[:n]


    def distortion(self, xyz, rgb, peak):
        """gp_compressor::distortion: the cloud (xyz (M, 3) float32, rgb (M, 3) uint8) against the object's input cloud, both directions,
        index 0 = decoded -> original.  Returns counts {"n_valid", "n_matched", "n_plane"}: (2,) and per metric in d1, d2, r, g, b, luma
        {"mse": (2,), "psnr": of the larger mse}, the layout of capi.Context.cloud_psnr.  D2 has the original side's normals only."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1, 3)
        out = np.zeros(24)
        err = C.create_string_buffer(512)
        if self.L.gpc_host_distortion(self.h, xyz.ctypes.data, rgb.ctypes.data, len(xyz), float(peak), out.ctypes.data, C.addressof(err),
                                      512) != 0:
            raise RuntimeError(f"distortion failed: {err.value.decode()}")
        res = {k: out[2 * j:2 * j + 2].astype(np.int64) for j, k in enumerate(("n_valid", "n_matched", "n_plane"))}
        res["d1"] = {"mse": tuple(out[6:8]), "psnr": out[18]}
        res["d2"] = {"mse": tuple(out[8:10]), "psnr": out[19]}
        for c, k in enumerate("rgb"):
            res[k] = {"mse": (out[10 + c], out[13 + c]), "psnr": out[20 + c]}
        res["luma"] = {"mse": tuple(out[16:18]), "psnr": out[23]}
        return res


def decompress_file(path, capacity_pts, device=0):
    """reconstruct the cloud from a model file alone: returns (xyz float32 (M,3), rgb uint8 (M,3))"""
    L = load()
    oxyz = np.zeros((max(capacity_pts, 1), 3), dtype=np.float32)
    orgb = np.zeros((max(capacity_pts, 1), 3), dtype=np.uint8)
    err = C.create_string_buffer(512)
    n = L.gpc_host_decompress_file(os.fsencode(path), device, oxyz.ctypes.data, orgb.ctypes.data, capacity_pts, C.addressof(err), 512)
    if n < 0:
        raise RuntimeError(f"decompress_file failed ({n}): {err.value.decode()}")
    return oxyz[:n], orgb[:n]


def synthetic_plane_cloud(n=10000, seed=1, extent=1.2):
    """BASELINE config 1 / SURVEY section 8(d) C1 (see synth.plane_cloud)"""
    from . import synth
    return synth.plane_cloud(n, seed, extent)
