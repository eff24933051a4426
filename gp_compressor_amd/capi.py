"""ctypes binding of the C-ABI in include/gpc.h (gp_compressor_amd/libgpc_hip.so).

This is exactly the binding a Python caller of the reference would add; the C++ host classes in
gp_compressor_amd/host/ use the same entry points.  There is NO fallback: if the shared library has not been
built (gp_compressor_amd.build.build() / __graft_entry__.build()) or no HIP device is present, calls raise.
"""
import ctypes as C
import os
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPC_LIB_PATH", os.path.join(HERE, "libgpc_hip.so"))   # override: diagnostic builds only

GPC_OK, GPC_EINVAL, GPC_ENOMEM, GPC_ENODEV, GPC_EHIP, GPC_ERANGE = 0, -22, -12, -19, -5, -34
CELL_UNOBSERVED, CELL_OCCUPIED, CELL_FREE = 0, 1, 2
STATUS_OK, STATUS_NOT_SPD, STATUS_NAN, STATUS_SIGMA_CLAMPED, STATUS_OVERFLOW, STATUS_NOT_CONVERGED = 0, 1, 2, 3, 4, 5
MAX_POINTS, MAX_BV = 1024, 256

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int32)


class Params(C.Structure):
    """struct gpc_params (include/gpc.h)."""
    _fields_ = [("sigmaf_sq", C.c_double), ("l_sq", C.c_double), ("noise", C.c_double), ("eps_tol", C.c_double),
                ("capacity", C.c_int32), ("noise_model", C.c_int32), ("ref_double_noise", C.c_int32),
                ("ref_field_delete_bug", C.c_int32), ("want_variance", C.c_int32), ("reserved", C.c_int32)]


class IrlsParams(C.Structure):
    """struct gpc_irls_params (include/gpc.h)."""
    _fields_ = [("max_iter", C.c_int32), ("reserved", C.c_int32), ("tol", C.c_double), ("f_init", C.c_double)]


class Hyper(C.Structure):
    """struct gpc_hyper (include/gpc.h): one candidate of gpc_dense_irls_select."""
    _fields_ = [("sigmaf_sq", C.c_double), ("l_sq", C.c_double), ("noise", C.c_double)]


class RegistrationParams(C.Structure):
    """struct gpc_registration_params (include/gpc.h)."""
    _fields_ = [("step", C.c_double), ("tol", C.c_double), ("min_steps", C.c_int32), ("max_steps", C.c_int32),
                ("ref_translation_sum", C.c_int32), ("reserved", C.c_int32)]


class RenderParams(C.Structure):
    """struct gpc_render_params (include/gpc.h)."""
    _fields_ = [("newton_iters", C.c_int32), ("use_w", C.c_int32), ("eps_rel", C.c_double), ("t_max", C.c_double)]


class DistortionParams(C.Structure):
    """struct gpc_distortion_params (include/gpc.h)."""
    _fields_ = [("cell", C.c_double), ("max_dist", C.c_double)]


# struct gpc_distortion_result (include/gpc.h), as a numpy record
DISTORTION_RESULT_DTYPE = np.dtype([("n_valid", "<i8"), ("n_matched", "<i8"), ("n_plane", "<i8"), ("sse_d1", "<f8"), ("max_d1", "<f8"),
                                    ("sse_d2", "<f8"), ("max_d2", "<f8"), ("sse_rgb", "<f8", (3,)), ("sse_luma", "<f8")])


class PatchesView(C.Structure):
    """struct gpc_patches_view (include/gpc.h): sizes + device addresses of a patch batch."""
    _fields_ = [("P", C.c_int32), ("n_total", C.c_int32), ("n_max", C.c_int32), ("m", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("off", "x0", "x1", "y", "rgb", "rotations", "means", "rgb_means", "W", "src")]


class GpcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gpc error {code}: {msg}")
        self.code = code


# every symbol include/gpc.h declares, with its prototype (the CPU test-suite checks the library exports all of them)
_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
# the eight probit IRLS entries: ctx, params, irls, [H, cand,] P, off, [n_max, n_total,] x0, x1, y, m, xs0, xs1, res, sz, then the outputs
_IRLS_HOST = [_vp, C.POINTER(Params), C.POINTER(IrlsParams), _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _d, _i]
_IRLS_DEV = _IRLS_HOST[:5] + [_i, _i] + _IRLS_HOST[5:]


def _irls_proto(head, outputs, select=False):
    return (C.c_int, head[:3] + ([_i, _vp] if select else []) + head[3:] + [_vp] * outputs)


PROTOTYPES = {
    "gpc_version": (C.c_int, []),
    "gpc_default_params_dense": (None, [C.POINTER(Params)]),
    "gpc_default_params_sparse": (None, [C.POINTER(Params), _i]),
    "gpc_ctx_create": (C.c_int, [C.POINTER(_vp), _i]),
    "gpc_ctx_set_stream": (C.c_int, [_vp, _vp]),
    "gpc_ctx_synchronize": (C.c_int, [_vp]),
    "gpc_dev_malloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "gpc_dev_free": (C.c_int, [_vp, _vp]),
    "gpc_dev_memcpy": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _i]),
    "gpc_host_alloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "gpc_host_free": (C.c_int, [_vp, _vp]),
    "gpc_ctx_destroy": (None, [_vp]),
    "gpc_last_error": (C.c_char_p, [_vp]),
    "gpc_last_dense_kernel": (C.c_char_p, [_vp]),
    "gpc_dense_fit_predict": (C.c_int, [_vp, C.POINTER(Params), _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpc_dense_fit_predict_dev": (C.c_int, [_vp, C.POINTER(Params), _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp,
                                            _vp, _vp, _vp, _vp]),
    "gpc_dense_fit_predict_grid": (C.c_int, [_vp, C.POINTER(Params), _i, _vp, _vp, _vp, _vp, _i, _d, _i, _vp, _vp, _vp]),
    "gpc_dense_fit_predict_grid_dev": (C.c_int, [_vp, C.POINTER(Params), _i, _vp, _i, _i, _vp, _vp, _vp, _i, _d, _i,
                                                 _vp, _vp, _vp]),
    # ctx, params, [H, cand,] P, off, [n_max, n_total,] x0, x1, y, ny, m, xs0, xs1, res, sz, then the outputs
    "gpc_dense_fit_predict_ev": (C.c_int, [_vp, C.POINTER(Params), _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _d, _i] + [_vp] * 5),
    "gpc_dense_fit_predict_ev_dev": (C.c_int, [_vp, C.POINTER(Params), _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _d, _i] + [_vp] * 5),
    "gpc_dense_select": (C.c_int, [_vp, C.POINTER(Params), _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _d, _i] + [_vp] * 7),
    "gpc_dense_select_dev": (C.c_int, [_vp, C.POINTER(Params), _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _d, _i] + [_vp] * 7),
    "gpc_default_params_irls": (None, [C.POINTER(IrlsParams)]),
    "gpc_dense_irls_fit_predict": _irls_proto(_IRLS_HOST, 5),
    "gpc_dense_irls_fit_predict_dev": _irls_proto(_IRLS_DEV, 5),
    "gpc_dense_irls_fit_predict_var": _irls_proto(_IRLS_HOST, 7),
    "gpc_dense_irls_fit_predict_var_dev": _irls_proto(_IRLS_DEV, 7),
    "gpc_dense_irls_fit_predict_ev": _irls_proto(_IRLS_HOST, 8),
    "gpc_dense_irls_fit_predict_ev_dev": _irls_proto(_IRLS_DEV, 8),
    "gpc_dense_irls_select": _irls_proto(_IRLS_HOST, 10, select=True),
    "gpc_dense_irls_select_dev": _irls_proto(_IRLS_DEV, 10, select=True),
    "gpc_noise_eval": (C.c_int, [_vp, _i, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "gpc_sparse_create": (C.c_int, [_vp, C.POINTER(Params), _i, _i, C.POINTER(_vp)]),
    "gpc_sparse_destroy": (None, [_vp]),
    "gpc_sparse_reset": (C.c_int, [_vp]),
    "gpc_sparse_set_trace": (C.c_int, [_vp, _vp]),
    "gpc_sparse_add": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpc_sparse_add_dev": (C.c_int, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "gpc_sparse_predict": (C.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "gpc_sparse_predict_dev": (C.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "gpc_sparse_predict_points": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "gpc_sparse_predict_points_dev": (C.c_int, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "gpc_sparse_predict_scattered": (C.c_int, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp]),
    "gpc_sparse_predict_scattered_dev": (C.c_int, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp]),
    "gpc_sparse_likelihood": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpc_sparse_likelihood_dev": (C.c_int, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gpc_sparse_train_sigmaf": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _d, _i, _vp, _vp, _vp, _vp]),
    "gpc_sparse_train_sigmaf_dev": (C.c_int, [_vp, _vp, _i, _vp, _vp, _vp, _d, _i, _vp, _vp, _vp, _vp]),
    "gpc_sparse_sizes": (C.c_int, [_vp, _vp]),
    "gpc_sparse_get_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "gpc_sparse_ld": (C.c_int, [_vp]),
    "gpc_sparse_set_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "gpc_sparse_remap": (C.c_int, [_vp, _i, _vp, C.POINTER(_vp)]),
    "gpc_sparse_prune": (C.c_int, [_vp, _i, _vp, _d, _vp, _vp, _vp, _vp]),
    "gpc_sparse_prune_dev": (C.c_int, [_vp, _i, _vp, _d, _vp, _vp, _vp, _vp]),
    "gpc_sparse_prune_rd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _d, _vp] + [_vp] * 7),
    "gpc_sparse_prune_rd_dev": (C.c_int, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _d, _vp] + [_vp] * 7),
    "gpc_sparse_quantize_rd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _d, _vp] + [_vp] * 8),
    "gpc_sparse_quantize_rd_dev": (C.c_int, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _d, _vp] + [_vp] * 8),
    "gpc_sparse_dequantize": (C.c_int, [_vp] * 6),
    "gpc_sparse_dequantize_dev": (C.c_int, [_vp] * 6),
    "gpc_rate_allocate": (C.c_int, [_vp, _i, _i, _vp, _vp, _vp, _vp, _d, _vp, _i, C.c_int64, _i, _vp, _vp, _vp, _vp]),
    "gpc_rate_allocate_dev": (C.c_int, [_vp, _i, _i, _vp, _vp, _vp, _vp, _d, _vp, _i, C.c_int64, _i, _vp, _vp, _vp, _vp]),
    "gpc_reproject": (C.c_int, [_vp, _i, _i] + [_vp] * 10),
    "gpc_reproject_dev": (C.c_int, [_vp, _i, _i] + [_vp] * 10),
    "gpc_project_cloud": (C.c_int, [_vp, _vp, _i, _d, _i, C.POINTER(_vp)]),
    "gpc_project_cloud_dev": (C.c_int, [_vp, _vp, _i, _d, _i, C.POINTER(_vp)]),
    "gpc_patches_view_dev": (C.c_int, [_vp, _vp]),
    "gpc_patches_fetch": (C.c_int, [_vp] * 11),
    "gpc_patches_destroy": (None, [_vp]),
    "gpc_patches_insert_cloud": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, C.POINTER(_vp), _vp]),
    "gpc_patches_insert_cloud_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, C.POINTER(_vp), _vp]),
    "gpc_patches_raycast": (C.c_int, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "gpc_patches_raycast_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "gpc_occupancy_batch_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpc_default_params_render": (None, [C.POINTER(RenderParams)]),
    "gpc_patches_render": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(RenderParams), _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gpc_patches_render_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(RenderParams), _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gpc_patches_render_attrs": (C.c_int, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "gpc_patches_render_attrs_dev": (C.c_int, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "gpc_camera_rays_dev": (C.c_int, [_vp, _vp, _d, _d, _d, _d, _i, _i, _vp]),
    "gpc_sparse_decode": (C.c_int, [_vp, _vp, _d, _i] + [_vp] * 5 + [_i] + [_vp] * 5),
    "gpc_sparse_decode_dev": (C.c_int, [_vp, _vp, _d, _i] + [_vp] * 5 + [_i] + [_vp] * 5),
    "gpc_default_params_distortion": (None, [C.POINTER(DistortionParams)]),
    "gpc_cloud_distortion": (C.c_int, [_vp, _vp, _i, _vp, _i, _vp, C.POINTER(DistortionParams), _vp, _vp, _vp, _vp]),
    "gpc_cloud_distortion_dev": (C.c_int, [_vp, _vp, _i, _vp, _i, _vp, C.POINTER(DistortionParams), _vp, _vp, _vp, _vp]),
    "gpc_patches_normals": (C.c_int, [_vp, _i, _vp]),
    "gpc_patches_normals_dev": (C.c_int, [_vp, _i, _vp]),
    "gpc_default_params_registration": (None, [C.POINTER(RegistrationParams)]),
    "gpc_registration_create": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "gpc_registration_destroy": (None, [_vp]),
    "gpc_registration_set_cloud": (C.c_int, [_vp, _vp, _i]),
    "gpc_registration_set_cloud_dev": (C.c_int, [_vp, _vp, _i]),
    "gpc_registration_step": (C.c_int, [_vp, C.POINTER(RegistrationParams), _vp]),
    "gpc_registration_run": (C.c_int, [_vp, C.POINTER(RegistrationParams), _vp, _vp]),
    "gpc_registration_get_transform": (C.c_int, [_vp, _vp, _vp]),
    "gpc_registration_get_cloud": (C.c_int, [_vp, _vp]),
    "gpc_registration_cloud_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_int)]),
    "gpc_registration_get_assignment": (C.c_int, [_vp, _vp, _vp]),
    "gpc_partition_patches": (C.c_int, [_i, _vp, _i, _i, _vp]),
    "gpc_comm_unique_id": (C.c_int, [_vp]),
    "gpc_comm_create": (C.c_int, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "gpc_comm_create_all": (C.c_int, [_i, C.POINTER(_vp), C.POINTER(_vp)]),
    "gpc_comm_adopt": (C.c_int, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "gpc_comm_destroy": (None, [_vp]),
    "gpc_comm_world": (C.c_int, [_vp]),
    "gpc_comm_rank": (C.c_int, [_vp]),
    "gpc_comm_library": (C.c_char_p, []),
    "gpc_comm_set_partition": (C.c_int, [_vp, _i, _vp]),
    "gpc_group_start": (C.c_int, []),
    "gpc_group_end": (C.c_int, []),
    "gpc_allgather_fstar_dev": (C.c_int, [_vp, _i, _vp, _vp, _vp]),
    "gpc_unpermute_fstar_dev": (C.c_int, [_vp, _i, _vp, _vp]),
    "gpc_test_exp_host": (None, [_vp, _vp, _i]),
    "gpc_test_exp_small_host": (None, [_vp, _vp, _i]),
    "gpc_test_quantize_host": (C.c_int, [_vp, _i, _i, _vp, _vp, _vp]),
    "gpc_test_rate_allocate_host": (C.c_int, [_i, _i, _vp, _vp, _vp, _vp, _d, _vp, _i, C.c_int64, _i, _vp, _vp, _vp, _vp]),
    "gpc_test_par_memcpy": (None, [_vp, _vp, C.c_size_t]),
    "gpc_test_dense_route": (C.c_int, [_i] * 11 + [_vp, _i, _vp]),
}

_lib = None


def load():
    """Load libgpc_hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # PyTorch wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's).  Whichever copy is mapped first
        # serves the whole process, and torch refuses to see the GPU when the system copy won: load torch's first.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise GpcError(GPC_ENODEV, f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                   "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    """Address of a numpy array (host), a torch tensor (host or device), an int, or None."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"], "array must be contiguous"
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        assert a.is_contiguous(), "tensor must be contiguous"
        return a.data_ptr()
    raise TypeError(type(a))


def default_params_dense(**kw):
    p = Params()
    load().gpc_default_params_dense(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_params_sparse(ny=1, **kw):
    p = Params()
    load().gpc_default_params_sparse(C.byref(p), ny)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_params_irls(**kw):
    p = IrlsParams()
    load().gpc_default_params_irls(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_params_registration(**kw):
    p = RegistrationParams()
    load().gpc_default_params_registration(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_params_render(**kw):
    p = RenderParams()
    load().gpc_default_params_render(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def psnr(sse, count, peak):
    """10 log10(peak^2 count / sse): the PSNR of `count` errors whose squares add up to sse.  +inf at sse == 0; NaN over no error."""
    import math
    if not count > 0 or sse != sse:
        return float("nan")
    if sse == 0:
        return float("inf")
    return 10.0 * math.log10(float(peak) * float(peak) * float(count) / float(sse))


def symmetric_psnr(ab, ba, peak):
    """The two directions' results of cloud_distortion -> per metric both mean square errors and the PSNR of the larger (Context.cloud_psnr)"""
    def pick(r, name):
        if name == "d1":
            return r["sse_d1"], r["n_matched"], peak
        if name == "d2":
            return r["sse_d2"], r["n_plane"], peak
        if name == "luma":
            return r["sse_luma"], r["n_matched"], 255.0
        return r["sse_rgb"]["rgb".index(name)], r["n_matched"], 255.0

    out = {"ab": ab, "ba": ba}
    for name in ("d1", "d2", "r", "g", "b", "luma"):
        pairs = [pick(r, name) for r in (ab, ba)]
        mse = tuple(float(s) / float(c) if c > 0 else float("nan") for s, c, _ in pairs)
        worst = None                                          # the direction with the larger mean square error; ties: a -> b
        for p, m in zip(pairs, mse):
            if m == m and (worst is None or m > worst[1]):
                worst = (p, m)
        out[name] = {"mse": mse, "psnr": psnr(*worst[0]) if worst else float("nan")}
    return out


class Context:
    """gpc_ctx: one per process per GPU."""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        h = _vp()
        rc = self.lib.gpc_ctx_create(C.byref(h), int(device))
        if rc != GPC_OK:
            raise GpcError(rc, "gpc_ctx_create failed (no HIP device?) -- there is no CPU fallback")
        self.h = h
        self._children = weakref.WeakSet()   # sparse handles must be destroyed before their context
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "h", None):
            for ch in list(self._children):
                ch.close()
            self.lib.gpc_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc):
        if rc != GPC_OK:
            raise GpcError(rc, self.lib.gpc_last_error(self.h).decode())

    def set_stream(self, stream):
        """stream: raw hipStream_t as int (e.g. torch.cuda.current_stream().cuda_stream; 0 is HIP's default stream),
        or None for the context's own non-blocking stream (GPC_STREAM_OWN)."""
        self._check(self.lib.gpc_ctx_set_stream(self.h, C.c_void_p(-1) if stream is None else C.c_void_p(int(stream))))

    def synchronize(self):
        self._check(self.lib.gpc_ctx_synchronize(self.h))

    def host_array(self, shape, dtype=np.float64):
        """a numpy array in page-locked memory (gpc_host_alloc): host-pointer entries transfer such buffers in place.
        The memory lives until the process ends or free_host_array(a) is called."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = _vp()
        self._check(self.lib.gpc_host_alloc(self.h, max(n, 8), C.byref(p)))
        buf = (C.c_char * max(n, 8)).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p
        return a

    def free_host_array(self, a):
        p = getattr(self, "_pinned", {}).pop(a.ctypes.data, None)
        if p is not None:
            self._check(self.lib.gpc_host_free(self.h, p))

    def rate_allocate(self, kmax, d0, d, need, w=None, w_all=1.0, unit=None, unit_all=24, refine=True, count=None):
        """gpc_rate_allocate (host arrays): how many removals each of the R rows takes -- kmax (R,) int32 options, errors d0 (R,) and
        d (R, ld), weights w (R,) or w_all, bytes per removal unit (R,) int32 or unit_all -- so that at least `need` bytes are saved at
        the smallest total weighted error.  Returns (k (R,) int32, result) and, with count (R,) int32, (k, target, result): target =
        max(1, count - k); result: dict of lambda, lambda_bits, saved, max_saving, feasible, switched_rows."""
        a = _rate_args(kmax, d0, d, w, unit, count)
        R, ld = a[2].shape
        k = np.zeros(R, dtype=np.int32)
        tg = None if count is None else np.zeros(R, dtype=np.int32)
        res = np.zeros(1, dtype=RATE_RESULT_DTYPE)
        self._check(self.lib.gpc_rate_allocate(self.h, R, ld, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), float(w_all), _ptr(a[4]),
                                               int(unit_all), int(need), int(bool(refine)), _ptr(a[5]), _ptr(k), _ptr(tg), _ptr(res)))
        return (k, rate_result(res)) if count is None else (k, tg, rate_result(res))

    def rate_allocate_dev(self, R, ld, kmax, d0, d, need, w=None, w_all=1.0, unit=None, unit_all=24, refine=True, count=None, k=None,
                          target=None, result=None):
        """gpc_rate_allocate_dev: device buffers (w, unit, count and each output may be None; result: 32 bytes, rate_result() reads
        them), enqueued on the context's stream"""
        self._check(self.lib.gpc_rate_allocate_dev(self.h, int(R), int(ld), _ptr(kmax), _ptr(d0), _ptr(d), _ptr(w), float(w_all),
                                                   _ptr(unit), int(unit_all), int(need), int(bool(refine)), _ptr(count), _ptr(k),
                                                   _ptr(target), _ptr(result)))

    def last_dense_kernel(self):
        return self.lib.gpc_last_dense_kernel(self.h).decode()

    # ---- dense, host (numpy) buffers -----------------------------------------------------------------------
    def dense_fit_predict(self, params, off, x0, x1, y, xs0, xs1, want_alpha=False):
        """Host-pointer entry (gpc_dense_fit_predict).  y: (ny, N).  Returns f_star (P, ny, m), v_star|None, status, [alpha]."""
        off = np.ascontiguousarray(off, dtype=np.int32)
        y = np.ascontiguousarray(np.atleast_2d(y), dtype=np.float64)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        xs0 = np.ascontiguousarray(xs0, dtype=np.float64)
        xs1 = np.ascontiguousarray(xs1, dtype=np.float64)
        P, ny, m = off.shape[0] - 1, y.shape[0], xs0.shape[0]
        f = np.full((P, ny, m), np.nan)
        v = np.full((P, m), np.nan) if params.want_variance else None
        st = np.full(P, -1, dtype=np.int32)
        al = np.full_like(y, np.nan) if want_alpha else None
        self._check(self.lib.gpc_dense_fit_predict(self.h, C.byref(params), P, _ptr(off), _ptr(x0), _ptr(x1), _ptr(y), ny,
                                                   m, _ptr(xs0), _ptr(xs1), _ptr(f), _ptr(v), _ptr(al), _ptr(st)))
        return (f, v, st, al) if want_alpha else (f, v, st)

    def dense_fit_predict_grid(self, params, off, x0, x1, y, res, sz, want_alpha=False):
        off = np.ascontiguousarray(off, dtype=np.int32)
        y = np.ascontiguousarray(np.atleast_2d(y), dtype=np.float64)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        P, ny, m = off.shape[0] - 1, y.shape[0], sz * sz
        f = np.full((P, ny, m), np.nan)
        st = np.full(P, -1, dtype=np.int32)
        al = np.full_like(y, np.nan) if want_alpha else None
        self._check(self.lib.gpc_dense_fit_predict_grid(self.h, C.byref(params), P, _ptr(off), _ptr(x0), _ptr(x1), _ptr(y),
                                                        ny, float(res), int(sz), _ptr(f), _ptr(al), _ptr(st)))
        return (f, st, al) if want_alpha else (f, st)

    # ---- dense GP with the log marginal likelihood, and the selection among candidates by it ---------------------------
    def _ev_host_args(self, params, off, x0, x1, y, xs0, xs1, res, sz, want_v, want_alpha, want_status):
        """What the two host entries share: the arguments of the C call from P to sz, the contiguous inputs behind their addresses
        (the caller keeps them alive over the call), and the outputs f (P, ny, m), v (P, m), alpha (ny, N), status (P,), log_ev (P, ny)
        filled with NaN / -1 (None where not wanted)."""
        off = np.ascontiguousarray(off, dtype=np.int32)
        y = np.ascontiguousarray(np.atleast_2d(y), dtype=np.float64)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        if xs0 is not None:
            xs0 = np.ascontiguousarray(xs0, dtype=np.float64)
            xs1 = np.ascontiguousarray(xs1, dtype=np.float64)
            m = xs0.shape[0]
        else:
            m = sz * sz
        P, ny = off.shape[0] - 1, y.shape[0]
        f = np.full((P, ny, m), np.nan)
        v = np.full((P, m), np.nan) if want_v else None
        al = np.full_like(y, np.nan) if want_alpha else None
        st = np.full(P, -1, dtype=np.int32) if want_status else None
        ev = np.full((P, ny), np.nan)
        keep = (off, x0, x1, y, xs0, xs1)
        mid = [P, _ptr(off), _ptr(x0), _ptr(x1), _ptr(y), ny, m, _ptr(xs0), _ptr(xs1), float(res), int(sz)]
        return mid, keep, (f, v, al, st, ev)

    def dense_fit_predict_ev(self, params, off, x0, x1, y, xs0=None, xs1=None, res=0.0, sz=0, want_v=True, want_alpha=True,
                             want_status=True, want_ev=True):
        """Host-pointer entry (gpc_dense_fit_predict_ev): the dense fit with the log marginal likelihood per patch and plane.  y: (ny, N).
        X* point-wise (xs0, xs1) or the sz x sz grid.  Returns f_star (P, ny, m), v_star (P, m), alpha (ny, N), status (P,),
        log_ev (P, ny) -- None where not wanted."""
        mid, keep, (f, v, al, st, ev) = self._ev_host_args(params, off, x0, x1, y, xs0, xs1, res, sz, want_v, want_alpha, want_status)
        if not want_ev:
            ev = None
        self._check(self.lib.gpc_dense_fit_predict_ev(self.h, C.byref(params), *mid, *map(_ptr, (f, v, al, st, ev))))
        return f, v, al, st, ev

    def dense_fit_predict_ev_dev(self, params, P, off, n_max, n_total, x0, x1, y, ny, m, xs0, xs1, res, sz, f_star,
                                 v_star=None, alpha_out=None, status=None, log_ev=None):
        self._check(self.lib.gpc_dense_fit_predict_ev_dev(self.h, C.byref(params), P, _ptr(off), n_max, n_total, _ptr(x0), _ptr(x1),
                                                          _ptr(y), ny, m, _ptr(xs0), _ptr(xs1), float(res), int(sz),
                                                          *map(_ptr, (f_star, v_star, alpha_out, status, log_ev))))

    def dense_select(self, params, candidates, off, x0, x1, y, xs0=None, xs1=None, res=0.0, sz=0, want_v=True, skip=()):
        """Host-pointer entry (gpc_dense_select): per patch the candidate (sigmaf_sq, l_sq, noise) of largest log marginal likelihood
        (summed over the planes) and its outputs.  Returns a dict of f_star (P, ny, m), v_star (P, m), alpha (ny, N), log_ev (P, ny),
        best (P,) int32 (-1: no eligible candidate), log_ev_all (H, P, ny), status (P,); names in `skip` are passed as NULL."""
        mid, keep, (f, v, al, st, ev) = self._ev_host_args(params, off, x0, x1, y, xs0, xs1, res, sz, want_v, True, True)
        H, P, ny = len(candidates), mid[0], mid[5]
        out = dict(f_star=f, v_star=v, alpha=al, log_ev=ev, best=np.full(P, -2, dtype=np.int32), log_ev_all=np.full((H, P, ny), np.nan),
                   status=st)
        for k in skip:
            out[k] = None
        arr = self.hyper_array(candidates)
        self._check(self.lib.gpc_dense_select(self.h, C.byref(params), H, C.addressof(arr), *mid,
                                              *map(_ptr, (out[k] for k in ("f_star", "v_star", "alpha", "log_ev", "best", "log_ev_all",
                                                                           "status")))))
        return out

    def dense_select_dev(self, params, candidates, P, off, n_max, n_total, x0, x1, y, ny, m, xs0, xs1, res, sz, f_star=None, v_star=None,
                         alpha_out=None, log_ev=None, best=None, log_ev_all=None, status=None):
        """gpc_dense_select_dev: device pointers throughout, except the candidates (host, read at call time)."""
        arr = self.hyper_array(candidates)
        self._check(self.lib.gpc_dense_select_dev(self.h, C.byref(params), len(candidates), C.addressof(arr), P, _ptr(off), n_max, n_total,
                                                  _ptr(x0), _ptr(x1), _ptr(y), ny, m, _ptr(xs0), _ptr(xs1), float(res), int(sz),
                                                  *map(_ptr, (f_star, v_star, alpha_out, log_ev, best, log_ev_all, status))))

    # ---- dense GP + probit functor, Newton / IRLS loop (BASELINE config 5) ---------------------------------------------
    def _irls_host_args(self, params, irls, off, x0, x1, y, xs0, xs1, res, sz, want_v, want_p):
        """What the four host entries share: the leading arguments of the C call (ctx .. sz), the contiguous inputs behind their
        addresses (the caller keeps them alive over the call), P, and the outputs f, v, p, alpha, fhat, iters, status, log_q filled
        with NaN / -1 (v, p: None where not wanted)."""
        off = np.ascontiguousarray(off, dtype=np.int32)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        if xs0 is not None:
            xs0 = np.ascontiguousarray(xs0, dtype=np.float64)
            xs1 = np.ascontiguousarray(xs1, dtype=np.float64)
            m = xs0.shape[0]
        else:
            m = sz * sz
        P = off.shape[0] - 1
        f = np.full((P, m), np.nan)
        v = np.full((P, m), np.nan) if want_v else None
        p = np.full((P, m), np.nan) if want_p else None
        al, fh = np.full_like(y, np.nan), np.full_like(y, np.nan)
        it, st = np.full(P, -1, dtype=np.int32), np.full(P, -1, dtype=np.int32)
        lq = np.full(P, np.nan)
        keep = (off, x0, x1, y, xs0, xs1)
        head = [self.h, C.byref(params), C.byref(irls), P, _ptr(off), _ptr(x0), _ptr(x1), _ptr(y), m, _ptr(xs0), _ptr(xs1), float(res), int(sz)]
        return head, keep, P, (f, v, p, al, fh, it, st, lq)

    def _irls_dev_args(self, params, irls, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz):
        """The leading arguments of the four _dev entries (ctx .. sz)."""
        return [self.h, C.byref(params), C.byref(irls), P, _ptr(off), n_max, n_total, _ptr(x0), _ptr(x1), _ptr(y), m, _ptr(xs0), _ptr(xs1),
                float(res), int(sz)]

    def dense_irls_fit_predict(self, params, irls, off, x0, x1, y, xs0=None, xs1=None, res=0.0, sz=0):
        """Host-pointer entry (gpc_dense_irls_fit_predict).  y: (N,) labels +-1.  X* point-wise (xs0, xs1) or the sz x sz grid.
        Returns f_star (P, m), alpha (N,), fhat (N,), iters (P,), status (P,)."""
        head, keep, P, (f, _, _, al, fh, it, st, _) = self._irls_host_args(params, irls, off, x0, x1, y, xs0, xs1, res, sz, False, False)
        self._check(self.lib.gpc_dense_irls_fit_predict(*head, *map(_ptr, (f, al, fh, it, st))))
        return f, al, fh, it, st

    def dense_irls_fit_predict_dev(self, params, irls, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz, f_star,
                                   alpha_out=None, fhat_out=None, iters=None, status=None):
        head = self._irls_dev_args(params, irls, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz)
        self._check(self.lib.gpc_dense_irls_fit_predict_dev(*head, *map(_ptr, (f_star, alpha_out, fhat_out, iters, status))))

    def dense_irls_fit_predict_var(self, params, irls, off, x0, x1, y, xs0=None, xs1=None, res=0.0, sz=0, want_v=True, want_p=True):
        """Host-pointer entry (gpc_dense_irls_fit_predict_var): dense_irls_fit_predict with the latent predictive variance v* and the
        occupancy probability p* = Phi(f* / sqrt(s20 + v*)) (noise_model 2 only).  Returns f_star, v_star, p_star (P, m) -- None where
        not wanted --, alpha (N,), fhat (N,), iters (P,), status (P,)."""
        head, keep, P, (f, v, p, al, fh, it, st, _) = self._irls_host_args(params, irls, off, x0, x1, y, xs0, xs1, res, sz, want_v, want_p)
        self._check(self.lib.gpc_dense_irls_fit_predict_var(*head, *map(_ptr, (f, v, p, al, fh, it, st))))
        return f, v, p, al, fh, it, st

    def dense_irls_fit_predict_var_dev(self, params, irls, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz, f_star,
                                       v_star=None, p_star=None, alpha_out=None, fhat_out=None, iters=None, status=None):
        head = self._irls_dev_args(params, irls, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz)
        self._check(self.lib.gpc_dense_irls_fit_predict_var_dev(*head, *map(_ptr, (f_star, v_star, p_star, alpha_out, fhat_out, iters, status))))

    def dense_irls_fit_predict_ev(self, params, irls, off, x0, x1, y, xs0=None, xs1=None, res=0.0, sz=0, want_v=True, want_p=True):
        """Host-pointer entry (gpc_dense_irls_fit_predict_ev): dense_irls_fit_predict_var with the Laplace approximation of the log
        marginal likelihood per patch.  Returns f_star, v_star, p_star (P, m) -- None where not wanted --, alpha (N,), fhat (N,),
        iters (P,), status (P,), log_q (P,)."""
        head, keep, P, (f, v, p, al, fh, it, st, lq) = self._irls_host_args(params, irls, off, x0, x1, y, xs0, xs1, res, sz, want_v, want_p)
        self._check(self.lib.gpc_dense_irls_fit_predict_ev(*head, *map(_ptr, (f, v, p, al, fh, it, st, lq))))
        return f, v, p, al, fh, it, st, lq

    def dense_irls_fit_predict_ev_dev(self, params, irls, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz, f_star,
                                      v_star=None, p_star=None, alpha_out=None, fhat_out=None, iters=None, status=None, log_q=None):
        head = self._irls_dev_args(params, irls, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz)
        self._check(self.lib.gpc_dense_irls_fit_predict_ev_dev(*head, *map(_ptr, (f_star, v_star, p_star, alpha_out, fhat_out, iters, status,
                                                                                  log_q))))

    @staticmethod
    def hyper_array(candidates):
        """A ctypes array of gpc_hyper from (sigmaf_sq, l_sq, noise) triples or Hyper objects."""
        arr = (Hyper * max(len(candidates), 1))()
        for i, c in enumerate(candidates):
            arr[i] = c if isinstance(c, Hyper) else Hyper(*(float(x) for x in c))
        return arr

    def dense_irls_select(self, params, irls, candidates, off, x0, x1, y, xs0=None, xs1=None, res=0.0, sz=0, want_v=True, want_p=True):
        """Host-pointer entry (gpc_dense_irls_select): per patch the candidate (sigmaf_sq, l_sq, noise) of largest Laplace evidence and
        its outputs.  Returns f_star, v_star, p_star (P, m) -- None where not wanted --, alpha (N,), fhat (N,), iters (P,), status (P,),
        log_q (P,), best (P,) int32 (-1: no eligible candidate), log_q_all (H, P)."""
        head, keep, P, (f, v, p, al, fh, it, st, lq) = self._irls_host_args(params, irls, off, x0, x1, y, xs0, xs1, res, sz, want_v, want_p)
        H = len(candidates)
        best = np.full(P, -2, dtype=np.int32)
        lq_all = np.full((H, P), np.nan)
        arr = self.hyper_array(candidates)
        self._check(self.lib.gpc_dense_irls_select(*head[:3], H, C.addressof(arr), *head[3:], *map(_ptr, (f, v, p, al, fh, lq, best, lq_all,
                                                                                                       it, st))))
        return f, v, p, al, fh, it, st, lq, best, lq_all

    def dense_irls_select_dev(self, params, irls, candidates, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz, f_star=None,
                              v_star=None, p_star=None, alpha_out=None, fhat_out=None, log_q=None, best=None, log_q_all=None,
                              iters=None, status=None):
        """gpc_dense_irls_select_dev: device pointers throughout, except the candidates (host, read at call time)."""
        arr = self.hyper_array(candidates)
        head = self._irls_dev_args(params, irls, P, off, n_max, n_total, x0, x1, y, m, xs0, xs1, res, sz)
        self._check(self.lib.gpc_dense_irls_select_dev(*head[:3], len(candidates), C.addressof(arr), *head[3:],
                                                       *map(_ptr, (f_star, v_star, p_star, alpha_out, fhat_out, log_q, best, log_q_all, iters,
                                                                   status))))

    def noise_eval(self, noise_model, s20, y, x, sigma_x):
        """gpc_noise_eval: the device's dx_ln / dx2_ln on arrays of (y, x, sigma_x) -> q, r"""
        y, x, sx = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (y, x, sigma_x))
        q = np.full_like(y, np.nan)
        r = np.full_like(y, np.nan)
        self._check(self.lib.gpc_noise_eval(self.h, int(noise_model), float(s20), len(y), _ptr(y), _ptr(x), _ptr(sx), _ptr(q), _ptr(r)))
        return q, r

    # ---- reprojection + colour clamp (row f3): predicted grids -> pcl::PointXYZRGB records ------------------------------
    POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"),
                            ("a", "u1"), ("pad", "<f4", (3,))])

    def reproject(self, xs0, xs1, f_star, rotations, means, c_star=None, rgb_means=None, bv_count=None):
        """gpc_reproject: f_star (P, m) [+ c_star (P, 3, m)] -> structured array of 32-byte points, compacted over trained patches"""
        f_star = np.ascontiguousarray(f_star, dtype=np.float64)
        P, m = f_star.shape
        xs0 = np.ascontiguousarray(xs0, dtype=np.float64)
        xs1 = np.ascontiguousarray(xs1, dtype=np.float64)
        R = np.ascontiguousarray(rotations, dtype=np.float64).reshape(P, 9)
        mu = np.ascontiguousarray(means, dtype=np.float64).reshape(P, 3)
        cs = None if c_star is None else np.ascontiguousarray(c_star, dtype=np.float64).reshape(P, 3, m)
        cm = None if rgb_means is None else np.ascontiguousarray(rgb_means, dtype=np.float64).reshape(P, 3)
        bv = None if bv_count is None else np.ascontiguousarray(bv_count, dtype=np.int32)
        cloud = np.zeros(max(P * m, 1), dtype=self.POINT_DTYPE)
        npts = np.zeros(1, dtype=np.int32)
        self._check(self.lib.gpc_reproject(self.h, P, m, _ptr(bv), _ptr(xs0), _ptr(xs1), _ptr(f_star), _ptr(cs), _ptr(R), _ptr(mu),
                                           _ptr(cm), _ptr(cloud), _ptr(npts)))
        return cloud[:int(npts[0])]

    def make_cloud(self, xyz, rgb):
        """(n, 3) float32 + (n, 3) uint8 -> array of pcl::PointXYZRGB records"""
        xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
        rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
        c = np.zeros(len(xyz), dtype=self.POINT_DTYPE)
        c["x"], c["y"], c["z"], c["w"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 1.0
        c["r"], c["g"], c["b"], c["a"] = rgb[:, 0], rgb[:, 1], rgb[:, 2], 255
        return c

    def project_cloud(self, cloud, res, sz, n=None):
        """gpc_project_cloud[_dev]: a host record array (make_cloud) or a device buffer of n records -> Patches"""
        h = _vp()
        if isinstance(cloud, np.ndarray):
            assert cloud.dtype == self.POINT_DTYPE
            cloud = np.ascontiguousarray(cloud)
            self._check(self.lib.gpc_project_cloud(self.h, _ptr(cloud) if len(cloud) else None, len(cloud), float(res), int(sz),
                                                   C.byref(h)))
        else:
            self._check(self.lib.gpc_project_cloud_dev(self.h, _ptr(cloud), int(n), float(res), int(sz), C.byref(h)))
        return Patches(self, h, float(res))

    def cloud_distortion(self, a, b, normals_b=None, cell=0.0, max_dist=float("inf"), want=("nn", "d2")):
        """gpc_cloud_distortion, one direction a -> b on host record arrays (make_cloud): for every point of a its EXACT nearest valid
        neighbour in b (ties: the lowest index), D1, D2 along normals_b (nb, 3) float32 if given, colour.  cell: voxel side of the
        search table, 0 = the library's choice (a performance knob: no output depends on it).  Returns a dict of the fields of
        gpc_distortion_result (n_valid, n_matched, n_plane, sse_d1, max_d1, sse_d2, max_d2, sse_rgb (3,), sse_luma) plus the per-point
        arrays named in want: nn (na,) int32, d2, e2 (na,) float64."""
        assert a.dtype == self.POINT_DTYPE and b.dtype == self.POINT_DTYPE
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        nb_ = None if normals_b is None else np.ascontiguousarray(normals_b, dtype=np.float32).reshape(len(b), 3)
        prm = DistortionParams(float(cell), float(max_dist))
        out = {k: np.zeros(max(len(a), 1), dtype=np.int32 if k == "nn" else np.float64) for k in ("nn", "d2", "e2") if k in want}
        res = np.zeros(1, dtype=DISTORTION_RESULT_DTYPE)
        self._check(self.lib.gpc_cloud_distortion(self.h, _ptr(a) if len(a) else None, len(a), _ptr(b) if len(b) else None, len(b),
                                                  _ptr(nb_) if nb_ is not None and len(b) else None, C.byref(prm), _ptr(out.get("nn")),
                                                  _ptr(out.get("d2")), _ptr(out.get("e2")), _ptr(res)))
        return dict({k: res[k][0] for k in DISTORTION_RESULT_DTYPE.names}, **{k: v[:len(a)] for k, v in out.items()})

    def cloud_distortion_dev(self, a, na, b, nb, normals_b=None, cell=0.0, max_dist=float("inf"), nn=None, d2=None, e2=None, result=None):
        """gpc_cloud_distortion_dev: device buffers (tensors or addresses) of na / nb records, normals_b (nb, 3) float32, outputs nn
        int32 / d2 / e2 float64 of na entries (each may be None).  With result (88 bytes on the device, DISTORTION_RESULT_DTYPE) the
        call is left enqueued on the context's stream; without, the result is fetched and returned as a dict."""
        import torch
        prm = DistortionParams(float(cell), float(max_dist))
        mine = None
        if result is None:
            mine = result = torch.zeros(DISTORTION_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
        self._check(self.lib.gpc_cloud_distortion_dev(self.h, _ptr(a), int(na), _ptr(b), int(nb), _ptr(normals_b), C.byref(prm), _ptr(nn),
                                                      _ptr(d2), _ptr(e2), _ptr(result)))
        if mine is None:
            return None
        self.synchronize()
        res = mine.cpu().numpy().view(DISTORTION_RESULT_DTYPE)
        return {k: res[k][0] for k in DISTORTION_RESULT_DTYPE.names}

    def cloud_psnr(self, a, b, peak, normals_a=None, normals_b=None, na=None, nb=None, cell=0.0):
        """Both directions of gpc_cloud_distortion and the symmetric figures a codec reports.  a, b: host record arrays, or device
        buffers with their record counts na, nb (normals then on the device too).  The direction a -> b uses normals_b, b -> a
        normals_a; a direction without normals has no D2.  Returns {"ab": result a -> b, "ba": result b -> a, and per metric in d1, d2,
        r, g, b, luma: {"mse": (a -> b, b -> a), "psnr": psnr()} of the direction with the LARGER mean square error (NaN ignored)}; the peak
        is `peak` for d1 and d2 and 255 for the colours.  A mean over no point is NaN."""
        if isinstance(a, np.ndarray):
            ab = self.cloud_distortion(a, b, normals_b, cell=cell, want=())
            ba = self.cloud_distortion(b, a, normals_a, cell=cell, want=())
        else:
            ab = self.cloud_distortion_dev(a, na, b, nb, normals_b, cell=cell)
            ba = self.cloud_distortion_dev(b, nb, a, na, normals_a, cell=cell)
        return symmetric_psnr(ab, ba, peak)

    def reproject_dev(self, P, m, bv_count, xs0, xs1, f_star, c_star, rotations, means, rgb_means, cloud, n_points):
        self._check(self.lib.gpc_reproject_dev(self.h, P, m, _ptr(bv_count), _ptr(xs0), _ptr(xs1), _ptr(f_star), _ptr(c_star),
                                               _ptr(rotations), _ptr(means), _ptr(rgb_means), _ptr(cloud), _ptr(n_points)))

    def camera_rays(self, R, fx, fy, cx, cy, width, height):
        """gpc_camera_rays_dev: the pinhole rays of a width x height image, pixel v * width + u -> R ((u - cx) / fx, (v - cy) / fy, 1), as a
        device tensor (width * height, 3) float64 for Patches.render.  R (3, 3): the camera's axes in the world.  Not normalised."""
        import torch
        Rc = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(3, 3).T)      # column-major
        dirs = torch.empty((int(width) * int(height), 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize(dirs.device)
        self._check(self.lib.gpc_camera_rays_dev(self.h, _ptr(Rc), float(fx), float(fy), float(cx), float(cy), int(width), int(height),
                                                 _ptr(dirs) if dirs.numel() else None))
        self.synchronize()
        return dirs

    # ---- dense, device buffers (torch tensors or raw addresses), asynchronous on the context's stream ---------
    def dense_fit_predict_dev(self, params, P, off, n_max, n_total, x0, x1, y, ny, m, xs0, xs1, f_star,
                              v_star=None, alpha_out=None, status=None):
        self._check(self.lib.gpc_dense_fit_predict_dev(self.h, C.byref(params), P, _ptr(off), n_max, n_total, _ptr(x0),
                                                       _ptr(x1), _ptr(y), ny, m, _ptr(xs0), _ptr(xs1), _ptr(f_star),
                                                       _ptr(v_star), _ptr(alpha_out), _ptr(status)))

    def dense_fit_predict_grid_dev(self, params, P, off, n_max, n_total, x0, x1, y, ny, res, sz, f_star,
                                   alpha_out=None, status=None):
        self._check(self.lib.gpc_dense_fit_predict_grid_dev(self.h, C.byref(params), P, _ptr(off), n_max, n_total,
                                                            _ptr(x0), _ptr(x1), _ptr(y), ny, float(res), int(sz),
                                                            _ptr(f_star), _ptr(alpha_out), _ptr(status)))


class Patches:
    """gpc_patches: the batch gp_compressor::project_cloud produces, resident on the device."""

    def __init__(self, ctx, h, res=None):
        self.ctx, self.lib, self.h = ctx, ctx.lib, h
        self.res = res                                     # the voxel side the batch was cut with (None: the creator did not say)
        self.view = PatchesView()
        ctx._check(self.lib.gpc_patches_view_dev(h, C.byref(self.view)))
        ctx._children.add(self)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpc_patches_destroy(self.h)
            self.h = None

    __del__ = close

    def fetch(self):
        """host copy as a dict of arrays; R[i] is the 3x3 matrix (columns normal, u, v)"""
        v = self.view
        P, N, m = v.P, v.n_total, v.m
        o = dict(off=np.zeros(P + 1, np.int32), x0=np.zeros(N), x1=np.zeros(N), y=np.zeros(N), rgb=np.zeros((3, N)),
                 R=np.zeros((P, 9)), mean=np.zeros((P, 3)), rgb_mean=np.zeros((P, 3)), W=np.zeros((P, m), np.uint8),
                 src=np.zeros(N, np.int32))
        self.ctx._check(self.lib.gpc_patches_fetch(self.h, *[_ptr(o[k]) for k in ("off", "x0", "x1", "y", "rgb", "R", "mean",
                                                                                  "rgb_mean", "W", "src")]))
        o["R"] = o["R"].reshape(P, 3, 3).transpose(0, 2, 1).copy()
        return o

    def normals(self, n, out=None):
        """gpc_patches_normals[_dev]: (n, 3) float32 for the cloud of n points this batch was cut from: the plane normal (column 0 of R)
        of the leaf that owns a point, NaN for a point no leaf owns.  out: a device buffer of 3 n floats to fill instead (returned)."""
        if out is not None:
            self.ctx._check(self.lib.gpc_patches_normals_dev(self.h, int(n), _ptr(out)))
            return out
        nrm = np.zeros((max(int(n), 1), 3), dtype=np.float32)
        self.ctx._check(self.lib.gpc_patches_normals(self.h, int(n), _ptr(nrm)))
        return nrm[:int(n)]

    def insert_cloud(self, cloud, min_nbr=100, depth=None, n=None):
        """gpc_patches_insert_cloud[_dev]: a registered scan -- host record array (Context.make_cloud) or device buffer of n records -- cut
        against this model.  depth: the model's depth Sparse (None: every leaf counts as trained).  Returns the new Patches (this
        one is untouched) and old_to_new (P,) int32."""
        h = _vp()
        o2n = np.full(max(self.view.P, 1), -1, dtype=np.int32)
        dh = depth.h if depth is not None else None
        if isinstance(cloud, np.ndarray):
            assert cloud.dtype == Context.POINT_DTYPE
            cloud = np.ascontiguousarray(cloud)
            rc = self.lib.gpc_patches_insert_cloud(self.ctx.h, self.h, dh, _ptr(cloud) if len(cloud) else None, len(cloud), int(min_nbr),
                                                   C.byref(h), _ptr(o2n))
        else:
            rc = self.lib.gpc_patches_insert_cloud_dev(self.ctx.h, self.h, dh, _ptr(cloud), int(n), int(min_nbr), C.byref(h), _ptr(o2n))
        self.ctx._check(rc)
        return Patches(self.ctx, h, self.res), o2n[:self.view.P]

    def raycast(self, cloud, origin, cells, depth=None, n=None):
        """gpc_patches_raycast[_dev] (train_classification): the rays from the sensor `origin` (3,) to the points of `cloud` -- the cloud
        this batch was cut from, a host record array or a device buffer of n records -- label `cells` (P, m) uint8, in place: a numpy
        array with a host cloud, a device tensor with a device cloud.  depth: the map's depth Sparse as it is BEFORE the scan is
        trained (None: every leaf counts as trained).  Returns counts (4,) int32: rays, rays that did nothing, occupied writes, free
        writes."""
        org = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        counts = np.zeros(4, dtype=np.int32)
        dh = depth.h if depth is not None else None
        v = self.view
        if isinstance(cloud, np.ndarray):
            assert cloud.dtype == Context.POINT_DTYPE
            cloud = np.ascontiguousarray(cloud)
            assert isinstance(cells, np.ndarray) and cells.dtype == np.uint8 and cells.size == v.P * v.m
            rc = self.lib.gpc_patches_raycast(self.ctx.h, self.h, dh, _ptr(cloud) if len(cloud) else None, len(cloud), _ptr(org),
                                              _ptr(cells), _ptr(counts))
        else:
            assert cells.numel() == v.P * v.m and cells.element_size() == 1
            rc = self.lib.gpc_patches_raycast_dev(self.ctx.h, self.h, dh, _ptr(cloud), int(n), _ptr(org), _ptr(cells), _ptr(counts))
        self.ctx._check(rc)
        return counts

    def render(self, origin, dirs, depth, rgb=None, cells=None, params=None, want=("leaf", "range", "local")):
        """gpc_patches_render[_dev]: the map seen along the rays origin (3,) + t dirs[i] -- dirs (n, 3) float64, a numpy array (then cells
        is a numpy array or None, and numpy arrays come back) or a device tensor (cells a device tensor or None, device tensors come
        back, complete on return).  depth / rgb: the map's Sparse objects (rgb None: colours 0); cells (P, m) uint8: occupancy labels,
        CELL_FREE cells let a ray through.  Returns a dict: cloud (n,) POINT_DTYPE records (device: (n, 32) uint8), counts (5,) int32 =
        rays, hits, rays that never met the grid, surface tests, tests rejected on the residual, and the outputs named in `want`:
        leaf (n,) int32 (-1 = miss), range (n,), local (n, 3) = (f, q1, q2); and, by render_attrs on the render's own leaf and local
        with this origin (so that the normals face the sensor): sigma (n,), conf (n,) the 0-100 confidence form, normal (n, 3)."""
        org = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        prm = params if params is not None else default_params_render()
        counts = np.zeros(5, dtype=np.int32)
        v = self.view
        rh = rgb.h if rgb is not None else None
        shapes = dict(leaf=((), np.int32), range=((), np.float64), local=((3,), np.float64))
        attrs = [k for k in ("sigma", "conf", "normal") if k in want]
        asked, want = tuple(want), [k for k in want if k not in attrs]
        assert set(want) <= set(shapes)
        if attrs:                                          # what the attrs entry reads
            want += [k for k in ("leaf", "local") if k not in want]
        out = {}
        if isinstance(dirs, np.ndarray):
            dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
            n = len(dirs)
            if cells is not None:
                assert isinstance(cells, np.ndarray) and cells.dtype == np.uint8 and cells.size == v.P * v.m
                cells = np.ascontiguousarray(cells)
            out["cloud"] = np.zeros(n, dtype=Context.POINT_DTYPE)
            for k in want:
                out[k] = np.zeros((n,) + shapes[k][0], dtype=shapes[k][1])
            entry = self.lib.gpc_patches_render
        else:
            import torch
            assert dirs.dtype == torch.float64 and dirs.numel() % 3 == 0
            n = dirs.numel() // 3
            if cells is not None:
                assert cells.numel() == v.P * v.m and cells.element_size() == 1
            out["cloud"] = torch.zeros((n, 32), dtype=torch.uint8, device=dirs.device)
            for k in want:
                out[k] = torch.zeros((n,) + shapes[k][0], dtype=torch.int32 if k == "leaf" else torch.float64, device=dirs.device)
            torch.cuda.synchronize(dirs.device)             # the buffers above were filled on torch's stream
            entry = self.lib.gpc_patches_render_dev
        arg = lambda a: _ptr(a) if (a is not None and n) else None
        self.ctx._check(entry(self.ctx.h, self.h, depth.h, rh, arg(cells), C.byref(prm), _ptr(org), arg(dirs), n, arg(out["cloud"]),
                              arg(out.get("leaf")), arg(out.get("range")), arg(out.get("local")), _ptr(counts)))
        if attrs:
            first = "sigma" if "sigma" in attrs else ("conf" if "conf" in attrs else None)
            sg, nm = self.render_attrs(out["leaf"], out["local"], depth, org, conf=first == "conf", want_sigma=first is not None,
                                       want_normal="normal" in attrs)
            if first:
                out[first] = sg
            if "normal" in attrs:
                out["normal"] = nm
            if "sigma" in attrs and "conf" in attrs:
                out["conf"] = self.render_attrs(out["leaf"], out["local"], depth, org, conf=True, want_normal=False)[0]
            for k in ("leaf", "local"):
                if k not in asked:
                    del out[k]
        out["counts"] = counts
        return out

    def render_attrs(self, leaf, local, depth, origin=None, conf=False, want_sigma=True, want_normal=True):
        """gpc_patches_render_attrs[_dev] on the leaf (n,) int32 and local (n, 3) float64 outputs of render (numpy arrays, or device
        tensors: then device tensors come back, complete on return): sigma (n,) -- the depth GP's predictive sigma at the hit, or with
        conf the 0-100 confidence form -- and normal (n, 3), the unit surface normal in the world, facing `origin` (3,) when one is
        given.  NaN at a miss.  Returns (sigma | None, normal | None)."""
        org = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        if isinstance(leaf, np.ndarray):
            leaf = np.ascontiguousarray(leaf, dtype=np.int32).reshape(-1)
            local = np.ascontiguousarray(local, dtype=np.float64).reshape(-1, 3)
            n = len(leaf)
            assert len(local) == n
            sg = np.zeros(n) if want_sigma else None
            nm = np.zeros((n, 3)) if want_normal else None
            entry = self.lib.gpc_patches_render_attrs
        else:
            import torch
            assert leaf.dtype == torch.int32 and local.dtype == torch.float64 and local.numel() == 3 * leaf.numel()
            n = leaf.numel()
            sg = torch.zeros(n, dtype=torch.float64, device=leaf.device) if want_sigma else None
            nm = torch.zeros((n, 3), dtype=torch.float64, device=leaf.device) if want_normal else None
            torch.cuda.synchronize(leaf.device)             # the buffers above were filled on torch's stream
            entry = self.lib.gpc_patches_render_attrs_dev
        arg = lambda a: _ptr(a) if (a is not None and n) else None
        self.ctx._check(entry(self.ctx.h, self.h, depth.h, n, arg(leaf), arg(local), _ptr(org), int(conf), arg(sg), arg(nm)))
        if entry is self.lib.gpc_patches_render_attrs_dev:
            self.ctx.synchronize()
        return sg, nm

    def decode(self, depth, rgb=None, cells=None, use_w=True, want=("leaf", "point"), device=False):
        """gpc_sparse_decode_dev on this batch: the cloud of the map's trained leaves at the grid points whose cell holds data -- W of
        the batch (use_w) and / or cells (P, m) uint8, a device tensor of occupancy labels (CELL_FREE cells are dropped).  depth / rgb:
        the Sparse objects trained on the batch (rgb None: colours 0).  Rotations, means, W, sz and res are the batch's own.  A sizing
        call, an exact allocation, the decode; complete on return.  Returns a dict: cloud (n,) POINT_DTYPE records in ascending (leaf,
        point), and what `want` names of leaf (n,) int32, point (n,) int32 (the grid index p) and count (P,) int32 (kept points per
        leaf).  device=True: device tensors instead of numpy arrays (cloud as (n, 32) uint8)."""
        import torch
        if self.res is None:
            raise ValueError("the Patches object does not know its res (create it through Context.project_cloud)")
        assert set(want) <= {"leaf", "point", "count"}
        v = self.view
        P, sz = v.P, int(round(v.m ** 0.5))
        assert sz * sz == v.m
        if cells is not None:
            assert cells.numel() == P * v.m and cells.element_size() == 1
        dev = cells.device if cells is not None else torch.device("cuda")
        npts = torch.zeros(1, dtype=torch.int32, device=dev)
        count = torch.zeros(max(P, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)                        # the buffers above were filled on torch's stream
        head = (rgb, self.res, sz, v.W if (use_w and P) else None, cells if P else None, v.rotations, v.means,
                v.rgb_means if rgb is not None else None)
        depth.decode_dev(*head, 0, None, count=count, n_points=npts)
        self.ctx.synchronize()
        n = int(npts.cpu()[0])
        cloud = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        out = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("leaf", "point") if k in want}
        torch.cuda.synchronize(dev)
        if n:
            depth.decode_dev(*head, n, cloud, leaf=out.get("leaf"), point=out.get("point"), n_points=npts)
            self.ctx.synchronize()
        if "count" in want:
            out["count"] = count[:P]
        out["cloud"] = cloud
        if not device:
            out = {k: t.cpu().numpy() for k, t in out.items()}
            out["cloud"] = out["cloud"].reshape(-1).view(Context.POINT_DTYPE)
        return out

    def occupancy_batch(self, cells):
        """gpc_occupancy_batch_dev: the labelled cells (device tensor (P, m) uint8) as the ragged batch the probit GP reads -- per leaf the
        observed cells in ascending cell index at their centres, y = +1 occupied / -1 free.  Returns device tensors off (P + 1,) int32,
        x0, x1, y (n_total,) float64 (views of P * m entries) and the host sizes n_total, n_max."""
        import torch
        v = self.view
        assert cells.numel() == v.P * v.m and cells.element_size() == 1
        off = torch.zeros(v.P + 1, dtype=torch.int32, device=cells.device)
        x0, x1, y = (torch.zeros(max(v.P * v.m, 1), dtype=torch.float64, device=cells.device) for _ in range(3))
        nt, nm = C.c_int32(0), C.c_int32(0)
        torch.cuda.synchronize(cells.device)               # the buffers above were filled on torch's stream
        self.ctx._check(self.lib.gpc_occupancy_batch_dev(self.ctx.h, self.h, _ptr(cells), _ptr(off), _ptr(x0), _ptr(x1), _ptr(y),
                                                         C.addressof(nt), C.addressof(nm)))
        N = int(nt.value)
        return off, x0[:N], x1[:N], y[:N], N, int(nm.value)


class Sparse:
    """gpc_sparse: P independent sparse_gp (ny=1) / sparse_gp_field (ny=3) states resident on the device."""

    def __init__(self, ctx, params, P, ny=1):
        self.ctx, self.lib, self.P, self.ny = ctx, ctx.lib, P, ny
        h = _vp()
        ctx._check(self.lib.gpc_sparse_create(ctx.h, C.byref(params), P, ny, C.byref(h)))
        self.h = h
        ctx._children.add(self)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpc_sparse_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        self.ctx._check(self.lib.gpc_sparse_reset(self.h))

    def remap(self, P_new, old_to_new):
        """gpc_sparse_remap: a new Sparse of P_new patches, patch old_to_new[i] holding this object's patch i, the others empty"""
        o2n = np.ascontiguousarray(old_to_new, dtype=np.int32)
        assert o2n.shape == (self.P,)
        h = _vp()
        self.ctx._check(self.lib.gpc_sparse_remap(self.h, int(P_new), _ptr(o2n) if self.P else None, C.byref(h)))
        g = Sparse.__new__(Sparse)
        g.ctx, g.lib, g.P, g.ny, g.h = self.ctx, self.lib, int(P_new), self.ny, h
        self.ctx._children.add(g)
        return g

    def add(self, off, x0, x1, y, perm=None, trace=False):
        """trace=True: also returns the decision bytes of the call (gpc_sparse_set_trace), (N,) uint8 in insertion order"""
        off = np.ascontiguousarray(off, dtype=np.int32)
        y = np.ascontiguousarray(np.atleast_2d(y), dtype=np.float64)
        assert y.shape[0] == self.ny and off.shape[0] == self.P + 1
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        st = np.full(self.P, -1, dtype=np.int32)
        tr, d_tr = None, _vp()
        if trace:
            tr = np.zeros(max(int(off[-1]), 1), dtype=np.uint8)
            self.ctx._check(self.lib.gpc_dev_malloc(self.ctx.h, tr.nbytes, C.byref(d_tr)))
            self.ctx._check(self.lib.gpc_dev_memcpy(self.ctx.h, d_tr, _ptr(tr), tr.nbytes, 1))
            self.ctx._check(self.lib.gpc_sparse_set_trace(self.h, d_tr))
        try:
            self.ctx._check(self.lib.gpc_sparse_add(self.h, _ptr(off), _ptr(x0), _ptr(x1), _ptr(y), _ptr(pm), _ptr(st)))
            if trace:
                self.ctx._check(self.lib.gpc_dev_memcpy(self.ctx.h, _ptr(tr), d_tr, tr.nbytes, 2))
        finally:
            if trace:
                self.lib.gpc_sparse_set_trace(self.h, None)
                self.lib.gpc_dev_free(self.ctx.h, d_tr)
        return (st, tr[:int(off[-1])]) if trace else st

    def add_dev(self, off, n_max, n_total, x0, x1, y, perm=None, status=None):
        self.ctx._check(self.lib.gpc_sparse_add_dev(self.h, _ptr(off), n_max, n_total, _ptr(x0), _ptr(x1), _ptr(y),
                                                    _ptr(perm), _ptr(status)))

    def predict(self, xs0, xs1, want_sigma=True, conf=False):
        xs0 = np.ascontiguousarray(xs0, dtype=np.float64)
        xs1 = np.ascontiguousarray(xs1, dtype=np.float64)
        m = xs0.shape[0]
        f = np.full((self.P, self.ny, m), np.nan)
        s = np.full((self.P, m), np.nan) if want_sigma else None
        st = np.full(self.P, -1, dtype=np.int32)
        self.ctx._check(self.lib.gpc_sparse_predict(self.h, m, _ptr(xs0), _ptr(xs1), _ptr(f), _ptr(s), int(conf), _ptr(st)))
        return f, s, st

    def predict_dev(self, m, xs0, xs1, f_star, sigma=None, conf=False, status=None):
        self.ctx._check(self.lib.gpc_sparse_predict_dev(self.h, m, _ptr(xs0), _ptr(xs1), _ptr(f_star), _ptr(sigma),
                                                        int(conf), _ptr(status)))

    def decode_dev(self, rgb, res, sz, W, cells, rotations, means, rgb_means, capacity, cloud, leaf=None, point=None, count=None,
                   n_points=None):
        """gpc_sparse_decode_dev with this object as the depth GP (rgb: the colour Sparse or None): device tensors or raw addresses,
        enqueued on the context's stream.  cloud None is the sizing call."""
        self.ctx._check(self.lib.gpc_sparse_decode_dev(self.h, rgb.h if rgb is not None else None, float(res), int(sz), _ptr(W), _ptr(cells),
                                                       _ptr(rotations), _ptr(means), _ptr(rgb_means), int(capacity), _ptr(cloud),
                                                       _ptr(leaf), _ptr(point), _ptr(count), _ptr(n_points)))

    def decode(self, rgb, res, sz, rotations, means, rgb_means=None, W=None, cells=None, capacity=None):
        """gpc_sparse_decode (host arrays, synchronous) with this object as the depth GP.  capacity None: a sizing call first, then
        exactly n_points records.  Returns cloud (min(n_points, capacity),) POINT_DTYPE, leaf, point (same length) int32, count (P,)
        int32 and n_points."""
        P, m = self.P, int(sz) * int(sz)
        f8 = lambda a, k: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(P, k)
        u1 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint8).reshape(P, m)
        head = (self.h, rgb.h if rgb is not None else None, float(res), int(sz), _ptr(u1(W)), _ptr(u1(cells)), _ptr(f8(rotations, 9)),
                _ptr(f8(means, 3)), _ptr(f8(rgb_means, 3)))
        count = np.zeros(max(P, 1), dtype=np.int32)
        npts = np.zeros(1, dtype=np.int32)
        if capacity is None:
            self.ctx._check(self.lib.gpc_sparse_decode(*head, 0, None, None, None, _ptr(count), _ptr(npts)))
            capacity = int(npts[0])
        cloud = np.zeros(max(capacity, 1), dtype=Context.POINT_DTYPE)
        leaf, point = np.zeros(max(capacity, 1), dtype=np.int32), np.zeros(max(capacity, 1), dtype=np.int32)
        self.ctx._check(self.lib.gpc_sparse_decode(*head, int(capacity), _ptr(cloud), _ptr(leaf), _ptr(point), _ptr(count), _ptr(npts)))
        w = min(int(npts[0]), int(capacity))
        return cloud[:w], leaf[:w], point[:w], count[:P], int(npts[0])

    def predict_points(self, off, x0, x1, want_sigma=False, conf=False):
        """predict_measurements with every patch on its own (ragged) point set: f (ny, N), sigma (N,)|None, status (P,)"""
        off = np.ascontiguousarray(off, dtype=np.int32)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        N = int(off[-1])
        assert off.shape[0] == self.P + 1 and x0.shape[0] == N and x1.shape[0] == N
        f = np.full((self.ny, N), np.nan)
        s = np.full(N, np.nan) if want_sigma else None
        st = np.full(self.P, -1, dtype=np.int32)
        self.ctx._check(self.lib.gpc_sparse_predict_points(self.h, _ptr(off), _ptr(x0), _ptr(x1), _ptr(f), _ptr(s), int(conf), _ptr(st)))
        return f, s, st

    def predict_points_dev(self, off, n_total, x0, x1, f, sigma=None, conf=False, status=None):
        self.ctx._check(self.lib.gpc_sparse_predict_points_dev(self.h, _ptr(off), int(n_total), _ptr(x0), _ptr(x1), _ptr(f),
                                                               _ptr(sigma), int(conf), _ptr(status)))

    def predict_scattered(self, patch, x0, x1, want_sigma=True, conf=False):
        """gpc_sparse_predict_scattered: predict_measurements at (patch[i], (x0[i], x1[i])) pairs in any order -- numpy arrays of one
        length n.  Entries whose patch is outside [0, P) are skipped (NaN).  Returns f (ny, n), sigma (n,)|None, status (P,), bit for
        bit what predict_points gives on the entries bucketed by patch in ascending i."""
        patch = np.ascontiguousarray(patch, dtype=np.int32)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        n = patch.shape[0]
        assert patch.shape == x0.shape == x1.shape == (n,)
        f = np.full((self.ny, n), np.nan)
        s = np.full(n, np.nan) if want_sigma else None
        st = np.full(self.P, -1, dtype=np.int32)
        arg = lambda a: _ptr(a) if (a is not None and n) else None
        self.ctx._check(self.lib.gpc_sparse_predict_scattered(self.h, n, arg(patch), arg(x0), arg(x1), 1, arg(f), arg(s),
                                                              int(conf), _ptr(st)))
        return f, s, st

    def predict_scattered_dev(self, n, patch, x0, x1, stride=1, f=None, sigma=None, conf=False, status=None):
        """gpc_sparse_predict_scattered_dev: device pointers (tensors or addresses), enqueued on the context's stream; entry i reads
        x0[i * stride], x1[i * stride]"""
        self.ctx._check(self.lib.gpc_sparse_predict_scattered_dev(self.h, int(n), _ptr(patch), _ptr(x0), _ptr(x1), int(stride), _ptr(f),
                                                                  _ptr(sigma), int(conf), _ptr(status)))

    def likelihood(self, off, x0, x1, y, want_dx=True, want_l=True):
        """compute_derivatives + compute_likelihoods (src/sparse_gp.h:44-45) on a ragged batch: dX (N, 3), l (N)"""
        off = np.ascontiguousarray(off, dtype=np.int32)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        y = np.ascontiguousarray(np.atleast_2d(y), dtype=np.float64)
        N = int(off[-1])
        assert y.shape == (self.ny, N) and off.shape[0] == self.P + 1
        dX = np.full((N, 3), np.nan) if want_dx else None
        l = np.full(N, np.nan) if want_l else None
        self.ctx._check(self.lib.gpc_sparse_likelihood(self.h, _ptr(off), _ptr(x0), _ptr(x1), _ptr(y), _ptr(dX), _ptr(l)))
        return dX, l

    def likelihood_dev(self, off, n_total, x0, x1, y, dX=None, l=None):
        self.ctx._check(self.lib.gpc_sparse_likelihood_dev(self.h, _ptr(off), int(n_total), _ptr(x0), _ptr(x1), _ptr(y),
                                                           _ptr(dX), _ptr(l)))

    def train_sigmaf(self, off, x0, x1, y, step=float(np.float32(1e-4)), max_counter=100):
        """the live part of train_parameters (src/sparse_gp.hpp:586-640) per patch: returns p0 (P,), iters (P,),
        ls (P, max_counter + 2), delta (P, 2)"""
        off = np.ascontiguousarray(off, dtype=np.int32)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        assert off.shape[0] == self.P + 1 and y.shape[0] == int(off[-1])
        p0 = np.full(self.P, np.nan)
        iters = np.full(self.P, -1, dtype=np.int32)
        ls = np.zeros((self.P, max_counter + 2))
        delta = np.full((self.P, 2), np.nan)
        self.ctx._check(self.lib.gpc_sparse_train_sigmaf(self.h, _ptr(off), _ptr(x0), _ptr(x1), _ptr(y), float(step), int(max_counter),
                                                         _ptr(p0), _ptr(iters), _ptr(ls), _ptr(delta)))
        return p0, iters, ls, delta

    def train_sigmaf_dev(self, off, n_total, x0, x1, y, step, max_counter, p0, iters, ls, delta):
        self.ctx._check(self.lib.gpc_sparse_train_sigmaf_dev(self.h, _ptr(off), int(n_total), _ptr(x0), _ptr(x1), _ptr(y), float(step),
                                                             int(max_counter), _ptr(p0), _ptr(iters), _ptr(ls), _ptr(delta)))

    def prune(self, keep=None, target=None, score_tol=0.0, want_trace=False):
        """gpc_sparse_prune (host arrays): every patch keeps removing its lowest-score basis vector until it holds `keep` (or its entry
        of `target`, (P,) int32) vectors, then while the lowest score is below score_tol.  In place; remap(P, arange(P)) is the copy to
        prune from.  Returns removed (P,) int32, and with want_trace also order (P, ld) int32 and scores (P, ld): the first removed[p]
        entries of a row are the removals in order, the others stay -1 / NaN."""
        tg = None if target is None else np.ascontiguousarray(target, dtype=np.int32)
        assert tg is None or tg.shape == (self.P,)
        ld = self.ld()
        rm = np.zeros(self.P, dtype=np.int32)
        order = np.full((self.P, ld), -1, dtype=np.int32) if want_trace else None
        scores = np.full((self.P, ld), np.nan) if want_trace else None
        self.ctx._check(self.lib.gpc_sparse_prune(self.h, 0 if keep is None else int(keep), _ptr(tg), float(score_tol), _ptr(rm),
                                                  _ptr(order), _ptr(scores), None))
        return (rm, order, scores) if want_trace else rm

    def prune_dev(self, keep=None, target=None, score_tol=0.0, removed=None, order=None, scores=None, status=None):
        """gpc_sparse_prune_dev: device buffers (each may be None), enqueued on the context's stream"""
        self.ctx._check(self.lib.gpc_sparse_prune_dev(self.h, 0 if keep is None else int(keep), _ptr(target), float(score_tol),
                                                      _ptr(removed), _ptr(order), _ptr(scores), _ptr(status)))

    def prune_rd(self, off, x0, x1, y, keep=None, target=None, max_mse=float("inf"), max_mse_p=None, want_trace=False):
        """gpc_sparse_prune_rd (host arrays): the removals of prune, each taken only while the mean square error of the state it would
        leave on the patch's own points -- patch p owns rows off[p] .. off[p+1]-1 of x0, x1 and y (ny, N) -- stays within max_mse (or its
        entry of max_mse_p, (P,)); stops at the first look-ahead beyond the bound.  In place.  Returns removed (P,) int32, mse0 (P,) the
        error before the call (NaN for a patch without points) and mse_next (P,) the look-ahead that stopped the patch (NaN when the
        floor keep / target stopped it); with want_trace also order (P, ld) int32, scores (P, ld) and mse (P, ld): the first removed[p]
        entries of a row are the removals in order and the error after each, the others stay -1 / NaN."""
        off = np.ascontiguousarray(off, dtype=np.int32)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        N = int(off[-1]) if len(off) else 0
        assert off.shape[0] == self.P + 1 and x0.shape[0] == N and x1.shape[0] == N and y.size == self.ny * N
        tg = None if target is None else np.ascontiguousarray(target, dtype=np.int32)
        bp = None if max_mse_p is None else np.ascontiguousarray(max_mse_p, dtype=np.float64)
        assert (tg is None or tg.shape == (self.P,)) and (bp is None or bp.shape == (self.P,))
        ld = self.ld()
        rm = np.zeros(self.P, dtype=np.int32)
        mse0, nxt = np.full(self.P, np.nan), np.full(self.P, np.nan)
        order = np.full((self.P, ld), -1, dtype=np.int32) if want_trace else None
        scores = np.full((self.P, ld), np.nan) if want_trace else None
        mse = np.full((self.P, ld), np.nan) if want_trace else None
        self.ctx._check(self.lib.gpc_sparse_prune_rd(self.h, _ptr(off), _ptr(x0), _ptr(x1), _ptr(y), 0 if keep is None else int(keep),
                                                     _ptr(tg), float(max_mse), _ptr(bp), _ptr(rm), _ptr(order), _ptr(scores), _ptr(mse),
                                                     _ptr(mse0), _ptr(nxt), None))
        return (rm, mse0, nxt, order, scores, mse) if want_trace else (rm, mse0, nxt)

    def prune_rd_dev(self, off, n_total, x0, x1, y, keep=None, target=None, max_mse=float("inf"), max_mse_p=None, removed=None, order=None,
                     scores=None, mse=None, mse0=None, mse_next=None, status=None):
        """gpc_sparse_prune_rd_dev: device buffers (each output may be None), enqueued on the context's stream"""
        self.ctx._check(self.lib.gpc_sparse_prune_rd_dev(self.h, _ptr(off), int(n_total), _ptr(x0), _ptr(x1), _ptr(y),
                                                         0 if keep is None else int(keep), _ptr(target), float(max_mse), _ptr(max_mse_p),
                                                         _ptr(removed), _ptr(order), _ptr(scores), _ptr(mse), _ptr(mse0), _ptr(mse_next),
                                                         _ptr(status)))

    def quantize_rd(self, off, x0, x1, y, bits_min=1, bits_max=16, max_mse=float("inf"), max_mse_p=None, want_curve=False):
        """gpc_sparse_quantize_rd (host arrays): per patch the smallest width w in bits_min .. bits_max at which the state, with BV and
        alpha rounded to w-bit codes over their float range, keeps its mean square error on the patch's own points within max_mse (or
        its entry of max_mse_p, (P,)).  The object is not modified.  Returns bits (P,) int32 (0: no width accepted, or an escaped patch
        -- no vectors, no points or a non-finite value), q_alpha (P, ny, ld) and q_bv (P, ld, 2) uint16 (zero where nothing was
        written), range (P, ny + 2, 2) float32 (NaN where not written), mse0 (P,), mse_q (P,); with want_curve also curve (P, 16), entry
        w - 1 the error at width w, NaN where not evaluated."""
        off = np.ascontiguousarray(off, dtype=np.int32)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        N = int(off[-1]) if len(off) else 0
        assert off.shape[0] == self.P + 1 and x0.shape[0] == N and x1.shape[0] == N and y.size == self.ny * N
        bp = None if max_mse_p is None else np.ascontiguousarray(max_mse_p, dtype=np.float64)
        assert bp is None or bp.shape == (self.P,)
        ld = self.ld()
        bits = np.zeros(self.P, dtype=np.int32)
        qa = np.zeros((self.P, self.ny, ld), dtype=np.uint16)
        qb = np.zeros((self.P, ld, 2), dtype=np.uint16)
        rng = np.full((self.P, self.ny + 2, 2), np.nan, dtype=np.float32)
        mse0, mseq = np.full(self.P, np.nan), np.full(self.P, np.nan)
        curve = np.full((self.P, 16), np.nan) if want_curve else None
        self.ctx._check(self.lib.gpc_sparse_quantize_rd(self.h, _ptr(off), _ptr(x0), _ptr(x1), _ptr(y), int(bits_min), int(bits_max),
                                                        float(max_mse), _ptr(bp), _ptr(bits), _ptr(qa), _ptr(qb), _ptr(rng), _ptr(mse0),
                                                        _ptr(mseq), _ptr(curve), None))
        return (bits, qa, qb, rng, mse0, mseq, curve) if want_curve else (bits, qa, qb, rng, mse0, mseq)

    def quantize_rd_dev(self, off, n_total, x0, x1, y, bits_min=1, bits_max=16, max_mse=float("inf"), max_mse_p=None, bits=None,
                        q_alpha=None, q_bv=None, range=None, mse0=None, mse_q=None, curve=None, status=None):
        """gpc_sparse_quantize_rd_dev: device buffers (each output may be None), enqueued on the context's stream"""
        self.ctx._check(self.lib.gpc_sparse_quantize_rd_dev(self.h, _ptr(off), int(n_total), _ptr(x0), _ptr(x1), _ptr(y), int(bits_min),
                                                            int(bits_max), float(max_mse), _ptr(max_mse_p), _ptr(bits), _ptr(q_alpha),
                                                            _ptr(q_bv), _ptr(range), _ptr(mse0), _ptr(mse_q), _ptr(curve), _ptr(status)))

    def dequantize(self, bv_count, bits, q_alpha, q_bv, range):
        """gpc_sparse_dequantize (host arrays, the layouts quantize_rd returns): every patch with bits in 1..16 gets the dequantised
        alpha and BV, the count bv_count and zero C and Q; a patch with bits 0 is not touched"""
        ld = self.ld()
        b = np.ascontiguousarray(bv_count, dtype=np.int32)
        w = np.ascontiguousarray(bits, dtype=np.int32)
        qa = np.ascontiguousarray(q_alpha, dtype=np.uint16)
        qb = np.ascontiguousarray(q_bv, dtype=np.uint16)
        rng = np.ascontiguousarray(range, dtype=np.float32)
        assert b.shape == w.shape == (self.P,) and qa.shape == (self.P, self.ny, ld) and qb.shape == (self.P, ld, 2)
        assert rng.shape == (self.P, self.ny + 2, 2)
        self.ctx._check(self.lib.gpc_sparse_dequantize(self.h, _ptr(b), _ptr(w), _ptr(qa), _ptr(qb), _ptr(rng)))

    def dequantize_dev(self, bv_count, bits, q_alpha, q_bv, range):
        """gpc_sparse_dequantize_dev: device buffers, enqueued on the context's stream"""
        self.ctx._check(self.lib.gpc_sparse_dequantize_dev(self.h, _ptr(bv_count), _ptr(bits), _ptr(q_alpha), _ptr(q_bv), _ptr(range)))

    def rd_curves_dev(self, off, n_total, x0, x1, y):
        """Every patch's whole rate-distortion curve, the object untouched: prune_rd_dev(keep=1, max_mse=inf) on an identity remap copy.
        Device batch as prune_rd_dev takes it.  Returns device tensors removed (P,) int32, mse0 (P,), mse (P, ld) -- NaN beyond
        removed[p]; enqueued, not synchronised."""
        import torch
        P, ld = self.P, self.ld()
        removed = torch.zeros(max(P, 1), dtype=torch.int32, device="cuda")
        mse0 = torch.full((max(P, 1),), float("nan"), dtype=torch.float64, device="cuda")
        mse = torch.full((max(P, 1), ld), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize(mse.device)
        cp = self.remap(P, np.arange(P, dtype=np.int32))
        try:
            cp.prune_rd_dev(off, n_total, x0, x1, y, keep=1, max_mse=float("inf"), removed=removed, mse=mse, mse0=mse0)
            self.ctx.synchronize()
        finally:
            cp.close()
        return removed, mse0, mse

    def prune_to_bytes(self, off, x0, x1, y, need, weight=None, refine=True):
        """Rate control to a byte budget: save at least `need` bytes of the model file (24 bytes per vector with ny = 1, 40 with ny = 3)
        by the removals that raise sum_p weight[p] n_p ny mse_p least.  The batch is prune_rd's (host arrays, or device tensors);
        weight (P,) defaults to 1.  The curves come from an identity remap copy, the allocation from Context.rate_allocate_dev, and the
        object itself is then pruned in place to b - k per patch (prune_dev(target=..., score_tol=0) replays the first k removals of
        the curve's chain).  Returns (k (P,) int32, result); an infeasible `need` prunes to choice(+inf) and reports feasible = 0."""
        import torch

        def dev(a, dt):
            return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda")
        off_h = off.cpu().numpy() if torch.is_tensor(off) else np.ascontiguousarray(off, dtype=np.int32)
        P, ld = self.P, self.ld()
        assert off_h.shape == (P + 1,)
        k = np.zeros(P, dtype=np.int32)
        if P == 0:
            return k, rate_result(np.zeros(1, dtype=RATE_RESULT_DTYPE))
        n_p = np.diff(off_h).astype(np.float64)
        wt = np.ones(P) if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
        assert wt.shape == (P,)
        d_off, d_x0, d_x1, d_y = dev(off, np.int32), dev(x0, np.float64), dev(x1, np.float64), dev(y, np.float64)
        d_w = torch.from_numpy(wt * n_p * float(self.ny)).to("cuda")
        d_count = torch.from_numpy(self.sizes()).to("cuda")
        d_k = torch.zeros(P, dtype=torch.int32, device="cuda")
        d_target = torch.zeros(P, dtype=torch.int32, device="cuda")
        d_res = torch.zeros(RATE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        removed, mse0, mse = self.rd_curves_dev(d_off, int(off_h[-1]), d_x0, d_x1, d_y)    # (synchronises: the buffers above are ready)
        self.ctx.rate_allocate_dev(P, ld, removed, mse0, mse, int(need), w=d_w, unit_all=24 if self.ny == 1 else 40, refine=refine,
                                   count=d_count, k=d_k, target=d_target, result=d_res)
        self.prune_dev(target=d_target, score_tol=0.0)
        self.ctx.synchronize()
        return d_k.cpu().numpy(), rate_result(d_res)

    def sizes(self):
        b = np.zeros(self.P, dtype=np.int32)
        self.ctx._check(self.lib.gpc_sparse_sizes(self.h, _ptr(b)))
        return b

    def ld(self):
        return self.lib.gpc_sparse_ld(self.h)

    def state(self):
        ld = self.ld()
        alpha = np.zeros((self.P, self.ny, ld))
        Cc = np.zeros((self.P, ld, ld))
        Q = np.zeros((self.P, ld, ld))
        BV = np.zeros((self.P, ld, 2))
        self.ctx._check(self.lib.gpc_sparse_get_state(self.h, _ptr(alpha), _ptr(Cc), _ptr(Q), _ptr(BV)))
        # C, Q are column-major per patch: [p][j][i] = M(i, j)
        return alpha, np.transpose(Cc, (0, 2, 1)).copy(), np.transpose(Q, (0, 2, 1)).copy(), BV


def _sparse_set_state(self, bv_count, alpha, BV, C_=None, Q=None):
    """gpc_sparse_set_state: alpha (P, ny, ld), BV (P, ld, 2), optional C/Q (P, ld, ld) as returned by state() (row-major views)"""
    ld = self.ld()
    bv = np.ascontiguousarray(bv_count, dtype=np.int32)
    al = np.ascontiguousarray(alpha, dtype=np.float64).reshape(self.P, self.ny, ld)
    bvv = np.ascontiguousarray(BV, dtype=np.float64).reshape(self.P, ld, 2)
    cc = None if C_ is None else np.ascontiguousarray(np.transpose(C_, (0, 2, 1)))
    qq = None if Q is None else np.ascontiguousarray(np.transpose(Q, (0, 2, 1)))
    self.ctx._check(self.lib.gpc_sparse_set_state(self.h, _ptr(bv), _ptr(al), _ptr(cc), _ptr(qq), _ptr(bvv)))


Sparse.set_state = _sparse_set_state


class Registration:
    """gpc_registration: gp_registration (src/gp_registration.cpp) on a model that is already on the device -- a Patches batch and
    the depth (ny=1) and colour (ny=3) Sparse objects trained on it.  Refers to the three, owns none: keep them open while this is."""

    def __init__(self, ctx, patches, depth, rgb):
        self.ctx, self.lib = ctx, ctx.lib
        h = _vp()
        ctx._check(self.lib.gpc_registration_create(ctx.h, patches.h, depth.h, rgb.h, C.byref(h)))
        self.h = h
        self.n = 0
        ctx._children.add(self)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpc_registration_destroy(self.h)
            self.h = None

    __del__ = close

    def set_cloud(self, cloud, n=None):
        """add_cloud: a host record array (Context.make_cloud) or a device buffer of n records; resets the pose and the step count"""
        if isinstance(cloud, np.ndarray):
            assert cloud.dtype == Context.POINT_DTYPE
            cloud = np.ascontiguousarray(cloud)
            self.ctx._check(self.lib.gpc_registration_set_cloud(self.h, _ptr(cloud) if len(cloud) else None, len(cloud)))
            self.n = len(cloud)
        else:
            self.ctx._check(self.lib.gpc_registration_set_cloud_dev(self.h, _ptr(cloud), int(n)))
            self.n = int(n)

    def step(self, params=None):
        """one registration_step: out (9,) = delta[6], ls, cls, n_used"""
        out = np.full(9, np.nan)
        prm = params if params is not None else default_params_registration()
        self.ctx._check(self.lib.gpc_registration_step(self.h, C.byref(prm), _ptr(out)))
        return out

    def run(self, params=None):
        """steps until registration_done(): returns trace (steps, 9), one row of step() output per step"""
        prm = params if params is not None else default_params_registration()
        trace = np.full((max(int(prm.max_steps), 1), 9), np.nan)
        steps = np.zeros(1, dtype=np.int32)
        self.ctx._check(self.lib.gpc_registration_run(self.h, C.byref(prm), _ptr(trace), _ptr(steps)))
        return trace[:min(int(steps[0]), len(trace))]

    def transform(self):
        """get_cloud_transformation: R_cloud (3, 3), t_cloud (3,)"""
        R = np.zeros(9)
        t = np.zeros(3)
        self.ctx._check(self.lib.gpc_registration_get_transform(self.h, _ptr(R), _ptr(t)))
        return R.reshape(3, 3).T.copy(), t

    def cloud(self):
        """the working cloud as a record array"""
        c = np.zeros(self.n, dtype=Context.POINT_DTYPE)
        self.ctx._check(self.lib.gpc_registration_get_cloud(self.h, _ptr(c) if self.n else None))
        return c

    def cloud_dev(self):
        """the working cloud where it is: (device address, n); valid until the next set_cloud or close"""
        p, n = _vp(), C.c_int(0)
        self.ctx._check(self.lib.gpc_registration_cloud_dev(self.h, C.byref(p), C.byref(n)))
        return (p.value or 0), int(n.value)

    def assignment(self):
        """what the last step assigned: owner (n,) int32 (-1 = unused), local (n, 3) = depth, x0, x1 in the owner's frame"""
        owner = np.full(self.n, -1, dtype=np.int32)
        local = np.zeros((self.n, 3))
        self.ctx._check(self.lib.gpc_registration_get_assignment(self.h, _ptr(owner), _ptr(local)))
        return owner, local


class Mapping:
    """gp_mapping (src/gp_mapping.cpp): a map -- a Patches batch with the depth (ny=1) and colour (ny=3) Sparse objects trained on it --
    that grows scan by scan.  Takes the three over: add_cloud replaces them by new objects and closes the old ones."""

    def __init__(self, ctx, patches, depth, rgb, params=None, min_nbr=100):
        self.ctx, self.patches, self.depth, self.rgb = ctx, patches, depth, rgb
        self.params = params if params is not None else default_params_registration()
        self.min_nbr = int(min_nbr)
        self.reg = Registration(ctx, patches, depth, rgb)
        # the occupancy labels of every leaf's cells (train_classification's `free`, with a third state): CELL_UNOBSERVED until a ray
        # of an inserted scan meets the cell
        import torch
        self.cells = torch.zeros((patches.view.P, patches.view.m), dtype=torch.uint8, device="cuda")

    def close(self):
        for o in (getattr(self, "reg", None), getattr(self, "depth", None), getattr(self, "rgb", None), getattr(self, "patches", None)):
            if o is not None:
                o.close()
        self.reg = self.depth = self.rgb = self.patches = self.cells = None

    def add_cloud(self, cloud, n=None, perm_depth=None, perm_rgb=None):
        """gp_mapping::add_cloud (:12-28): register the scan (host record array or device buffer of n records) against the map; if the
        loop stopped before max_steps (:22) insert it (insert_into_map) and train the leaf GPs on what was inserted (train_processes),
        else drop it (:26).  perm_depth / perm_rgb: optional insertion orders for the new batch (device, as Sparse.add_dev takes them).
        Returns (steps, inserted)."""
        self.reg.set_cloud(cloud, n)
        steps = len(self.reg.run(self.params))             # = step_nbr: set_cloud restarted the count
        if steps >= self.params.max_steps:
            self.reg.set_cloud(np.zeros(0, dtype=Context.POINT_DTYPE))
            return steps, False
        d_cloud, m = self.reg.cloud_dev()
        pt, o2n = self.patches.insert_cloud(d_cloud, self.min_nbr, self.depth, n=m)
        v = pt.view
        gd, gc = self.depth.remap(v.P, o2n), self.rgb.remap(v.P, o2n)
        # train_classification (:148, before train_processes): the leaves the scan trains below do not count as trained yet
        import torch
        cells = torch.zeros((v.P, v.m), dtype=torch.uint8, device=self.cells.device)
        cells[torch.from_numpy(o2n.astype(np.int64)).to(cells.device)] = self.cells
        torch.cuda.synchronize(cells.device)
        pt.raycast(d_cloud, self.reg.transform()[1], cells, depth=gd, n=m)
        self.cells = cells
        gd.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y, perm_depth)
        gc.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb, perm_rgb)
        self.ctx.synchronize()
        reg = Registration(self.ctx, pt, gd, gc)
        for o in (self.reg, self.depth, self.rgb, self.patches):
            o.close()
        self.reg, self.patches, self.depth, self.rgb = reg, pt, gd, gc
        return steps, True

    def prune(self, keep_depth, keep_rgb, score_tol_depth=0.0, score_tol_rgb=0.0):
        """Bound the map: prune the depth and the colour GP of every leaf in place (Sparse.prune_dev).  The Registration object refers
        to the same two objects and sees the pruned state; later add_cloud calls may grow the leaves again, up to their capacity."""
        self.depth.prune_dev(keep=keep_depth, score_tol=score_tol_depth)
        self.rgb.prune_dev(keep=keep_rgb, score_tol=score_tol_rgb)
        self.ctx.synchronize()

    def prune_to_error(self, max_mse_depth, max_mse_rgb, keep_depth=1, keep_rgb=1):
        """Bound the map by distortion: prune the depth and the colour GP of every leaf in place (Sparse.prune_rd_dev) while the mean
        square error on the points of the map's current batch -- the last inserted scan -- stays within max_mse_depth / max_mse_rgb.
        Leaves the scan did not touch have no points there and are left alone.  Returns removed (P,) int32 per GP: (depth, colour)."""
        import torch
        v = self.patches.view
        rm = torch.zeros((2, max(v.P, 1)), dtype=torch.int32, device=self.cells.device)
        torch.cuda.synchronize(rm.device)
        self.depth.prune_rd_dev(v.off, v.n_total, v.x0, v.x1, v.y, keep=keep_depth, max_mse=max_mse_depth, removed=rm[0])
        self.rgb.prune_rd_dev(v.off, v.n_total, v.x0, v.x1, v.rgb, keep=keep_rgb, max_mse=max_mse_rgb, removed=rm[1])
        self.ctx.synchronize()
        out = rm.cpu().numpy()
        return out[0, :v.P], out[1, :v.P]

    def prune_to_bytes(self, need, w_depth=0.0, w_rgb=0.0):
        """Bound the map by size: save at least `need` bytes of its model (24 bytes per depth vector, 40 per colour vector) in ONE
        allocation over the 2 P rows of both GPs, depth then colour, on the curves of the map's current batch (Sparse.rd_curves_dev).
        A row's weight is w_g n_p ny; w_depth / w_rgb = 0 means normalise: w_g = 1 / sum_p n_p ny mse0_p of that GP, summed in
        ascending leaf order, so that the objective is the sum of the two relative total errors.  Leaves the last scan did not touch
        have no error there (d0 = NaN) and stay as they are.  Both objects are pruned in place.  Returns (k_depth, k_rgb, result)."""
        import torch
        v = self.patches.view
        P = v.P
        if P == 0:
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), rate_result(np.zeros(1, dtype=RATE_RESULT_DTYPE))
        off_h = np.zeros(P + 1, dtype=np.int32)
        self.ctx._check(self.ctx.lib.gpc_dev_memcpy(self.ctx.h, _ptr(off_h), v.off, off_h.nbytes, 2))
        n_p = np.diff(off_h).astype(np.float64)
        gps = ((self.depth, v.y, float(w_depth)), (self.rgb, v.rgb, float(w_rgb)))
        ld = max(g.ld() for g, _, _ in gps)
        kmax = torch.zeros(2 * P, dtype=torch.int32, device="cuda")
        d0 = torch.full((2 * P,), float("nan"), dtype=torch.float64, device="cuda")
        d = torch.full((2 * P, ld), float("nan"), dtype=torch.float64, device="cuda")
        w = np.zeros(2 * P)
        for i, (g, y, wg) in enumerate(gps):
            removed, mse0, mse = g.rd_curves_dev(v.off, v.n_total, v.x0, v.x1, y)
            kmax[i * P:(i + 1) * P], d0[i * P:(i + 1) * P], d[i * P:(i + 1) * P, :g.ld()] = removed[:P], mse0[:P], mse[:P]
            if wg == 0.0:
                total = 0.0
                for n, e in zip(n_p, mse0[:P].cpu().numpy()):
                    if n > 0 and np.isfinite(e):
                        total += n * float(g.ny) * float(e)
                wg = 1.0 / total if total > 0.0 and np.isfinite(total) else 1.0
            w[i * P:(i + 1) * P] = wg * n_p * float(g.ny)
        d_w = torch.from_numpy(w).to("cuda")
        d_unit = torch.from_numpy(np.repeat(np.array([24, 40], dtype=np.int32), P)).to("cuda")
        d_count = torch.from_numpy(np.concatenate([self.depth.sizes(), self.rgb.sizes()])).to("cuda")
        d_k = torch.zeros(2 * P, dtype=torch.int32, device="cuda")
        d_target = torch.zeros(2 * P, dtype=torch.int32, device="cuda")
        d_res = torch.zeros(RATE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize(d_res.device)
        self.ctx.rate_allocate_dev(2 * P, ld, kmax, d0, d, int(need), w=d_w, unit=d_unit, count=d_count, k=d_k, target=d_target,
                                   result=d_res)
        self.depth.prune_dev(target=d_target[:P], score_tol=0.0)
        self.rgb.prune_dev(target=d_target[P:], score_tol=0.0)
        self.ctx.synchronize()
        k = d_k.cpu().numpy()
        return k[:P], k[P:], rate_result(d_res)

    def render(self, origin, dirs, params=None, use_cells=True, want=("leaf", "range", "local")):
        """The map as a sensor at `origin` sees it along `dirs` (Context.camera_rays, or any (n, 3) float64 device tensor): Patches.render
        on the map's current batch, depth and colour GPs; use_cells: cells a scan saw through (CELL_FREE) do not stop a ray."""
        return self.patches.render(origin, dirs, self.depth, self.rgb, self.cells if use_cells else None, params, want)

    def decode(self, use_cells=True, use_w=True, want=("leaf", "point"), device=False):
        """The map as a cloud: Patches.decode on the map's current batch, depth and colour GPs -- every trained leaf's grid points whose
        cell holds data (use_w: the batch's W) and that no scan saw through (use_cells: cells labelled CELL_FREE are dropped)."""
        return self.patches.decode(self.depth, self.rgb, self.cells if use_cells else None, use_w, want, device)

    def _occupancy_args(self):
        """What the occupancy calls share: P, m, sz of the leaf grids and the labelled batch (off, x0, x1, y, n_total, n_max)."""
        pt = self.patches
        if pt.res is None:
            raise ValueError("the map's Patches object does not know its res (create it through Context.project_cloud)")
        P, msz = pt.view.P, pt.view.m
        return P, msz, int(round(msz ** 0.5)), pt.occupancy_batch(self.cells)

    def occupancy(self, params, irls=None):
        """The occupancy layer of the map: the probit GP (dense_irls_fit_predict_dev; params: noise_model 1 or 2) trained per leaf on the
        labelled cells, evaluated on the leaf's sz x sz grid.  Returns device tensors f_star (P, m) float64 -- the latent mean, > 0
        towards occupied, 0 for a leaf without an observed cell -- and status (P,) int32."""
        import torch
        P, msz, sz, (off, x0, x1, y, n_total, n_max) = self._occupancy_args()
        f = torch.zeros((P, msz), dtype=torch.float64, device=self.cells.device)
        st = torch.full((P,), -1, dtype=torch.int32, device=self.cells.device)
        torch.cuda.synchronize(self.cells.device)
        self.ctx.dense_irls_fit_predict_dev(params, irls if irls is not None else default_params_irls(), P, off, n_max, n_total, x0, x1, y,
                                            msz, None, None, self.patches.res, sz, f, status=st)
        self.ctx.synchronize()
        return f, st

    def occupancy_probability(self, params, irls=None):
        """The occupancy layer as a probability (dense_irls_fit_predict_var_dev; params: noise_model 2): per leaf, on its sz x sz grid,
        p = P(occupied) = Phi(f / sqrt(s20 + v)) with the latent mean f and the latent predictive variance v of the probit GP trained
        on the labelled cells.  Returns device tensors p, f, v (P, m) float64 and status (P,) int32; a leaf without an observed cell
        has p = 0.5, f = 0, v = sigmaf_sq."""
        import torch
        P, msz, sz, (off, x0, x1, y, n_total, n_max) = self._occupancy_args()
        p, f, v = (torch.zeros((P, msz), dtype=torch.float64, device=self.cells.device) for _ in range(3))
        st = torch.full((P,), -1, dtype=torch.int32, device=self.cells.device)
        torch.cuda.synchronize(self.cells.device)
        self.ctx.dense_irls_fit_predict_var_dev(params, irls if irls is not None else default_params_irls(), P, off, n_max, n_total, x0, x1,
                                                y, msz, None, None, self.patches.res, sz, f, v_star=v, p_star=p, status=st)
        self.ctx.synchronize()
        return p, f, v, st

    def occupancy_select(self, params, candidates, irls=None):
        """Per-leaf hyper-parameter selection for the occupancy layer (dense_irls_select_dev on occupancy_batch; params: the base,
        noise_model 2; candidates: (sigmaf_sq, l_sq, noise) triples): per leaf the candidate of largest Laplace evidence log q(y | X, theta)
        and its read-out on the leaf's sz x sz grid.  Returns device tensors p, f, v (P, m) float64, best (P,) int32 (-1: no candidate's fit
        converged with a finite evidence; the leaf's p, f, v and log_q are then NaN), log_q (P,) float64 and status (P,) int32; a leaf
        without an observed cell has best = 0, p = 0.5, f = 0, v = candidates[0]'s sigmaf_sq and log_q = 0."""
        import torch
        P, msz, sz, (off, x0, x1, y, n_total, n_max) = self._occupancy_args()
        dev = self.cells.device
        p, f, v = (torch.zeros((P, msz), dtype=torch.float64, device=dev) for _ in range(3))
        lq = torch.zeros((P,), dtype=torch.float64, device=dev)
        best = torch.full((P,), -2, dtype=torch.int32, device=dev)
        st = torch.full((P,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.ctx.dense_irls_select_dev(params, irls if irls is not None else default_params_irls(), candidates, P, off, n_max, n_total, x0,
                                       x1, y, msz, None, None, self.patches.res, sz, f_star=f, v_star=v, p_star=p, log_q=lq, best=best,
                                       status=st)
        self.ctx.synchronize()
        return p, f, v, best, lq, st


class Comm:
    """gpc_comm: the communicator of the single all-gather (one per context).  Comm(ctx, world, rank, unique_id) creates one
    through RCCL (unique_id: the 128 bytes of Comm.unique_id() on rank 0); Comm.all(ctxs) is the one-process form."""

    def __init__(self, ctx, world=1, rank=0, unique_id=None, handle=None):
        self.ctx, self.lib = ctx, ctx.lib
        if handle is None:
            uid = unique_id if unique_id is not None else Comm.unique_id()
            buf = (C.c_char * 128).from_buffer_copy(uid)
            handle = _vp()
            ctx._check(self.lib.gpc_comm_create(ctx.h, world, rank, C.addressof(buf), C.byref(handle)))
        self.h = handle
        ctx._children.add(self)

    @staticmethod
    def unique_id():
        buf = (C.c_char * 128)()
        rc = load().gpc_comm_unique_id(C.addressof(buf))
        if rc != GPC_OK:
            raise GpcError(rc, "gpc_comm_unique_id (RCCL not found?)")
        return bytes(buf)

    @staticmethod
    def all(ctxs):
        lib = load()
        n = len(ctxs)
        hs = (_vp * n)(*[c.h for c in ctxs])
        outs = (_vp * n)()
        rc = lib.gpc_comm_create_all(n, hs, outs)
        if rc != GPC_OK:
            raise GpcError(rc, lib.gpc_last_error(ctxs[0].h).decode())
        return [Comm(ctxs[i], handle=_vp(outs[i])) for i in range(n)]

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpc_comm_destroy(self.h)
            self.h = None

    __del__ = close

    def set_partition(self, P, slots):
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        self.ctx._check(self.lib.gpc_comm_set_partition(self.h, int(P), _ptr(sl)))

    def allgather_fstar_dev(self, row_doubles, local_f, gathered, f_star=None):
        self.ctx._check(self.lib.gpc_allgather_fstar_dev(self.h, int(row_doubles), _ptr(local_f), _ptr(gathered), _ptr(f_star)))

    def unpermute_fstar_dev(self, row_doubles, gathered, f_star):
        self.ctx._check(self.lib.gpc_unpermute_fstar_dev(self.h, int(row_doubles), _ptr(gathered), _ptr(f_star)))


def partition_patches(off, world, sparse_capacity=0):
    """gpc_partition_patches: returns slot_patch (world, S) with patch ids (-1 = padding)."""
    off = np.ascontiguousarray(off, dtype=np.int32)
    P = off.shape[0] - 1
    S = (P + world - 1) // world if world > 0 else 0
    out = np.zeros(max(world * S, 1), dtype=np.int32)
    rc = load().gpc_partition_patches(P, _ptr(off), world, sparse_capacity, _ptr(out))
    if rc != GPC_OK:
        raise GpcError(rc, "gpc_partition_patches")
    return out[:world * S].reshape(world, S)


def exp_host(x, small=False):
    """the kernels' exp() evaluated on the host: table-driven (any x) or the small-argument polynomial (-2^-5 <= x <= 0)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    (load().gpc_test_exp_small_host if small else load().gpc_test_exp_host)(_ptr(x), _ptr(out), x.size)
    return out


def test_quantize_host(v, w):
    """gpc_test_quantize_host: the kernels' scalar quantiser on one array at width w -- codes (b,) uint16, range (lo, hi) float32 (2,),
    the dequantised values (b,)"""
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    q = np.zeros(v.size, dtype=np.uint16)
    rng = np.zeros(2, dtype=np.float32)
    deq = np.zeros(v.size)
    rc = load().gpc_test_quantize_host(_ptr(v), v.size, int(w), _ptr(q), _ptr(rng), _ptr(deq))
    if rc != GPC_OK:
        raise GpcError(rc, "gpc_test_quantize_host")
    return q, rng, deq


test_quantize_host.__test__ = False      # (a library call, not a pytest case)

# struct gpc_rate_result (include/gpc.h), 32 bytes
RATE_RESULT_DTYPE = np.dtype([("lambda", "<f8"), ("saved", "<i8"), ("max_saving", "<i8"), ("feasible", "<i4"), ("switched_rows", "<i4")])


def rate_result(buf):
    """a gpc_rate_result -- a RATE_RESULT_DTYPE array, or 32 bytes as a uint8 tensor / array -- as a dict, with the multiplier's bits"""
    if hasattr(buf, "cpu"):
        buf = buf.cpu().numpy()
    r = np.ascontiguousarray(buf).view(RATE_RESULT_DTYPE).ravel()[0]
    return dict(lambda_bits=int(np.array(r["lambda"]).view(np.uint64)), **{"lambda": float(r["lambda"])}, saved=int(r["saved"]),
                max_saving=int(r["max_saving"]), feasible=int(r["feasible"]), switched_rows=int(r["switched_rows"]))


def _rate_args(kmax, d0, d, w, unit, count):
    """the host arrays of a rate allocation in the types the C entries read, shapes checked"""
    kmax = np.ascontiguousarray(kmax, dtype=np.int32)
    d0 = np.ascontiguousarray(d0, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    assert d.ndim == 2 and kmax.shape == d0.shape == (d.shape[0],)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    unit = None if unit is None else np.ascontiguousarray(unit, dtype=np.int32)
    count = None if count is None else np.ascontiguousarray(count, dtype=np.int32)
    assert all(a is None or a.shape == kmax.shape for a in (w, unit, count))
    return kmax, d0, d, w, unit, count


def test_rate_allocate_host(kmax, d0, d, need, w=None, w_all=1.0, unit=None, unit_all=24, refine=True, count=None):
    """gpc_test_rate_allocate_host: Context.rate_allocate's rule from the same source on the CPU, no context and no device"""
    a = _rate_args(kmax, d0, d, w, unit, count)
    R, ld = a[2].shape
    k = np.zeros(R, dtype=np.int32)
    tg = None if count is None else np.zeros(R, dtype=np.int32)
    res = np.zeros(1, dtype=RATE_RESULT_DTYPE)
    rc = load().gpc_test_rate_allocate_host(R, ld, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), float(w_all), _ptr(a[4]), int(unit_all),
                                            int(need), int(bool(refine)), _ptr(a[5]), _ptr(k), _ptr(tg), _ptr(res))
    if rc != GPC_OK:
        raise GpcError(rc, "gpc_test_rate_allocate_host")
    return (k, rate_result(res)) if count is None else (k, tg, rate_result(res))


test_rate_allocate_host.__test__ = False


ROUTE_KINDS = {-1: "no route", 0: "nothing", 1: "one-wave", 2: "register", 3: "tiled", 4: "generic", 5: "split"}
ROUTE_SHAPE = ("w1_npad", "w1_slots", "nt", "export_factor", "waves", "npad", "per_cu", "nt17", "need_big")


def dense_route(P, n_max, n_total=None, ny=1, m=16, variance=False, pointwise=False, alpha_out=False, num_cus=256, irls=False,
                w1_refused=False):
    """gpc_test_dense_route: (kind, name, shape) the dense dispatcher chooses for a batch with these facts under the GPC_* switches of
    the environment -- the rule alone, no GPU.  n_total=None: a uniform batch (P * n_max)."""
    name = C.create_string_buffer(96)
    shape = np.zeros(len(ROUTE_SHAPE), dtype=np.int32)
    kind = load().gpc_test_dense_route(P, n_max, P * n_max if n_total is None else n_total, ny, m, int(variance), int(pointwise),
                                       int(alpha_out), num_cus, int(irls), int(w1_refused), name, len(name), _ptr(shape))
    return ROUTE_KINDS[kind], name.value.decode(), dict(zip(ROUTE_SHAPE, shape.tolist()))
