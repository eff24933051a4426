"""The two distortion-bounded prune entries at the C-ABI, without a GPU: include/gpc.h declares them, the library exports them, the
Python prototypes follow the declarations parameter by parameter, and a NULL object is refused before anything touches a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gpc_sparse_prune_rd", "gpc_sparse_prune_rd_dev")


@pytest.fixture(scope="module")
def capi():
    from gp_compressor_amd import build, capi as m
    build.build()
    m.load()
    return m


def _declared(name):
    """the parameter types of `name` as include/gpc.h declares it"""
    hdr = open(os.path.join(ROOT, "include", "gpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p.strip()).replace(" ", "") for p in m.group(1).split(",")]


def test_entries_are_declared_exported_and_bound(capi):
    lib = C.CDLL(capi.LIB_PATH)
    ctype = {"int": C.c_int, "double": C.c_double}
    for name in ENTRIES:
        assert hasattr(lib, name), name
        res, args = capi.PROTOTYPES[name]
        want = [ctype.get(t, C.c_void_p) for t in _declared(name)]
        assert res is C.c_int and len(args) == len(want), (name, len(args), len(want))
        assert all(a is w for a, w in zip(args, want)), (name, args, want)
    host, dev = _declared(ENTRIES[0]), _declared(ENTRIES[1])
    assert len(host) == 16 and dev == host[:2] + ["int"] + host[2:]           # the _dev form adds n_total after off
    assert host == ["gpc_sparse*", "constint32_t*", "constdouble*", "constdouble*", "constdouble*", "int", "constint32_t*", "double",
                    "constdouble*", "int32_t*", "int32_t*", "double*", "double*", "double*", "double*", "int32_t*"]


def test_null_object_is_refused(capi):
    L = capi.load()
    assert L.gpc_sparse_prune_rd(None, None, None, None, None, 1, None, 1.0, None, *[None] * 7) == capi.GPC_EINVAL
    assert L.gpc_sparse_prune_rd_dev(None, None, 0, None, None, None, 1, None, 1.0, None, *[None] * 7) == capi.GPC_EINVAL


def test_python_layers_expose_the_feature(capi):
    from gp_compressor_amd import host_api
    for cls, names in ((capi.Sparse, ("prune_rd", "prune_rd_dev")), (capi.Mapping, ("prune_to_error",)),
                       (host_api.GpCompressor, ("prune_to_error",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    src = open(os.path.join(ROOT, "gp_compressor_amd", "host", "gp_compressor.hpp")).read()
    assert re.search(r"prune_to_error\(double max_mse_depth, double max_mse_rgb, int keep_depth = 1, int keep_rgb = 1\)", src)
