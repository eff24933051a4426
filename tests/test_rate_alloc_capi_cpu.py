"""The three rate-allocation entries at the C-ABI, without a GPU: include/gpc.h declares them, the library exports them, the Python
prototypes follow the declarations parameter by parameter, a NULL context is refused before anything touches a device, and the Python
and C++ layers expose the feature."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gpc_rate_allocate", "gpc_rate_allocate_dev", "gpc_test_rate_allocate_host")


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
    ctype = {"int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}
    for name in ENTRIES:
        assert hasattr(lib, name), name
        res, args = capi.PROTOTYPES[name]
        want = [ctype.get(t, C.c_void_p) for t in _declared(name)]
        assert res is C.c_int and len(args) == len(want), (name, len(args), len(want))
        assert all(a is w for a, w in zip(args, want)), (name, args, want)
    host, dev, twin = (_declared(n) for n in ENTRIES)
    assert host == dev and twin == host[1:]                                   # the twin takes no context
    assert host == ["gpc_ctx*", "int", "int", "constint32_t*", "constdouble*", "constdouble*", "constdouble*", "double", "constint32_t*",
                    "int", "int64_t", "int", "constint32_t*", "int32_t*", "int32_t*", "gpc_rate_result*"]


def test_result_record_layout(capi):
    hdr = open(os.path.join(ROOT, "include", "gpc.h")).read()
    m = re.search(r"typedef struct gpc_rate_result \{(.*?)\} gpc_rate_result;", hdr, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "double lambda; int64_t saved, max_saving; int32_t feasible, switched_rows;"
    dt = capi.RATE_RESULT_DTYPE
    assert dt.itemsize == 32 and dt.names == ("lambda", "saved", "max_saving", "feasible", "switched_rows")
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 24, 28]


def test_null_context_is_refused(capi):
    L = capi.load()
    for name in ENTRIES[:2]:
        assert getattr(L, name)(None, 0, 1, None, None, None, None, 1.0, None, 24, 0, 1, None, None, None, None) == capi.GPC_EINVAL


def test_python_layers_expose_the_feature(capi):
    from gp_compressor_amd import host_api
    for cls, names in ((capi.Context, ("rate_allocate", "rate_allocate_dev")), (capi.Sparse, ("prune_to_bytes", "rd_curves_dev")),
                       (capi.Mapping, ("prune_to_bytes",)), (host_api.GpCompressor, ("prune_to_bytes", "model_bytes"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert callable(capi.test_rate_allocate_host) and callable(capi.rate_result)
    src = open(os.path.join(ROOT, "gp_compressor_amd", "host", "gp_compressor.hpp")).read()
    assert re.search(r"size_t model_bytes\(\) const;", src)
    assert re.search(r"prune_to_bytes\(size_t budget_bytes, double w_depth = 0, double w_rgb = 0\)", src)
    assert "gpc_host_prune_to_bytes" in open(os.path.join(ROOT, "gp_compressor_amd", "host", "gp_compressor.cpp")).read()


def test_switch_is_read_by_the_allocator_only():
    src = open(os.path.join(ROOT, "gp_compressor_amd", "csrc", "rate_alloc.hip")).read()
    assert src.count('getenv("GPC_ALLOC_BLOCKS")') == 1                        # once per call, before the launches
