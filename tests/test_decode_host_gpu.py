"""gp_compressor::load_compressed_masked through the host class: the rows of load_compressed() that the occupancy mask W selects, on the
host-producer and on the device-producer path, by bits (the rule: tests/decode_cases.py)."""
import numpy as np
import pytest

import decode_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from gp_compressor_amd import host_api
    host_api.build()
    return host_api


@pytest.mark.parametrize("on_device", [False, True], ids=["host-producer", "device-producer"])
def test_masked_load_is_the_masked_rows(H, on_device):
    res, sz = 0.15, 10
    m = sz * sz
    xyz, rgb = H.synthetic_plane_cloud(2500, seed=1, extent=0.45)
    g = H.GpCompressor(xyz, rgb, res=res, sz=sz, model="sparse", seed=7)
    g.set_gpu_producer(on_device)
    g.set_sparse_kernel(1.0, (res / 2) ** 2, 1e-2, 25.0, 40)
    full_xyz, full_rgb, _, _ = g.roundtrip()
    P = g.L.gpc_host_patch_count(g.h)
    assert P > 4 and len(full_xyz) == P * m                   # every leaf is trained: record L m + p is point (L, p)
    W = np.zeros((P, m), dtype=np.uint8)
    g.L.gpc_host_get_mask(g.h, W.ctypes.data)
    keep = DC.kept(np.ones(P, dtype=np.int32), sz, W)
    assert 0 < keep.sum() < P * m
    mx, mc = g.load_compressed(masked=True)
    assert len(mx) == int(keep.sum()) == int(np.count_nonzero(W))
    assert np.array_equal(mx.view(np.uint32), full_xyz.reshape(P, m, 3)[keep].view(np.uint32))
    assert np.array_equal(mc, full_rgb.reshape(P, m, 3)[keep])
    # load_compressed() itself is what it was
    again_xyz, again_rgb = g.load_compressed()
    assert np.array_equal(again_xyz.view(np.uint32), full_xyz.view(np.uint32)) and np.array_equal(again_rgb, full_rgb)


def test_masked_load_refuses_what_it_does_not_cover(H):
    res, sz = 0.15, 10
    xyz, rgb = H.synthetic_plane_cloud(2500, seed=1, extent=0.45)
    d = H.GpCompressor(xyz, rgb, res=res, sz=sz, model="dense")
    with pytest.raises(RuntimeError, match="sparse model only"):
        d.load_compressed(masked=True)
    s = H.GpCompressor(xyz, rgb, res=res, sz=sz, model="sparse", seed=7)
    s.set_devices([0])
    with pytest.raises(RuntimeError, match="single-device"):
        s.load_compressed(masked=True)
