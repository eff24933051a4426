"""gp_compressor::distortion through the host class, and Context.cloud_psnr, against the NumPy restatement run on the same two clouds
(tests/distortion_ref.py), by bits: the plane cloud of tests/test_decode_host_gpu.py."""
import math

import numpy as np
import pytest

import distortion_ref as DR

pytestmark = pytest.mark.gpu

RES, SZ, PEAK = 0.15, 10, 0.45


@pytest.fixture(scope="module")
def trained():
    from gp_compressor_amd import capi, host_api
    host_api.build()
    xyz, rgb = host_api.synthetic_plane_cloud(2500, seed=1, extent=0.45)
    g = host_api.GpCompressor(xyz, rgb, res=RES, sz=SZ, model="sparse", seed=7)
    g.set_sparse_kernel(1.0, (RES / 2) ** 2, 1e-2, 25.0, 40)
    g.set_field_delete_bug(False)
    dxyz, drgb, _, _ = g.roundtrip()
    ctx = capi.Context(0)
    yield capi, ctx, g, (xyz, rgb), (dxyz, drgb)
    ctx.close()


def _same_report(got, want):
    for k in DR.METRICS:
        assert DR.same_bits(np.array(got[k]["mse"], dtype=np.float64), np.array(want[k]["mse"], dtype=np.float64)), (k, got[k], want[k])
        assert DR.same_bits(np.array(got[k]["psnr"], dtype=np.float64), np.array(want[k]["psnr"], dtype=np.float64)), (k, got[k], want[k])


def test_host_class_and_binding_agree_with_the_restatement(trained):
    capi, ctx, g, (xyz, rgb), (dxyz, drgb) = trained
    orig, dec = ctx.make_cloud(xyz, rgb), ctx.make_cloud(dxyz, drgb)
    pt = ctx.project_cloud(orig, RES, SZ)
    normals = pt.normals(len(orig))
    assert DR.same_bits(normals, DR.patches_normals(pt.fetch(), len(orig)))
    pt.close()
    want = DR.cloud_psnr(dec, orig, PEAK, normals_b=normals)           # a = decoded, b = original
    print({k: want[k] for k in DR.METRICS})
    host = g.distortion(dxyz, drgb, PEAK)
    _same_report(host, want)
    for j, r in enumerate((want["ab"], want["ba"])):
        assert [host[k][j] for k in ("n_valid", "n_matched", "n_plane")] == [r[k] for k in ("n_valid", "n_matched", "n_plane")]
    bound = ctx.cloud_psnr(dec, orig, PEAK, normals_b=normals)
    _same_report(bound, want)
    DR.assert_same(bound["ab"], want["ab"], DR.RESULT_KEYS)
    DR.assert_same(bound["ba"], want["ba"], DR.RESULT_KEYS)
    assert math.isnan(want["d2"]["mse"][1]) and want["d2"]["mse"][0] > 0 and 20.0 < want["d1"]["psnr"] < 120.0


def test_a_cloud_against_itself(trained):
    _, ctx, g, (xyz, rgb), _ = trained
    own = g.distortion(xyz, rgb, PEAK)
    for k in ("d1", "d2", "r", "g", "b", "luma"):
        assert own[k]["mse"][0] == 0.0 and own[k]["psnr"] == float("inf"), (k, own[k])
    cloud = ctx.make_cloud(xyz, rgb)
    both = ctx.cloud_psnr(cloud, cloud, PEAK)
    assert both["d1"]["mse"] == (0.0, 0.0) and both["d1"]["psnr"] == float("inf") and math.isnan(both["d2"]["psnr"])


def test_pruning_to_one_vector_does_not_lower_d1(trained):
    _, _, g, _, (dxyz, drgb) = trained
    before = g.distortion(dxyz, drgb, PEAK)
    assert sum(g.prune(1, 1)) > 0
    pxyz, prgb = g.load_compressed()
    after = g.distortion(pxyz, prgb, PEAK)
    print("d1 mse before", before["d1"]["mse"], "after", after["d1"]["mse"])
    assert max(after["d1"]["mse"]) >= max(before["d1"]["mse"]) and after["d1"]["psnr"] <= before["d1"]["psnr"]
