"""Rate control through the upper layers: gp_compressor::prune with the model file (host class, gpc_host_prune) and Mapping.prune."""
import os

import numpy as np
import pytest

from gp_compressor_amd import synth
import mapping_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from gp_compressor_amd import host_api
    host_api.build()
    return host_api


def test_prune_shrinks_the_model_file_by_its_vectors(H, tmp_path):
    """Small planar cloud: save_model before and after prune differ by exactly 24 bytes per depth vector and 40 per colour vector
    removed; load_model of the pruned file reconstructs the cloud of the pruned in-memory object bit for bit."""
    res, sz = 0.15, 10
    xyz, rgb = H.synthetic_plane_cloud(2500, seed=1, extent=0.45)
    g = H.GpCompressor(xyz, rgb, res=res, sz=sz, model="sparse", seed=7)
    g.set_sparse_kernel(1.0, (res / 4) ** 2, 1e-2, 25.0, 40)
    full, pruned = str(tmp_path / "full.gpcm"), str(tmp_path / "pruned.gpcm")
    n_full = g.save_model(full)                                  # trains
    P = g.L.gpc_host_patch_count(g.h)
    assert P > 4 and n_full == os.path.getsize(full)
    xyz0, rgb0 = g.load_compressed()
    # (the colour GP keeps the reference's field deletion, which multiplies where the derivation divides -- ref_field_delete_bug, the
    # host class's default: a couple of removals per patch stay finite, a long chain diverges as it does while training)
    rd, rc = g.prune(10, 38)
    assert rd > 0 and rc > 0
    n_pruned = g.save_model(pruned)
    assert n_full - n_pruned == 24 * rd + 40 * rc
    xyz1, rgb1 = g.load_compressed()
    xyz2, rgb2 = H.decompress_file(pruned, P * sz * sz)
    assert len(xyz1) == len(xyz0) > 0
    assert np.array_equal(xyz2.view(np.uint32), xyz1.view(np.uint32)) and np.array_equal(rgb2, rgb1)
    # the pruned model is another model (fewer vectors), close to the full one on this smooth surface
    assert not np.array_equal(xyz1.view(np.uint32), xyz0.view(np.uint32))
    assert np.max(np.abs(xyz1 - xyz0)) < 0.02
    # a second prune to the same counts removes nothing; the score branch alone takes every depth GP to one vector
    assert g.prune(10, 38) == (0, 0)
    rd2, rc2 = g.prune(10, 38, float("inf"), 0.0)
    assert n_pruned - g.save_model(pruned) == 24 * rd2 and 0 < rd2 <= (10 - 1) * P and rc2 == 0
    # what prune does not cover throws, as save_model does
    d = H.GpCompressor(xyz, rgb, res=res, sz=sz, model="dense")
    with pytest.raises(RuntimeError):
        d.prune(10, 38)
    with pytest.raises(RuntimeError):
        g.prune(0, 38)


def test_mapping_prune_then_grow_and_render():
    """Mapping.prune bounds the map's two objects in place; the Registration object sees the pruned state: add_cloud registers against
    it, inserts and trains, and the basis counts stay within the capacity; render runs on the result."""
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    RES, SZ = mc.RES, mc.SZ
    kw_d = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1e-3, capacity=24)
    # (the colour field deletes as its derivation says, ref_field_delete_bug = 0: with the reference's multiply a chain of 80 removals
    # diverges, as the field recursion of these colours does through its own deletions at a small capacity, and the registration that
    # follows would read NaN likelihoods)
    kw_c = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1.0, capacity=100, ref_field_delete_bug=0)
    xyz, rgb = mc.model_cloud()
    pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), RES, SZ)
    b = pt.fetch()
    P = pt.view.P
    perm = synth.sattolo_perms(b["off"], seed=6)
    gd = capi.Sparse(ctx, capi.default_params_sparse(1, **kw_d), P, 1)
    gc = capi.Sparse(ctx, capi.default_params_sparse(3, **kw_c), P, 3)
    assert np.all(gd.add(b["off"], b["x0"], b["x1"], b["y"][None, :], perm) == 0)
    assert np.all(gc.add(b["off"], b["x0"], b["x1"], np.ascontiguousarray(b["rgb"]), perm) == 0)
    bd0, bc0 = gd.sizes(), gc.sizes()
    prm = capi.default_params_registration(step=1e-7, tol=1e300, min_steps=2, max_steps=10)
    mp = capi.Mapping(ctx, pt, gd, gc, params=prm, min_nbr=20)
    mp.prune(12, 20)
    assert np.array_equal(mp.depth.sizes(), np.minimum(bd0, 12)) and np.array_equal(mp.rgb.sizes(), np.minimum(bc0, 20))
    assert np.any(bd0 > 12) and np.any(bc0 > 20)
    S, cs = mc.overlapping_scan()
    steps, inserted = mp.add_cloud(ctx.make_cloud(S, cs))
    assert inserted and mp.depth.P == mp.rgb.P == mp.patches.view.P > P
    bd, bc = mp.depth.sizes(), mp.rgb.sizes()
    assert np.all(bd <= 24) and np.all(bc <= 100) and np.any(bd > 12)      # the leaves the scan reached grew again, within capacity
    look_down = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])
    dirs = ctx.camera_rays(look_down, 14.0, 14.0, 11.0, 8.0, 23, 17)
    out = mp.render(np.array([0.4, 0.4, 1.0]), dirs)
    counts = out["counts"]
    assert counts[0] == 23 * 17 and counts[1] > 0
    mp.close()
    ctx.close()
