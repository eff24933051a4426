"""Distortion-bounded rate control through the host class: gp_compressor::prune_to_error (gpc_host_prune_to_error) with the model file."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import prune_rd_ref as rd
import prune_ref as pr

pytestmark = pytest.mark.gpu
GATE_MSE = pr.GATE_FACTOR * rd.E64_MSE


@pytest.fixture(scope="module")
def H():
    from gp_compressor_amd import host_api
    host_api.build()
    return host_api


def _read_model(path, capi):
    """the GPCM v1 file (gp_compressor::save_model): params of the two GPs and per patch (BV, alpha) of each"""
    raw = open(path, "rb").read()
    assert raw[:4] == b"GPCM"
    version, = struct.unpack_from("<I", raw, 4)
    res, sz, P, psz = struct.unpack_from("<diiI", raw, 8)
    assert version == 1 and psz == C.sizeof(capi.Params)
    pos = 8 + 8 + 4 + 4 + 4
    prm = []
    for _ in range(2):
        prm.append(capi.Params.from_buffer_copy(raw[pos:pos + psz]))
        pos += psz
    leaves = []
    for _ in range(P):
        pos += 15 * 8
        bd, bc = struct.unpack_from("<ii", raw, pos)
        pos += 8
        take = lambda k: np.frombuffer(raw, dtype="<f8", count=k, offset=pos).copy()
        bvd = take(2 * bd).reshape(bd, 2); pos += 16 * bd
        ad = take(bd).reshape(1, bd); pos += 8 * bd
        bvc = take(2 * bc).reshape(bc, 2); pos += 16 * bc
        ac = take(3 * bc).reshape(3, bc); pos += 24 * bc
        leaves.append(((ad, bvd), (ac, bvc)))
    assert pos == len(raw)
    return prm, leaves


def _leaf_mse(capi, ctx, prm, states, ny, batch, y):
    """per-leaf training error of the (BV, alpha) states through capi: set_state without C and Q, predict_points, the rule's sum"""
    P = len(states)
    g = capi.Sparse(ctx, prm, P, ny)
    ld = g.ld()
    b = np.array([a.shape[1] for a, _ in states], dtype=np.int32)
    alpha, BV = np.zeros((P, ny, ld)), np.zeros((P, ld, 2))
    for i, (a, v) in enumerate(states):
        alpha[i, :, :b[i]], BV[i, :b[i]] = a, v
    g.set_state(b, alpha, BV)
    f, _, _ = g.predict_points(batch["off"], batch["x0"], batch["x1"])
    g.close()
    off = batch["off"]
    out = np.full(P, np.nan)
    for i in range(P):
        s = slice(off[i], off[i + 1])
        r = y[:, s] - f[:, s]
        e = np.zeros(off[i + 1] - off[i])
        for c in range(ny):
            e = e + r[c] * r[c]
        out[i] = rd.class_sum(e) / (len(e) * ny)
    return out, b


def test_prune_to_error_shrinks_the_model_file_within_the_bound(H, tmp_path):
    """The synthetic plane cloud of tests/test_prune_host_gpu.py: the file shrinks by exactly 24 bytes per depth vector and 40 per colour
    vector removed, load_model + load_compressed works on it, and every leaf's training error, recomputed from the file's (BV, alpha)
    through capi, stays within the bound."""
    from gp_compressor_amd import capi
    capi.load()
    res, sz = 0.15, 10
    xyz, rgb = H.synthetic_plane_cloud(2500, seed=1, extent=0.45)
    g = H.GpCompressor(xyz, rgb, res=res, sz=sz, model="sparse", seed=7)
    # (capacity 100 and the colour field deleting as its derivation says: with the host class's defaults -- the reference's field deletion,
    # ref_field_delete_bug, at capacity 40 -- the colour field of this cloud diverges while it trains, no leaf has a finite colour error and
    # nothing of the colour half could be seen)
    g.set_sparse_kernel(1.0, (res / 4) ** 2, 1e-2, 25.0, 100)
    g.set_field_delete_bug(0)
    full, pruned = str(tmp_path / "full.gpcm"), str(tmp_path / "pruned.gpcm")
    batch = g.project_cloud()                                    # the batch save_model trains on
    n_full = g.save_model(full)                                  # trains
    P = g.L.gpc_host_patch_count(g.h)
    assert P > 4 and P == len(batch["off"]) - 1 and n_full == os.path.getsize(full)
    yd, yc = batch["y"][None, :], np.ascontiguousarray(batch["rgb"])
    ctx = capi.Context(0)
    prm, leaves = _read_model(full, capi)
    m0d, bd0 = _leaf_mse(capi, ctx, prm[0], [l[0] for l in leaves], 1, batch, yd)
    m0c, bc0 = _leaf_mse(capi, ctx, prm[1], [l[1] for l in leaves], 3, batch, yc)
    # one bound per GP for all leaves: twice the worst leaf's own error, so every leaf has room and most shed a good part of their basis
    assert np.all(np.isfinite(m0d)) and np.all(np.isfinite(m0c)) and np.all(m0d > 0) and np.all(m0c > 0)
    Bd, Bc = 2.0 * float(m0d.max()), 2.0 * float(m0c.max())
    rdp, rcp = g.prune_to_error(Bd, Bc)
    assert rdp > 0 and rcp > 0
    n_pruned = g.save_model(pruned)
    assert n_full - n_pruned == 24 * rdp + 40 * rcp and n_pruned == os.path.getsize(pruned)
    prm1, leaves1 = _read_model(pruned, capi)
    m1d, bd1 = _leaf_mse(capi, ctx, prm1[0], [l[0] for l in leaves1], 1, batch, yd)
    m1c, bc1 = _leaf_mse(capi, ctx, prm1[1], [l[1] for l in leaves1], 3, batch, yc)
    ctx.close()
    assert int(np.sum(bd0 - bd1)) == rdp and int(np.sum(bc0 - bc1)) == rcp and np.all(bd1 >= 1) and np.all(bc1 >= 1)
    print(f"{P} leaves: depth {bd0.sum()} -> {bd1.sum()} vectors, worst error {m0d.max():.3e} -> {m1d.max():.3e} (bound {Bd:.3e}); "
          f"colour {bc0.sum()} -> {bc1.sum()}, {m0c.max():.3e} -> {m1c.max():.3e} (bound {Bc:.3e})")
    assert np.all(m1d <= Bd * (1 + GATE_MSE)) and np.all(m1c <= Bc * (1 + GATE_MSE))
    # the two halves take their own bound and their own floor: a zero bound on one side leaves that side alone
    g2 = H.GpCompressor(xyz, rgb, res=res, sz=sz, model="sparse", seed=7)
    g2.set_sparse_kernel(1.0, (res / 4) ** 2, 1e-2, 25.0, 100)
    g2.set_field_delete_bug(0)
    r_d, r_c = g2.prune_to_error(Bd, 0.0)
    assert r_d == rdp and r_c == 0
    r_d, r_c = g2.prune_to_error(0.0, Bc, 1, int(bc1.max()))
    assert r_d == 0 and r_c == int(np.sum(np.maximum(bc0 - int(bc1.max()), 0))) and r_c <= rcp      # the floor holds per leaf
    # the smaller file is a model: load_model, then load_compressed, gives the cloud of the pruned in-memory object bit for bit
    xyz1, rgb1 = g.load_compressed()
    xyz2, rgb2 = H.decompress_file(pruned, P * sz * sz)
    assert len(xyz1) > 0 and np.array_equal(xyz2.view(np.uint32), xyz1.view(np.uint32)) and np.array_equal(rgb2, rgb1)
    # a second call with the same bounds and a floor at the counts reached removes nothing; the preconditions of prune() hold here too
    assert g.prune_to_error(Bd, Bc, int(bd1.max()), int(bc1.max())) == (0, 0)
    d = H.GpCompressor(xyz, rgb, res=res, sz=sz, model="dense")
    with pytest.raises(RuntimeError):
        d.prune_to_error(Bd, Bc)
    with pytest.raises(RuntimeError):
        g.prune_to_error(Bd, Bc, 0, 1)
    with pytest.raises(RuntimeError):
        g.prune_to_error(float("nan"), Bc)
