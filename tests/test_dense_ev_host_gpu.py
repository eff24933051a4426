"""GPU tests of the host class's per-leaf hyper-parameter selection (gp_compressor::set_dense_candidates, host/gp_compressor.hpp) on the
C1 cloud of test_host_gpu.py with gp_model::dense: without candidates nothing changes; with depth candidates the winners are those of
capi.Context.dense_select on the same batch and the round-trip cloud is the one assembled from that call's grids.

The C1 batch (64 leaves of at most ~200 points) runs on the register kernel, whose alpha repeats to a rounding or two run to run
(tests/test_dense_gpu.py::test_dense_golden): two clouds of the same computation are compared to two float32 roundings of the
coordinates' scale and one grey level, not to the bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES, SZ = 0.15, 20
# gaussian_process.h's defaults, the same amplitude and noise at a length scale of a third of the leaf, and a unit-amplitude model
CANDS = [(0.05 ** 2, 3.0 ** 2, 0.04 ** 2), (0.05 ** 2, 0.05 ** 2, 0.04 ** 2), (1.0, 0.5 ** 2, 1e-4)]


@pytest.fixture(scope="module")
def H():
    from gp_compressor_amd import host_api
    host_api.load()
    return host_api


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _compressor(H):
    xyz, rgb = H.synthetic_plane_cloud(10000, seed=1)
    return H.GpCompressor(xyz, rgb, res=RES, sz=SZ, model="dense", seed=7)


def _same_cloud(a, b):
    (xa, ca), (xb, cb) = a, b
    assert xa.shape == xb.shape and ca.shape == cb.shape
    scale = float(np.max(np.abs(xb)))
    assert float(np.max(np.abs(xa.astype(np.float64) - xb.astype(np.float64)))) <= 2 * 2.0 ** -23 * scale
    assert int(np.max(np.abs(ca.astype(np.int32) - cb.astype(np.int32)))) <= 1


def test_without_candidates_nothing_changes(H):
    """No candidates, or two empty lists: the call of test_compress_roundtrip_c1[dense], no per-leaf results."""
    g0 = _compressor(H)
    a = g0.roundtrip()
    g1 = _compressor(H)
    g1.set_dense_candidates([], [])
    b = g1.roundtrip()
    _same_cloud(a[:2], b[:2])
    assert a[2:] == b[2:]
    for g in (g0, g1):
        # the last dense call was the colour plane's plain grid entry (64 leaves of at most 256 points, three planes: the register
        # kernel without the export), not the select's evidence route
        assert g.last_dense_kernel() in ("dense_mfma_nt12", "dense_mfma_nt16"), g.last_dense_kernel()
        assert len(g.dense_best_depth()) == 0 and len(g.dense_best_rgb()) == 0 and len(g.dense_evidence_depth()) == 0


def test_depth_candidates_are_dense_select_on_the_batch(H, gp):
    """Three depth candidates: dense_best_depth() and dense_evidence_depth() are capi.Context.dense_select's on the fetched batch, and the
    cloud is the reprojection of that call's depth grids with the colour grids of the plain entry."""
    capi, ctx = gp
    g = _compressor(H)
    g.set_dense_candidates(CANDS, [])
    oxyz, orgb, _, _ = g.roundtrip()
    batch = g.project_cloud(device=True)
    off = batch["off"]
    P, m = len(off) - 1, SZ * SZ
    best = g.dense_best_depth()
    assert best.shape == (P,) and len(g.dense_best_rgb()) == 0
    assert g.last_dense_kernel() in ("dense_mfma_nt12", "dense_mfma_nt16")     # the colour plane had no candidates: the plain entry
    prm = capi.default_params_dense()
    sel = ctx.dense_select(prm, CANDS, off, batch["x0"], batch["x1"], batch["y"][None, :], res=RES, sz=SZ, want_v=False)
    s = np.sort(sel["log_ev_all"][:, :, 0], axis=0)
    print("winners %s, smallest margin %.3f" % (np.bincount(best, minlength=3).tolist(), float(np.min(s[-1] - s[-2]))))
    assert np.min(s[-1] - s[-2]) > 1e-6          # no leaf is a near-tie that a rounding could turn
    assert np.array_equal(best, sel["best"]) and np.all(best >= 0)
    ev = g.dense_evidence_depth()
    assert np.all(np.abs(ev - sel["log_ev"][:, 0]) <= 1e-10 * (1.0 + np.abs(ev)))        # two calls on the register kernel
    c, st = ctx.dense_fit_predict_grid(prm, off, batch["x0"], batch["x1"], batch["rgb"], RES, SZ)
    assert np.all(st == 0)
    g0 = RES * ((np.arange(SZ) + 0.5) / SZ - 0.5)
    xs0, xs1 = np.tile(g0, SZ), np.repeat(g0, SZ)
    R9 = np.ascontiguousarray(batch["R"].transpose(0, 2, 1)).reshape(P, 9)
    cloud = ctx.reproject(xs0, xs1, np.ascontiguousarray(sel["f_star"][:, 0, :]), R9, batch["mean"], c, batch["rgb_mean"],
                          np.diff(off).astype(np.int32))
    assert len(cloud) == len(oxyz) == P * m
    _same_cloud((oxyz, orgb), (np.stack([cloud["x"], cloud["y"], cloud["z"]], 1), np.stack([cloud["r"], cloud["g"], cloud["b"]], 1)))


def test_rgb_candidates_and_the_sharded_refusal(H):
    """Colour candidates decide by the sum over the three channels and leave the depth plane alone; candidates together with
    set_devices throw in either order and say why."""
    g = _compressor(H)
    g.set_dense_candidates([], CANDS[:2])
    oxyz, orgb, _, _ = g.roundtrip()
    assert len(g.dense_best_depth()) == 0 and len(g.dense_evidence_depth()) == 0
    assert g.last_dense_kernel().endswith("+ dense_gauss_evidence"), g.last_dense_kernel()
    b = g.dense_best_rgb()
    assert b.shape == (64,) and np.all((b >= 0) & (b < 2)) and len(oxyz) == 64 * SZ * SZ
    with pytest.raises(RuntimeError, match="candidates"):
        g.set_devices([0])
    g2 = _compressor(H)
    g2.set_devices([0])
    with pytest.raises(RuntimeError, match="set_devices"):
        g2.set_dense_candidates(CANDS, [])
    g2.set_devices([])
    g2.set_dense_candidates(CANDS, [])
