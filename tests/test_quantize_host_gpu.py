"""The bit-packed model file through the host class: gp_compressor::save_model_quantized (gpc_host_save_model_quantized) writes GPCM
version 2, load_model reads versions 1 and 2.  The file is parsed and dequantised in NumPy (tests/quantize_ref.py)."""
import os

import numpy as np
import pytest

import prune_rd_ref as rd
import prune_ref as pr
import quantize_ref as qr

pytestmark = pytest.mark.gpu
GATE_MSE = pr.GATE_FACTOR * qr.e64()


@pytest.fixture(scope="module")
def H():
    from gp_compressor_amd import host_api
    host_api.build()
    return host_api


def _leaf_mse(capi, ctx, prm, states, ny, batch, y):
    """per-leaf training error of the (alpha, BV) states through capi: set_state without C and Q, predict_points, the rule's sum (the
    helper of tests/test_prune_rd_host_gpu.py); also returns the object, still loaded"""
    P = len(states)
    g = capi.Sparse(ctx, prm, P, ny)
    ld = g.ld()
    b = np.array([a.shape[1] for a, _ in states], dtype=np.int32)
    alpha, BV = np.zeros((P, ny, ld)), np.zeros((P, ld, 2))
    for i, (a, v) in enumerate(states):
        alpha[i, :, :b[i]], BV[i, :b[i]] = a, v
    g.set_state(b, alpha, BV)
    f, _, _ = g.predict_points(batch["off"], batch["x0"], batch["x1"])
    off = batch["off"]
    out = np.full(P, np.nan)
    for i in range(P):
        s = slice(off[i], off[i + 1])
        r = y[:, s] - f[:, s]
        e = np.zeros(off[i + 1] - off[i])
        for c in range(ny):
            e = e + r[c] * r[c]
        out[i] = rd.class_sum(e) / (len(e) * ny)
    return out, g


def _make(H, xyz, rgb, res, sz, model="sparse"):
    g = H.GpCompressor(xyz, rgb, res=res, sz=sz, model=model, seed=7)
    if model == "sparse":
        # (capacity 100 and the colour field deleting as its derivation says: tests/test_prune_rd_host_gpu.py)
        g.set_sparse_kernel(1.0, (res / 4) ** 2, 1e-2, 25.0, 100)
        g.set_field_delete_bug(0)
    return g


def test_save_model_quantized(H, tmp_path):
    from gp_compressor_amd import capi
    capi.load()
    res, sz = 0.15, 10
    xyz, rgb = H.synthetic_plane_cloud(2500, seed=1, extent=0.45)
    g = _make(H, xyz, rgb, res, sz)
    full, packed, unpacked = (str(tmp_path / n) for n in ("full.gpcm", "packed.gpcm", "unpacked.gpcm"))
    batch = g.project_cloud()
    n_full = g.save_model(full)                                  # trains
    P = g.L.gpc_host_patch_count(g.h)
    assert P > 4 and n_full == os.path.getsize(full)
    v1 = qr.parse_model(open(full, "rb").read())
    assert v1["version"] == 1 and len(v1["patches"]) == P and qr.file_bytes(v1) == n_full
    prm = [capi.Params.from_buffer_copy(p) for p in v1["params"]]
    yd, yc = batch["y"][None, :], np.ascontiguousarray(batch["rgb"])
    ys = (yd, yc)
    ctx = capi.Context(0)
    raw = [[(p["gps"][k]["alpha"], p["gps"][k]["BV"]) for p in v1["patches"]] for k in range(2)]
    m0, objs = zip(*[_leaf_mse(capi, ctx, prm[k], raw[k], (1, 3)[k], batch, ys[k]) for k in range(2)])
    assert all(np.all(np.isfinite(m)) and np.all(m > 0) for m in m0)
    # one bound per GP for all leaves: 1.1 x the worst leaf's own error
    B = [1.1 * float(m.max()) for m in m0]
    n_packed = g.save_model_quantized(packed, B[0], B[1])
    assert n_packed == os.path.getsize(packed)
    v2 = qr.parse_model(open(packed, "rb").read())
    assert v2["version"] == 2 and v2["res"] == v1["res"] and v2["sz"] == v1["sz"] and v2["params"] == v1["params"] and len(v2["patches"]) == P
    # the size is the v2 byte formula over the parsed widths and counts, and smaller than the raw file
    assert n_packed == qr.file_bytes(v2) and n_packed < n_full
    widths = np.array([[gp["w"] for gp in p["gps"]] for p in v2["patches"]])
    counts = np.array([[gp["b"] for gp in p["gps"]] for p in v2["patches"]])
    coef = [sum(qr.gp_bytes(int(b), ny, int(w)) for b, w in zip(counts[:, k], widths[:, k])) for k, ny in enumerate((1, 3))]
    coef1 = [sum(qr.gp_bytes(int(b), ny, 0) for b in counts[:, k]) for k, ny in enumerate((1, 3))]
    print(f"{P} leaves: file {n_full} -> {n_packed} bytes; coefficient payload depth {coef1[0]} -> {coef[0]}, colour {coef1[1]} -> {coef[1]}; "
          f"widths depth {widths[:, 0].min()}..{widths[:, 0].max()}, colour {widths[:, 1].min()}..{widths[:, 1].max()}")
    assert np.all(widths[counts > 1] >= 1) and np.all(widths <= 16)
    for p, q in zip(v1["patches"], v2["patches"]):
        assert all(np.array_equal(p[k], q[k]) for k in ("R", "mean", "rgb_mean")) and [gp["b"] for gp in p["gps"]] == [gp["b"] for gp in q["gps"]]
    # the widths, ranges and codes of the file are those gpc_sparse_quantize_rd gives on the raw states of the v1 file
    for k in range(2):
        bits, qa, qb, rng, _, _ = objs[k].quantize_rd(batch["off"], batch["x0"], batch["x1"], ys[k], max_mse=B[k])
        for i, p in enumerate(v2["patches"]):
            gp = p["gps"][k]
            b = gp["b"]
            if gp["w"] == 0:                                       # (the writer keeps a leaf raw when its quantised form would not be smaller)
                assert bits[i] == 0 or qr.gp_bytes(b, (1, 3)[k], int(bits[i])) >= qr.gp_bytes(b, (1, 3)[k], 0)
                continue
            assert gp["w"] == bits[i] and np.array_equal(gp["q_alpha"], qa[i, :, :b]) and np.array_equal(gp["q_bv"], qb[i, :b])
            assert gp["range"].tobytes() == rng[i].tobytes()
        objs[k].close()
    # every leaf's training error, recomputed from the parsed and dequantised (BV, alpha), is within its bound
    deq = qr.to_v1(v2)
    for k in range(2):
        m1, o = _leaf_mse(capi, ctx, prm[k], [(p["gps"][k]["alpha"], p["gps"][k]["BV"]) for p in deq["patches"]], (1, 3)[k], batch, ys[k])
        o.close()
        print(f"GP {k}: worst leaf error {m0[k].max():.4e} -> {m1.max():.4e} (bound {B[k]:.4e})")
        assert np.all(m1 <= B[k] * (1 + GATE_MSE))
    ctx.close()
    # the dequantised doubles as a v1 file: load_model of both, then load_compressed, gives the same cloud bit for bit
    open(unpacked, "wb").write(qr.pack_model(deq))
    cap = P * sz * sz
    xyz2, rgb2 = H.decompress_file(packed, cap)
    xyz1, rgb1 = H.decompress_file(unpacked, cap)
    assert len(xyz2) > 0 and np.array_equal(xyz2.view(np.uint32), xyz1.view(np.uint32)) and np.array_equal(rgb2, rgb1)
    # v1 files still load, and the object was not modified by the quantised save
    xyz0, rgb0 = g.load_compressed()
    xyzf, rgbf = H.decompress_file(full, cap)
    assert np.array_equal(xyzf.view(np.uint32), xyz0.view(np.uint32)) and np.array_equal(rgbf, rgb0)
    again = str(tmp_path / "again.gpcm")
    assert g.save_model(again) == n_full and open(again, "rb").read() == open(full, "rb").read()
    # a bound nothing meets: every leaf raw, the v1 payload plus two bytes per leaf
    rawfile = str(tmp_path / "raw.gpcm")
    assert g.save_model_quantized(rawfile, 0.0, 0.0) == n_full + 2 * P
    vr = qr.parse_model(open(rawfile, "rb").read())
    assert all(gp["w"] == 0 for p in vr["patches"] for gp in p["gps"])
    xyzr, rgbr = H.decompress_file(rawfile, cap)
    assert np.array_equal(xyzr.view(np.uint32), xyz0.view(np.uint32)) and np.array_equal(rgbr, rgb0)
    # a leaf of one vector is smaller raw than as ranges plus codes: the writer keeps it raw whatever the bound accepts
    one = _make(H, xyz, rgb, res, sz)
    one.prune(1, 1)
    onefile = str(tmp_path / "one.gpcm")
    n_one = one.save_model_quantized(onefile, float("inf"), float("inf"))
    v_one = qr.parse_model(open(onefile, "rb").read())
    assert all(gp["w"] == 0 and gp["b"] == 1 for p in v_one["patches"] for gp in p["gps"]) and n_one == qr.file_bytes(v_one)
    xyz_a, rgb_a = one.load_compressed()
    xyz_b, rgb_b = H.decompress_file(onefile, cap)
    assert np.array_equal(xyz_b.view(np.uint32), xyz_a.view(np.uint32)) and np.array_equal(rgb_b, rgb_a)
    # the exceptions: the dense model, the multi-device flow, arguments the library refuses
    with pytest.raises(RuntimeError):
        _make(H, xyz, rgb, res, sz, model="dense").save_model_quantized(str(tmp_path / "x.gpcm"), B[0], B[1])
    m = _make(H, xyz, rgb, res, sz)
    m.set_devices([0])
    with pytest.raises(RuntimeError):
        m.save_model_quantized(str(tmp_path / "x.gpcm"), B[0], B[1])
    for bad in (dict(bits_min=0), dict(bits_max=17), dict(bits_min=9, bits_max=8)):
        with pytest.raises(RuntimeError):
            g.save_model_quantized(str(tmp_path / "x.gpcm"), B[0], B[1], **bad)
    with pytest.raises(RuntimeError):
        g.save_model_quantized(str(tmp_path / "x.gpcm"), float("nan"), B[1])
    with pytest.raises(RuntimeError):
        H.decompress_file(str(tmp_path / "missing.gpcm"), cap)
