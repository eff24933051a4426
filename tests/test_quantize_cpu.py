"""The quantise rule on the CPU (tests/quantize_ref.py): the library's scalar quantiser against the restatement bit for bit, the conditions
the GPU cases of tests/test_quantize_gpu.py rest on, the float64 against the longdouble evaluation of the quantised error, and the GPCM v2
packer / parser pair.

Measured here (oracle-trained states of prune_ref.REGIMES, ny = 1 and 3, every patch):
  widths chosen at B = 1.1 mse0: depth 9..13 bits, colour 3..6; at B = 2 mse0: depth 7..11, colour 3..4 (bits_min = 1);
  smallest relative distance of an evaluated error to its bound 3.0e-04 (capacity 40, ny = 1, B = 1.1 mse0): no patch within
  prune_rd_ref.BAND;
  float64 against longdouble on the same dequantised bits: 2.54e-14 (capacity 16, ny = 1; ny = 3 stays below 9e-16), far within
  prune_rd_ref.E64_MSE = 7.84e-11, so quantize_ref.E64_MSE_Q stays None and the GPU gates use E64_MSE.
"""
import os
import re

import numpy as np
import pytest

import prune_rd_ref as rd
import prune_ref as pr
import quantize_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = (1.1, 2.0)


@pytest.fixture(scope="module")
def capi():
    from gp_compressor_amd import build, capi as m
    build.build()
    m.load()
    return m


@pytest.fixture(scope="module")
def runs(oracle):
    """(cap, ny, factor) -> the restatement's run of every patch of the regime at B = factor x mse0"""
    out = {}
    for cap, div, n, P, ny in rd.regimes():
        states = pr.oracle_states(oracle, cap, div, n, P, ny)
        pts = rd.points(cap, n, P, ny)[4]
        kw = pr.kernel_kw(cap, div, ny)
        for f in BOUNDS:
            out[(cap, ny, f)] = [(qr.quantize_rd(st[0], st[3], x0, x1, y, lambda m, f=f: f * m, kw), (x0, x1, y), kw)
                                 for st, (x0, x1, y) in zip(states, pts)]
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _host_inputs():
    rng = np.random.default_rng(7)
    cases = [("random b=%d" % b, rng.normal(size=b) * 10.0 ** rng.integers(-3, 3)) for b in (2, 3, 17, 100, 131)]
    cases.append(("uniform", rng.uniform(-0.075, 0.075, 64)))
    cases.append(("b=1", np.array([0.3])))
    cases.append(("b=1 float", np.array([0.25])))
    cases.append(("equal, a float", np.full(9, 1.5)))
    cases.append(("equal, zero", np.zeros(4)))
    cases.append(("equal, not a float", np.full(9, 0.1)))
    cases.append(("tiny", np.array([1e-300, -1e-300, 0.0, 5e-301])))
    cases.append(("tiny positive", np.array([1e-300, 2e-300])))
    cases.append(("huge", np.array([1e30, -1e30, 3.3e29, -7.7e28, 0.0])))
    cases.append(("mixed", np.array([1e30, -1e-300, 1.0, -1.0])))
    cases.append(("halves", np.array([0.0, 0.5, 1.5, 2.5, 3.0])))          # (v - lo) / step lands on .5 at w = 2: round-half-even
    return cases


def test_quantize_host_is_the_restatement(capi):
    for name, v in _host_inputs():
        for w in range(1, 17):
            q, rng_, deq = capi.test_quantize_host(v, w)
            rq, rr, rv = qr.quantize_array(v, w)
            assert _same_bits(q, rq), (name, w, q, rq)
            assert _same_bits(rng_, rr), (name, w, rng_, rr)
            assert _same_bits(deq, rv), (name, w, deq, rv)
            assert float(rng_[0]) <= v.min() and float(rng_[1]) >= v.max()
            assert np.all(q <= (1 << w) - 1)
    # the range is the tightest float interval; a step of zero gives code 0 and the value itself
    q, r, d = capi.test_quantize_host(np.full(9, 1.5), 5)
    assert np.all(q == 0) and r[0] == r[1] == np.float32(1.5) and np.all(d == 1.5)
    q, r, d = capi.test_quantize_host(np.full(9, 0.1), 5)
    assert float(r[0]) < 0.1 < float(r[1]) and r[1] == np.nextafter(r[0], np.float32(1)) and len(set(q.tolist())) == 1
    q, r, d = capi.test_quantize_host(np.array([0.0, 0.5, 1.5, 2.5, 3.0]), 2)
    assert list(q) == [0, 0, 2, 2, 3]
    # the error of a value is at most half a step (+ the rounding of the arithmetic)
    v = np.random.default_rng(1).normal(size=200)
    for w in (1, 4, 8, 12, 16):
        q, r, d = capi.test_quantize_host(v, w)
        step = (float(r[1]) - float(r[0])) / ((1 << w) - 1)
        assert np.max(np.abs(d - v)) <= 0.5 * step * (1 + 1e-12)
    L = capi.load()
    for b, w in ((0, 4), (3, 0), (3, 17)):
        assert L.gpc_test_quantize_host(v.ctypes.data, b, w, None, None, None) == capi.GPC_EINVAL
    assert L.gpc_test_quantize_host(None, 3, 4, None, None, None) == capi.GPC_EINVAL


def test_gpu_case_conditions(runs):
    """what tests/test_quantize_gpu.py assumes: at most 5 % of a case's patches within BAND of their bound, a width found everywhere"""
    smallest = np.inf
    for (cap, ny, f), rs in runs.items():
        bits = [r["bits"] for r, _, _ in rs]
        band = [r["band"] for r, _, _ in rs]
        near = sum(b_ <= rd.BAND for b_ in band)
        smallest = min(smallest, min(band))
        print(f"cap {cap} ny {ny} B = {f} mse0: widths {min(bits)}..{max(bits)}, smallest band {min(band):.2e}, within BAND {near}/{len(rs)}")
        assert near <= 0.05 * len(rs)
        assert all(not r["escaped"] and 1 <= r["bits"] <= 16 and r["mse_q"] <= r["bound"] for r, _, _ in rs)
        for r, _, _ in rs:
            w = r["bits"]
            assert np.all(np.isnan(r["curve"][w:])) and not np.any(np.isnan(r["curve"][:w])) and np.all(r["curve"][:w - 1] > r["bound"])
    print(f"smallest relative distance of an evaluated error to its bound: {smallest:.2e}")


def test_e64_mse_q(runs):
    """float64 against longdouble evaluation of the error of the same dequantised bits, every evaluated width"""
    worst = 0.0
    for (cap, ny, f), rs in runs.items():
        w_case = 0.0
        for r, (x0, x1, y), kw in rs:
            for w, (a2, v2) in r["states"].items():
                eld = rd.mse_of(a2, v2, x0, x1, y, kw["sigmaf_sq"], kw["l_sq"], np.longdouble)
                w_case = max(w_case, rd.rel(r["curve"][w - 1], eld))
        print(f"cap {cap} ny {ny} B = {f} mse0: float64 vs longdouble {w_case:.3e}")
        worst = max(worst, w_case)
    print(f"E64_MSE_Q measured: {worst:.3e} (gate figure {qr.e64():.3e})")
    assert worst <= qr.e64()


def test_rule_edges():
    rng = np.random.default_rng(2)
    b, n = 7, 50
    alpha, BV = rng.normal(size=(3, b)), rng.uniform(-0.07, 0.07, size=(b, 2))
    x0, x1, y = rng.uniform(-0.07, 0.07, n), rng.uniform(-0.07, 0.07, n), rng.normal(size=(3, n))
    kw = dict(sigmaf_sq=1.0, l_sq=0.03 ** 2)
    full = qr.quantize_rd(alpha, BV, x0, x1, y, 0.0, kw)
    assert full["bits"] == 0 and np.isnan(full["mse_q"]) and not np.any(np.isnan(full["curve"])) and not full["escaped"]
    assert qr.quantize_rd(alpha, BV, x0, x1, y, np.inf, kw, bits_min=3)["bits"] == 3
    r = qr.quantize_rd(alpha, BV, x0, x1, y, np.nan, kw)
    assert r["bits"] == 0 and np.array_equal(r["curve"], full["curve"])
    k = int(np.argmin(full["curve"]))                    # the first width within the bound wins
    r = qr.quantize_rd(alpha, BV, x0, x1, y, float(full["curve"][k]), kw)
    assert r["bits"] == 1 + int(np.argmax(full["curve"] <= full["curve"][k])) and r["mse_q"] == full["curve"][r["bits"] - 1]
    assert np.all(np.isnan(r["curve"][r["bits"]:]))
    a2, v2 = qr.dequantize(r["q_alpha"], r["q_bv"], r["range"], r["bits"])
    assert _same_bits(a2, r["alpha"]) and _same_bits(v2, r["BV"])
    # 16 bits: the error of the quantised state approaches the raw one
    assert abs(float(full["curve"][15]) - float(full["mse0"])) <= 1e-3 * float(full["mse0"])
    bad = alpha.copy()
    bad[1, 2] = np.nan
    for args in ((bad, BV, x0, x1, y), (alpha[:, :0], BV[:0], x0, x1, y), (alpha, BV, x0[:0], x1[:0], y[:, :0])):
        r = qr.quantize_rd(*args, np.inf, kw)
        assert r["escaped"] and r["bits"] == 0 and np.isnan(r["mse_q"]) and r["range"] is None


def test_v2_pack_parse_round_trip():
    rng = np.random.default_rng(5)
    patches = []
    for i, (bd, bc, wd, wc) in enumerate(((5, 9, 7, 3), (0, 4, 0, 16), (13, 0, 1, 0), (8, 8, 0, 0), (1, 1, 11, 5), (30, 21, 13, 2))):
        gps = []
        for ny, b, w in ((1, bd, wd), (3, bc, wc)):
            if w == 0:
                gps.append(dict(b=b, w=0, alpha=rng.normal(size=(ny, b)), BV=rng.normal(size=(b, 2))))
            else:
                gps.append(dict(b=b, w=w, range=rng.normal(size=(ny + 2, 2)).astype(np.float32),
                                q_alpha=rng.integers(0, 1 << w, size=(ny, b)).astype(np.uint16),
                                q_bv=rng.integers(0, 1 << w, size=(b, 2)).astype(np.uint16)))
        patches.append(dict(R=rng.normal(size=9), mean=rng.normal(size=3), rgb_mean=rng.normal(size=3), gps=gps))
    model = dict(version=2, res=0.15, sz=8, params=(bytes(range(48)), bytes(range(48, 96))), patches=patches)
    buf = qr.pack_model(model)
    assert len(buf) == qr.file_bytes(model)
    back = qr.parse_model(buf)
    assert back["version"] == 2 and back["res"] == 0.15 and back["sz"] == 8 and back["params"] == model["params"]
    for p, q in zip(patches, back["patches"]):
        assert all(_same_bits(p[k], q[k]) for k in ("R", "mean", "rgb_mean"))
        for g, h in zip(p["gps"], q["gps"]):
            assert g["b"] == h["b"] and g["w"] == h["w"]
            for k in g:
                if k not in ("b", "w"):
                    assert _same_bits(g[k], h[k]), k
    assert qr.pack_model(back) == buf
    # LSB-first: code k occupies bits k w .. (k + 1) w - 1 of the stream, bit j of the stream is bit j % 8 of byte j // 8
    assert qr.pack_bits([0b101, 0b011, 0b110], 3) == bytes([0b10011101, 0b1])
    assert list(qr.unpack_bits(bytes([0b10011101, 0b1]), 3, 3)) == [0b101, 0b011, 0b110]
    # a v1 file of the dequantised model parses back to the dequantised doubles
    v1 = qr.to_v1(back)
    b1 = qr.pack_model(v1)
    assert len(b1) == qr.file_bytes(v1) and len(b1) > len(buf)
    again = qr.parse_model(b1)
    g, h = back["patches"][0]["gps"][1], again["patches"][0]["gps"][1]
    a, v = qr.dequantize(g["q_alpha"], g["q_bv"], g["range"], g["w"])
    assert _same_bits(h["alpha"], a) and _same_bits(h["BV"], v)


def test_header_declares_the_new_symbols(capi):
    hdr = open(os.path.join(ROOT, "include", "gpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gpc_[a-z0-9_]+)\s*\(", hdr))
    new = {"gpc_sparse_quantize_rd", "gpc_sparse_quantize_rd_dev", "gpc_sparse_dequantize", "gpc_sparse_dequantize_dev",
           "gpc_test_quantize_host"}
    assert new <= declared and new <= set(capi.PROTOTYPES)
    lib = capi.load()
    assert all(hasattr(lib, s) for s in new)
