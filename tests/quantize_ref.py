"""NumPy restatement of the quantise rule (include/gpc.h, gpc_sparse_quantize_rd / gpc_sparse_dequantize), of the GPCM v2 model file
(gp_compressor::save_model_quantized) and the cases the quantise tests share, on top of prune_rd_ref.

The scalar quantiser, for an array v[0..b) of finite doubles and a width w in 1..16:

    lo = the largest float <= min v, hi = the smallest float >= max v         (numpy.float32 rounds to nearest; numpy.nextafter mends it)
    step = (hi - lo) / (2^w - 1)
    q_i = step > 0 ? clamp(rint((v_i - lo) / step), 0, 2^w - 1) : 0           (numpy.rint is round-half-even)
    v'_i = lo + q_i * step                                                     (NumPy rounds the product and the sum separately)

Per patch (alpha (ny, b), BV (b, 2), points x0, x1, y (ny, n), bound B): the ny + 2 arrays -- BV column 0, BV column 1, the alpha planes
-- are quantised separately at one width; the widths bits_min .. bits_max are tried in ascending order and the first whose error
prune_rd_ref.mse_of(alpha', BV') is <= B wins.  b == 0, n == 0 or a non-finite value: the patch escapes (bits 0, nothing else).
"""
import struct

import numpy as np

import prune_rd_ref as rd

# E64_MSE_Q: the largest relative gap between the float64 and the longdouble evaluation of prune_rd_ref.mse_of on the same dequantised
# bits, over every width evaluated for the bounds 1.1 mse0 and 2 mse0 on the oracle-trained states of every regime.  None: the measurement
# of tests/test_quantize_cpu.py::test_e64_mse_q stays within prune_rd_ref.E64_MSE, which is then the figure the gates use.
E64_MSE_Q = None


def e64():
    return rd.E64_MSE if E64_MSE_Q is None else E64_MSE_Q


# ---- rule 1 ---------------------------------------------------------------------------------------------------------------------------

def f32_down(v):
    f = np.float32(v)
    return np.nextafter(f, np.float32(-np.inf)) if float(f) > float(v) else f


def f32_up(v):
    f = np.float32(v)
    return np.nextafter(f, np.float32(np.inf)) if float(f) < float(v) else f


def q_range(v):
    """(lo, hi) as float32"""
    v = np.asarray(v, dtype=np.float64)
    return f32_down(v.min()), f32_up(v.max())


def q_step(lo, hi, w):
    return (np.float64(hi) - np.float64(lo)) / np.float64((1 << w) - 1)


def q_codes(v, lo, hi, w):
    v = np.asarray(v, dtype=np.float64)
    step = q_step(lo, hi, w)
    if not step > 0:
        return np.zeros(v.shape, dtype=np.uint16)
    with np.errstate(all="ignore"):
        r = np.rint((v - np.float64(lo)) / step)
    return np.where(r > 0, np.minimum(r, float((1 << w) - 1)), 0.0).astype(np.uint16)


def q_values(q, lo, hi, w):
    t = np.asarray(q).astype(np.float64) * q_step(lo, hi, w)
    return np.float64(lo) + t


def quantize_array(v, w):
    """codes (uint16), (lo, hi) float32 (2,), dequantised values"""
    lo, hi = q_range(v)
    q = q_codes(v, lo, hi, w)
    return q, np.array([lo, hi], dtype=np.float32), q_values(q, lo, hi, w)


# ---- rules 2 and 3 on one patch ---------------------------------------------------------------------------------------------------------

def arrays_of(alpha, BV):
    """the ny + 2 arrays in the order of `range`: BV column 0, BV column 1, the alpha planes"""
    return [BV[:, 0], BV[:, 1]] + [alpha[c] for c in range(alpha.shape[0])]


def state_ranges(alpha, BV):
    return np.array([q_range(a) for a in arrays_of(alpha, BV)], dtype=np.float32)           # (ny + 2, 2)


def state_codes(alpha, BV, rng, w):
    """q_alpha (ny, b), q_bv (b, 2)"""
    q = [q_codes(a, rng[k, 0], rng[k, 1], w) for k, a in enumerate(arrays_of(alpha, BV))]
    return np.stack(q[2:], 0), np.stack(q[:2], 1)


def dequantize(q_alpha, q_bv, rng, w):
    """alpha' (ny, b), BV' (b, 2)"""
    BV = np.stack([q_values(q_bv[:, k], rng[k, 0], rng[k, 1], w) for k in range(2)], 1)
    alpha = np.stack([q_values(q_alpha[c], rng[2 + c, 0], rng[2 + c, 1], w) for c in range(q_alpha.shape[0])], 0)
    return alpha, BV


def quantize_rd(alpha, BV, x0, x1, y, bound, kw, bits_min=1, bits_max=16, dtype=np.float64):
    """The rule on one patch.  bound: a number, or a callable mse0 -> bound.  Returns dict(bits, mse0, mse_q, curve (16, NaN where not
    evaluated), range, q_alpha, q_bv, alpha, BV (the accepted dequantised state), bound, band, escaped, states: w -> (alpha', BV'))."""
    alpha, BV = np.asarray(alpha, dtype=np.float64), np.asarray(BV, dtype=np.float64)
    ny, b = alpha.shape
    n = len(x0)
    sf, l_sq = kw["sigmaf_sq"], kw["l_sq"]
    mse0 = rd.mse_of(alpha, BV, x0, x1, y, sf, l_sq, dtype)
    B = bound(mse0) if callable(bound) else bound
    out = dict(bits=0, mse0=mse0, mse_q=np.nan, curve=np.full(16, np.nan, dtype=dtype), range=None, q_alpha=None, q_bv=None, alpha=None,
               BV=None, bound=B, band=np.inf, escaped=True, states={})
    if b == 0 or n == 0 or not (np.all(np.isfinite(alpha)) and np.all(np.isfinite(BV))):
        return out
    out["escaped"] = False
    rng = out["range"] = state_ranges(alpha, BV)
    for w in range(bits_min, bits_max + 1):
        qa, qb = state_codes(alpha, BV, rng, w)
        a2, v2 = dequantize(qa, qb, rng, w)
        e = rd.mse_of(a2, v2, x0, x1, y, sf, l_sq, dtype)
        out["curve"][w - 1] = e
        out["states"][w] = (a2, v2)
        if np.isfinite(float(e)) and np.isfinite(float(B)) and float(B) > 0:
            out["band"] = min(out["band"], abs(float(e) - float(B)) / float(B))
        if e <= B:
            out.update(bits=w, mse_q=e, q_alpha=qa, q_bv=qb, alpha=a2, BV=v2)
            break
    return out


# ---- GPCM v2 -----------------------------------------------------------------------------------------------------------------------------
# little-endian.  Header as v1: "GPCM", u32 version, f64 res, i32 sz, i32 P, u32 psz, two parameter structs of psz bytes (kept opaque).
# Per patch: f64 R[9], mean[3], rgb_mean[3]; i32 b_depth, b_rgb; (v2 only) u8 w_depth, w_rgb; then the depth GP (ny = 1) and the colour GP
# (ny = 3), each either raw (w == 0, and always in v1): f64 BV[b][2], alpha[ny][b]; or quantised: f32 (lo, hi) x (ny + 2), then the codes
# of BV0[0..b), BV1[0..b), alpha plane 0[0..b), .. bit-packed LSB-first at w bits each, zero-padded to a whole byte.

def pack_bits(codes, w):
    codes = np.asarray(codes, dtype=np.uint32).ravel()
    bits = ((codes[:, None] >> np.arange(w, dtype=np.uint32)[None, :]) & 1).astype(np.uint8).ravel()
    return np.packbits(bits, bitorder="little").tobytes()


def unpack_bits(buf, count, w):
    bits = np.unpackbits(np.frombuffer(buf, dtype=np.uint8), bitorder="little")[:count * w].reshape(count, w).astype(np.uint32)
    return (bits << np.arange(w, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint16)


def packed_bytes(b, ny, w):
    return (b * (ny + 2) * w + 7) // 8


def gp_bytes(b, ny, w):
    """payload of one GP of one patch"""
    return 8 * b * (ny + 2) if w == 0 else 8 * (ny + 2) + packed_bytes(b, ny, w)


def header_bytes(psz):
    return 4 + 4 + 8 + 8 + 4 + 2 * psz


def file_bytes(model):
    """the byte count of the file pack_model writes (the v2 formula for version 2, v1's for version 1)"""
    n = header_bytes(len(model["params"][0]))
    for p in model["patches"]:
        n += 15 * 8 + 8 + (2 if model["version"] == 2 else 0)
        for ny, g in zip((1, 3), p["gps"]):
            n += gp_bytes(g["b"], ny, g["w"] if model["version"] == 2 else 0)
    return n


def pack_model(model):
    """model: dict(version, res, sz, params (2 byte strings), patches: [dict(R (9,), mean (3,), rgb_mean (3,), gps: [depth, colour])]);
    a GP is dict(b, w, and for w == 0: alpha (ny, b), BV (b, 2); for w > 0: range (ny + 2, 2) float32, q_alpha (ny, b), q_bv (b, 2))"""
    ver = model["version"]
    out = [b"GPCM", struct.pack("<Idii", ver, model["res"], model["sz"], len(model["patches"])), struct.pack("<I", len(model["params"][0])),
           model["params"][0], model["params"][1]]
    for p in model["patches"]:
        out += [np.asarray(p[k], dtype="<f8").tobytes() for k in ("R", "mean", "rgb_mean")]
        out.append(struct.pack("<ii", *(g["b"] for g in p["gps"])))
        if ver == 2:
            out.append(struct.pack("<BB", *(g["w"] for g in p["gps"])))
        for g in p["gps"]:
            if ver == 1 or g["w"] == 0:
                out += [np.asarray(g["BV"], dtype="<f8").tobytes(), np.asarray(g["alpha"], dtype="<f8").tobytes()]
            else:
                out.append(np.asarray(g["range"], dtype="<f4").tobytes())
                out.append(pack_bits(np.concatenate([g["q_bv"][:, 0], g["q_bv"][:, 1], np.asarray(g["q_alpha"]).ravel()]), g["w"]))
    return b"".join(out)


def parse_model(buf):
    """inverse of pack_model (versions 1 and 2)"""
    assert buf[:4] == b"GPCM"
    ver, res, sz, P = struct.unpack_from("<Idii", buf, 4)
    psz, = struct.unpack_from("<I", buf, 24)
    pos = 28
    params = (buf[pos:pos + psz], buf[pos + psz:pos + 2 * psz])
    pos += 2 * psz
    patches = []

    def take(dtype, count):
        nonlocal pos
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=pos).copy()
        pos += a.nbytes
        return a

    for _ in range(P):
        p = dict(R=take("<f8", 9), mean=take("<f8", 3), rgb_mean=take("<f8", 3))
        bs = take("<i4", 2)
        ws = take("u1", 2) if ver == 2 else np.zeros(2, dtype=np.uint8)
        p["gps"] = []
        for ny, b, w in zip((1, 3), bs.tolist(), ws.tolist()):
            g = dict(b=b, w=w)
            if w == 0:
                g["BV"] = take("<f8", 2 * b).reshape(b, 2)
                g["alpha"] = take("<f8", ny * b).reshape(ny, b)
            else:
                g["range"] = take("<f4", 2 * (ny + 2)).reshape(ny + 2, 2)
                nb = packed_bytes(b, ny, w)
                q = unpack_bits(buf[pos:pos + nb], b * (ny + 2), w).reshape(ny + 2, b)
                pos += nb
                g["q_bv"] = np.stack([q[0], q[1]], 1)
                g["q_alpha"] = q[2:].copy()
            p["gps"].append(g)
        patches.append(p)
    assert pos == len(buf), (pos, len(buf))
    return dict(version=ver, res=res, sz=sz, params=params, patches=patches)


def to_v1(model):
    """the same model with every quantised GP dequantised by rule 1 and stored raw"""
    patches = []
    for p in model["patches"]:
        gps = []
        for g in p["gps"]:
            if g["w"] == 0:
                gps.append(dict(b=g["b"], w=0, alpha=g["alpha"], BV=g["BV"]))
            else:
                a, v = dequantize(g["q_alpha"], g["q_bv"], g["range"], g["w"])
                gps.append(dict(b=g["b"], w=0, alpha=a, BV=v))
        patches.append(dict(R=p["R"], mean=p["mean"], rgb_mean=p["rgb_mean"], gps=gps))
    return dict(version=1, res=model["res"], sz=model["sz"], params=model["params"], patches=patches)
