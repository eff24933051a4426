"""NumPy restatement of gpc_cloud_distortion and gpc_patches_normals (include/gpc.h), by brute force: float -> double, the d2 formula in
its association, argmin (which returns the FIRST minimum: the tie rule, lowest index of B), the chunked sum.  Every operation is one
IEEE double operation in NumPy as on the device, so the GPU tests compare by bits."""
import math

import numpy as np

from gp_compressor_amd import capi

POINT = capi.Context.POINT_DTYPE
CHUNK = 4096


def make_cloud(xyz, rgb=None):
    """(n, 3) float32 [+ (n, 3) uint8] -> pcl::PointXYZRGB records (Context.make_cloud without a context)"""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    c = np.zeros(len(xyz), dtype=POINT)
    c["x"], c["y"], c["z"], c["w"], c["a"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 1.0, 255
    if rgb is not None:
        rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
        c["r"], c["g"], c["b"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    return c


def xyz_of(cloud):
    return np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(np.float64)


def chunked_sum(v):
    """The sum rule: chunks of 4096 consecutive entries; inside a chunk entry i goes to class i mod 64, each class adds its entries in
    ascending i from +0.0, the 64 class sums go through the xor tree d = 32 .. 1; the chunk sums by the same rule until one is left."""
    v = np.asarray(v, dtype=np.float64).ravel()
    if v.size == 0:
        return 0.0
    lane = np.arange(64)
    while True:
        c = -(-len(v) // CHUNK)
        pad = np.zeros(c * CHUNK)
        pad[:len(v)] = v
        t = pad.reshape(c, 64, 64)                 # [chunk][step][class]
        s = np.zeros((c, 64))
        for j in range(64):
            s = s + t[:, j, :]
        for d in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lane ^ d]
        v = s[:, 0].copy()
        if c == 1:
            return float(v[0])


def distortion(a, b, normals_b=None, max_dist=float("inf"), block=2048):
    """One direction a -> b on record arrays: the dict Context.cloud_distortion returns with want = (nn, d2, e2)."""
    pa, pb = xyz_of(a), xyz_of(b)
    na = len(a)
    va, vb = np.isfinite(pa).all(1), np.flatnonzero(np.isfinite(pb).all(1))
    q = pb[vb]
    nn = np.full(na, -1, dtype=np.int32)
    d2 = np.full(na, np.nan)
    e2 = np.full(na, np.nan)
    dxyz = np.zeros((na, 3))
    md2 = np.float64(max_dist) * np.float64(max_dist)
    if len(vb):
        for lo in range(0, na, block):
            rows = np.flatnonzero(va[lo:lo + block]) + lo
            if not len(rows):
                continue
            with np.errstate(over="ignore", invalid="ignore"):
                dx = pa[rows, 0][:, None] - q[None, :, 0]
                dy = pa[rows, 1][:, None] - q[None, :, 1]
                dz = pa[rows, 2][:, None] - q[None, :, 2]
                dd = (dx * dx + dy * dy) + dz * dz
            j = np.argmin(dd, axis=1)              # the first minimum: the lowest index of B among ties
            r = np.arange(len(rows))
            best = dd[r, j]
            ok = best <= md2
            nn[rows[ok]] = vb[j[ok]]
            d2[rows[ok]] = best[ok]
            dxyz[rows[ok]] = np.stack([dx[r, j], dy[r, j], dz[r, j]], 1)[ok]
    m = nn >= 0
    if normals_b is not None:
        nrm = np.asarray(normals_b, dtype=np.float32).reshape(len(b), 3)[np.where(m, nn, 0)].astype(np.float64)
        pl = m & np.isfinite(nrm).all(1)
        with np.errstate(invalid="ignore", over="ignore"):
            e = (dxyz[:, 0] * nrm[:, 0] + dxyz[:, 1] * nrm[:, 1]) + dxyz[:, 2] * nrm[:, 2]
        e2[pl] = (e * e)[pl]
    else:
        pl = np.zeros(na, dtype=bool)
    dc = np.zeros((na, 3))
    for k, ch in enumerate("rgb"):
        dc[m, k] = a[ch][m].astype(np.int64) - b[ch][nn[m]].astype(np.int64)
    luma = (0.2126 * dc[:, 0] + 0.7152 * dc[:, 1]) + 0.0722 * dc[:, 2]
    zero = np.zeros(na)
    return dict(n_valid=int(va.sum()), n_matched=int(m.sum()), n_plane=int(pl.sum()),
                sse_d1=chunked_sum(np.where(m, d2, zero)), max_d1=float(d2[m].max()) if m.any() else 0.0,
                sse_d2=chunked_sum(np.where(pl, e2, zero)), max_d2=float(e2[pl].max()) if pl.any() else 0.0,
                sse_rgb=np.array([chunked_sum(dc[:, k] * dc[:, k]) for k in range(3)]), sse_luma=chunked_sum(luma * luma),
                nn=nn, d2=d2, e2=e2)


def psnr(sse, count, peak):
    if not count > 0 or sse != sse:
        return float("nan")
    if sse == 0:
        return float("inf")
    return 10.0 * math.log10(float(peak) * float(peak) * float(count) / float(sse))


METRICS = {"d1": ("sse_d1", None, "n_matched"), "d2": ("sse_d2", None, "n_plane"), "r": ("sse_rgb", 0, "n_matched"),
           "g": ("sse_rgb", 1, "n_matched"), "b": ("sse_rgb", 2, "n_matched"), "luma": ("sse_luma", None, "n_matched")}


def cloud_psnr(a, b, peak, normals_a=None, normals_b=None):
    """Both directions; per metric the two mean square errors (NaN over no point) and the PSNR of the larger one (peak 255 for colours)"""
    ab, ba = distortion(a, b, normals_b), distortion(b, a, normals_a)
    out = {"ab": ab, "ba": ba}
    for name, (key, k, cnt) in METRICS.items():
        pk = peak if name in ("d1", "d2") else 255.0
        rows = [(float(r[key] if k is None else r[key][k]), int(r[cnt])) for r in (ab, ba)]
        mse = tuple(s / c if c > 0 else float("nan") for s, c in rows)
        worst = None
        for (s, c), m in zip(rows, mse):
            if m == m and (worst is None or m > worst[2]):
                worst = (s, c, m)
        out[name] = {"mse": mse, "psnr": psnr(worst[0], worst[1], pk) if worst else float("nan")}
    return out


def patches_normals(batch, n):
    """gpc_patches_normals from a fetched batch (Patches.fetch): R[L][:, 0] as float32 at the points leaf L owns, NaN elsewhere"""
    out = np.full((n, 3), np.nan, dtype=np.float32)
    off, src = batch["off"], batch["src"]
    for L in range(len(off) - 1):
        out[src[off[L]:off[L + 1]]] = batch["R"][L][:, 0].astype(np.float32)
    return out


def same_bits(x, y):
    """equal as numbers and in the places of the NaN"""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape:
        return False
    if x.dtype.kind != "f":
        return bool(np.array_equal(x, y))
    nx, ny = np.isnan(x), np.isnan(y)
    w = x.dtype.itemsize
    return bool(np.array_equal(nx, ny) and np.array_equal(x[~nx].view(f"u{w}"), y[~ny].view(f"u{w}")))


RESULT_KEYS = ("n_valid", "n_matched", "n_plane", "sse_d1", "max_d1", "sse_d2", "max_d2", "sse_rgb", "sse_luma")


def assert_same(got, want, keys=RESULT_KEYS + ("nn", "d2", "e2")):
    for k in keys:
        assert same_bits(np.asarray(got[k]), np.asarray(want[k])), (k, got[k], want[k])
