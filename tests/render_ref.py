"""NumPy restatement of the renderer (test infrastructure; the product never imports this module).

gpc_patches_render (include/gpc.h, csrc/render.hip): every ray o + t d walks the voxels of the map front to back and stops at the
first trained leaf whose depth GP's mean surface it meets inside that leaf's window.  `grid` / `batch` are the dicts of mapping_ref /
raycast_cases (voxels handled in UNSHIFTED coordinates c = k - koff); a GP is its parameters and its state per leaf:
gp = dict(sf, l_sq, b (P,), alpha (P, ny, ld), BV (P, ld, 2)), as Sparse.state() returns them.

The walk and frame arithmetic is evaluated in the kernel's association on np.float64 scalars (no contraction), so the voxel lists are
the kernel's exactly.  The GP sums are not: the kernel uses the library's table-driven exp (an ulp from np.exp) and a fused multiply-add in
the squared distance.  So next to every ray's outcome the restatement returns the ray's MARGIN: the smallest distance (a length) to a
decision boundary over every surface test on its path, up to and including the accepted one.  An outcome whose margin is far above
the rounding of the sums is the kernel's outcome too; one below it may legitimately differ.
"""
import numpy as np

INF = np.float64(np.inf)
NAN = np.float64(np.nan)
FREE = 2
C_HALF = np.float64(np.float32(-0.5))

DEFAULTS = dict(newton_iters=4, use_w=1, eps_rel=1e-6, t_max=np.inf)
# The eps_rel of the scenes that are compared with the kernel decision by decision.  Those comparisons leave out rays whose margin is
# below 1e-6 res, and one of the distances in the margin is that of |g| to eps_rel res: a converged solve has |g| ~ 1e-12, so with the
# default eps_rel = 1e-6 its margin is 1e-6 res less a hair -- every hit would be left out by construction.  Ten times the default puts
# a converged solve 9e-6 res from that boundary and leaves everything else as it is.
EPS_REL_SCENES = 1e-5


def gp_of(params, sizes, state):
    """a Sparse object's (params, sizes(), state()) as the restatement reads it"""
    alpha, _, _, BV = state
    return dict(sf=float(params.sigmaf_sq), l_sq=float(params.l_sq), b=np.asarray(sizes), alpha=alpha, BV=BV)


def gp_mean(gp, L, q1, q2, grad=True):
    """f (ny,) = sum_j alpha_j k_j and (fx, fy) (ny,) each at q, over the leaf's basis"""
    b = int(min(gp["b"][L], gp["BV"].shape[1]))
    al, bv = gp["alpha"][L][:, :b], gp["BV"][L][:b]
    d0, d1 = q1 - bv[:, 0], q2 - bv[:, 1]
    k = gp["sf"] * np.exp((C_HALF / gp["l_sq"]) * (d0 * d0 + d1 * d1))
    w = al * k
    f = np.array([np.cumsum(r)[-1] if b else 0.0 for r in w])
    if not grad:
        return f
    s1 = np.array([np.cumsum(r * (bv[:, 0] - q1))[-1] if b else 0.0 for r in w])
    s2 = np.array([np.cumsum(r * (bv[:, 1] - q2))[-1] if b else 0.0 for r in w])
    return f, s1 / gp["l_sq"], s2 / gp["l_sq"]


def entry(grid, o, d):
    """(meets, t_in, start voxel unshifted) of the ray against the grid box"""
    koff, kmax, mn, res = grid["koff"], grid["kmax"], grid["mn"], grid["res"]
    tn, tf, ok = -INF, INF, True
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        for a in range(3):
            lo = mn[a] + np.float64(0 - koff[a]) * res
            hi = mn[a] + np.float64(kmax[a] + 1 - koff[a]) * res
            if d[a] != 0.0:
                t1, t2 = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
                tn, tf = max(tn, min(t1, t2)), min(tf, max(t1, t2))
            elif not (lo <= o[a] < hi):
                ok = False
        if not (ok and tn <= tf and tf >= 0.0):
            return False, NAN, None
        t_in = max(tn, np.float64(0.0))
        c = np.zeros(3, np.int64)
        for a in range(3):
            kd = np.floor(((o[a] + t_in * d[a]) - mn[a]) / res) + np.float64(koff[a])
            c[a] = int(min(max(kd, 0.0), np.float64(kmax[a]))) - koff[a]
    return True, t_in, c


def exit_params(grid, c, o, d):
    """per axis the parameter at which the ray leaves voxel c (inf for d_a == 0)"""
    x = [INF, INF, INF]
    with np.errstate(divide="ignore", over="ignore"):
        for a in range(3):
            if d[a] == 0.0:
                continue
            kf = c[a] + 1 if d[a] > 0.0 else c[a]
            x[a] = ((grid["mn"][a] + np.float64(kf) * grid["res"]) - o[a]) / d[a]
    return x


def step(grid, c, o, d):
    """the axis the ray leaves voxel c across (first that attains the minimum), or -1; tie: two exit parameters are equal"""
    best, ax, tie = INF, -1, False
    x = exit_params(grid, c, o, d)
    for a in range(3):
        if d[a] == 0.0:
            continue
        if x[a] < best or ax < 0:
            best, ax = x[a], a
    tie = sum(1 for a in range(3) if d[a] != 0.0 and x[a] == best) > 1
    return ax, tie


def surface(batch, grid, gp, L, c, o, d, prm, W, cells):
    """the surface test of leaf L in voxel c: dict(accept, finite, resid, t, f, q1, q2, x, gprime, margin)"""
    R, mu = batch["R"][L], batch["mean"][L]
    res, sz, half = grid["res"], grid["sz"], grid["half"]
    tol = np.float64(prm["eps_rel"]) * res
    t_max = np.float64(prm["t_max"])
    with np.errstate(all="ignore"):
        e = [o[a] - mu[a] for a in range(3)]
        a_ = [R[0, j] * e[0] + R[1, j] * e[1] + R[2, j] * e[2] for j in range(3)]
        c_ = [R[0, j] * d[0] + R[1, j] * d[1] + R[2, j] * d[2] for j in range(3)]
        num = R[0, 0] * (mu[0] - o[0]) + R[1, 0] * (mu[1] - o[1]) + R[2, 0] * (mu[2] - o[2])
        t = num / c_[0]
        gprime = NAN
        for it in range(int(prm["newton_iters"]) + 1):
            q1, q2 = a_[1] + t * c_[1], a_[2] + t * c_[2]
            f, fx, fy = (v[0] for v in gp_mean(gp, L, q1, q2))
            g = (a_[0] + t * c_[0]) - f
            gprime = c_[0] - (fx * c_[1] + fy * c_[2])
            if it < int(prm["newton_iters"]):
                t = t - g / gprime
        out = dict(accept=False, finite=False, resid=False, t=t, f=f, q1=q1, q2=q2, x=None, gprime=gprime, margin=INF, leaf=L)
        if not all(np.isfinite(v) for v in (t, q1, q2, f, g)):
            return out
        out["finite"] = True
        ok = True
        if not abs(g) <= tol:
            out["resid"], ok = True, False
        if not (t > 0.0 and t <= t_max):
            ok = False
        if q1 > half or q1 < -half or q2 > half or q2 < -half:
            ok = False
        x = np.array([((R[i, 0] * f + R[i, 1] * q1) + R[i, 2] * q2) + mu[i] for i in range(3)])
        cen = grid["mn"] + (c.astype(np.float64) + 0.5) * res
        ex = x - cen
        r2 = ex[0] * ex[0] + ex[1] * ex[1] + ex[2] * ex[2]
        if not r2 <= grid["radius"] * grid["radius"]:
            ok = False
        u1, u2 = np.float64(sz) * (q1 / res + 0.5), np.float64(sz) * (q2 / res + 0.5)
        cell = sz * min(max(int(u1), 0), sz - 1) + min(max(int(u2), 0), sz - 1)
        if prm["use_w"] and W[L, cell] == 0:
            ok = False
        if cells is not None and cells[L, cell] == FREE:
            ok = False
        # distances to the decision boundaries, as lengths
        dn = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        m = [abs(abs(q1) - half), abs(abs(q2) - half), abs(np.sqrt(r2) - grid["radius"]), abs(t) * dn, abs(abs(g) - tol),
             abs(u1 - np.rint(u1)) * res / sz, abs(u2 - np.rint(u2)) * res / sz, abs(gprime) / abs(c_[0]) * res]
        if np.isfinite(t_max):
            m.append(abs(t - t_max) * dn)
        out.update(accept=ok, x=x, margin=min(m), cell=cell)
    return out


def render(batch, grid, depth, origin, dirs, params=None, cells=None, rgb=None):
    """Returns a list with one dict per ray: leaf (-1 = miss), t, local (3,), x (3,) float64, rgb (3,) float64 = colour GP mean +
    rgb_mean before the flatten (None without rgb), outside, visited [unshifted voxels], tests [surface() dicts], gprime (at the
    accepted solution), margin, tie (two exit parameters were equal at a step)."""
    prm = dict(DEFAULTS, **(params or {}))
    o = np.asarray(origin, dtype=np.float64)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    vox = grid["vox"] - grid["koff"]
    leaf_of = {tuple(int(x) for x in v): L for L, v in enumerate(vox)}
    lo_c, hi_c = -grid["koff"], grid["kmax"] - grid["koff"]
    W = batch.get("W")
    out = []
    for d in dirs:
        r = dict(leaf=-1, t=NAN, local=np.full(3, NAN), x=np.full(3, NAN), rgb=None, outside=True, visited=[], tests=[], gprime=NAN,
                 margin=INF, tie=False)
        out.append(r)
        if not np.all(np.isfinite(d)) or not np.any(d != 0.0) or len(vox) == 0:
            continue
        meets, t_in, c = entry(grid, o, d)
        if not meets:
            continue
        r["outside"] = False
        for _ in range(int(np.sum(grid["kmax"])) + 1):
            r["visited"].append(tuple(int(v) for v in c))
            L = leaf_of.get(r["visited"][-1], -1)
            if L >= 0 and depth["b"][L] > 0:
                s = surface(batch, grid, depth, L, c, o, d, prm, W, cells)
                r["tests"].append(s)
                r["margin"] = min(r["margin"], s["margin"])
                if s["accept"]:
                    r.update(leaf=L, t=s["t"], local=np.array([s["f"], s["q1"], s["q2"]]), x=s["x"], gprime=s["gprime"])
                    if rgb is not None:
                        r["rgb"] = gp_mean(rgb, L, s["q1"], s["q2"], grad=False) + batch["rgb_mean"][L]
                    break
            ax, tie = step(grid, c, o, d)
            r["tie"] = r["tie"] or tie
            if ax < 0:
                break
            c[ax] += 1 if d[ax] > 0.0 else -1
            if c[ax] < lo_c[ax] or c[ax] > hi_c[ax]:
                break
    return out


def counts_of(rays):
    """[rays, hits, rays that never met the grid, surface tests, tests rejected on the residual]"""
    return np.array([len(rays), sum(r["leaf"] >= 0 for r in rays), sum(r["outside"] for r in rays), sum(len(r["tests"]) for r in rays),
                     sum(s["resid"] for r in rays for s in r["tests"])], dtype=np.int32)


def camera_rays(R, fx, fy, cx, cy, width, height):
    """gpc_camera_rays_dev: pixel v * width + u -> R ((u - cx) / fx, (v - cy) / fy, 1), R (3, 3) with the camera's axes as columns"""
    R = np.asarray(R, dtype=np.float64)
    v, u = np.divmod(np.arange(width * height), width) if width * height else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    x, y = (u.astype(np.float64) - cx) / fx, (v.astype(np.float64) - cy) / fy
    return np.stack([(R[a, 0] * x + R[a, 1] * y) + R[a, 2] for a in range(3)], axis=1)


def flatten(x):
    """rp_flatten: x.cast<short>() as the x86-64 reference evaluates it, then the clamp to 0 .. 255"""
    if not np.isfinite(x):
        return 255
    w = -2 ** 31 if (x >= 2147483648.0 or x < -2147483648.0) else int(x)
    v = ((w & 0xffff) ^ 0x8000) - 0x8000
    return min(max(v, 0), 255)
