"""NumPy restatement of the allocation rule of gpc_rate_allocate (include/gpc.h), written from the header's text with separate products and
sums, and a brute-force enumerator for tiny problems.  Not a test module: the tests of the host twin and of the kernels compare against it
bit for bit."""
import itertools
import struct

import numpy as np

INF_BITS = 0x7FF0000000000000


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", int(b)))[0]


def to_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


class Problem:
    """R rows: kmax (R,) int32, d0 (R,), d (R, ld), w (R,) or None with w_all, unit (R,) int32 or None with unit_all"""

    def __init__(self, kmax, d0, d, w=None, w_all=1.0, unit=None, unit_all=24):
        self.kmax = np.ascontiguousarray(kmax, dtype=np.int32)
        self.d0 = np.ascontiguousarray(d0, dtype=np.float64)
        self.d = np.ascontiguousarray(d, dtype=np.float64)
        self.R, self.ld = self.d.shape
        self.w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        self.w_all = float(w_all)
        self.unit = None if unit is None else np.ascontiguousarray(unit, dtype=np.int32)
        self.unit_all = int(unit_all)
        # what the rule works with: clamped counts, units >= 1, one weight per row, the curve with e(0) in front
        self.km = np.clip(self.kmax.astype(np.int64), 0, self.ld)
        self.u = np.maximum(np.full(self.R, self.unit_all, dtype=np.int64) if self.unit is None else self.unit.astype(np.int64), 1)
        self.wr = np.full(self.R, self.w_all) if self.w is None else self.w
        self.e = np.concatenate([self.d0[:, None], self.d], axis=1)              # (R, ld + 1): e[r, k]
        with np.errstate(invalid="ignore", over="ignore"):
            self.D = self.wr[:, None] * self.e                                    # one rounded product each

    def args(self):
        """the arguments of the C entries between (R, ld) and need"""
        return (self.kmax, self.d0, self.d, self.w, self.w_all, self.unit, self.unit_all)


def choice(pb, lam):
    """choice_r(lambda) for every row, (R,) int64"""
    ks = np.arange(pb.ld + 1, dtype=np.int64)[None, :]
    rate = pb.u[:, None] * (pb.km[:, None] - ks)                                  # int64; negative beyond kmax: not an option
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(rate == 0, 0.0, np.float64(lam) * rate.astype(np.float64))   # the product, rounded
        c = pb.D + t                                                              # the sum, rounded
    ok = (ks <= pb.km[:, None]) & ~np.isnan(c)
    fixed = ~ok[:, 0]                                                             # c(0) is NaN
    cmin = np.min(np.where(ok, c, np.inf), axis=1)
    hit = ok & (c == cmin[:, None])                                               # the options that attain the minimum ...
    best = np.max(np.where(hit, ks, 0), axis=1)                                   # ... the largest of them
    return np.where(fixed, 0, best).astype(np.int64)


def saving(pb, k):
    return int(np.sum(pb.u * np.asarray(k, dtype=np.int64)))


def allocate(pb, need, refine=True, count=None):
    """the whole rule: dict(k, target, lambda_bits, saved, max_saving, feasible, switched_rows)"""
    need = int(need)
    inf = float("inf")
    k_inf = choice(pb, inf)
    max_saving = saving(pb, k_inf)
    switched = 0
    if max_saving < need:
        k, lam, feasible = k_inf, inf, 0
    else:
        feasible = 1
        k_zero = choice(pb, 0.0)
        if saving(pb, k_zero) >= need:
            k, lam = k_zero, 0.0
        else:
            lo, hi = 0, INF_BITS
            steps = 0
            while hi - lo > 1:
                mid = lo + (hi - lo) // 2
                if saving(pb, choice(pb, from_bits(mid))) >= need:
                    hi = mid
                else:
                    lo = mid
                steps += 1
            assert steps <= 63
            lam = from_bits(hi)
            k_hi = choice(pb, lam)
            k = k_hi
            if refine:
                k_lo = choice(pb, from_bits(lo))
                delta = pb.u * (k_hi - k_lo)
                E = saving(pb, k_lo) + np.concatenate([[0], np.cumsum(delta)[:-1]])
                k_ref = np.where(E < need, k_hi, k_lo)
                if saving(pb, k_ref) >= need:
                    k = k_ref
                switched = int(np.sum(k != k_lo))
    out = dict(k=k.astype(np.int32), lambda_bits=to_bits(lam), saved=saving(pb, k), max_saving=max_saving, feasible=feasible,
               switched_rows=switched, target=None)
    if count is not None:
        out["target"] = np.maximum(1, np.asarray(count, dtype=np.int64) - k).astype(np.int32)
    return out


def total_error(pb, k):
    """sum_r D_r(k_r), in ascending r"""
    return float(sum(float(pb.D[r, int(k[r])]) for r in range(pb.R)))


def brute_force(pb):
    """every allocation of a tiny problem: list of (saving, total error, k)"""
    out = []
    for k in itertools.product(*[range(int(m) + 1) for m in pb.km]):
        out.append((saving(pb, k), total_error(pb, k), k))
    return out


# ---- the problems both test modules run ------------------------------------------------------------------------------------------

def random_problem(seed, R, ld, kind="random", units="24", weights="all"):
    rng = np.random.default_rng(seed)
    kmax = rng.integers(0, ld + 1, size=R).astype(np.int32)
    if kind == "monotone":
        d = np.cumsum(rng.random((R, ld + 1)) ** 3, axis=1) * rng.random((R, 1)) * 10.0
    elif kind == "identical":
        row = np.cumsum(np.sort(rng.random(ld + 1)))                             # convex: a multiplier moves a row by one removal
        d = np.tile(row, (R, 1))
        kmax[:] = ld
    elif kind == "integer":
        d = rng.integers(0, 6, size=(R, ld + 1)).astype(np.float64)
    else:
        d = rng.random((R, ld + 1)) * 10.0                                        # non-monotone
    d0, d = d[:, 0].copy(), np.ascontiguousarray(d[:, 1:])
    if kind == "nan":
        d[rng.random(d.shape) < 0.2] = np.nan
        d0[rng.random(R) < 0.2] = np.nan
    if kind == "kmax0":
        kmax[::2] = 0
    unit = None
    if units == "mixed":
        unit = np.where(rng.random(R) < 0.5, 24, 40).astype(np.int32)
    w = None if weights == "all" else (rng.random(R) * 3.0)
    return Problem(kmax, d0, d, w=w, w_all=1.0 if kind == "integer" else 0.75, unit=unit, unit_all=24)


def needs_of(pb):
    """the byte counts the issue lists: -5, 0, 1, a quarter, a half, max_saving, max_saving + 1"""
    ms = saving(pb, choice(pb, float("inf")))
    return [-5, 0, 1, ms // 4, ms // 2, ms, ms + 1]
