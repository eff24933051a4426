"""CPU model of the one-wave kernel's backward stream with paired L_kk^-T images (csrc/dense_mfma_w1.hip, csrc/mfma_tile.h; -m "not gpu").

The 256-point instance of dense_w1_kernel writes the sixteen triangular L_kk^-T of a patch two per image (mf_tri_pack: tile 2 p on and
above the diagonal; tile 2 p + 1 with rows and columns reversed strictly below it, its diagonal in an LDS array), writes none for the last
step (the backward solve reads them from the step's L_cc^-1 images in LDS, transposed index), and walks a stream of NP^2 / 2 compile-time
positions aligned at the even column count.  This file replays, lane by lane in NumPy, with the MFMA lane maps of
test_mfma_layout_model.py:
  * the lane masks (mf_tri_mask), pack (mf_tri_pack) and unpack (mf_tri_upper / mf_tri_lower),
  * the transposed and the reversed-transposed LDS read (mf_img_load_t / mf_img_load_tr),
  * the position -> (column, tile | pair) map (w1_pstream_pair, stream_addr) with its skips for a factor of nt < NP tile columns,
  * the column close with the reversed index (bw_close, REV),
and checks alpha against a plain triangular solve for every tile count: 1 .. 16 with the 256-point instance's stream (NP = 16), and
1 .. 32 with a stream of NP = 32 columns.  (The shipped 512-point instance keeps one L_kk^-T image per tile -- the diagonals' LDS would cost
it a workgroup per CU -- so NP = 32 pins the map itself, for the day it is wanted.)  It also counts the images the stream requests: every
off-diagonal tile once, every pair of a step before the last once, nothing else but the slot's first image.
"""
import numpy as np
import pytest

from test_mfma_layout_model import IMG_LS, LG, LR, img_rc, mfma

W1_C = 4


def tri_mask(s, kind):
    """mf_tri_mask: bit l set when element (row l & 15, column (l >> 4) + 4 s) of register s is on/above (0), on (1), below (2) the diagonal."""
    m = 0
    for l in range(64):
        r, c = l & 15, (l >> 4) + 4 * s
        if (r <= c) if kind == 0 else (r == c) if kind == 1 else (r > c):
            m |= 1 << l
    return m


def lanes(mask):
    return np.array([(mask >> l) & 1 for l in range(64)], dtype=bool)


def image_of(M):
    """operand image registers of a 16 x 16 matrix: (64, 4), register s of lane l = M[l & 15][(l >> 4) + 4 s]"""
    return np.stack([M[LR, LG + 4 * s] for s in range(4)], axis=1)


def lds_image_of(M):
    """the 256 doubles of the image in LDS / in the workspace"""
    out = np.zeros(256)
    out[IMG_LS] = image_of(M)
    return out


def img_load_t(img):
    return np.stack([img[[img_rc(LG[l] + 4 * s, LR[l]) for l in range(64)]] for s in range(4)], axis=1)


def img_load_tr(img):
    return np.stack([img[[img_rc(15 - LG[l] - 4 * s, 15 - LR[l]) for l in range(64)]] for s in range(4)], axis=1)


def tri_pack(up, lo):
    return np.stack([np.where(lanes(tri_mask(s, 0)), up[:, s], lo[:, s]) for s in range(4)], axis=1)


def tri_upper(p):
    return np.stack([np.where(lanes(tri_mask(s, 0)), p[:, s], 0.0) for s in range(4)], axis=1)


def tri_lower(p, dg):
    return np.stack([np.where(lanes(tri_mask(s, 1)), dg, np.where(lanes(tri_mask(s, 2)), p[:, s], 0.0)) for s in range(4)], axis=1)


def pstream_pair(q):
    pp = 0
    while 2 * (pp + 1) * (pp + 1) <= q:
        pp += 1
    return pp


def decode(q):
    """position -> ("pair", pp) | ("tile", kk, t, closes_even_column)"""
    pp = pstream_pair(q)
    i = q - 2 * pp * pp
    if i == 2 * pp:
        return ("pair", pp)
    kk, t = (2 * pp, i) if i < 2 * pp else (2 * pp + 1, i - 2 * pp - 1)
    return ("tile", kk, t, i == 4 * pp + 1)


def test_masks_partition_the_image():
    seen_diag = 0
    for s in range(4):
        up, dg, lo = tri_mask(s, 0), tri_mask(s, 1), tri_mask(s, 2)
        assert up | lo == (1 << 64) - 1 and up & lo == 0 and dg & up == dg
        seen_diag += bin(dg).count("1")
        # the diagonal of register s: lanes 16 g + g + 4 s
        assert dg == sum(1 << (16 * g + g + 4 * s) for g in range(4))
    assert seen_diag == 16
    assert sum(bin(tri_mask(s, 2)).count("1") for s in range(4)) == 120


def test_pack_and_unpack_two_triangles():
    rng = np.random.default_rng(1)
    A = np.tril(rng.normal(size=(16, 16)))        # two L^-1
    B = np.tril(rng.normal(size=(16, 16)))
    la, lb = lds_image_of(A), lds_image_of(B)
    up, lo = img_load_t(la), img_load_tr(lb)
    assert np.array_equal(up, image_of(A.T))
    J = np.eye(16)[::-1]
    assert np.array_equal(lo, image_of(J @ B.T @ J))
    dgl = np.array([lb[img_rc(15 - i, 15 - i)] for i in range(16)])
    pk = tri_pack(up, lo)
    assert np.array_equal(tri_upper(pk), up)
    assert np.array_equal(tri_lower(pk, dgl[LR]), lo)


def test_stream_positions():
    for NP in (16, 32):
        slen = NP * NP // 2
        assert pstream_pair(slen - 1) == NP // 2 - 1 and pstream_pair(slen) == NP // 2
        kinds = [decode(q) for q in range(slen)]
        assert sum(1 for k in kinds if k[0] == "pair") == NP // 2
        tiles = [(k[1], k[2]) for k in kinds if k[0] == "tile"]
        assert sorted(tiles) == [(kk, t) for kk in range(NP) for t in range(kk)]
        # the pair's image stands between the tiles of its two columns, and the even column closes behind its last tile
        for q, k in enumerate(kinds):
            if k[0] == "pair":
                pp = k[1]
                assert all(kinds[q - 1 - t] == ("tile", 2 * pp, 2 * pp - 1 - t, False) for t in range(2 * pp))
                assert all(kinds[q + 1 + t][:3] == ("tile", 2 * pp + 1, t) for t in range(2 * pp + 1))
                assert kinds[q + 2 * pp + 1][3] and not any(kinds[q + 1 + t][3] for t in range(2 * pp))


def close(zv, wsc_from, k, img, has_w, rev):
    """bw_close: alpha_k = M (z_k - w_k) as four MFMAs; REV: img is the image of J M J, right-hand side and result index-reversed."""
    ub = np.zeros((64, 4))
    for q4 in range(4):
        e = LG + 4 * q4
        e = 15 - e if rev else e
        u = zv[16 * k + e] - (wsc_from[e] if has_w else 0.0)
        ub[:, q4] = np.where(LR == 0, u, 0.0)
    D = np.zeros((64, 4))
    for s in range(4):
        D = mfma(img[:, s], ub[:, s], D)
    for r in range(4):
        e = LG + 4 * r
        e = 15 - e if rev else e
        sel = LR == 0
        zv[16 * k + e[sel]] = D[sel, r]


def run_stream(nt, NP, seed):
    rng = np.random.default_rng(seed)
    n = 16 * nt
    L = np.tril(rng.normal(size=(n, n))) * (0.3 / np.sqrt(n))       # (rows of unit-order weight: L^-T stays well conditioned at n = 512)
    L[np.arange(n), np.arange(n)] = rng.uniform(1.0, 2.0, n)
    z = rng.normal(size=n)
    want = np.linalg.solve(L.T, z)
    tile = {(i, j): image_of(L[16 * i:16 * i + 16, 16 * j:16 * j + 16]) for i in range(nt) for j in range(i)}
    linv = [lds_image_of(np.linalg.inv(L[16 * k:16 * k + 16, 16 * k:16 * k + 16])) for k in range(nt)]
    # ---- the factorization's side: every step but the last writes its two packed images and their diagonals ----
    poison = np.full(256, np.nan)
    pairs, dgl = {}, {}
    LinvC = [poison.copy() for _ in range(W1_C)]
    for k in range(0, nt, W1_C):
        nc = min(W1_C, nt - k)
        LinvC = [linv[k + c] if c < nc else poison.copy() for c in range(W1_C)]      # (what the last step leaves behind)
        if k + W1_C < nt:
            for h in range(2):
                lo_img = LinvC[2 * h + 1]
                pairs[(k >> 1) + h] = tri_pack(img_load_t(LinvC[2 * h]), img_load_tr(lo_img))
                dgl[(k >> 1) + h] = np.array([lo_img[img_rc(15 - i, 15 - i)] for i in range(16)])
    # ---- the stream ----
    nte, kls = (nt + 1) & ~1, (nt - 1) & ~(W1_C - 1)
    zv = z.copy()
    requested = []

    def fetch(q):
        d = decode(q)
        if d[0] == "pair":
            k = nte - 1 - 2 * d[1]
            if k >= 1 and k - 1 < kls:
                requested.append(("pair", k >> 1))
                return pairs[k >> 1]
            return None
        k = nte - 1 - d[1]
        if k >= 0 and k + 1 + d[2] < nt:
            requested.append(("tile", k + 1 + d[2], k))
            return tile[(k + 1 + d[2], k)]
        return None

    pa = np.zeros((64, 4))
    held = None

    def wsc(pa):
        w = np.zeros(16)
        for s in range(4):
            for g in range(4):
                w[g + 4 * s] = pa[LG == g, s].sum()          # mf_row_reduce4: component (l >> 4) + 4 s summed over the row's 16 lanes
        return w

    for q in range(NP * NP // 2):
        img = fetch(q)
        d = decode(q)
        if d[0] == "pair":
            pp = d[1]
            k = nte - 1 - 2 * pp
            if k >= 1:
                in_lds = pp < W1_C // 2 and k - 1 >= kls
                if in_lds:
                    lo = img_load_tr(LinvC[k - kls])
                else:
                    held = lds_image_of(np.zeros((16, 16)))
                    held[IMG_LS] = tri_upper(img)                     # (parked in LinvC's last image)
                    assert pp >= W1_C // 2 or k - kls < W1_C - 1      # ... which no pair still to come reads
                    lo = tri_lower(img, dgl[k >> 1][LR])
                if k < nt:
                    close(zv, wsc(pa), k, lo, pp > 0, True)
                    pa[:] = 0.0
        else:
            _, kk, t, closes = d
            k = nte - 1 - kk
            if k >= 0 and k + 1 + t < nt:
                pa += img * zv[16 * (k + 1 + t) + LR][:, None]
            if closes and k >= 0:
                in_lds = (kk >> 1) < W1_C // 2 and k >= kls
                up = img_load_t(LinvC[k - kls]) if in_lds else held[IMG_LS]
                close(zv, wsc(pa), k, up, True, False)
                pa[:] = 0.0
    return zv, want, requested, kls


@pytest.mark.parametrize("NP", [16, 32])
def test_stream_solves_the_triangular_system_at_every_tile_count(NP):
    for nt in range(1, NP + 1):
        got, want, requested, kls = run_stream(nt, NP, seed=100 + nt)
        assert np.all(np.isfinite(got)), nt
        assert np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want)), nt      # two fp64 solves; a wrong lane or position is O(1)
        # every off-diagonal tile once, every pair of a step before the last once, nothing twice
        assert len(set(requested)) == len(requested)
        assert sorted(r for r in requested if r[0] == "tile") == sorted(("tile", i, j) for i in range(nt) for j in range(i))
        assert sorted(r[1] for r in requested if r[0] == "pair") == list(range(kls // 2))
