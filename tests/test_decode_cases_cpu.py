"""The cases of the masked decoder are what they claim, and the libraries export its entries -- without a GPU (tests/decode_cases.py)."""
import numpy as np
import pytest

import decode_cases as DC


@pytest.mark.parametrize("sz", DC.SIZES + (DC.SZ_GLOBAL_ROW,))
def test_patterns_have_the_counts_they_claim(sz):
    m = sz * sz
    names = DC.patterns_for(m)
    assert {"all", "none", "first", "last", "checker", "half", "last_block", "row_gx0"} <= set(names)
    for k in (63, 64, 65):
        assert (f"k{k}" in names) == (m >= k)
    for name in names:
        k = DC.pattern(name, sz, seed=1)
        assert k.shape == (m,) and k.dtype == bool
        claim = DC.claimed_count(name, m, sz)
        if claim is not None:
            assert int(k.sum()) == claim, (name, sz)
    # the counts the block structure of the emit kernel turns on are all there where the grid can hold them
    have = {int(DC.pattern(n, sz, seed=1).sum()) for n in names}
    assert {0, 1, m} <= have and {k for k in (63, 64, 65) if k <= m} <= have
    if m > 64:
        lb = DC.pattern("last_block", sz, seed=1)
        assert not lb[:64 * ((m - 1) // 64)].any() and lb[64 * ((m - 1) // 64):].all()


@pytest.mark.parametrize("sz", [s for s in DC.SIZES if s > 1])
def test_row_pattern_tells_the_transposition(sz):
    """A decoder that reads W[L, p] where it should read W[L, c(p)] keeps another set under `row gx = 0 only`."""
    m = sz * sz
    k = DC.pattern("row_gx0", sz, seed=1)
    assert np.array_equal(np.flatnonzero(k), np.arange(0, m, sz))
    W = DC.to_cells(k, sz).astype(np.uint8)[None, :]
    assert np.array_equal(np.flatnonzero(W[0]), np.arange(sz))             # the cells sz * 0 + gy: the first sz of the row
    right = DC.kept(np.array([1]), sz, W)[0]
    wrong = W[0] != 0                                                      # the same bytes read without the transposition
    assert np.array_equal(right, k) and not np.array_equal(right, wrong)
    assert right.sum() == wrong.sum() == sz                                # ... with the same count: only the order of the set tells


def test_cell_function_is_a_transposition():
    for sz in DC.SIZES:
        c = DC.cell_of(np.arange(sz * sz), sz)
        assert sorted(c) == list(range(sz * sz))
        assert np.array_equal(DC.cell_of(c, sz), np.arange(sz * sz))       # its own inverse
        g = np.arange(sz * sz).reshape(sz, sz)
        assert np.array_equal(g.T.reshape(-1), c)


@pytest.mark.parametrize("kind", DC.MASK_KINDS)
def test_masks_and_rule(kind):
    P, sz = 19, 9
    m = sz * sz
    b = np.arange(P) % 4                                                   # every fourth leaf is not decoded
    W, cells = DC.masks(P, sz, kind, rot=2)
    names = DC.leaf_patterns(P, sz, 2)
    assert set(names) == set(DC.patterns_for(m))                           # 19 leaves carry every pattern
    if W is not None:
        assert set(np.unique(W)) == {0, 1, 255}
    if cells is not None:
        assert set(np.unique(cells)) == {DC.CELL_UNOBSERVED, DC.CELL_OCCUPIED, DC.CELL_FREE}
    leaf, point, count, n = DC.rule(b, sz, W, cells)
    assert n == len(leaf) == len(point) == count.sum() and np.all(count[b == 0] == 0)
    key = leaf.astype(np.int64) * m + point
    assert np.all(np.diff(key) > 0)                                        # ascending (L, p), no point twice
    for i in range(P):
        want = DC.pattern(names[i], sz, 11 + i)
        if kind == "both":
            want = want & DC.pattern(DC.leaf_patterns(P, sz, 7)[i], sz, 11 + i)
        got = np.zeros(m, dtype=bool)
        got[point[leaf == i]] = True
        assert np.array_equal(got, want if b[i] > 0 else np.zeros(m, dtype=bool)), (i, names[i])
    # no mask keeps every point of every decoded leaf
    assert DC.rule(b, sz)[3] == m * int(np.sum(b > 0))


def test_pairs_and_scan_cases():
    for name in DC.PAIRS:
        Bd, Bc = DC.pair(name)
        assert Bd["ny"] == 1 and (Bc is None or (Bc["ny"] == 3 and Bc["P"] == Bd["P"]))
    Bd, Bc = DC.pair("cap100-reversed")
    full = int(np.argmax(Bd["b"]))
    assert Bd["b"][full] > 100 and Bc["b"][full] == 0                      # an empty colour basis under a full depth basis
    assert Bd["b"][0] == 0 and Bc["b"][0] > 100                            # ... and the reverse
    # either side of every step of the scan's segment length
    per = lambda P: (P + DC.SCAN_THREADS - 1) // DC.SCAN_THREADS
    for k in (1, 2):
        assert k * DC.SCAN_THREADS in DC.SCAN_P and k * DC.SCAN_THREADS + 1 in DC.SCAN_P
        assert per(k * DC.SCAN_THREADS) == k and per(k * DC.SCAN_THREADS + 1) == k + 1
    assert DC.SZ_GLOBAL_ROW ** 2 > DC.ROW_LDS_MAX >= (DC.SZ_GLOBAL_ROW - 1) ** 2


def test_libraries_export_the_decoder():
    from gp_compressor_amd import capi, host_api
    hip = capi.load()
    for name in ("gpc_sparse_decode", "gpc_sparse_decode_dev"):
        assert name in capi.PROTOTYPES and hasattr(hip, name), name
    assert hasattr(host_api.load(), "gpc_host_load_compressed_masked")
