"""The CPU oracle alone on every case of dense_nonfinite_cases.py: it must show exactly the pattern test_dense_nonfinite_gpu.py demands of
the kernels -- the status, which entries are NaN, which non-finite, which zero or the prior -- and, where the pattern says "as in the
clean run", the BITS of the clean run.  So every condition of the GPU test is one the reference arithmetic meets itself (oracle/gpc_oracle.c
takes no special case: its pivot test is !(d > 0.0)), and the one place where the kernels' contract departs from it is recorded: an EMPTY
patch under a non-finite X*, where the oracle's v* is NaN (it evaluates k(x*, x*) = sf * exp(c |x* - x*|^2) there as everywhere) and
the kernels, which evaluate nothing for an empty patch, write the prior."""
import numpy as np
import pytest

import dense_nonfinite_cases as NF


def _bits_equal(a, b, mask):
    return np.array_equal(a[mask].view(np.uint64), b[mask].view(np.uint64))


def _oracle_failures(e, out, clean, has_v):
    """The shared pattern, the oracle's own NaN where the kernels owe the prior, and the bits of the clean run everywhere else"""
    bad = NF.pattern_failures(e, out, entry_has_v=has_v)
    if not _bits_equal(out["f"], clean["f"], e["f_clean"]):
        bad.append("f*: clean entries differ from the clean run")
    if not _bits_equal(out["al"], clean["al"], e["al_clean"]):
        bad.append("alpha: clean entries differ from the clean run")
    if has_v:
        if not _bits_equal(out["v"], clean["v"], e["v_clean"]):
            bad.append("v*: clean entries differ from the clean run")
        own_nan = e["v_prior_oracle_nan"]
        if not np.all(np.isnan(out["v"][own_nan])):
            bad.append("v*: the oracle's k(x*, x*) of a non-finite x* is not NaN")
        if not np.all(out["v"][e["v_prior"] & ~own_nan] == NF.REGIME[0]):
            bad.append("v*: a prior entry is not sigma_f^2")
    return bad


@pytest.mark.parametrize("family", list(NF.FAMILIES))
def test_oracle_shows_the_pattern_of_every_training_poison(oracle, family):
    failures = []
    for case in NF.train_cases():
        if case[0] != family:
            continue
        e = NF.expect(case)
        out, ran = NF.oracle_case(oracle, case)
        clean = NF.oracle_clean(oracle, case[0], case[1])
        assert ran == [case[4] - 1, case[4], case[4] + 1] and min(ran) >= 0     # a clean patch on either side was run with the poisoned one
        sizes = NF.FAMILIES[family]
        nt = [(sizes[i] + 15) // 16 for i in ran]
        assert nt[0] != nt[1] != nt[2] and min(nt) > 0, "the neighbours are clean patches of other tile counts than the poisoned one"
        for entry in ("grid", "pts"):
            for msg in _oracle_failures(e, out[entry], clean[entry], entry == "pts"):
                failures.append((NF.case_id(case), entry, msg))
    # (non-finite, not NaN, is the pattern of a y poison: an infinite y at the LAST point of a patch, or at its only one, leaves the
    # oracle's own alpha and f* with infinities -- nothing is left to cancel them against)
    assert not failures, failures


@pytest.mark.parametrize("family", ["n256", "n512"])
def test_oracle_whole_batch_agrees_with_the_three_patch_run(oracle, family):
    """oracle_case runs the poisoned patch with its two neighbours and takes the rest from the clean run: one whole-batch run per kind shows
    the same bits (the tiled family is left out: its 1024-point patch is a second of CPU per run and no other code path)"""
    for case in NF.train_cases():
        if case[0] == family and case[3] == "c":
            b, q = NF.poisoned(case)
            whole = NF._oracle_run(oracle, b, q, False)
            part = NF.oracle_case(oracle, case)[0]["pts"]
            for k in ("st", "f", "al", "v"):
                assert np.array_equal(whole[k], part[k], equal_nan=k != "st"), (NF.case_id(case), k)


@pytest.mark.parametrize("family", list(NF.FAMILIES))
def test_oracle_shows_the_pattern_of_every_xstar_poison(oracle, family):
    failures = []
    for case in NF.xs_cases():
        if case[0] != family:
            continue
        out, _ = NF.oracle_case(oracle, case)
        for msg in _oracle_failures(NF.expect(case), out["pts"], NF.oracle_clean(oracle, case[0], case[1])["pts"], True):
            failures.append((NF.case_id(case), msg))
    assert not failures, failures


def test_cases_cover_what_the_gpu_test_relies_on():
    cases = NF.train_cases()
    for fam, sizes in NF.FAMILIES.items():
        assert 0 in sizes and 1 in sizes and len(set(sizes)) == len(sizes)
        for ny in (1, 3):
            mine = [c for c in cases if c[0] == fam and c[1] == ny]
            assert {c[2] for c in mine} == set(NF.KINDS) and {c[3] for c in mine} >= {"a", "b", "c", "d"}
            for c in mine:
                n, pts = sizes[c[4]], c[5]
                if c[3] == "a":
                    assert max(pts) < 16
                elif c[3] == "b":
                    assert min(pts) >= 16 * ((n - 1) // 16) > 0
                elif c[3] in ("c", "c17"):
                    assert n % 16 and n - 1 in pts
                else:
                    assert n == 1
            if ny == 3:
                assert {c[6] for c in mine if c[2] in NF.Y_KINDS} == {0, 1, 2}
    assert sum(1024 == s for s in NF.FAMILIES["tiled"]) == 1
    cols = {p[2] for p in NF.XS_POISONS}
    assert any(c < 16 for c in cols) and any(c >= 16 * (NF.M_PTS // 16) for c in cols) and NF.M_PTS % 16
    assert {p[1] for p in NF.XS_POISONS if p[0] == "xs_nan"} == {0, 1}


@pytest.mark.parametrize("ny", [1, 3])
def test_oracle_on_the_stride_batch_and_its_successor_pairs(oracle, ny):
    (off, x0, x1, y), clean_b, kind, chan = NF.stride_batch(ny)
    n = np.diff(off)
    assert len(n) == NF.STRIDE_P and n.min() >= 17 and n.max() == 47 and not np.any(n % 16 == 0)
    assert abs(np.mean(kind >= 0) - 1.0 / 3.0) < 0.03 and all(abs(np.mean(kind == k) - 1.0 / 9.0) < 0.02 for k in range(3))
    q = NF.xstars()
    out, clean = NF._oracle_run(oracle, (off, x0, x1, y), q, False), NF._oracle_run(oracle, clean_b, q, False)
    assert np.all(clean["st"] == 0)
    bad = _oracle_failures(NF.stride_expect(ny, NF.M_PTS), out, clean, True)
    assert not bad, bad
    # every stride at which a launcher hands a workgroup, a slot or an LDS image on, in the layout the GPU test runs it in
    counts = {}
    for name, G in list(NF.GRIDS.items()) + [("GPC_W1_SLOTS=%d" % s, s) for s in NF.W1_SLOTS]:
        for chunks in (1, NF.STRIDE_CHUNKS):
            pairs = NF.successor_pairs(G, chunks, ny)
            counts[(name, chunks)] = len(pairs)
            if len(pairs):
                assert np.all(kind[pairs[:, 0]] >= 0) and np.all(kind[pairs[:, 1]] < 0) and np.all(n[pairs[:, 0]] > n[pairs[:, 1]])
    print(counts)
    for (name, chunks), k in counts.items():
        # in one chunk every stride has its pairs; in the pipeline's four chunks of 1050 patches a stride of 1024 leaves 26 candidates
        # per chunk, which is why the GPU test also runs the batch unchunked (GPC_HOST_NO_PIPELINE)
        if chunks == 1 or "1024" not in str(NF.GRIDS.get(name, "")):
            assert k >= NF.MIN_PAIRS, (name, chunks, k)
