"""The table of the stream-order runs (stream_cases.py) against include/gpc.h, without a GPU: every entry that enqueues work on the device
-- every gpc_*_dev function, and the object calls gpc_sparse_remap, gpc_registration_step and gpc_registration_run -- is named by a case of
tests/test_stream_order_gpu.py, or is one of the two entries that launch nothing.  An entry added to the header without a case fails
here."""
import os
import re

import numpy as np

import stream_cases as SC
from gpc_header import OBJECT_CALLS, ROOT, comment_of as _comment_of, declared as _declared, launching as _launching


def _uncovered(declared, cased, exempt):
    return sorted(_launching(declared) - set(cased) - set(exempt))


def test_every_launching_entry_has_a_case_or_an_exemption():
    assert _uncovered(_declared(), SC.entries_with_a_case(), SC.EXEMPT) == []


def test_an_entry_without_a_record_is_found():
    """the check above can fail: an entry the header gains, and an entry whose case is taken out of the table, are reported by name"""
    declared = _declared()
    assert _uncovered(declared | {"gpc_new_kernel_dev"}, SC.entries_with_a_case(), SC.EXEMPT) == ["gpc_new_kernel_dev"]
    for gone in ("gpc_reproject_dev", "gpc_sparse_prune_dev", "gpc_registration_step"):
        assert _uncovered(declared, SC.entries_with_a_case() - {gone}, SC.EXEMPT) == [gone]


def test_records_name_only_what_the_header_declares():
    declared = _declared()
    for what, names in (("case", SC.entries_with_a_case()), ("exempt", SC.EXEMPT)):
        assert set(names) <= declared, (what, sorted(set(names) - declared))
    assert not set(SC.EXEMPT) & SC.entries_with_a_case()
    # an exemption is for an entry that launches nothing, and says so
    assert set(SC.EXEMPT) == {"gpc_patches_view_dev", "gpc_registration_cloud_dev"}
    assert all(r.startswith("launches nothing") for r in SC.EXEMPT.values())
    assert OBJECT_CALLS <= SC.entries_with_a_case()


def test_case_ids_are_unique_and_records_are_whole():
    ids = [c.id for c in SC.CASES]
    assert len(ids) == len(set(ids))
    for c in SC.CASES:
        assert c.rule in ("bits", "RUN_TOL") and c.entries and c.note and c.outputs, c.id
        assert callable(c.inputs) and callable(c.setup), c.id
        assert c.syncs is False or (isinstance(c.syncs, tuple) and c.syncs[0] is True and isinstance(c.syncs[1], int)), c.id
        # the one tolerance goes with the one kernel whose sums meet in arrival order
        if c.rule == "RUN_TOL":
            assert c.id.startswith("dense-") and "register" in c.note, c.id
        # a smaller share is an integer output's, and the note says why
        for k in c.share:
            assert k in c.outputs or k.split(".")[0] in c.outputs, (c.id, k)
            assert k.split(".")[-1] in c.note or k in c.note, (c.id, k)
    import test_dense_ev_gpu
    assert test_dense_ev_gpu.RUN_TOL == 1e-12


def test_every_switch_of_a_case_is_in_designs_switch_table():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = re.search(r"^## [0-9a-z]+\. Switches\n(.*?)(?=^## )", design, flags=re.S | re.M)          # (as test_capi_cpu.py parses it)
    assert sec, "DESIGN.md has no section \"Switches\""
    table = dict(re.findall(r"^\| `(GPC_[A-Z0-9_]+)` \| [^|]* \| ([^|]*) \|", sec.group(1), flags=re.M))
    used = {k for c in SC.CASES for k in c.env}
    assert used and used <= set(table), sorted(used - set(table))
    assert all(k in SC.SWITCHES for k in used)


def test_syncs_is_what_the_header_says():
    for c in SC.CASES:
        for e in c.entries:
            text, first, last = _comment_of(e)
            if c.syncs:
                assert re.search("synchronis", text, flags=re.I) and "never synchronises" not in text, (c.id, e)
                line = open(os.path.join(ROOT, "include", "gpc.h")).read().split("\n")[c.syncs[1] - 1]
                assert first <= c.syncs[1] <= last and re.search("synchronis", line, flags=re.I), (c.id, e, c.syncs[1], line)
    # ... the comment of an entry is found: these three say what the issue quotes
    assert "never synchronises" in _comment_of("gpc_sparse_prune_dev")[0]
    assert "SYNCHRONISES" in _comment_of("gpc_cloud_distortion_dev")[0]
    assert "call gpc_ctx_synchronize before switching" in re.sub(r"\s+\*?\s*", " ", _comment_of("gpc_ctx_set_stream")[0])
    # ... and an entry whose comment says "never synchronises" has no case that claims otherwise
    for c in SC.CASES:
        if c.syncs:
            assert all("never synchronises" not in _comment_of(e)[0] for e in c.entries), c.id


def test_the_decoy_changes_values_and_never_an_address():
    """both input sets have the same keys, shapes and types; every index array -- by name or by type -- is ONE object in both; at least one
    value array differs, in more than half of its elements"""
    for c in SC.CASES:
        real, decoy = c.inputs()
        assert SC.same_index_arrays(real, decoy, c.blind) is None, (c.id, SC.same_index_arrays(real, decoy, c.blind))
        if c.blind:                                            # no decoy can reach the entry, and the record says why
            assert isinstance(c.blind, str) and len(c.blind) > 20 and all(real[k] is decoy[k] for k in real), c.id
            continue
        rows = lambda a: a if (a.dtype == np.uint8 and a.ndim == 2) else np.ascontiguousarray(a).reshape(-1, 1)      # (32-byte records)
        shares = [np.mean(np.any(rows(real[k]) != rows(decoy[k]), axis=1)) for k in real if real[k] is not decoy[k]]
        assert max(shares) > 0.5, (c.id, shares)
    # ... and the check can fail: an index array that is an equal COPY, and a decoy that is the real set
    real, decoy = SC.CASES[0].inputs()
    assert "off" in SC.same_index_arrays(real, dict(decoy, off=real["off"].copy()))
    assert "blind" in SC.same_index_arrays(real, dict(real))


def test_the_forks_have_their_cases():
    ids = {c.id for c in SC.CASES}
    for want in ("dense-split-out-heavy", "dense-split-in-heavy", "sparse-predict-sigma-heavy-le16", "sparse-predict-sigma-heavy-17to32",
                 "sparse-predict-sigma-heavy-gt32", "sparse-predict-mean", "sparse-predict-sigma", "sparse-predict-sigma-regular", "sparse-predict-points",
                 "sparse-predict-scattered", "sparse-add-default", "sparse-add-no-rows", "reproject", "render-attrs", "dense-split-hinted",
                 "render", "render-counts"):
        assert want in ids, want
    for route in ("register", "one-wave", "tiled"):
        assert {"dense-%s-var" % route, "dense-%s-ev" % route, "dense-%s-select" % route} <= ids
    assert {"dense-generic-var", "dense-generic-ev"} <= ids
    # the split batches hold patches of all three size classes, the heavy class the most work; the heavy objects one patch in each
    # of the other two buckets
    by_id = {c.id: c for c in SC.CASES}
    for cid, heavy in (("dense-split-out-heavy", 2), ("dense-split-in-heavy", 1)):
        n = np.diff(by_id[cid].inputs()[0]["off"])
        cls = np.where(n <= 256, 0, np.where(n <= 272, 1, 2))
        work = [float(np.sum(n[cls == k].astype(np.float64) ** 3)) for k in range(3)]
        assert all(np.any(cls == k) for k in range(3)) and int(np.argmax(work)) == heavy and n.max() > 272 and n.min() == 0, (cid, work)
    for which, (heavy, one, two) in SC._HEAVY_B.items():
        bucket = lambda b: 0 if b <= 16 else 1 if b <= 32 else 2
        assert sorted(bucket(b) for b in (heavy, one, two)) == [0, 1, 2] and max(heavy, one, two) <= SC.HEAVY_CAP
