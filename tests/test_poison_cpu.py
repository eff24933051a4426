"""The table of the poison runs (poison_cases.py) against include/gpc.h, without a GPU: every entry that enqueues work on the device --
every gpc_*_dev function, and the object calls gpc_sparse_remap, gpc_registration_step and gpc_registration_run -- is named by a case of
tests/test_poison_gpu.py, by a test elsewhere that runs it under GPC_POISON_LDS, or by an exemption with its reason.  An entry added to
the header without one of the three fails here."""
import os
import re

import poison_cases as PC
from gpc_header import OBJECT_CALLS, ROOT, declared as _declared, launching as _launching      # noqa: F401

TESTS = os.path.join(ROOT, "tests")


def _uncovered(declared, cased, covered, exempt):
    return sorted(_launching(declared) - set(cased) - set(covered) - set(exempt))


def test_every_launching_entry_has_a_case_a_test_or_an_exemption():
    assert _uncovered(_declared(), PC.entries_with_a_case(), PC.COVERED_ELSEWHERE, PC.EXEMPT) == []


def test_an_entry_without_a_record_is_found():
    """the check above can fail: an entry the header gains, and an entry whose case is taken out of the table, are reported by name"""
    declared = _declared()
    assert _uncovered(declared | {"gpc_new_kernel_dev"}, PC.entries_with_a_case(), PC.COVERED_ELSEWHERE, PC.EXEMPT) == ["gpc_new_kernel_dev"]
    cased = PC.entries_with_a_case() - {"gpc_reproject_dev"}
    assert _uncovered(declared, cased, PC.COVERED_ELSEWHERE, PC.EXEMPT) == ["gpc_reproject_dev"]


def test_records_name_only_what_the_header_declares():
    declared = _declared()
    for what, names in (("case", PC.entries_with_a_case()), ("covered elsewhere", PC.COVERED_ELSEWHERE), ("exempt", PC.EXEMPT)):
        assert set(names) <= declared, (what, sorted(set(names) - declared))
    assert not set(PC.COVERED_ELSEWHERE) & set(PC.EXEMPT)
    assert not (set(PC.COVERED_ELSEWHERE) | set(PC.EXEMPT)) & PC.entries_with_a_case()
    assert all(isinstance(r, str) and len(r) > 20 for r in PC.EXEMPT.values())


def _sets_the_switch(path, test):
    """the named test exists in the file, and its own body switches the poison on"""
    src = open(path).read()
    m = re.search(r"^def %s\(.*?(?=^(?:def |@pytest|class |# ----)|\Z)" % re.escape(test), src, flags=re.S | re.M)
    return bool(m) and re.search(r"""setenv\(\s*(?:"GPC_POISON_LDS"|env)\s*,""", m.group(0)) is not None and "GPC_POISON_LDS" in m.group(0)


def test_covered_elsewhere_points_at_tests_that_set_the_switch():
    for entry, (fname, test) in PC.COVERED_ELSEWHERE.items():
        assert _sets_the_switch(os.path.join(TESTS, fname), test), (entry, fname, test)
    # ... and the check can fail: a test that exists without the switch, and a test that does not exist
    assert not _sets_the_switch(os.path.join(TESTS, "test_quantize_gpu.py"), "test_dequantize")
    assert not _sets_the_switch(os.path.join(TESTS, "test_quantize_gpu.py"), "test_no_such_test")


def test_case_ids_are_unique_and_rules_are_known():
    ids = [c.id for c in PC.CASES]
    assert len(ids) == len(set(ids))
    for c in PC.CASES:
        assert c.rule in ("bits", "RUN_TOL") and c.entries and c.note and callable(c.run), c.id
        # the one tolerance goes with the one kernel whose sums meet in arrival order
        if c.rule == "RUN_TOL":
            assert c.id.startswith("dense-") and ("_nt" in c.note or "register kernel" in c.note), c.id
    import test_dense_ev_gpu
    assert test_dense_ev_gpu.RUN_TOL == 1e-12


def test_every_switch_of_a_case_is_in_designs_switch_table():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = re.search(r"^## [0-9a-z]+\. Switches\n(.*?)(?=^## )", design, flags=re.S | re.M)          # (as test_capi_cpu.py parses it)
    assert sec, "DESIGN.md has no section \"Switches\""
    rows = re.findall(r"^\| `(GPC_[A-Z0-9_]+)` \| [^|]* \| ([^|]*) \|", sec.group(1), flags=re.M)
    table = dict(rows)
    assert len(table) > 20
    used = {k for c in PC.CASES for k in c.env} | {PC.POISON}
    assert used <= set(table), sorted(used - set(table))
    assert set(PC.SWITCHES) <= set(table), sorted(set(PC.SWITCHES) - set(table))
    assert all(k in PC.SWITCHES for k in used)
    assert "tests/test_poison_gpu.py" in table[PC.POISON]


def test_every_dense_route_and_every_sparse_add_switch_has_a_case():
    import dense_accuracy_cases as DA
    import test_dense_accuracy_gpu as TA
    ids = {c.id for c in PC.CASES}
    for route in TA.ROUTES:
        for family in DA.FAMILIES:
            for ny in (1, 3):
                assert "dense-mean-%s-%s-ny%d" % (route, family, ny) in ids
    by_id = {c.id: c for c in PC.CASES}
    for route, env in TA.ROUTES.items():
        assert by_id["dense-mean-%s-n256-ny1" % route].env == env
    add_envs = [c.env for c in PC.CASES if c.id.startswith("sparse-add-")]
    assert {} in add_envs
    for sw in ("NO_SMALL", "WIDE", "RES", "FULL", "NO_FUSE", "NO_LIST", "NO_ROWS", "NO_ROWS2", "NO_MID"):
        assert {"GPC_SPARSE_" + sw: "1"} in add_envs, sw
