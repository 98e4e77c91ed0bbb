"""Coverage bookkeeping of the planner stage tests (CPU): every tconv instantiation with a planner mode (K5 / DOWN / UP / P1) that
csrc/tconv_*.hip builds has an entry in tests/planner_stage_coverage.py -- the case of tests/planner_stage_cases.py that reaches it, or the
reason why one U-Net evaluation cannot.  tests/test_hip_planner_stages.py asserts on the GPU that the named cases do reach them."""
from tests import planner_stage_cases as PC
from tests.planner_stage_coverage import COVERAGE, REACHED, UNREACHED


def test_every_planner_instantiation_has_an_entry():
    inst = PC.instantiations()
    assert len(inst) >= 100, f"the instantiation lists were not read: {len(inst)} rows"
    missing = [f"{PC.plan_text(k)} ({inst[k]})" for k in sorted(inst) if k not in COVERAGE]
    stale = [PC.plan_text(k) for k in sorted(COVERAGE) if k not in inst]
    assert not missing, "instantiations without a case or a reason in tests/planner_stage_coverage.py:\n  " + "\n  ".join(missing)
    assert not stale, "entries for instantiations that are no longer built:\n  " + "\n  ".join(stale)


def test_entries_name_a_case_or_give_a_reason():
    ids = {PC.case_id(c) for c in PC.all_cases()}
    for k, (how, what) in COVERAGE.items():
        assert how in (REACHED, UNREACHED), (k, how)
        if how == REACHED:
            assert what in ids, f"{PC.plan_text(k)}: no case {what!r}"
        else:
            assert isinstance(what, str) and len(what) > 20 and "\n" not in what, f"{PC.plan_text(k)}: one line of reason, got {what!r}"


def test_the_lists_hold_every_mode_and_form():
    """The reader of the lists sees what the issue counts: the four planner modes, one and two row blocks, the K-split copies and all five
    arithmetic forms (split 0 .. 4)."""
    inst = PC.instantiations()
    assert {k[0] for k in inst} == {0, 1, 2, 3}
    assert {k[8] for k in inst} == {0, 1, 2, 3, 4} and {k[6] for k in inst} == {1, 2} and {k[7] for k in inst} == {0, 1}


def test_cases_are_unique_and_options_known():
    cases = PC.all_cases()
    assert len({PC.case_id(c) for c in cases}) == len(cases)
    for B in (49, 300, 1030, 1043):
        rows = PC.ref_rows(B)
        assert len(rows) <= 48 and {0, 15, 16, 31, 32, B - 1, (B - 1) // 16 * 16, (B - 1) // 32 * 32} <= set(rows)
        assert all(any(e * B // 8 <= r < (e + 1) * B // 8 for r in rows) for e in range(8))
    x, k, c = PC.inputs("t8", 7)
    x2, k2, c2 = PC.inputs("t8", 3, first=4)
    assert (x[4:] == x2).all() and (k[4:] == k2).all() and (c[4:] == c2).all()          # row n by (seed, n) only
    assert int(k[0]) == 0 and int(k[1]) == 99
    assert float((x[2] - x[2].mean(0)).abs().max()) < 1e-2 and float(x[1].abs().max()) <= 1.0
