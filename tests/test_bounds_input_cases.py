"""The bounds cases of the backward for the input alone (tests/bounds_input_cases.py) against include/pdecnn.h, on the
CPU: registered into the case table of tests/bounds_cases.py while the suite is collected, so that
tests/test_bounds_cases.py checks them with every other case; here: every new entry point has a case, each case ends in
the call it is named after with a workspace of exactly the queried size, and the table's own cases are what they were."""
import ctypes as C

import bounds_cases as BC
import bounds_input_cases as BI

BI.register()
HDR = BC.header_functions()


def _built(case):
    ctx = BC.SpecCtx()
    calls, expect = case.build(ctx)
    return ctx, calls, expect


def test_registered_once_and_the_old_cases_stay():
    ids = [c.id for c in BC.CASES]
    assert len(ids) == len(set(ids))
    BI.register()
    assert [c.id for c in BC.CASES] == ids
    old = [c for c in BC.CASES if not isinstance(c, BI.InputCase)]
    assert len(old) == len(ids) - len(BI.TABLE_CASES) and not any(c.p.get("input") for c in old)
    assert all(BC.BY_ID[c.id] is c for c in BI.TABLE_CASES)


def test_every_new_entry_point_has_a_case_in_the_table():
    writing = BC.writing_functions()
    called = {fn for c in BC.CASES for fn, _ in _built(c)[1]}
    for f in BI.NEW_FUNCTIONS:
        assert f in writing and f in called, f
    assert not [f for f in writing if f not in called and f not in BC.EXCLUDED]
    every = {fn for c in BI.MATRIX_CASES for fn, _ in _built(c)[1]}
    assert set(BI.NEW_FUNCTIONS) <= every


def test_cases_end_in_the_input_backward_with_the_queried_workspace():
    lib = BC.lib()
    for c in BI.TABLE_CASES + BI.MATRIX_CASES:
        ctx, calls, expect = _built(c)
        fam = BC._adi_fam(c.p)
        fn, amap = calls[-1]
        assert fn == fam + "backward_input" + ("_states" if c.p.get("emit") else ""), c.id
        assert amap["fwd_workspace"] == ("fws" if c.p.get("reuse", True) else None), c.id
        d = ctx.values["d"]
        assert ctx.shapes["iws"] == (getattr(lib, fam + "backward_input_workspace_bytes")(C.byref(d)),), c.id
        assert ctx.roles["gu_input"] == "out" and ctx.shapes["gu_input"] == ctx.shapes["gu"] and ctx.dtypes["gu_input"] == ctx.dtypes["gu"]
        args = BC.call_args(ctx, HDR[fn], amap)                  # KeyError: a parameter of the header without a binding
        assert len(args) == len(HDR[fn])
        for f, a, want in expect:
            assert getattr(lib, f)(*a) == want, (c.id, f, want)
