"""The bounds cases of the explicit and Jacobi layers' input backward (tests/bounds_input_explicit_cases.py) against the
header that declares their entry points (include/pdecnn_explicit_input.h, included by pdecnn.h), on the CPU.  The cases are
not part of the table of tests/bounds_cases.py; the checks tests/test_bounds_cases.py applies to a case of that table are
applied to them here, with its own helpers: the header and ``_lib.SIGNATURES_EXPLICIT_INPUT`` name the same functions with
the same argument counts, every writing entry point of the new header has a case, every parameter is bound, roles fit
constness, element counts and alignments are the header's, ids are unique, the cases are small.  Beside that: every new
call gets a workspace of exactly the queried size (none where the query is 0), and the queries are smaller than the full
calls'."""
import os

import bounds_cases as BC
import bounds_input_explicit_cases as BE
import test_bounds_cases as TBC

HDR = BE.header_functions()
NEW = {f: ps for f, ps in HDR.items() if f not in BC.header_functions()}


def _built(case):
    ctx = BC.SpecCtx()
    calls, expect = case.build(ctx)
    return ctx, calls, expect


def test_the_new_header_declares_what_the_table_of_signatures_binds():
    from cnn_with_pde_amd import _lib
    assert '#include "pdecnn_explicit_input.h"' in open(os.path.join(BC.ROOT, "include", "pdecnn.h")).read()
    assert sorted(NEW) == sorted(_lib.SIGNATURES_EXPLICIT_INPUT) == sorted(BE.NEW_FUNCTIONS + BE.QUERIES)
    for f, ps in NEW.items():
        assert len(ps) == len(_lib.SIGNATURES_EXPLICIT_INPUT[f][1]), f
    assert not set(_lib.SIGNATURES_EXPLICIT_INPUT) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SMALL_INPUT) |
                                                      set(_lib.SIGNATURES_MIXED_INPUT))
    lib = _lib.load()
    for f in _lib.SIGNATURES_EXPLICIT_INPUT:
        assert getattr(lib, f).argtypes == _lib.SIGNATURES_EXPLICIT_INPUT[f][1], f


def test_every_writing_entry_point_of_the_new_header_has_a_case():
    writing = sorted(f for f, ps in NEW.items() if any((ptr and not const) or "workspace" in name for name, ptr, const in ps))
    assert writing == sorted(BE.NEW_FUNCTIONS)
    called = {fn for c in BE.CASES for fn, _ in _built(c)[1]}
    assert set(writing) <= called, set(writing) - called
    assert sorted(set(NEW) - set(writing)) == sorted(BE.QUERIES)


def test_ids_are_unique_and_not_the_tables():
    ids = [c.id for c in BE.CASES]
    assert len(ids) == len(set(ids)) and not set(ids) & {c.id for c in BC.CASES}
    assert all(c.switch is None for c in BE.CASES)


def test_every_parameter_is_bound_and_roles_fit_constness():
    for c in BE.CASES:
        ctx, calls, expect = _built(c)
        written = set()
        for fn, amap in calls:
            params = HDR[fn]
            assert not set(amap) - {n for n, _, _ in params}, (c.id, fn)
            args = BC.call_args(ctx, params, amap)              # KeyError: a parameter without a binding
            assert len(args) == len(params)
            for pname, buf, const in BC.bound_buffers(ctx, params, amap):
                role = ctx.roles[buf]
                if const:
                    assert role == "in" or buf in written or role in ("inout", "carry", "ws"), (c.id, fn, pname, buf, role)
                else:
                    assert role != "in", f"{c.id}: {fn} may write {pname}, bound to the input {buf}"
                    written.add(buf)
        for name, role in ctx.roles.items():
            if role in ("out", "ws", "carry", "inout"):
                assert name in written, f"{c.id}: {role} buffer {name} is handed to no writable parameter"


def test_the_new_calls_take_no_u_no_states_and_no_parameter_gradients():
    for f in BE.NEW_FUNCTIONS:
        names = {n for n, _, _ in NEW[f]}
        assert not names & {"u", "states", "g_alpha_base", "g_channel_scaling", "g_a_row", "g_b_col"}, (f, names)
        assert {"gout", "gu"} <= names
        assert ("emit_mask" in names) == f.endswith("_states"), f
    for c in BE.CASES:
        ctx, calls, _ = _built(c)
        fn, amap = calls[-1]
        assert fn in BE.NEW_FUNCTIONS and len(calls) == 3, c.id
        bound = {buf for _, buf, _ in BC.bound_buffers(ctx, HDR[fn], amap)}
        assert not bound & {"u", "states", "out", "gu", "g_alpha_base", "g_channel_scaling", "g_a_row", "g_b_col"}, (c.id, bound)


def test_element_counts_dtypes_and_sizes_are_the_headers():
    for c in BE.CASES:
        ctx = _built(c)[0]
        for name, want in TBC._header_counts(c, ctx).items():
            assert TBC._numel(ctx, name) == want, (c.id, name, ctx.shapes[name], want)
        for mine, full in BE.twins(c):
            assert ctx.roles[mine] == "out" and ctx.shapes[mine] == ctx.shapes[full] and ctx.dtypes[mine] == ctx.dtypes[full], \
                (c.id, mine, full)
        assert BE.twins(c)
        assert sum(ctx.nbytes(n) for n in ctx.roles) < 96 << 20


def test_the_alignment_of_every_buffer_is_the_headers():
    seen = 0
    for c in BE.CASES:
        ctx, calls, _ = _built(c)
        assert set(ctx.aligns) == set(ctx.roles)
        for fn, amap in calls:
            for pname, buf, _ in BC.bound_buffers(ctx, HDR[fn], amap):
                want = TBC._header_align(c, fn, pname, ctx.dtypes[buf])
                assert ctx.aligns[buf] == want, (c.id, fn, pname, buf, ctx.aligns[buf], want)
                seen += 1
    assert seen > 500


def test_the_requested_cases_are_there():
    """A case per dispatch, each plain and emitting: register planes, float4 columns, scalar columns, the one-workgroup
    Jacobi kernel, the tiled one over two launches, float64."""
    from cnn_with_pde_amd import _lib as L
    lib = BC.lib()
    ex = [c.p for c in BE.CASES if c.family == "explicit"]
    for name, pick in (("wave", lambda p: p["io"] != "f64" and (p["H"], p["W"]) in ((16, 16), (32, 32), (64, 64))),
                       ("float4", lambda p: p["io"] != "f64" and p["W"] % 4 == 0 and p["H"] != p["W"]),
                       ("column", lambda p: p["io"] != "f64" and p["W"] % 4 != 0),
                       ("float64", lambda p: p["io"] == "f64")):
        sel = [p for p in ex if pick(p)]
        assert any(p.get("emit") for p in sel) and any(not p.get("emit") for p in sel), name
    assert {(p["H"], p["W"]) for p in ex if p["io"] != "f64"} >= {(16, 16), (32, 32), (64, 64)}
    assert {p["io"] for p in ex} == set(BC.IO3) | {"f64"}
    jac = [c.p for c in BE.CASES if c.family == "jacobi"]
    for p in jac:
        assert lib.pde_jacobi_plane_path(p["H"], p["W"]) == p["path"]
    for name, pick in (("one workgroup", lambda p: p["path"] == 1 and p["io"] != "f64"),
                       ("tiled, two launches", lambda p: p["path"] == 2 and p["nt"] > L.PDE_JACOBI_TILED_K),
                       ("float64", lambda p: p["io"] == "f64")):
        sel = [p for p in jac if pick(p)]
        assert any(p.get("emit") for p in sel) and any(not p.get("emit") for p in sel), name
    assert {p["io"] for p in jac} == set(BC.IO3) | {"f64"}


def test_the_new_calls_get_the_queried_workspaces():
    lib = BC.lib()
    for c in BE.CASES:
        ctx, calls, _ = _built(c)
        fn, a = calls[-1]
        p = c.p
        if c.family == "jacobi" and p["api"].startswith("f64"):
            assert "workspace" not in a and "iws" not in ctx.roles, c.id
            continue
        n = BE.query(c)
        assert a["workspace_bytes"] == n and (a["workspace"] is None) == (n == 0) and ("iws" in ctx.roles) == (n > 0), c.id
        if n:
            assert ctx.shapes["iws"] == (n,)
        if c.family == "explicit":
            f64 = p["io"] == "f64"
            wave = not f64 and (p["H"], p["W"]) in ((16, 16), (32, 32), (64, 64))
            one = -(-(p["B"] * p["C"] * p["H"] * p["W"] * (8 if f64 else 4)) // 256) * 256
            assert n == (0 if wave or p["nt"] == 1 else 2 * one), (c.id, n)        # 0 for register planes and for one step
            full = ctx.shapes["ws"][0]
        else:
            img = -(-(p["B"] * (p["H"] + 2) * (p["W"] + 2) * 4) // 256) * 256
            assert n == (0 if p["path"] == 1 else 2 * img), (c.id, n)              # 0 on plane path 1, two padded images on path 2
            full = ctx.shapes["bws"][0]
        assert n < full, (c.id, n, full)


def test_the_queries_answer_zero_for_what_they_refuse():
    from cnn_with_pde_amd import _lib as L
    lib = BC.lib()
    assert lib.pde_explicit5_backward_input_workspace_bytes(0, 2, 5, 7, L.PDE_IO_F32, 3) == 0
    assert lib.pde_explicit5_backward_input_workspace_bytes(2, 2, 5, 0, L.PDE_IO_F32, 3) == 0
    assert lib.pde_explicit5_f64_backward_input_workspace_bytes(2, 2, 0, 7, 3) == 0
    assert lib.pde_jacobi_io_backward_input_workspace_bytes(2, 65, 8, 3, 7) == 0                 # no such tensor type
    assert lib.pde_jacobi_io_backward_input_workspace_bytes(0, 65, 8, 3, L.PDE_IO_F32) == 0
    assert lib.pde_jacobi_io_backward_input_workspace_bytes(2, 65, L.PDE_JACOBI_MAX_HW + 1, 3, L.PDE_IO_F32) == 0
    assert lib.pde_jacobi_io_backward_input_workspace_bytes(2, 65, 3, 3, L.PDE_IO_F32) == 0      # W < 4: not served
