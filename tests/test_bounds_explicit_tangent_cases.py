"""The bounds cases of the explicit and Jacobi layers' tangent-linear pass (tests/bounds_explicit_tangent_cases.py) against
the header that declares its entry points (include/pdecnn_explicit_tangent.h, included by pdecnn.h), on the CPU.  The cases
are not part of the table of tests/bounds_cases.py; the checks tests/test_bounds_cases.py applies to a case of that table
are applied to them here: the header and ``_lib.SIGNATURES_EXPLICIT_TANGENT`` name the same functions with the same
argument counts, every writing entry point of the new header has a case, every parameter is bound, roles fit constness,
element counts are the header's, every buffer sits at the alignment the header asks of its pointer in that call and every
workspace at 16 bytes, ids are unique, the cases are small.  Beside that: every call gets a workspace of exactly the
queried size (none where the query is 0), and the requested dispatches are all there."""
import os

import torch

import bounds_cases as BC
import bounds_explicit_tangent_cases as BX

HDR = BX.header_functions()
NEW = {f: ps for f, ps in HDR.items() if f not in BC.header_functions()}


def _built(case):
    ctx = BC.SpecCtx()
    calls, expect = case.build(ctx)
    return ctx, calls, expect


def test_the_new_header_declares_what_the_table_of_signatures_binds():
    from cnn_with_pde_amd import _lib
    assert '#include "pdecnn_explicit_tangent.h"' in open(os.path.join(BC.ROOT, "include", "pdecnn.h")).read()
    assert sorted(NEW) == sorted(_lib.SIGNATURES_EXPLICIT_TANGENT) == sorted(BX.NEW_FUNCTIONS + BX.QUERIES)
    for f, ps in NEW.items():
        assert len(ps) == len(_lib.SIGNATURES_EXPLICIT_TANGENT[f][1]), f
    assert not set(_lib.SIGNATURES_EXPLICIT_TANGENT) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SMALL_INPUT) |
                                                        set(_lib.SIGNATURES_MIXED_INPUT) |
                                                        set(_lib.SIGNATURES_EXPLICIT_INPUT) | set(_lib.SIGNATURES_TANGENT))
    lib = _lib.load()
    for f in _lib.SIGNATURES_EXPLICIT_TANGENT:
        assert getattr(lib, f).argtypes == _lib.SIGNATURES_EXPLICIT_TANGENT[f][1], f


def test_every_writing_entry_point_of_the_new_header_has_a_case():
    writing = sorted(f for f, ps in NEW.items() if any((ptr and not const) or "workspace" in name for name, ptr, const in ps))
    assert writing == sorted(BX.NEW_FUNCTIONS)
    called = {fn for c in BX.CASES for fn, _ in _built(c)[1]}
    assert set(writing) <= called, set(writing) - called
    assert sorted(set(NEW) - set(writing)) == sorted(BX.QUERIES)


def test_ids_are_unique_and_not_the_tables():
    ids = [c.id for c in BX.CASES]
    assert len(ids) == len(set(ids)) and not set(ids) & {c.id for c in BC.CASES}
    assert all(c.switch is None for c in BX.CASES)


def test_every_parameter_is_bound_and_roles_fit_constness():
    for c in BX.CASES:
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


def test_the_tangent_call_is_the_last_and_binds_what_the_case_says():
    for c in BX.CASES:
        ctx, calls, _ = _built(c)
        fn, amap = calls[-1]
        f64 = c.p["io"] == "f64"
        want = {"explicit": "pde_explicit5_f64_tangent" if f64 else "pde_explicit5_tangent",
                "jacobi": "pde_jacobi_f64_tangent" if f64 else "pde_jacobi_io_tangent"}[c.family]
        assert fn == want and fn in BX.NEW_FUNCTIONS and len(calls) == 2 and "forward" in calls[0][0], c.id
        with_du, given = BX.MODES[c.p["tan"]]
        names = BX.TANGENTS[c.family]
        bound = {p for p, _, _ in BC.bound_buffers(ctx, HDR[fn], amap)}
        assert ("du" in bound) == with_du and {k for k in names if k in bound} == {names[i] for i in given}, (c.id, bound)
        assert with_du or given, c.id                             # never all three NULL
        assert ("y" in bound) == (not c.p.get("no_y")) and "dy" in bound and "u" in bound, c.id
        outs = {buf for _, buf, const in BC.bound_buffers(ctx, HDR[fn], amap) if not const}
        ins = {buf for _, buf, const in BC.bound_buffers(ctx, HDR[fn], amap) if const}
        assert not outs & ins and "y_fwd" not in outs, c.id       # outputs overlap no input, and are the call's own


def test_element_counts_dtypes_and_sizes_are_the_headers():
    for c in BX.CASES:
        ctx = _built(c)[0]
        p = c.p
        io, kt = BC.IO[p["io"]][1], (torch.float64 if p["io"] == "f64" else torch.float32)
        if c.family == "explicit":
            n = p["B"] * p["C"] * p["H"] * p["W"]                 # u, du, y, dy: [B][C][H][W]; parameters: [C]
            want = dict(alpha_base=(p["C"], kt), channel_scaling=(p["C"], kt), d_alpha_base=(p["C"], kt),
                        d_channel_scaling=(p["C"], kt), states=((p["nt"] - 1) * n, kt))
        else:
            n = p["B"] * p["H"] * p["W"]                          # u, du, y, dy: [B][H][W]; a_row: [H], b_col: [W]
            want = dict(a_row=(p["H"], kt), d_a_row=(p["H"], kt), b_col=(p["W"], kt), d_b_col=(p["W"], kt))
        want.update(u=(n, io), du=(n, io), y=(n, io), dy=(n, io), y_fwd=(n, io))
        for name in ctx.roles:
            if ctx.dtypes[name] == torch.uint8:
                continue
            numel = 1
            for s in ctx.shapes[name]:
                numel *= s
            assert (numel, ctx.dtypes[name]) == want[name], (c.id, name, ctx.shapes[name], ctx.dtypes[name])
        for mine, full in BX.twins(c):
            assert ctx.roles[mine] == "out" and ctx.shapes[mine] == ctx.shapes[full] and ctx.dtypes[mine] == ctx.dtypes[full]
        assert sum(ctx.nbytes(n) for n in ctx.roles) < 96 << 20


def test_the_alignment_of_every_buffer_is_the_headers():
    """Four elements for u, du, y, dy of an explicit call whose W is a multiple of 4 (float64: never), the element for every
    other tensor and for every parameter vector, 16 bytes for the workspaces."""
    seen = 0
    for c in BX.CASES:
        ctx, calls, _ = _built(c)
        assert set(ctx.aligns) == set(ctx.roles)
        four = c.family == "explicit" and c.p["io"] != "f64" and c.p["W"] % 4 == 0
        for fn, amap in calls:
            for pname, buf, _ in BC.bound_buffers(ctx, HDR[fn], amap):
                item = torch.empty((), dtype=ctx.dtypes[buf]).element_size()
                if "workspace" in pname:
                    want = 16
                elif pname in ("u", "du", "y", "dy", "out", "states"):
                    want = 4 * item if four else item
                else:
                    want = item
                assert ctx.aligns[buf] == want, (c.id, fn, pname, buf, ctx.aligns[buf], want)
                seen += 1
    assert seen > 250


def test_the_requested_cases_are_there():
    from cnn_with_pde_amd import _lib as L
    lib = BC.lib()
    ex = [c.p for c in BX.CASES if c.family == "explicit"]
    for name, pick in (("wave", lambda p: p["io"] != "f64" and (p["H"], p["W"]) in BX.WAVE),
                       ("float4", lambda p: p["io"] != "f64" and p["W"] % 4 == 0 and (p["H"], p["W"]) not in BX.WAVE),
                       ("column", lambda p: p["io"] != "f64" and p["W"] % 4 != 0)):
        sel = [p for p in ex if pick(p)]
        assert {p["io"] for p in sel} == set(BC.IO3), name
        assert any(p["nt"] == 1 for p in sel) and any(p["nt"] > 2 for p in sel), name
    assert {(p["H"], p["W"]) for p in ex if p["io"] != "f64"} >= set(BX.WAVE)
    assert any(p["io"] == "f64" and p["nt"] == 1 for p in ex) and any(p["io"] == "f64" and p["nt"] > 1 for p in ex)
    jac = [c.p for c in BX.CASES if c.family == "jacobi"]
    K = L.PDE_JACOBI_TANGENT_TILED_K
    for p in jac:
        if p["io"] != "f64":
            assert lib.pde_jacobi_plane_path(p["H"], p["W"]) == p["path"]
    one = [p for p in jac if p["io"] != "f64" and p["path"] == 1]
    tiled = [p for p in jac if p["io"] != "f64" and p["path"] == 2]
    assert {p["io"] for p in one} == set(BC.IO3) and {p["io"] for p in tiled} == set(BC.IO3)
    assert (64, 64) in {(p["H"], p["W"]) for p in one} and any(p["nt"] == 0 for p in one)
    assert {K, K + 1} <= {p["nt"] for p in tiled} and any(p["nt"] > 2 * K for p in tiled)
    assert any(p["io"] == "f64" and (p["H"], p["W"]) == (64, 64) for p in jac)
    for fam in (ex, jac):
        assert {p["tan"] for p in fam} == set(BX.MODES)
        assert any(p.get("no_y") for p in fam)
    assert sum(1 for c in BX.CASES if BX.twins(c)) > len(BX.CASES) // 2


def test_the_calls_get_the_queried_workspaces():
    from cnn_with_pde_amd import _lib as L
    up = lambda n: -(-n // 256) * 256                                                                     # noqa: E731
    for c in BX.CASES:
        ctx, calls, _ = _built(c)
        fn, a = calls[-1]
        p = c.p
        if c.family == "jacobi" and p["io"] == "f64":
            assert "workspace" not in a and "tws" not in ctx.roles, c.id
            continue
        n = BX.query(c)
        assert a["workspace_bytes"] == n and (a["workspace"] is None) == (n == 0) and ("tws" in ctx.roles) == (n > 0), c.id
        if n:
            assert a["workspace"] == "tws" and ctx.shapes["tws"] == (n,)
        if c.family == "explicit":
            f64 = p["io"] == "f64"
            wave = not f64 and (p["H"], p["W"]) in BX.WAVE
            need = 0 if (wave or p["nt"] == 1) else 4 * up(p["B"] * p["C"] * p["H"] * p["W"] * (8 if f64 else 4))
        else:
            need = 4 * up(p["B"] * p["H"] * p["W"] * 4) if (p["path"] == 2 and p["nt"] > L.PDE_JACOBI_TANGENT_TILED_K) else 0
        assert n == need, (c.id, n, need)
    assert any(BX.query(c) > 0 for c in BX.CASES if c.family == "explicit")
    assert any(BX.query(c) > 0 for c in BX.CASES if c.family == "jacobi")


def test_the_queries_answer_zero_for_what_they_refuse():
    from cnn_with_pde_amd import _lib as L
    lib = BC.lib()
    assert lib.pde_explicit5_tangent_workspace_bytes(0, 2, 5, 7, L.PDE_IO_F32, 3) == 0
    assert lib.pde_explicit5_tangent_workspace_bytes(2, 2, 5, 0, L.PDE_IO_F32, 3) == 0
    assert lib.pde_explicit5_tangent_workspace_bytes(2, 2, 5, 7, 7, 3) == 0                       # no such tensor type
    assert lib.pde_explicit5_f64_tangent_workspace_bytes(2, 2, 0, 7, 3) == 0
    assert lib.pde_jacobi_io_tangent_workspace_bytes(2, 65, 8, 13, 7) == 0
    assert lib.pde_jacobi_io_tangent_workspace_bytes(0, 65, 8, 13, L.PDE_IO_F32) == 0
    assert lib.pde_jacobi_io_tangent_workspace_bytes(2, 65, L.PDE_JACOBI_MAX_HW + 1, 13, L.PDE_IO_F32) == 0
    assert lib.pde_jacobi_io_tangent_workspace_bytes(2, 65, 3, 13, L.PDE_IO_F32) == 0            # W < 4: not served
