"""The bounds cases of the tangent-linear pass (tests/bounds_tangent_cases.py) against the header that declares its entry
points (include/pdecnn_tangent.h, included by pdecnn.h), on the CPU.  The cases are not part of the table of
tests/bounds_cases.py; the checks tests/test_bounds_cases.py applies to a case of that table are applied to them here: the
header and ``_lib.SIGNATURES_TANGENT`` name the same functions with the same argument counts, every writing entry point of
the new header has a case, every parameter is bound, roles fit constness, element counts are the header's, every buffer
sits at its element's alignment and every workspace at 16 bytes, ids are unique, the cases are small.  Beside that: every
call gets a workspace of exactly the queried size, and the requested dispatches are all there."""
import os

import torch

import bounds_cases as BC
import bounds_tangent_cases as BT

HDR = BT.header_functions()
NEW = {f: ps for f, ps in HDR.items() if f not in BC.header_functions()}


def _built(case):
    ctx = BC.SpecCtx()
    calls, expect = case.build(ctx)
    return ctx, calls, expect


def test_the_new_header_declares_what_the_table_of_signatures_binds():
    from cnn_with_pde_amd import _lib
    assert '#include "pdecnn_tangent.h"' in open(os.path.join(BC.ROOT, "include", "pdecnn.h")).read()
    assert sorted(NEW) == sorted(_lib.SIGNATURES_TANGENT) == sorted(BT.NEW_FUNCTIONS + BT.QUERIES)
    for f, ps in NEW.items():
        assert len(ps) == len(_lib.SIGNATURES_TANGENT[f][1]), f
    assert not set(_lib.SIGNATURES_TANGENT) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SMALL_INPUT) |
                                               set(_lib.SIGNATURES_MIXED_INPUT) | set(_lib.SIGNATURES_EXPLICIT_INPUT))
    lib = _lib.load()
    for f in _lib.SIGNATURES_TANGENT:
        assert getattr(lib, f).argtypes == _lib.SIGNATURES_TANGENT[f][1], f


def test_every_writing_entry_point_of_the_new_header_has_a_case():
    writing = sorted(f for f, ps in NEW.items() if any((ptr and not const) or "workspace" in name for name, ptr, const in ps))
    assert writing == sorted(BT.NEW_FUNCTIONS)
    called = {fn for c in BT.CASES for fn, _ in _built(c)[1]}
    assert set(writing) <= called, set(writing) - called
    assert sorted(set(NEW) - set(writing)) == sorted(BT.QUERIES)


def test_ids_are_unique_and_not_the_tables():
    ids = [c.id for c in BT.CASES]
    assert len(ids) == len(set(ids)) and not set(ids) & {c.id for c in BC.CASES}
    assert all(c.switch is None for c in BT.CASES)


def test_every_parameter_is_bound_and_roles_fit_constness():
    for c in BT.CASES:
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
    for c in BT.CASES:
        ctx, calls, _ = _built(c)
        fn, amap = calls[-1]
        assert fn in BT.NEW_FUNCTIONS and fn == BC._adi_fam(c.p) + "tangent", c.id
        assert len(calls) == (2 if BT.has_forward_twin(c.p) else 1), c.id
        with_du, names = BT.MODES[c.p["tan"]]
        bound = {p for p, _, _ in BC.bound_buffers(ctx, HDR[fn], amap)}
        assert ("du" in bound) == with_du and {k for k in BT.TANGENTS if k in bound} == set(names), (c.id, bound)
        assert with_du or names, c.id                             # never all five NULL
        assert ("y" in bound) == (not c.p.get("no_y")) and "dy" in bound and "u" in bound, c.id
        outs = {buf for _, buf, const in BC.bound_buffers(ctx, HDR[fn], amap) if not const}
        ins = {buf for _, buf, const in BC.bound_buffers(ctx, HDR[fn], amap) if const}
        assert not outs & ins, c.id                               # outputs overlap no input


def test_element_counts_dtypes_and_sizes_are_the_headers():
    for c in BT.CASES:
        ctx = _built(c)[0]
        p = c.p
        n, par = p["B"] * p["C"] * p["H"] * p["W"], p["C"] * p["H"] * p["W"]   # u, du, y, dy: [B][C][H][W]; parameters: [C][H][W]
        io, kt = BC.IO[p["io"]][1], (torch.float64 if p["io"] == "f64" else torch.float32)
        want = dict(u=(n, io), du=(n, io), y=(n, io), dy=(n, io), y_fwd=(n, io))
        want.update({k: (par, kt) for k in BT.TANGENTS + ("alpha_base", "beta_base", "alpha_slope", "beta_slope")})
        for name in ctx.roles:
            if ctx.dtypes[name] == torch.uint8:
                continue
            numel = 1
            for s in ctx.shapes[name]:
                numel *= s
            assert (numel, ctx.dtypes[name]) == want[name], (c.id, name, ctx.shapes[name], ctx.dtypes[name])
        for mine, full in BT.twins(c):
            assert ctx.roles[mine] == "out" and ctx.shapes[mine] == ctx.shapes[full] and ctx.dtypes[mine] == ctx.dtypes[full]
        assert sum(ctx.nbytes(n) for n in ctx.roles) < 96 << 20


def test_the_alignment_of_every_buffer_is_the_headers():
    """The element for tensors and parameters — at the fused sizes too —, 16 bytes for the workspaces."""
    seen = 0
    for c in BT.CASES:
        ctx, calls, _ = _built(c)
        assert set(ctx.aligns) == set(ctx.roles)
        for fn, amap in calls:
            for pname, buf, _ in BC.bound_buffers(ctx, HDR[fn], amap):
                want = 16 if "workspace" in pname else torch.empty((), dtype=ctx.dtypes[buf]).element_size()
                assert ctx.aligns[buf] == want, (c.id, fn, pname, buf, ctx.aligns[buf], want)
                seen += 1
    assert seen > 250


def test_the_requested_cases_are_there():
    ps = [c.p for c in BT.CASES]
    sq = [p for p in ps if p["H"] == p["W"] and p["io"] != "f64"]
    assert {p["H"] for p in sq} >= {2, 3, 9, 10, 17, 28, 32, 33, 65, 128}
    assert {p["io"] for p in sq} == set(BC.IO3)
    rect = [p for p in ps if p.get("rect") and p["io"] != "f64"]
    assert {(p["H"], p["W"]) for p in rect} >= {(2, 128), (128, 3), (5, 12)} and {p["io"] for p in rect} == set(BC.IO3)
    f64 = [p for p in ps if p["io"] == "f64"]
    lds = lambda p: 2 * p["H"] * (p["W"] + 1) * 8 <= 160 * 1024                                          # noqa: E731
    assert any(lds(p) for p in f64) and any(not lds(p) for p in f64)
    assert any(not lds(p) and p.get("rect") for p in f64) and any(not lds(p) and not p.get("rect") for p in f64)
    assert (101, 101, 1, 1) in {(p["H"], p["W"], p["B"], p["C"]) for p in f64}
    assert {p["tan"] for p in ps} == set(BT.MODES)
    assert any(p.get("no_y") for p in ps) and any(BT.twins(c) for c in BT.CASES)
    assert {p["split"] for p in ps} == {"strang", "lie"} and {p["steps"] for p in ps} == {1, 2}


def test_the_calls_get_the_queried_workspaces():
    lib = BC.lib()
    up = lambda n: -(-n // 256) * 256                                                                     # noqa: E731
    for c in BT.CASES:
        ctx, calls, _ = _built(c)
        fn, a = calls[-1]
        p = c.p
        n = BT.query(c)
        assert n > 0 and a["workspace"] == "tws" and a["workspace_bytes"] == n and ctx.shapes["tws"] == (n,), c.id
        size = 8 if p["io"] == "f64" else 4
        S = p["steps"] * (2 if p["split"] == "lie" else 3)
        hw = p["H"] * p["W"]
        need = up(S * p["C"] * 4 * hw * size) + up(16 * 96 if size == 4 else 32 * 96) + up(S * p["C"] * hw * size)
        if 2 * p["H"] * (p["W"] + 1) * size > 160 * 1024:
            need += up(min(p["B"], -(-256 // p["C"])) * p["C"] * p["H"] * (p["W"] + 1) * size)
        assert n == need, (c.id, n, need)
