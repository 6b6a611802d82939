"""The bounds cases of the fused tangent-linear pass (tests/bounds_tangent_fused_cases.py) against the header that declares
its entry points (include/pdecnn_tangent_fused.h, included by pdecnn.h), on the CPU.  The cases are not part of the table of
tests/bounds_cases.py; the checks tests/test_bounds_cases.py applies to a case of that table are applied to them here: the
header and ``_lib.SIGNATURES_TANGENT_FUSED`` name the same functions with the same argument counts, the writing entry point
has a case, every parameter is bound, roles fit constness, element counts are the header's, every buffer sits at 16 bytes,
ids are unique, the cases are small.  Beside that: every call gets a workspace of exactly the queried size, which is the
header's formula, and the requested dispatches are all there."""
import os

import torch

import bounds_cases as BC
import bounds_tangent_cases as BT
import bounds_tangent_fused_cases as BF

HDR = BF.header_functions()
NEW = {f: ps for f, ps in HDR.items() if f not in BC.header_functions()}


def _built(case):
    ctx = BC.SpecCtx()
    calls, expect = case.build(ctx)
    return ctx, calls, expect


def test_the_new_header_declares_what_the_table_of_signatures_binds():
    from cnn_with_pde_amd import _lib
    assert '#include "pdecnn_tangent_fused.h"' in open(os.path.join(BC.ROOT, "include", "pdecnn.h")).read()
    assert sorted(NEW) == sorted(_lib.SIGNATURES_TANGENT_FUSED) == sorted(BF.NEW_FUNCTIONS + BF.QUERIES)
    for f, ps in NEW.items():
        assert len(ps) == len(_lib.SIGNATURES_TANGENT_FUSED[f][1]), f
    assert not set(_lib.SIGNATURES_TANGENT_FUSED) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SMALL_INPUT) |
                                                     set(_lib.SIGNATURES_MIXED_INPUT) | set(_lib.SIGNATURES_EXPLICIT_INPUT) |
                                                     set(_lib.SIGNATURES_TANGENT) | set(_lib.SIGNATURES_EXPLICIT_TANGENT))
    lib = _lib.load()
    for f in _lib.SIGNATURES_TANGENT_FUSED:
        assert getattr(lib, f).argtypes == _lib.SIGNATURES_TANGENT_FUSED[f][1], f


def test_the_writing_entry_point_of_the_new_header_has_a_case():
    writing = sorted(f for f, ps in NEW.items() if any((ptr and not const) or "workspace" in name for name, ptr, const in ps))
    assert writing == sorted(BF.NEW_FUNCTIONS)
    called = {fn for c in BF.CASES for fn, _ in _built(c)[1]}
    assert set(writing) <= called, set(writing) - called
    assert sorted(set(NEW) - set(writing)) == sorted(BF.QUERIES)


def test_ids_are_unique_and_not_the_tables():
    ids = [c.id for c in BF.CASES]
    assert len(ids) == len(set(ids)) and not set(ids) & ({c.id for c in BC.CASES} | {c.id for c in BT.CASES})
    assert all(c.switch is None for c in BF.CASES)


def test_every_parameter_is_bound_and_roles_fit_constness():
    for c in BF.CASES:
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
    for c in BF.CASES:
        ctx, calls, _ = _built(c)
        fn, amap = calls[-1]
        assert fn == "pde_adi_tangent_fused" and len(calls) == 2 and calls[0][0] == "pde_adi_forward", c.id
        with_du, names = BT.MODES[c.p["tan"]]
        bound = {p for p, _, _ in BC.bound_buffers(ctx, HDR[fn], amap)}
        assert ("du" in bound) == with_du and {k for k in BT.TANGENTS if k in bound} == set(names), (c.id, bound)
        assert with_du or names, c.id                             # never all five NULL
        assert ("y" in bound) == (not c.p.get("no_y")) and "dy" in bound and "u" in bound, c.id
        outs = {buf for _, buf, const in BC.bound_buffers(ctx, HDR[fn], amap) if not const}
        ins = {buf for _, buf, const in BC.bound_buffers(ctx, HDR[fn], amap) if const}
        assert not outs & ins, c.id                               # outputs overlap no input


def test_element_counts_dtypes_and_sizes_are_the_headers():
    for c in BF.CASES:
        ctx = _built(c)[0]
        p = c.p
        n, par = p["B"] * p["C"] * p["H"] * p["W"], p["C"] * p["H"] * p["W"]   # u, du, y, dy: [B][C][N][N]; parameters: [C][N][N]
        io = BC.IO[p["io"]][1]
        want = dict(u=(n, io), du=(n, io), y=(n, io), dy=(n, io), y_fwd=(n, io))
        want.update({k: (par, torch.float32) for k in BT.TANGENTS + ("alpha_base", "beta_base", "alpha_slope", "beta_slope")})
        for name in ctx.roles:
            if ctx.dtypes[name] == torch.uint8:
                continue
            numel = 1
            for s in ctx.shapes[name]:
                numel *= s
            assert (numel, ctx.dtypes[name]) == want[name], (c.id, name, ctx.shapes[name], ctx.dtypes[name])
        for mine, full in BF.twins(c):
            assert ctx.roles[mine] == "out" and ctx.shapes[mine] == ctx.shapes[full] and ctx.dtypes[mine] == ctx.dtypes[full]
        assert sum(ctx.nbytes(n) for n in ctx.roles) < 16 << 20


def test_the_alignment_of_every_buffer_is_the_headers():
    """16 bytes for tensors, parameters, tangents and workspaces alike."""
    seen = 0
    for c in BF.CASES:
        ctx, calls, _ = _built(c)
        assert set(ctx.aligns) == set(ctx.roles)
        for fn, amap in calls:
            for pname, buf, _ in BC.bound_buffers(ctx, HDR[fn], amap):
                assert ctx.aligns[buf] == 16, (c.id, fn, pname, buf, ctx.aligns[buf])
                seen += 1
    assert seen > 150


def test_the_requested_cases_are_there():
    ps = [c.p for c in BF.CASES]
    assert all(p["H"] == p["W"] for p in ps) and {p["H"] for p in ps} == set(BF.FUSED)
    assert {p["io"] for p in ps} == set(BC.IO3)
    assert {p["tan"] for p in ps} == set(BT.MODES)
    assert any(p.get("no_y") for p in ps) and any(BF.twins(c) for c in BF.CASES)
    assert {p["split"] for p in ps} == {"strang", "lie"} and {p["steps"] for p in ps} >= {1, 2, 4}
    assert (1, 1) in {(p["B"], p["C"]) for p in ps}
    assert any(p["B"] > 16 and p["B"] % 16 for p in ps)           # a ragged second chunk
    assert any(p["C"] % 8 == 0 for p in ps)
    sweeps = lambda p: p["steps"] * (2 if p["split"] == "lie" else 3)                                     # noqa: E731
    assert any(sweeps(p) <= 3 for p in ps) and any(sweeps(p) > 3 for p in ps)      # resident records, and the ring


def test_the_calls_get_the_queried_workspaces():
    import ctypes as C
    lib = BC.lib()
    up = lambda n: -(-n // 256) * 256                                                                     # noqa: E731
    for c in BF.CASES:
        ctx, calls, _ = _built(c)
        fn, a = calls[-1]
        p = c.p
        n = BF.query(c)
        assert n > 0 and a["workspace"] == "tws" and a["workspace_bytes"] == n and ctx.shapes["tws"] == (n,), c.id
        S = p["steps"] * (2 if p["split"] == "lie" else 3)
        fwd = lib.pde_adi_forward_workspace_bytes(C.byref(BC._adi_desc(p)))
        assert n == fwd + up(S * p["C"] * 32 * 36 * 4), (c.id, n, fwd)
