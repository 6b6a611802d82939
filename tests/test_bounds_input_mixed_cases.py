"""The bounds cases of the channel-operator layers' input backward (tests/bounds_input_mixed_cases.py) against the header
that declares their entry points (include/pdecnn_mixed_input.h, included by pdecnn.h), on the CPU.  The cases are not part
of the table of tests/bounds_cases.py; the checks tests/test_bounds_cases.py applies to a case of that table are applied to
them here, with its own helpers: the header and ``_lib.SIGNATURES_MIXED_INPUT`` name the same functions with the same
argument counts, every writing entry point of the new header has a case, every parameter is bound, roles fit constness,
element counts and alignments are the header's, ids are unique, the cases are small.  Beside that: every new call gets a
workspace of exactly the queried size (none where the query is 0), and the queries are smaller than the full calls'."""
import ctypes as C
import os

import bounds_cases as BC
import bounds_input_mixed_cases as BM
import test_bounds_cases as TBC

HDR = BM.header_functions()
NEW = {f: ps for f, ps in HDR.items() if f not in BC.header_functions()}


def _built(case):
    ctx = BC.SpecCtx()
    calls, expect = case.build(ctx)
    return ctx, calls, expect


def test_the_new_header_declares_what_the_table_of_signatures_binds():
    from cnn_with_pde_amd import _lib
    assert '#include "pdecnn_mixed_input.h"' in open(os.path.join(BC.ROOT, "include", "pdecnn.h")).read()
    assert sorted(NEW) == sorted(_lib.SIGNATURES_MIXED_INPUT) == sorted(BM.NEW_FUNCTIONS + BM.QUERIES)
    for f, ps in NEW.items():
        assert len(ps) == len(_lib.SIGNATURES_MIXED_INPUT[f][1]), f
    assert not set(_lib.SIGNATURES_MIXED_INPUT) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SMALL_INPUT))
    lib = _lib.load()
    for f in _lib.SIGNATURES_MIXED_INPUT:
        assert getattr(lib, f).argtypes == _lib.SIGNATURES_MIXED_INPUT[f][1], f


def test_every_writing_entry_point_of_the_new_header_has_a_case():
    writing = sorted(f for f, ps in NEW.items() if any((ptr and not const) or "workspace" in name for name, ptr, const in ps))
    assert writing == sorted(BM.NEW_FUNCTIONS)
    called = {fn for c in BM.CASES for fn, _ in _built(c)[1]}
    assert set(writing) <= called, set(writing) - called
    assert sorted(set(NEW) - set(writing)) == sorted(BM.QUERIES)


def test_ids_are_unique_and_not_the_tables():
    ids = [c.id for c in BM.CASES]
    assert len(ids) == len(set(ids)) and not set(ids) & {c.id for c in BC.CASES}
    assert all(c.switch is None for c in BM.CASES)


def test_every_parameter_is_bound_and_roles_fit_constness():
    for c in BM.CASES:
        ctx, calls, expect = _built(c)
        written = set()
        for fn, amap in calls:
            params = HDR[fn]
            assert not set(amap) - {n for n, _, _ in params}, (c.id, fn)
            args = BC.call_args(ctx, params, amap)              # KeyError: a parameter without a binding
            assert len(args) == len(params)
            for (n, _, _), a in zip(params, args):
                if n in BC.NULL_BY_DEFAULT:
                    assert a is None, (c.id, fn, n)
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


def test_element_counts_dtypes_and_sizes_are_the_headers():
    for c in BM.CASES:
        ctx = _built(c)[0]
        for name, want in TBC._header_counts(c, ctx).items():
            assert TBC._numel(ctx, name) == want, (c.id, name, ctx.shapes[name], want)
        for mine, full in BM.twins(c):
            assert ctx.roles[mine] == "out" and ctx.shapes[mine] == ctx.shapes[full] and ctx.dtypes[mine] == ctx.dtypes[full], \
                (c.id, mine, full)
        assert BM.twins(c)
        assert sum(ctx.nbytes(n) for n in ctx.roles) < 96 << 20


def test_the_alignment_of_every_buffer_is_the_headers():
    seen = 0
    for c in BM.CASES:
        ctx, calls, _ = _built(c)
        assert set(ctx.aligns) == set(ctx.roles)
        for fn, amap in calls:
            for pname, buf, _ in BC.bound_buffers(ctx, HDR[fn], amap):
                want = TBC._header_align(c, fn, pname, ctx.dtypes[buf])
                assert ctx.aligns[buf] == want, (c.id, fn, pname, buf, ctx.aligns[buf], want)
                seen += 1
    assert seen > 500


def test_the_requested_cases_are_there():
    """Every path of the channel operator's backward on the tensor types it serves, both modes of the layer, the one-launch
    forward, the fragment table of the C = 128 fused path, float64."""
    mixed = [c.p for c in BM.CASES if c.family == "mixed"]
    assert {p["mode"] for p in mixed} == {1, 2} and {p["io"] for p in mixed} == set(BC.IO3)
    assert {p["C"] for p in mixed} == {5, 32, 64, 96, 128} and any(p["one_launch"] for p in mixed)
    mix = [c.p for c in BM.CASES if c.family == "mix" and c.p["io"] != "f64"]
    assert {(p["bwd_path"], p["io"] == "f32") for p in mix} == {("scalar", True), ("scalar", False), ("split3", True),
                                                               ("fused", True), ("fused", False), ("mfma16", False)}
    assert {p["C"] for p in mix if p["bwd_path"] == "split3"} == {32, 64, 96}
    assert {p["C"] for p in mix if p["bwd_path"] == "fused"} == {32, 64, 96, 128}
    assert any(p["HW"] % 64 for p in mix if p["bwd_path"] == "split3")               # a ragged last tile
    for fam in ("mix", "blend"):
        assert any(c.p["io"] == "f64" for c in BM.CASES if c.family == fam)
    assert {c.p["io"] for c in BM.CASES if c.family == "steps"} == set(BC.IO3)


def test_the_new_calls_get_the_queried_workspaces():
    lib = BC.lib()
    for c in BM.CASES:
        ctx, calls, _ = _built(c)
        by_fn = {}
        for fn, amap in calls:
            by_fn.setdefault(fn, []).append(amap)
        if c.family == "mixed":
            d, sps = ctx.values["d"], ctx.values["sweeps_per_step"]
            assert [f for f, _ in calls] == ["pde_adi_mixed_forward", "pde_adi_mixed_backward", "pde_adi_mixed_forward_input",
                                             "pde_adi_mixed_backward_input"], c.id
            nf = lib.pde_adi_mixed_forward_input_workspace_bytes(C.byref(d), sps)
            fa, = by_fn["pde_adi_mixed_forward_input"]
            assert fa["workspace_bytes"] == nf and (fa["workspace"] is None) == (nf == 0), c.id
            one_tensor = -(-ctx.nbytes("u") // 256) * 256
            assert nf == (0 if c.p["one_launch"] else 2 * one_tensor), (c.id, nf)
            ba, = by_fn["pde_adi_mixed_backward_input"]
            ni = lib.pde_adi_mixed_backward_input_workspace_bytes(C.byref(d), sps)
            assert ba["workspace_bytes"] == ni == ctx.shapes["iws"][0], c.id
            assert 2 * one_tensor <= ni < lib.pde_adi_mixed_backward_workspace_bytes(C.byref(d), sps, 0), c.id
            assert lib.pde_adi_mixed_backward_input_one_launch(C.byref(d), sps) == 0
        elif c.family == "mix" and c.p["io"] != "f64":
            a, = by_fn["pde_channel_mix_backward_input"]
            n = lib.pde_channel_mix_backward_input_workspace_bytes(c.p["B"], c.p["C"], c.p["HW"])
            assert a["workspace_bytes"] == n and (a["workspace"] is None) == (n == 0), c.id
            assert n < lib.pde_channel_mix_backward_workspace_bytes(c.p["B"], c.p["C"], c.p["HW"]), c.id
        elif c.family == "steps":
            assert len(by_fn["pde_adi_backward_input_step"]) == c.p["steps"], c.id


def test_the_queries_answer_zero_for_what_they_refuse():
    from cnn_with_pde_amd import _lib as L
    lib = BC.lib()
    d = BC._adi_desc(dict(B=2, C=5, H=10, W=10, io="f32", steps=2))           # no fused kernels at N = 10: no per-step calls
    assert isinstance(d, L.PdeAdiDesc)
    assert lib.pde_adi_mixed_forward_input_workspace_bytes(C.byref(d), 3) == 0
    assert lib.pde_adi_mixed_backward_input_workspace_bytes(C.byref(d), 3) == 0
    d = BC._adi_desc(dict(B=2, C=5, H=8, W=8, io="f32", steps=2))
    assert lib.pde_adi_mixed_backward_input_workspace_bytes(C.byref(d), 4) == 0   # 6 sweeps are no whole number of steps of 4
    assert lib.pde_channel_mix_backward_input_workspace_bytes(0, 5, 64) == 0
