"""The bounds cases of the one-launch layers' input backward (tests/bounds_input_small_cases.py) against the header that
declares their entry points (include/pdecnn_small_input.h, included by pdecnn.h), on the CPU.  The cases are not part of
the table of tests/bounds_cases.py; the checks tests/test_bounds_cases.py applies to a case of that table are applied
to them here, with its own helpers: every writing entry point of the new header has a case, every parameter is bound,
roles fit constness, element counts and alignments are the header's, ids are unique, the cases are small.  Beside that:
each case ends in the call it is named after with a workspace of exactly the queried size, and hands the fields the
shared-input call must not touch over as inputs."""
import ctypes as C

import torch

import bounds_cases as BC
import bounds_input_small_cases as BS
import test_bounds_cases as TBC

HDR = BS.header_functions()
ALL = BS.TABLE_CASES + BS.MATRIX_CASES


def _built(case):
    ctx = BC.SpecCtx()
    calls, expect = case.build(ctx)
    return ctx, calls, expect


def test_the_new_header_declares_what_the_table_of_signatures_binds():
    from cnn_with_pde_amd import _lib
    new = {f: ps for f, ps in HDR.items() if f not in BC.header_functions()}
    assert sorted(new) == sorted(_lib.SIGNATURES_SMALL_INPUT)
    for f, ps in new.items():
        assert len(ps) == len(_lib.SIGNATURES_SMALL_INPUT[f][1]), f
    assert not set(_lib.SIGNATURES_SMALL_INPUT) & set(_lib.SIGNATURES)


def test_every_writing_entry_point_of_the_new_header_has_a_case():
    new = {f: ps for f, ps in HDR.items() if f not in BC.header_functions()}
    writing = sorted(f for f, ps in new.items() if any((ptr and not const) or "workspace" in name for name, ptr, const in ps))
    assert writing == sorted(BS.NEW_FUNCTIONS)
    called = {fn for c in BS.TABLE_CASES for fn, _ in _built(c)[1]}
    assert set(writing) <= called, set(writing) - called
    assert sorted(set(new) - set(writing)) == ["pde_adi_small_backward_input_workspace_bytes"]     # a host query


def test_ids_are_unique_and_not_the_tables():
    ids = [c.id for c in ALL]
    assert len(ids) == len(set(ids)) and not set(ids) & {c.id for c in BC.CASES}
    assert all(c.switch is None for c in ALL)


def test_every_parameter_is_bound_and_roles_fit_constness():
    for c in ALL:
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
            if role in ("out", "ws", "carry", "inout") and not name.endswith(tuple(f"_{i}" for i in range(4))):
                assert name in written, f"{c.id}: {role} buffer {name} is handed to no writable parameter"


def test_element_counts_dtypes_and_sizes_are_the_headers():
    for c in ALL:
        ctx = _built(c)[0]
        if not (c.family == "multi" and c.p.get("layers")):       # (the header's counts are written out for three layers)
            for name, want in TBC._header_counts(c, ctx).items():
                assert TBC._numel(ctx, name) == want, (c.id, name, ctx.shapes[name], want)
        dt = BC.IO[c.p["io"]][1]
        for name in ("u", "y", "gy", "gu", "out", "states", "traj", "gu_input", "y_input"):
            if name in ctx.dtypes:
                assert ctx.dtypes[name] == dt, (c.id, name)
        assert sum(ctx.nbytes(n) for n in ctx.roles) < 96 << 20
        if c.p.get("emit"):
            assert c.p["emit"] < 1 << (c.p["steps"] - 1) and c.p["emit"] >> (c.p["steps"] - 2) & 1


def test_the_alignment_of_every_buffer_is_the_headers():
    seen = 0
    for c in ALL:
        ctx, calls, _ = _built(c)
        assert set(ctx.aligns) == set(ctx.roles)
        for fn, amap in calls:
            for pname, buf, _ in BC.bound_buffers(ctx, HDR[fn], amap):
                want = TBC._header_align(c, fn, pname, ctx.dtypes[buf])
                assert ctx.aligns[buf] == want, (c.id, fn, pname, buf, ctx.aligns[buf], want)
                seen += 1
        if c.family == "multi":                                  # pointers that travel inside the struct
            for buf in ctx.roles:
                field = BC.param_of(buf)
                if buf != field or buf == "weights":
                    item = torch.empty((), dtype=ctx.dtypes[buf]).element_size()
                    want = 16 if ctx.dtypes[buf] == torch.uint8 else (item if field in BC.ELEMENT_ALIGNED else 16)
                    assert ctx.aligns[buf] == want, (c.id, buf, ctx.aligns[buf], want)
                    seen += 1
    assert seen > 300


def test_the_requested_cases_are_there():
    """N = 16, C = 3, B = 3, K = 2 in fp32 / bf16 / fp16; both modes, the skip blend, an emission mask; the group side by
    side, and two layers side by side in the matrix."""
    small = [c for c in BS.TABLE_CASES if c.family == "small"]
    for io in BC.IO3:
        mine = [c.p for c in small if c.p["io"] == io]
        assert all((p["H"], p["C"], p["B"], p["steps"]) == (16, 3, 3, 2) for p in mine)
        assert any(p.get("skip") for p in mine) and any(p.get("emit") for p in mine)
        assert any(c.family == "multi" and c.p["io"] == io and c.p["B"] < 1024 for c in BS.TABLE_CASES)
        assert any(c.family == "multi" and c.p["io"] == io and c.p.get("layers") == 2 for c in BS.MATRIX_CASES)
    assert {p["mode"] for p in (c.p for c in small)} == {1, 2}
    assert {c.p.get("split", "strang") for c in ALL} == {"strang", "lie"}


def test_cases_end_in_the_input_backward_with_the_queried_workspace():
    lib = BC.lib()
    for c in ALL:
        ctx, calls, _ = _built(c)
        fn, amap = calls[-1]
        if c.family == "small":
            d, sps = ctx.values["d"], ctx.values["sweeps_per_step"]
            assert fn == "pde_adi_small_backward_input" + ("_states" if c.p.get("emit") else ""), c.id
            assert ctx.shapes["iws"] == (lib.pde_adi_small_backward_input_workspace_bytes(C.byref(d), sps),), c.id
            assert amap["workspace"] == "iws" and amap["workspace_bytes"] == ctx.shapes["iws"][0] and amap["gu"] == "gu_input"
            assert ctx.roles["gu_input"] == "out" and ctx.shapes["gu_input"] == ctx.shapes["gu"]
            names = [f for f, _ in calls]
            assert names[:2] == ["pde_adi_small_forward" + ("_states" if c.p.get("emit") else ""),
                                 "pde_adi_small_backward" + ("_states" if c.p.get("emit") else "")]
            assert ("pde_adi_small_forward_input" in names) == (not c.p.get("emit")), c.id
            if not c.p.get("emit"):
                assert ctx.roles["y_input"] == "out" and ctx.shapes["y_input"] == ctx.shapes["y"]
        else:
            assert [f for f, _ in calls] == ["pde_adi_multi_forward", "pde_adi_multi_backward_input"], c.id
            arr, nl = ctx.values["layers"], ctx.values["num_layers"]
            assert nl == len(BS.multi_layers(c.p)) and nl > 1 and c.p["B"] < 1024           # side by side: the slabs are used
            for i in range(nl):
                d = arr[i].desc.contents
                want = lib.pde_adi_small_backward_input_workspace_bytes(C.byref(d), arr[i].sweeps_per_step)
                assert ctx.shapes[f"bws_{i}"] == (want,) and arr[i].workspace_bytes == want, c.id
                assert want == -(-(ctx.nbytes("gu")) // 256) * 256                            # one tensor, rounded up to 256 bytes
                for k in BS.UNTOUCHED:
                    assert ctx.roles[f"{k}_{i}"] == "in", (c.id, k)


def test_the_query_is_smaller_than_the_full_backwards():
    """The slab alone: below the full backward's workspace, which holds the partial sums next to it."""
    lib = BC.lib()
    for c in BS.TABLE_CASES:
        if c.family == "small":
            ctx, _, _ = _built(c)
            d, sps = ctx.values["d"], ctx.values["sweeps_per_step"]
            assert 0 < lib.pde_adi_small_backward_input_workspace_bytes(C.byref(d), sps) < \
                lib.pde_adi_small_backward_workspace_bytes(C.byref(d), sps, 0)
