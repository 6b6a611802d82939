"""The case table of the bounds test (tests/bounds_cases.py) against include/pdecnn.h, on the CPU: every entry point that
writes device memory has a case or a stated reason, every case binds every parameter its entry points declare, pointers
to const memory and to writable memory are bound to buffers of a fitting role, the element counts are the header's, ids
are unique and every switch is a getenv string of csrc/.  Builders run on a recording context here: no kernel runs (the
workspace queries and path functions are host code)."""
import glob
import os
import re

import pytest
import torch

import bounds_cases as BC

HDR = BC.header_functions()


def _built(case):
    ctx = BC.SpecCtx()
    calls, expect = case.build(ctx)
    return ctx, calls, expect


@pytest.fixture(scope="module")
def built():
    return {c.id: _built(c) for c in BC.CASES}


def test_header_parse_matches_the_ctypes_table():
    from cnn_with_pde_amd import _lib
    assert sorted(HDR) == sorted(_lib.SIGNATURES)
    for fn, params in HDR.items():
        assert len(params) == len(_lib.SIGNATURES[fn][1]), fn
    p = dict((n, (ptr, const)) for n, ptr, const in HDR["pde_gate_combine_backward"])
    assert p["ys"] == (True, True) and p["gys"] == (True, False) and p["dots"] == (True, False) and p["L"] == (False, False)
    assert dict((n, c) for n, _, c in HDR["pde_adi_backward"])["ckpt_mask"] is True


def test_every_writing_entry_point_is_covered_or_excluded(built):
    called = {fn for _, calls, _ in built.values() for fn, _ in calls}
    writing = BC.writing_functions()
    assert len(writing) > 60
    missing = [f for f in writing if f not in called and f not in BC.EXCLUDED]
    assert not missing, f"no bounds case for {missing}"
    for f, why in BC.EXCLUDED.items():
        assert f in writing and f not in called and why.strip(), f
        # excluded functions write host memory only: none of their pointers is a tensor or a workspace
        assert not any(n.endswith("workspace") and not n.startswith("has_") for n, _, _ in HDR[f]), f
    print(f"{len(writing)} writing entry points: {len(writing) - len(BC.EXCLUDED)} covered by {len(BC.CASES)} cases, "
          f"{len(BC.EXCLUDED)} excluded")
    for f in writing:
        print(f"  {f}: " + (f"excluded: {BC.EXCLUDED[f]}" if f in BC.EXCLUDED else
                            f"{sum(1 for _, calls, _ in built.values() if any(fn == f for fn, _ in calls))} cases"))


def test_ids_are_unique_and_switches_exist():
    ids = [c.id for c in BC.CASES]
    assert len(ids) == len(set(ids))
    src = ""
    for path in glob.glob(os.path.join(BC.ROOT, "cnn-with-pde_amd", "csrc", "*")):
        if os.path.isfile(path) and not path.endswith((".o", ".so")):
            src += open(path, errors="replace").read()
    names = set(re.findall(r'getenv\(\s*"([A-Z0-9_]+)"', src))
    for sw in BC.SWITCHES:
        name, _, value = sw.partition("=")
        assert name in names and value, sw
    used = {c.switch for c in BC.CASES if c.switch}
    assert used == set(BC.SWITCHES), (used ^ set(BC.SWITCHES))


def test_every_parameter_is_bound_and_roles_fit_constness(built):
    for cid, (ctx, calls, expect) in built.items():
        written = set()
        for fn, amap in calls:
            params = HDR[fn]
            assert not set(amap) - {n for n, _, _ in params}, (cid, fn, set(amap) - {n for n, _, _ in params})
            args = BC.call_args(ctx, params, amap)              # KeyError: a parameter without a binding
            assert len(args) == len(params)
            for name in BC.NULL_BY_DEFAULT:                     # the pinned-host mirror and its event: NULL in every case
                for (n, _, _), a in zip(params, args):
                    if n == name:
                        assert a is None, (cid, fn, n)
            for pname, buf, const in BC.bound_buffers(ctx, params, amap):
                role = ctx.roles[buf]
                if const:
                    assert role == "in" or buf in written or role in ("inout", "carry", "ws"), (cid, fn, pname, buf, role)
                else:
                    assert role != "in", f"{cid}: {fn} may write {pname}, bound to the input {buf}"
                    written.add(buf)
        for name, role in ctx.roles.items():
            if role in ("out", "ws", "carry", "inout") and not name.endswith(tuple(f"_{i}" for i in range(4))):
                assert name in written, f"{cid}: {role} buffer {name} is handed to no writable parameter"
        for fn, args, want in expect:
            assert fn in HDR


def test_the_cases_reach_the_kernels_they_are_named_after(built, monkeypatch):
    """The dispatch functions are host code: without a switch in the environment every case outside the switch children
    must get the path it states (the children assert the same under their switch, on the GPU)."""
    for sw in BC.SWITCHES:
        monkeypatch.delenv(sw.partition("=")[0], raising=False)
    lib = BC.lib()
    n = 0
    for c in BC.CASES:
        if c.switch is None:
            for fn, args, want in built[c.id][2]:
                assert getattr(lib, fn)(*args) == want, (c.id, fn, want)
                n += 1
    assert n > 100


def _numel(ctx, name):
    n = 1
    for s in ctx.shapes[name]:
        n *= s
    return n


def _header_counts(case, ctx):
    """{buffer: elements} as the header's comments state them, written out independently of the builders."""
    p, fam = case.p, case.family
    if fam in ("adi", "steps", "small", "mixed", "multi"):
        B, Cc, H, W = p["B"], p["C"], p["H"], p["W"]
        n, par = B * Cc * H * W, Cc * H * W                       # u, y, gy, gu: (B,C,N,N); parameters: (C,N,N)
        sps = 2 if p.get("split") == "lie" else 3
    if fam == "adi":
        S = p["steps"] * sps
        c = dict(u=n, y=n, gy=n, gu=n, kappa_max=S, alpha_base=par, beta_slope=par, g_alpha_base=par, g_beta_base=par,
                 g_alpha_slope=par, g_beta_slope=par)
        if p.get("emit"):                                        # states[slot][B][C][N][N], slots = set bits
            c["states"] = c["gstates"] = BC.popcount(p["emit"]) * n
        return c
    if fam == "steps":
        return dict(x0=n, x1=n, g0=n, kappa_max=3 * p["steps"], g_alpha_base=par, g_beta_slope=par)
    if fam == "small":                                           # states: K tensors of u's shape; gM (C,C)
        c = dict(u=n, y=n, gu=n, states=p["steps"] * n, gM=Cc * Cc, M=Cc * Cc, kappa_max=sps * p["steps"], g_beta_base=par)
        if p.get("emit"):
            c["traj"] = c["gtraj"] = BC.popcount(p["emit"]) * n
        if p.get("skip"):
            c["skip_weight"] = c["g_skip_weight"] = 1
        return c
    if fam == "mixed":                                           # with y given `states` needs 2K-1 tensors only
        return dict(u=n, y=n, gu=n, states=(2 * p["steps"] - 1) * n, gM=Cc * Cc, M=Cc * Cc, g_alpha_slope=par)
    if fam == "multi":
        c = dict(u=n, out=n, gu=n, gy=n)
        for i, (_, steps) in enumerate(BC.MULTI_LAYERS):         # K_i tensors; plane_sums (B,C); g_weight a scalar
            c.update({f"states_{i}": steps * n, f"plane_sums_{i}": B * Cc, f"g_plane_sums_{i}": B * Cc, f"gM_{i}": Cc * Cc,
                      f"g_weight_{i}": 1, f"gys_{i}": n, f"g_alpha_base_{i}": par, f"kappa_max_{i}": 3 * steps})
        return c
    if fam == "mix":                                             # u, out: (B,C,HW); M, gM: (C,C)
        n = p["B"] * p["C"] * p["HW"]
        return dict(u=n, gout=n, out=n, gu=n, gu2=n, gu3=n, M=p["C"] ** 2, gM=p["C"] ** 2, gM2=p["C"] ** 2)
    if fam == "blend":
        return dict(u0=p["n"], u=p["n"], g=p["n"], out=p["n"], g_u0=p["n"], g_u=p["n"], skip_weight=1, g_skip_weight=1)
    if fam == "gate":                                            # ys: L tensors (B,C,HW); gates, dots: (B,C); weights (L)
        n = p["B"] * p["C"] * p["hw"][0] * p["hw"][1]
        c = dict(g=n, out=n, weights=p["L"])
        for i in range(p["L"]):
            c.update({f"ys_{i}": n, f"gys_{i}": n, f"gates_{i}": p["B"] * p["C"], f"dots_{i}": p["B"] * p["C"]})
        return c
    if fam == "bn_pool":                                         # out (B,2C,4,4), argmax (B,C,4,4), mean / invstd (C)
        B, Cc, N = p["B"], p["C"], p["N"]
        return dict(x=B * Cc * N * N, gx=B * Cc * N * N, out=B * 2 * Cc * 16, gout=B * 2 * Cc * 16, argmax=B * Cc * 16, mean=Cc,
                    invstd=Cc, ggamma=Cc, gbeta=Cc, running_mean=Cc, running_var=Cc)
    if fam == "explicit":                                        # states: (num_steps-1) tensors of u's shape
        n = p["B"] * p["C"] * p["H"] * p["W"]
        c = dict(u=n, out=n, gout=n, gu=n, alpha_base=p["C"], channel_scaling=p["C"], g_alpha_base=p["C"],
                 g_channel_scaling=p["C"])
        if p["nt"] > 1:
            c["states"] = (p["nt"] - 1) * n
        if p.get("emit"):
            c["traj"] = c["gtraj"] = BC.popcount(p["emit"]) * n
        return c
    if fam == "jacobi":                                          # u, out (B,H,W); a_row[H], b_col[W]
        n = p["B"] * p["H"] * p["W"]
        c = dict(u=n, out=n, gout=n, gu=n, a_row=p["H"], b_col=p["W"], g_a_row=p["H"], g_b_col=p["W"])
        if p.get("emit"):
            c["states"] = c["gstates"] = BC.popcount(p["emit"]) * n
        return c
    if fam == "sym":                                             # X, base, out, P, H: (B,D); K, gK: (D,D); the rest (D)
        B, D = p["B"], p["D"]
        c = dict(X=B * D, K=D * D, P=B * D, H=B * D, out=B * D, dP=B * D, gX=B * D, gK=D * D, g_out=B * D, mean=D, invstd=D,
                 bn_weight=D, bn_bias=D, g_bn_weight=D, g_bn_bias=D, running_mean=D, running_var=D)
        if p["kind"] != "f32":
            c["K16"] = D * D
        return c
    raise AssertionError(fam)


def test_element_counts_are_the_headers(built):
    for c in BC.CASES:
        ctx = built[c.id][0]
        for name, want in _header_counts(c, ctx).items():
            assert _numel(ctx, name) == want, (c.id, name, ctx.shapes[name], want)


def test_masks_reach_the_last_state_that_may_be_emitted_or_parked(built):
    """Per family at least one case sets bit n-2 of its emission mask (n sweeps or steps: the header allows bits 0 .. n-2), and
    the fused ADI cases bit n-2 of the checkpoint mask."""
    top = {}
    for c in BC.CASES:
        if c.p.get("emit"):
            p = c.p
            n = {"adi": lambda: p["steps"] * (2 if p.get("split") == "lie" else 3), "small": lambda: p["steps"],
                 "explicit": lambda: p["nt"], "jacobi": lambda: p["nt"]}[c.family]()
            assert p["emit"] < 1 << (n - 1), c.id                   # nothing above the allowed range
            key = (c.family, c.id.split("-")[1] if c.family == "adi" else p.get("api", ""), p.get("io"))
            top[key] = top.get(key, False) or bool(p["emit"] >> (n - 2) & 1)
    assert len(top) >= 20 and all(top.values()), [k for k, v in top.items() if not v]
    assert any(c.family == "adi" and c.p.get("ckpt", 0) >> 4 & 1 for c in BC.CASES)


def test_written_slices_of_the_one_launch_states(built):
    """pdecnn.h: the one-launch wide forward writes states[2k+1] (mode 1) or states[2k] (mode 2) and states[2K-1], which is
    `y` in these cases (`states` then holds 2K-1 tensors)."""
    seen = 0
    for c in BC.CASES:
        ctx = built[c.id][0]
        if c.family == "mixed" and c.switch is None:
            assert (ctx.roles["states"] == "carry") == bool(c.p["one_launch"]), c.id
        if c.family == "mixed" and ctx.roles["states"] == "carry":      # (built without its switch, a PDE_WIDE=0 case too)
            K = c.p["steps"]
            want = [2 * k + 1 for k in range(K) if 2 * k + 1 < 2 * K - 1] if c.p["mode"] == 1 else [2 * k for k in range(K)]
            assert ctx.roles["states"] == "carry" and ctx.written_slots == {"states": want}, c.id
            seen += 1
        else:
            assert not ctx.written_slots, c.id
    assert seen >= 2


def test_dtypes_of_the_io_tensors(built):
    for c in BC.CASES:
        ctx = built[c.id][0]
        io = c.p.get("io")
        if io is None or c.family in ("sym", "bn_pool"):
            continue
        dt = BC.IO[io][1]
        for name in ("u", "y", "gy", "gu", "out", "gout", "states", "traj"):
            if name in ctx.dtypes and not (c.family == "explicit" and name == "states"):
                assert ctx.dtypes[name] == dt, (c.id, name)
        if c.family == "explicit" and "states" in ctx.dtypes:       # FP32 whatever io_dtype (double in the f64 form)
            assert ctx.dtypes["states"] == (torch.float64 if io == "f64" else torch.float32)


def test_workspaces_are_the_queried_sizes_unrounded(built):
    """At least one workspace of the table is no multiple of 256 bytes — what functional._workspace and the allocator round
    away — and none is declared larger than its query (the builders pass the query's value through)."""
    sizes = [ctx.shapes[n][0] for ctx, _, _ in built.values() for n, r in ctx.roles.items()
             if r in ("ws", "carry") and ctx.dtypes[n] == torch.uint8]
    assert sizes and any(s % 256 for s in sizes), "every workspace of the table is a multiple of 256 bytes"
    print(f"{len(sizes)} workspaces, {sum(1 for s in sizes if s % 256)} of them no multiple of 256 bytes, "
          f"smallest {min(sizes)}, largest {max(sizes)}")


def test_the_cases_are_small(built):
    for cid, (ctx, _, _) in built.items():
        total = sum(ctx.nbytes(n) for n in ctx.roles)
        assert total < 96 << 20, (cid, total)


# ---------------------------------------------------------------------------------------------------- alignment
_WHOLE_SCHEDULE = ("forward", "backward", "forward_states", "backward_states", "backward_input", "backward_input_states",
                   "kappa_max")
_EXPLICIT_IO = ("u", "out", "gout", "gu", "traj", "gtraj")


def _header_align(case, fn, pname, dtype):
    """Bytes the Alignment section of pdecnn.h asks of parameter ``pname`` of ``fn`` in this case — written out from the
    header's text, independently of the builders."""
    item = torch.empty((), dtype=dtype).element_size()
    p = case.p
    if "workspace" in pname:
        return 16
    if pname in BC.header_element_aligned():
        return item
    for prefix, names in BC.header_element_aligned_in().items():
        if fn.startswith(prefix) and pname in names:
            return item
    elementwise = ("_f64_" in fn or fn.startswith(("pde_adi_rect_", "pde_jacobi_")) or
                   (fn.startswith("pde_explicit5_") and p["W"] % 4 != 0) or
                   (fn in tuple("pde_adi_" + s for s in _WHOLE_SCHEDULE) and BC.lib().pde_adi_line_length_path(p["H"]) == 2))
    if elementwise:
        return item
    if fn.startswith("pde_explicit5_") and pname in _EXPLICIT_IO and item == 2:
        return 8
    return 16


def test_the_alignment_table_is_the_headers(built):
    """Every exception the header names is in the table and vice versa; every buffer a call is handed carries the alignment
    the header asks of that parameter (a buffer bound to several parameters: of each of them)."""
    assert BC.header_element_aligned() == BC.ELEMENT_ALIGNED
    assert BC.header_element_aligned_in() == BC.ELEMENT_ALIGNED_IN
    declared = {n for ps in HDR.values() for n, ptr, _ in ps if ptr}
    from cnn_with_pde_amd import _lib
    declared |= {f for f, _ in _lib.PdeSmallLayer._fields_}
    assert not BC.ELEMENT_ALIGNED - declared, BC.ELEMENT_ALIGNED - declared
    seen, less = 0, set()
    for c in BC.CASES:
        ctx, calls, _ = built[c.id]
        assert set(ctx.aligns) == set(ctx.roles)
        for fn, amap in calls:
            for pname, buf, _ in BC.bound_buffers(ctx, HDR[fn], amap):
                want = _header_align(c, fn, pname, ctx.dtypes[buf])
                assert ctx.aligns[buf] == want, (c.id, fn, pname, buf, ctx.aligns[buf], want)
                seen += 1
                if want < 16:
                    less.add(pname)
        if c.family in ("multi", "gate"):                        # pointers that travel inside a struct or an array
            for buf in ctx.roles:
                field = BC.param_of(buf)
                if buf != field or buf == "weights":
                    item = torch.empty((), dtype=ctx.dtypes[buf]).element_size()
                    want = 16 if (ctx.dtypes[buf] == torch.uint8) else (item if field in BC.ELEMENT_ALIGNED else 16)
                    assert ctx.aligns[buf] == want, (c.id, buf, ctx.aligns[buf], want)
                    seen += 1
    assert seen > 5000 and BC.ELEMENT_ALIGNED - {"kappa_max_host", "weight_ptr", "gates", "dots", "plane_sums", "g_weight"} <= less, \
        BC.ELEMENT_ALIGNED - less
    print(f"{seen} (call, parameter) bindings carry the header's alignment; below 16 bytes: {sorted(less)}")
