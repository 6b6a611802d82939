"""Bounds cases of the input-only backward of the one-launch C <= 4 layers (pde_adi_small_forward_input,
pde_adi_small_backward_input[_states], pde_adi_multi_backward_input), as an extension of the case table of
tests/bounds_cases.py kept in a file of its own — the pattern of tests/bounds_input_cases.py.

A one-layer case is a ``small`` case of that table — the forward, the full backward, built by
``bounds_cases.build_small`` unchanged — followed by ``pde_adi_small_forward_input`` into an output of its own
(``y_input``; it factorises into the same steps workspace, which the full forward filled with the same values) and the
input backward on the same gy / gtraj / mask with an output (``gu_input``) and a workspace (``iws``) of its own, of exactly
the queried size.  A one-layer call touches no scratch: ``iws`` must come back as it went in.

A shared-input case is the forward of the table's ``multi`` family followed by ``pde_adi_multi_backward_input`` on the
same array of ``PdeSmallLayer``.  Its ``workspace`` fields hold the slabs (``bws_i``, exactly the queried size: side by
side the kernel writes a whole tensor there), and the fields the call must not touch — the coefficient gradients, ``gM``,
``g_weight`` — point at INPUT buffers: they are handed over non-NULL, checked for alignment like every pointer of the
struct, and must hold afterwards what they held before.  The full backward does not run in these cases (it would need the
``workspace`` fields for itself); tests/test_gpu_bounds_input_small.py calls it on the side for the bitwise comparison.

The new entry points are declared in include/pdecnn_small_input.h (which pdecnn.h includes), and bound in
``_lib.SIGNATURES_SMALL_INPUT``: ``header_functions()`` here is the parse of tests/bounds_cases.py over both headers, and
the runners (``test_gpu_bounds._run`` / ``check_case``, ``test_alignment_refusal.sweep_case``) are handed that.  The cases
are NOT appended to ``bounds_cases.CASES``: that table, and the tests that hold it to pdecnn.h, stay what they were;
tests/test_bounds_input_small_cases.py applies the table's checks of a case to these.  ``MATRIX_CASES`` hold two layers side
by side among others."""
import ctypes as C

import torch

import bounds_cases as BC

NEW_FUNCTIONS = ["pde_adi_multi_backward_input", "pde_adi_small_backward_input", "pde_adi_small_backward_input_states",
                 "pde_adi_small_forward_input"]
#: fields of PdeSmallLayer the input backward must leave alone, bound to inputs in the shared-input cases
UNTOUCHED = ("g_alpha_base", "g_beta_base", "g_alpha_slope", "g_beta_slope", "gM", "g_weight")


class SmallInputCase(BC.Case):
    """A ``small`` case with the forward that parks nothing and the input backward behind its calls."""

    def build(self, ctx):
        p = dict(self.p)
        calls, expect = BC.build_small(ctx, p)
        lib = BC.lib()
        d = ctx.values["d"]
        sps = ctx.values["sweeps_per_step"]
        shape = (p["B"], p["C"], p["H"], p["W"])
        dt = BC.IO[p["io"]][1]
        ctx.out("gu_input", shape, dt)
        ni = ctx.ws("iws", lib.pde_adi_small_backward_input_workspace_bytes(C.byref(d), sps))
        assert ni > 0, ni
        calls = list(calls)
        ba = {"gu": "gu_input", "steps_workspace": "sws", "workspace": "iws", "workspace_bytes": ni}
        if p.get("emit"):
            calls.append(("pde_adi_small_backward_input_states", ba))
            return calls, expect
        ctx.out("y_input", shape, dt)
        fa = {"y": "y_input", "steps_workspace": "sws", "workspace_bytes": ctx.shapes["sws"][0]}
        if not p.get("skip"):
            fa["skip_weight"] = ba["skip_weight"] = None
        calls.append(("pde_adi_small_forward_input", fa))
        calls.append(("pde_adi_small_backward_input", ba))
        return calls, expect


def multi_layers(p):
    return BC.MULTI_LAYERS[:p.get("layers", len(BC.MULTI_LAYERS))]


class MultiInputCase(BC.Case):
    """The forward of a shared-input group and its input backward on one array of PdeSmallLayer."""

    def build(self, ctx):
        from cnn_with_pde_amd import _lib as L
        p = dict(self.p)
        l = BC.lib()
        g = BC._gen(p)
        dt = BC.IO[p["io"]][1]
        shape = (p["B"], p["C"], p["H"], p["W"])
        specs = multi_layers(p)
        nl, sps = len(specs), 3
        ctx.inp("u", torch.randn(shape, generator=g), dt)
        ctx.inp("gy", torch.randn(shape, generator=g), dt)
        ctx.inp("weights", torch.softmax(torch.randn(nl, generator=g), 0))
        ctx.out("out", shape, dt)
        ctx.out("gu", shape, dt)
        arr = (L.PdeSmallLayer * nl)()
        keep = []
        for i, (ldt, steps) in enumerate(specs):
            q = dict(p, dt=ldt, steps=steps)
            d = BC._adi_desc(q)
            keep.append(d)
            s = f"_{i}"
            ctx.inp("M" + s, BC._matrix(p["C"], g))
            BC._adi_params(ctx, q, g, s)
            ctx.out("states" + s, (steps,) + shape, dt)
            ctx.out("plane_sums" + s, shape[:2], torch.float32)
            ctx.out("kappa_max" + s, (d.num_sweeps,), torch.float32)
            ctx.inp("gys" + s, torch.randn(shape, generator=g), dt)
            ctx.inp("g_plane_sums" + s, torch.randn(shape[:2], generator=g))
            for k in UNTOUCHED:                      # non-NULL, aligned, and not written: inputs
                kshape = {"gM": (p["C"], p["C"]), "g_weight": (1,)}.get(k, shape[1:])
                ctx.inp(k + s, torch.randn(kshape, generator=g))
            ns = ctx.ws("sws" + s, l.pde_adi_steps_workspace_bytes(C.byref(d), sps), "carry")
            ni = ctx.ws("bws" + s, l.pde_adi_small_backward_input_workspace_bytes(C.byref(d), sps))
            assert ns > 0 and ni > 0
            a = arr[i]
            a.desc, a.sweeps_per_step, a.mode = C.pointer(d), sps, 1
            for k in ("M", "alpha_base", "beta_base", "alpha_slope", "beta_slope", "states", "plane_sums", "kappa_max", "gys",
                      "g_plane_sums") + UNTOUCHED:
                setattr(a, k, ctx.ptr(k + s) or None)
            a.weight, a.weight_ptr = 0.0, (ctx.ptr("weights", 4 * i) or None)
            a.steps_workspace, a.steps_workspace_bytes = ctx.ptr("sws" + s) or None, ns
            a.workspace, a.workspace_bytes = ctx.ptr("bws" + s) or None, ni
        ctx.val("num_layers", nl)
        ctx.val("layers", arr)
        ctx.val("_keep", keep)
        return [("pde_adi_multi_forward", {}), ("pde_adi_multi_backward_input", {})], []


def _small(**p):
    cid = (f"small-input-c{p['C']}-n{p['H']}-b{p['B']}-{p['io']}-{BC._sched_id(p['steps'], p.get('split', 'strang'))}"
           f"-m{p['mode']}{'s' if p.get('skip') else ''}-em{p.get('emit', 0):x}")
    return SmallInputCase(cid, "small", dict(p, frozen=True))


def _multi(**p):
    cid = f"multi-input-n{p['H']}-c{p['C']}-b{p['B']}-{p['io']}-l{p.get('layers', len(BC.MULTI_LAYERS))}"
    return MultiInputCase(cid, "multi", dict(p, frozen=True))


def _table_cases():
    """N = 16, C = 3, B = 3, K = 2 in the three tensor types: both modes, the skip blend, an emission mask; the three-layer
    group side by side."""
    out = []
    base = dict(B=3, C=3, H=16, W=16, steps=2)
    for io in BC.IO3:
        out.append(_small(io=io, mode=1, **base))
        out.append(_small(io=io, mode=2, skip=True, **base))
        out.append(_small(io=io, mode=1 if io == "bf16" else 2, emit=BC._all_but_last(2), **base))
        out.append(_multi(B=3, C=3, H=16, W=16, io=io))
    out.append(_small(io="f32", mode=2, **base))
    out.append(_small(io="bf16", mode=1, split="lie", **base))
    return out


def _matrix_cases():
    """Two layers side by side; the Lie pattern with a mask; the largest plane; a group one after the other would need
    B >= 1024 and is left to tests/test_gpu_backward_input_small.py."""
    out = []
    for io in BC.IO3:
        out.append(_multi(B=3, C=3, H=16, W=16, io=io, layers=2))
    out.append(_small(B=3, C=3, H=16, W=16, steps=2, io="f16", mode=2, split="lie", emit=BC._all_but_last(2)))
    out.append(_small(B=5, C=4, H=32, W=32, steps=2, io="f32", mode=2, skip=True))
    out.append(_small(B=1, C=1, H=28, W=28, steps=2, io="bf16", mode=1))
    return out


TABLE_CASES = _table_cases()
MATRIX_CASES = _matrix_cases()


def header_functions():
    """``bounds_cases.header_functions()`` with the functions of include/pdecnn_small_input.h added."""
    import os
    import re
    out = dict(BC.header_functions())
    src = open(os.path.join(BC.ROOT, "include", "pdecnn_small_input.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for m in re.finditer(r"\b(pde_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        params = []
        for q in m.group(2).split(","):
            q = " ".join(q.split())
            if q in ("", "void"):
                continue
            name = re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(\[\d*\])?$", q).group(1)
            params.append((name, "*" in q or "[" in q, q.startswith("const ")))
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = params
    return out
