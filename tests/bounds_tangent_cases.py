"""Bounds cases of the tangent-linear pass of the implicit sweeps (include/pdecnn_tangent.h: pde_adi_tangent,
pde_adi_f64_tangent, pde_adi_rect_tangent, pde_adi_rect_f64_tangent), as an extension of the case table of
tests/bounds_cases.py kept in a file of its own — the pattern of tests/bounds_input_explicit_cases.py.

A case declares the tensors of one tangent call — u, du, the four parameters (the table's own ``_adi_params``), their four
tangents, y, dy — every one of them at its ELEMENT's alignment, which is all the header asks of this call at every plane
size, and a workspace ``tws`` of exactly the queried size.  ``tan`` says which of the five tangents are given (the others
are NULL), ``no_y`` leaves y NULL.  Where the family's forward runs the any-size kernels (every plane but the fused
squares 8, 12, ..., 32 of the fp32 family) the forward runs first on the same u into ``y_fwd``, which the tangent call's y
must equal bit for bit (``twins``).  One case per dispatch: every tensor type, line lengths 2 .. 128 with the kGenBatch
remainders, the fused sizes, thin rectangles, float64 with the planes in LDS and (beyond 100 x 100) with the primal plane
in the workspace.

The cases are NOT appended to ``bounds_cases.CASES``: that table, and the tests that hold it to pdecnn.h, stay what they
were; tests/test_bounds_tangent_cases.py applies the table's checks of a case to these."""
import ctypes as C

import torch

import bounds_cases as BC

NEW_FUNCTIONS = ["pde_adi_tangent", "pde_adi_f64_tangent", "pde_adi_rect_tangent", "pde_adi_rect_f64_tangent"]
#: host queries: no device memory
QUERIES = [f + "_workspace_bytes" for f in NEW_FUNCTIONS]
HEADER = "pdecnn_tangent.h"
TANGENTS = ("d_alpha_base", "d_beta_base", "d_alpha_slope", "d_beta_slope")
#: ``tan`` -> (du given, parameter tangents given)
MODES = {"all": (True, TANGENTS), "du": (True, ()), "params": (False, TANGENTS), "one": (False, ("d_beta_slope",)),
         "du+one": (True, ("d_alpha_base",))}


def query(case):
    """The call's workspace query for the case's descriptor."""
    return getattr(BC.lib(), BC._adi_fam(case.p) + "tangent_workspace_bytes")(C.byref(BC._adi_desc(case.p)))


def has_forward_twin(p):
    """Whether the family's forward of this plane runs the any-size kernels too (then y is its y bit for bit)."""
    return not (BC._adi_fam(p) == "pde_adi_" and BC.fused_line_length(p["H"]))


def build_tangent(ctx, p):
    l = BC.lib()
    g = BC._gen(p)
    dt = BC.IO[p["io"]][1]
    kt = torch.float64 if p["io"] == "f64" else torch.float32
    d = ctx.val("d", BC._adi_desc(p))
    shape = (p["B"], p["C"], p["H"], p["W"])
    fam = BC._adi_fam(p)
    ctx.vec_elems = 1                                            # one element at a time in every kernel of this call
    with_du, names = MODES[p["tan"]]
    ctx.inp("u", torch.randn(shape, generator=g), dt)
    if with_du:
        ctx.inp("du", torch.randn(shape, generator=g), dt)
    BC._adi_params(ctx, p, g)
    for k in names:
        ctx.inp(k, torch.randn(shape[1:], generator=g), kt)
    if not p.get("no_y"):
        ctx.out("y", shape, dt)
    ctx.out("dy", shape, dt, param="y")
    calls = []
    if has_forward_twin(p):
        ctx.out("y_fwd", shape, dt, param="y")
        nf = ctx.ws("fws", getattr(l, fam + "forward_workspace_bytes")(C.byref(d)))
        calls.append((fam + "forward", {"y": "y_fwd", "kappa_max": None, "workspace": "fws", "workspace_bytes": nf}))
    n = ctx.ws("tws", getattr(l, fam + "tangent_workspace_bytes")(C.byref(d)))
    assert n > 0
    a = {"du": "du" if with_du else None, "y": None if p.get("no_y") else "y", "workspace": "tws", "workspace_bytes": n}
    a.update({k: (k if k in names else None) for k in TANGENTS})
    calls.append((fam + "tangent", a))
    return calls, []


class TangentCase(BC.Case):
    def build(self, ctx):
        return build_tangent(ctx, dict(self.p))


def twins(case):
    """(buffer of the tangent call, buffer of the forward it must equal bit for bit)"""
    return [("y", "y_fwd")] if has_forward_twin(case.p) and not case.p.get("no_y") else []


def _cases():
    out = []

    def add(H, W, io, tan, B=3, Cc=2, steps=1, split="strang", **kw):
        rect = H != W
        p = dict(B=B, C=Cc, H=H, W=W, io=io, steps=steps, split=split, tan=tan, dt=0.05, clampmove=True, **kw)
        if rect:
            p["rect"] = True
        size = f"{H}x{W}" if rect else f"n{H}"
        out.append(TangentCase(f"tangent-{size}-b{B}c{Cc}-{io}-{BC._sched_id(steps, split)}-{tan}" +
                               ("-noy" if kw.get("no_y") else ""), "adi", p))

    modes = ("all", "params", "one", "du+one", "du")
    # squares of the fp32 family: the shortest lines, the batch of 8 with and without a remainder, the fused sizes (the
    # any-size kernels here too), one past them, the second wave, the longest line
    for i, N in enumerate((2, 3, 9, 10, 17, 28, 32, 33, 65, 100, 128)):
        add(N, N, BC.IO3[i % 3], modes[i % len(modes)], steps=1 + i % 2, split=("strang", "lie")[i % 2])
    add(12, 12, "f32", "all", no_y=True)
    add(36, 36, "bf16", "params", B=1, Cc=1, no_y=True)
    # rectangles
    for i, (H, W) in enumerate(((5, 9), (2, 128), (128, 2), (128, 3), (5, 12))):
        add(H, W, BC.IO3[i % 3], modes[i % len(modes)], steps=1 + i % 2, split=("lie", "strang")[i % 2])
    # float64: two planes in LDS up to 100 x 100, beyond it the primal plane in the workspace
    for i, N in enumerate((2, 9, 100, 101, 128)):
        add(N, N, "f64", modes[i % len(modes)], steps=1, split=("strang", "lie")[i % 2])
    add(101, 101, "f64", "all", B=1, Cc=1, split="lie", no_y=True)
    add(5, 9, "f64", "all")
    add(81, 128, "f64", "params", split="lie")                   # 81 x 129 doubles twice: beyond the LDS
    add(100, 128, "f64", "du+one", B=1, Cc=3, split="lie")
    return out


CASES = _cases()


def header_functions():
    """``bounds_cases.header_functions()`` with the functions of include/pdecnn_tangent.h added."""
    import os
    import re
    out = dict(BC.header_functions())
    src = open(os.path.join(BC.ROOT, "include", HEADER)).read()
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
