"""Bounds cases of the tangent-linear pass of the explicit 5-point and the Jacobi layers
(include/pdecnn_explicit_tangent.h: pde_explicit5_tangent, pde_explicit5_f64_tangent, pde_jacobi_io_tangent,
pde_jacobi_f64_tangent), as an extension of the case table of tests/bounds_cases.py kept in a file of its own — the
pattern of tests/bounds_tangent_cases.py.

A case declares the tensors of one tangent call — u, du, the two parameter vectors, their two tangents, y, dy — each at
the alignment the header asks of its pointer in THIS call (four elements for the tensors of an explicit call whose W is a
multiple of 4, the element everywhere else; 16 bytes for a workspace), and a workspace ``tws`` of exactly the queried
size — none where the query is 0.  ``tan`` says which of the three tangents are given (the others are NULL), ``no_y``
leaves y NULL.  The family's forward runs first on the same u into ``y_fwd``, which the tangent call's y must equal bit
for bit (``twins``).  One case per dispatch: register planes, float4 columns, single columns, the one-workgroup Jacobi
kernel, the tiled one on both sides of the steps of one launch, float64; every tensor type the family takes.

The cases are NOT appended to ``bounds_cases.CASES``: that table, and the tests that hold it to pdecnn.h, stay what they
were; tests/test_bounds_explicit_tangent_cases.py applies the table's checks of a case to these."""
import torch

import bounds_cases as BC

NEW_FUNCTIONS = ["pde_explicit5_tangent", "pde_explicit5_f64_tangent", "pde_jacobi_io_tangent", "pde_jacobi_f64_tangent"]
#: host queries: no device memory
QUERIES = ["pde_explicit5_tangent_workspace_bytes", "pde_explicit5_f64_tangent_workspace_bytes",
           "pde_jacobi_io_tangent_workspace_bytes"]
HEADER = "pdecnn_explicit_tangent.h"
TANGENTS = {"explicit": ("d_alpha_base", "d_channel_scaling"), "jacobi": ("d_a_row", "d_b_col")}
#: ``tan`` -> (du given, parameter tangents given, by position)
MODES = {"all": (True, (0, 1)), "du": (True, ()), "params": (False, (0, 1)), "one": (False, (1,)), "du+one": (True, (0,))}
WAVE = ((16, 16), (32, 32), (64, 64))


def query(case):
    """The call's workspace query for the case's dimensions."""
    lib, p = BC.lib(), case.p
    if case.family == "explicit":
        if p["io"] == "f64":
            return lib.pde_explicit5_f64_tangent_workspace_bytes(p["B"], p["C"], p["H"], p["W"], p["nt"])
        return lib.pde_explicit5_tangent_workspace_bytes(p["B"], p["C"], p["H"], p["W"], BC.IO[p["io"]][0], p["nt"])
    if p["io"] == "f64":
        return 0                                                 # the float64 Jacobi call takes no workspace
    return lib.pde_jacobi_io_tangent_workspace_bytes(p["B"], p["H"], p["W"], p["nt"], BC.IO[p["io"]][0])


def _tangent_args(ctx, case, names, with_du, given):
    a = {"du": "du" if with_du else None, "y": None if case.p.get("no_y") else "y"}
    a.update({k: (k if i in given else None) for i, k in enumerate(names)})
    if not (case.family == "jacobi" and case.p["io"] == "f64"):
        n = query(case)
        a.update(workspace=None, workspace_bytes=0)
        if n:
            a.update(workspace="tws", workspace_bytes=ctx.ws("tws", n))
    return a


class ExplicitTangentCase(BC.Case):
    def build(self, ctx):
        p = dict(self.p)
        g = BC._gen(p)
        B, Cc, H, W, nt, f64 = p["B"], p["C"], p["H"], p["W"], p["nt"], p["io"] == "f64"
        code, dt = BC.IO[p["io"]]
        pt = torch.float64 if f64 else torch.float32
        names = TANGENTS["explicit"]
        with_du, given = MODES[p["tan"]]
        ctx.vec_elems = 1 if (f64 or W % 4) else 4               # float4 rows: four elements per access, 8 bytes of 16-bit ones
        ctx.also_element = BC.ELEMENT_ALIGNED_IN["pde_explicit5_"] | frozenset(names)
        for k, v in (("B", B), ("C", Cc), ("H", H), ("W", W), ("io_dtype", code), ("num_steps", nt), ("dt", 0.01), ("eps", 1e-6),
                     ("max_coeff", 0.15), ("relax", 0.1)):
            ctx.val(k, v)
        shape = (B, Cc, H, W)
        ctx.inp("u", torch.randn(shape, generator=g), dt)
        if with_du:
            ctx.inp("du", torch.randn(shape, generator=g), dt)
        ctx.inp("alpha_base", 0.05 + 0.1 * torch.rand(Cc, generator=g), pt)
        ctx.inp("channel_scaling", 1 + 0.1 * torch.randn(Cc, generator=g), pt)
        for i, k in enumerate(names):
            if i in given:
                ctx.inp(k, torch.randn(Cc, generator=g), pt)
        if not p.get("no_y"):
            ctx.out("y", shape, dt, param="out")
        ctx.out("dy", shape, dt, param="out")
        ctx.out("y_fwd", shape, dt, param="out")
        st = {"states": None}
        if nt > 1:
            ctx.out("states", (nt - 1,) + shape, pt)             # the forward's own chain for generic sizes (fp32 / doubles)
            st = {}
        f = "pde_explicit5_f64_" if f64 else "pde_explicit5_"
        calls = [(f + "forward", dict(st, out="y_fwd"))]
        calls.append((f + "tangent", _tangent_args(ctx, self, names, with_du, given)))
        return calls, []


class JacobiTangentCase(BC.Case):
    def build(self, ctx):
        l = BC.lib()
        p = dict(self.p)
        g = BC._gen(p)
        B, H, W, nt, f64 = p["B"], p["H"], p["W"], p["nt"], p["io"] == "f64"
        code, dt = BC.IO[p["io"]]
        pt = torch.float64 if f64 else torch.float32
        names = TANGENTS["jacobi"]
        with_du, given = MODES[p["tan"]]
        ctx.vec_elems = 1                                        # the Jacobi kernels move one element at a time
        ctx.also_element = frozenset(names)
        for k, v in (("B", B), ("H", H), ("W", W), ("nt", nt), ("io_dtype", code)):
            ctx.val(k, v)
        ctx.inp("u", torch.randn(B, H, W, generator=g), dt)
        if with_du:
            ctx.inp("du", torch.randn(B, H, W, generator=g), dt)
        ctx.inp("a_row", 0.05 + 0.15 * torch.rand(H, generator=g), pt)
        ctx.inp("b_col", 0.05 + 0.15 * torch.rand(W, generator=g), pt)
        for i, (k, n) in enumerate(zip(names, (H, W))):
            if i in given:
                ctx.inp(k, 0.1 * torch.randn(n, generator=g), pt)
        if not p.get("no_y"):
            ctx.out("y", (B, H, W), dt, param="out")
        ctx.out("dy", (B, H, W), dt, param="out")
        ctx.out("y_fwd", (B, H, W), dt, param="out")
        expect = []
        if f64:
            calls = [("pde_jacobi_f64_forward", {"out": "y_fwd"})]
        else:
            expect = [("pde_jacobi_plane_path", (H, W), p["path"])]
            nf = l.pde_jacobi_forward_workspace_bytes(B, H, W, nt)
            fa = {"out": "y_fwd", "workspace": None, "workspace_bytes": 0}
            if nf:
                fa.update(workspace="fws", workspace_bytes=ctx.ws("fws", nf))
            calls = [("pde_jacobi_io_forward_ws", fa)]
        calls.append(("pde_jacobi_f64_tangent" if f64 else "pde_jacobi_io_tangent",
                      _tangent_args(ctx, self, names, with_du, given)))
        return calls, expect


def twins(case):
    """(buffer of the tangent call, buffer of the forward it must equal bit for bit)"""
    return [] if case.p.get("no_y") else [("y", "y_fwd")]


def _cases():
    out = []
    modes = ("all", "params", "one", "du+one", "du")
    n = [0]

    def ex(H, W, io, nt, B=3, Cc=2, tan=None, **kw):
        tan = tan or modes[n[0] % len(modes)]
        n[0] += 1
        p = dict(B=B, C=Cc, H=H, W=W, io=io, nt=nt, tan=tan, **kw)
        out.append(ExplicitTangentCase(f"explicit-tangent-{H}x{W}-b{B}c{Cc}-{io}-nt{nt}-{tan}" + ("-noy" if kw.get("no_y") else ""),
                                       "explicit", p))

    # register planes: one launch; B * C = 6, 3 and 3 planes leave the last workgroup of four waves ragged
    ex(16, 16, "f32", 3)
    ex(32, 32, "bf16", 2, Cc=1)
    ex(64, 64, "f16", 2, B=1, Cc=3)
    ex(16, 16, "f32", 1, tan="one", no_y=True)
    # float4 columns (one launch per step through the four fp32 images), then single columns
    for io in BC.IO3:
        ex(12, 20, io, 3)
    ex(12, 20, "f32", 1)                                         # one step: no workspace
    ex(12, 20, "f32", 2, tan="all", no_y=True)                   # two steps: one image of each pair
    ex(1, 4, "f32", 2)
    for io in BC.IO3:
        ex(5, 7, io, 3)
    ex(3, 1, "f32", 3)
    ex(5, 7, "bf16", 1)
    ex(1, 1, "f32", 2, tan="all")
    ex(5, 7, "f64", 1)
    ex(5, 7, "f64", 3)
    ex(16, 16, "f64", 3, tan="all", no_y=True)

    def jac(H, W, io, nt, B=3, tan=None, **kw):
        tan = tan or modes[n[0] % len(modes)]
        n[0] += 1
        p = dict(B=B, H=H, W=W, nt=nt, io=io, tan=tan, path=2 if max(H, W) > 64 else 1, **kw)
        out.append(JacobiTangentCase(f"jacobi-tangent-{H}x{W}-b{B}-{io}-nt{nt}-{tan}" + ("-noy" if kw.get("no_y") else ""),
                                     "jacobi", p))

    # the one-workgroup kernel
    jac(4, 4, "f32", 10)
    jac(5, 7, "f16", 10)
    jac(64, 64, "bf16", 10, tan="all")                          # the largest LDS image
    jac(48, 48, "f32", 10, no_y=True)
    jac(5, 7, "f32", 0, tan="du")                                # no step: y = u, dy = du
    # the tiled kernel: one launch (nt = 10), chained launches (nt = 11, 12, 21) through the four fp32 images
    jac(65, 8, "f32", 10)
    jac(65, 8, "f32", 12, tan="all")
    jac(97, 130, "f16", 12)
    jac(65, 65, "bf16", 11, B=1, no_y=True)
    jac(70, 66, "f32", 21, B=1)
    jac(5, 7, "f64", 10)
    jac(64, 64, "f64", 10, B=2, tan="all")
    jac(9, 4, "f64", 3, no_y=True)
    return out


CASES = _cases()


def header_functions():
    """``bounds_cases.header_functions()`` with the functions of include/pdecnn_explicit_tangent.h added."""
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
