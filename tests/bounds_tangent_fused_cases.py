"""Bounds cases of the tangent-linear pass on the fused two-sided solver (include/pdecnn_tangent_fused.h:
pde_adi_tangent_fused), as an extension of the case table of tests/bounds_cases.py kept in a file of its own — the pattern of
tests/bounds_tangent_cases.py.

A case declares the tensors of one call — u, du, the four parameters (the table's own ``_adi_params``), their four tangents,
y, dy — every one of them at 16 bytes, which is what the header asks of this call (its kernels read 16 bytes wide), and a
workspace ``tws`` of exactly the queried size.  ``tan`` says which of the five tangents are given (the others are NULL),
``no_y`` leaves y NULL.  The fused forward runs first on the same u into ``y_fwd``, which the tangent call's y must equal
bit for bit (``twins``).  One case per dispatch: every fused line length, every tensor type, one plane, a ragged second chunk
(B = 17: sixteen planes per workgroup iteration), records resident (one step) and staged through the ring (two steps and
more), with and without the dco ring.

The cases are NOT appended to ``bounds_cases.CASES``: that table, and the tests that hold it to pdecnn.h, stay what they
were; tests/test_bounds_tangent_fused_cases.py applies the table's checks of a case to these."""
import ctypes as C

import torch

import bounds_cases as BC
from bounds_tangent_cases import MODES, TANGENTS

NEW_FUNCTIONS = ["pde_adi_tangent_fused"]
#: host queries: no device memory
QUERIES = ["pde_adi_tangent_fused_workspace_bytes"]
HEADER = "pdecnn_tangent_fused.h"
FUSED = (8, 12, 16, 20, 24, 28, 32)


def query(case):
    """The call's workspace query for the case's descriptor."""
    return BC.lib().pde_adi_tangent_fused_workspace_bytes(C.byref(BC._adi_desc(case.p)))


def build_tangent(ctx, p):
    l = BC.lib()
    g = BC._gen(p)
    dt = BC.IO[p["io"]][1]
    d = ctx.val("d", BC._adi_desc(p))
    shape = (p["B"], p["C"], p["H"], p["W"])
    with_du, names = MODES[p["tan"]]
    ctx.inp("u", torch.randn(shape, generator=g), dt)
    if with_du:
        ctx.inp("du", torch.randn(shape, generator=g), dt)
    BC._adi_params(ctx, p, g)
    for k in names:
        ctx.inp(k, torch.randn(shape[1:], generator=g), torch.float32)
    if not p.get("no_y"):
        ctx.out("y", shape, dt)
    ctx.out("dy", shape, dt, param="y")
    ctx.out("y_fwd", shape, dt, param="y")
    nf = ctx.ws("fws", l.pde_adi_forward_workspace_bytes(C.byref(d)))
    calls = [("pde_adi_forward", {"y": "y_fwd", "kappa_max": None, "workspace": "fws", "workspace_bytes": nf})]
    n = ctx.ws("tws", l.pde_adi_tangent_fused_workspace_bytes(C.byref(d)))
    assert n > 0
    a = {"du": "du" if with_du else None, "y": None if p.get("no_y") else "y", "workspace": "tws", "workspace_bytes": n}
    a.update({k: (k if k in names else None) for k in TANGENTS})
    calls.append(("pde_adi_tangent_fused", a))
    return calls, []


class TangentFusedCase(BC.Case):
    def build(self, ctx):
        return build_tangent(ctx, dict(self.p))


def twins(case):
    """(buffer of the tangent call, buffer of the forward it must equal bit for bit)"""
    return [] if case.p.get("no_y") else [("y", "y_fwd")]


def _cases():
    out = []

    def add(N, io, tan, B=3, Cc=2, steps=1, split="strang", **kw):
        p = dict(B=B, C=Cc, H=N, W=N, io=io, steps=steps, split=split, tan=tan, dt=0.05, clampmove=True, **kw)
        out.append(TangentFusedCase(f"tangent-fused-n{N}-b{B}c{Cc}-{io}-{BC._sched_id(steps, split)}-{tan}" +
                                    ("-noy" if kw.get("no_y") else ""), "adi", p))

    modes = ("all", "params", "one", "du+one", "du")
    for i, N in enumerate(FUSED):
        add(N, BC.IO3[i % 3], modes[i % len(modes)], steps=1 + i % 2, split=("strang", "lie")[i % 2])
    add(8, "f32", "all", B=1, Cc=1)                               # one plane: seven waves idle
    add(12, "bf16", "params", B=17, Cc=3, steps=2)                # a second, ragged chunk; the ring turns over
    add(32, "f32", "all", B=17, Cc=1, steps=4)                    # twelve sweeps through three slots
    add(28, "f16", "all", B=2, Cc=9, split="lie", steps=3)
    add(32, "f32", "params", no_y=True)
    add(16, "bf16", "all", B=1, Cc=1, steps=2, no_y=True)
    add(32, "f16", "du", B=5, Cc=8, steps=2)                      # the XCD-ordered block map (C a multiple of 8)
    return out


CASES = _cases()


def header_functions():
    """``bounds_cases.header_functions()`` with the functions of include/pdecnn_tangent_fused.h added."""
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
