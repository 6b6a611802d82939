"""Bounds cases of the input-only backward of the explicit 5-point and the Jacobi layers (include/pdecnn_explicit_input.h:
pde_explicit5[_f64]_backward_input[_states], pde_jacobi_io_backward_input[_states], pde_jacobi_f64_backward_input[_states]),
as an extension of the case table of tests/bounds_cases.py kept in a file of its own — the pattern of
tests/bounds_input_mixed_cases.py.

Every case is a case of that table's ``explicit`` or ``jacobi`` family, built by the table's builder unchanged, so the
full forward and backward run first; then the new call runs on the same ``gout`` (and ``gtraj`` / ``gstates`` and mask) with
an output of its own, ``gu_input``, and a workspace ``iws`` of exactly the queried size — none where the query is 0.  One
case per dispatch, each plain and emitting: register planes (one launch), float4 columns, scalar columns, the
one-workgroup Jacobi kernel, the tiled one over two launches, float64.

tests/test_gpu_bounds_input_explicit.py compares ``gu_input`` bit for bit with the full call's ``gu`` of the same case.
The cases are NOT appended to ``bounds_cases.CASES``: that table, and the tests that hold it to pdecnn.h, stay what they
were; tests/test_bounds_input_explicit_cases.py applies the table's checks of a case to these."""
import bounds_cases as BC

NEW_FUNCTIONS = ["pde_explicit5_backward_input", "pde_explicit5_backward_input_states", "pde_explicit5_f64_backward_input",
                 "pde_explicit5_f64_backward_input_states", "pde_jacobi_io_backward_input", "pde_jacobi_io_backward_input_states",
                 "pde_jacobi_f64_backward_input", "pde_jacobi_f64_backward_input_states"]
#: host queries: no device memory
QUERIES = ["pde_explicit5_backward_input_workspace_bytes", "pde_explicit5_f64_backward_input_workspace_bytes",
           "pde_jacobi_io_backward_input_workspace_bytes"]
HEADER = "pdecnn_explicit_input.h"


def query(case):
    """The new call's workspace query for the case's dimensions."""
    lib, p = BC.lib(), case.p
    if case.family == "explicit":
        if p["io"] == "f64":
            return lib.pde_explicit5_f64_backward_input_workspace_bytes(p["B"], p["C"], p["H"], p["W"], p["nt"])
        return lib.pde_explicit5_backward_input_workspace_bytes(p["B"], p["C"], p["H"], p["W"], BC.IO[p["io"]][0], p["nt"])
    if p["api"].startswith("f64"):
        return 0                                                 # the float64 Jacobi calls take no workspace
    return lib.pde_jacobi_io_backward_input_workspace_bytes(p["B"], p["H"], p["W"], p["nt"], BC.IO[p["io"]][0])


class InputCase(BC.Case):
    def build(self, ctx):
        p = dict(self.p)
        calls, expect = BC.BUILDERS[self.family](ctx, p)
        calls = list(calls)
        full = calls[-1][0] if self.family == "explicit" else calls[1][0]
        assert "_backward" in full
        ctx.out("gu_input", ctx.shapes["gu"], ctx.dtypes["gu"], param="gu")
        a = {"gu": "gu_input"}
        if not (self.family == "jacobi" and p["api"].startswith("f64")):
            n = query(self)
            a.update(workspace=None, workspace_bytes=0)
            if n:
                a.update(workspace="iws", workspace_bytes=ctx.ws("iws", n))
        calls.append((full.replace("_backward", "_backward_input"), a))
        return calls, expect


def twins(case):
    """(buffer of the new call, buffer of the full call it must equal bit for bit)"""
    return [("gu_input", "gu")]


def _cases():
    out = []
    B4 = BC._all_but_last(4)

    def ex(H, W, io, nt, emit=0, B=3, Cc=2):
        tag = f"em{emit:x}" if emit else f"nt{nt}"
        p = dict(B=B, C=Cc, H=H, W=W, io=io, nt=nt)
        if emit:
            p["emit"] = emit
        out.append(InputCase(f"explicit-input-{H}x{W}-b{B}c{Cc}-{io}-{tag}", "explicit", p))

    # register planes: one launch; B * C = 3 and 6 planes leave the last workgroup of four waves ragged
    for (H, W), io, B, Cc in (((16, 16), "f32", 3, 2), ((32, 32), "bf16", 3, 1), ((64, 64), "f16", 1, 3)):
        ex(H, W, io, 3, B=B, Cc=Cc)
        ex(H, W, io, 4, emit=B4, B=B, Cc=Cc)
    ex(16, 16, "f32", 1)
    # float4 columns (one launch per step through the two fp32 buffers), then scalar columns
    for (H, W), ios in (((12, 20), BC.IO3), ((5, 7), BC.IO3), ((3, 1), ("f32",))):
        for io in ios:
            ex(H, W, io, 3)
            ex(H, W, io, 4, emit=B4)
    ex(12, 20, "f32", 1)                                         # one step: gout straight to gu, no workspace
    ex(5, 7, "bf16", 1)
    ex(12, 20, "f32", 2)                                         # two steps: one of the two buffers
    for H, W in ((5, 7), (16, 16)):
        ex(H, W, "f64", 1)
        ex(H, W, "f64", 3)
        ex(H, W, "f64", 4, emit=B4)

    def jac(H, W, io, nt, api, emit=0, B=3):
        path = 2 if max(H, W) > 64 else 1
        p = dict(B=B, H=H, W=W, nt=nt, io=io, api=api, path=path)
        if emit:
            p["emit"] = emit
        out.append(InputCase(f"jacobi-input-{api}-{H}x{W}-{io}-nt{nt}" + (f"-em{emit:x}" if emit else ""), "jacobi", p))

    # the one-workgroup kernel
    for (H, W), io in (((4, 4), "f32"), ((5, 7), "f16"), ((64, 64), "bf16"), ((48, 48), "f32")):
        jac(H, W, io, 10, "io")
        jac(H, W, io, 10, "states", emit=BC._all_but_last(10))
    jac(5, 7, "f32", 10, "states", emit=BC._bits(0))
    # the tiled kernel: one launch (nt = 10), two launches (nt = 12; the emitted states 10 and 11 straddle the boundary)
    for (H, W), io in (((65, 8), "f32"), ((97, 130), "f16"), ((65, 65), "bf16")):
        jac(H, W, io, 10, "io")
        jac(H, W, io, 12, "ws")
        jac(H, W, io, 12, "states", emit=BC._bits(0, 9, 10))
    for H, W in ((5, 7), (64, 64)):
        jac(H, W, "f64", 10, "f64")
        jac(H, W, "f64", 10, "f64_states", emit=BC._all_but_last(10))
    return out


CASES = _cases()


def header_functions():
    """``bounds_cases.header_functions()`` with the functions of include/pdecnn_explicit_input.h added."""
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
