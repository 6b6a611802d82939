"""Bounds cases of the input-only backward of the layers with a channel operator above C = 4 (include/pdecnn_mixed_input.h:
pde_channel_mix[_f64]_backward_input, pde_skip_blend[_f64]_backward_input, pde_adi_backward_input_step,
pde_adi_mixed_forward_input, pde_adi_mixed_backward_input), as an extension of the case table of tests/bounds_cases.py kept
in a file of its own — the pattern of tests/bounds_input_small_cases.py.

Every case is a case of that table's family — ``mixed``, ``steps``, ``mix`` or ``blend``, built by the table's builder
unchanged, so the full calls run first — followed by the new calls on the same inputs with outputs of their own
(``*_input``) and workspaces of exactly the queried size:

  mixed   pde_adi_mixed_forward_input into ``y_input`` (it factorises into the same steps workspace, which the full forward
          filled with the same values; scratch ``fiws`` where the query is not 0) and pde_adi_mixed_backward_input into
          ``gu_input`` (scratch ``iws``);
  steps   pde_adi_backward_input_step for k = K-1 .. 0 into ``gi<k>``, the chain the full step calls walk into ``g<k>``;
  mix     pde_channel_mix[_f64]_backward_input into ``gu_input`` (``iws`` where the query is not 0: C = 128 fused);
  blend   pde_skip_blend[_f64]_backward_input into ``g_u0_input`` / ``g_u_input``.

tests/test_gpu_bounds_input_mixed.py compares each ``*_input`` bit for bit with the full call's output of the same case.
The cases are NOT appended to ``bounds_cases.CASES``: that table, and the tests that hold it to pdecnn.h, stay what they
were; tests/test_bounds_input_mixed_cases.py applies the table's checks of a case to these.  None sits behind an
environment switch (the PDE_MIX_* arrangements: tests/test_gpu_backward_input_mixed.py)."""
import ctypes as C

import bounds_cases as BC

NEW_FUNCTIONS = ["pde_adi_backward_input_step", "pde_adi_mixed_backward_input", "pde_adi_mixed_forward_input",
                 "pde_channel_mix_backward_input", "pde_channel_mix_f64_backward_input", "pde_skip_blend_backward_input",
                 "pde_skip_blend_f64_backward_input"]
#: host queries: no device memory
QUERIES = ["pde_adi_mixed_backward_input_one_launch", "pde_adi_mixed_backward_input_workspace_bytes",
           "pde_adi_mixed_forward_input_workspace_bytes", "pde_channel_mix_backward_input_workspace_bytes"]
#: (buffer of the new call, buffer of the full call it must equal bit for bit), per family; ``steps`` adds gi<k> / g<k>
TWINS = {"mixed": [("y_input", "y"), ("gu_input", "gu")], "mix": [("gu_input", "gu")],
         "blend": [("g_u0_input", "g_u0"), ("g_u_input", "g_u")], "steps": []}


class InputCase(BC.Case):
    def build(self, ctx):
        p = dict(self.p)
        calls, expect = BC.BUILDERS[self.family](ctx, p)
        calls = list(calls)
        getattr(self, "_" + self.family)(ctx, p, calls)
        return calls, expect

    def _mixed(self, ctx, p, calls):
        lib = BC.lib()
        d, sps = ctx.values["d"], ctx.values["sweeps_per_step"]
        shape, dt = (p["B"], p["C"], p["H"], p["W"]), BC.IO[p["io"]][1]
        ctx.out("y_input", shape, dt)
        ctx.out("gu_input", shape, dt)
        fa = {"y": "y_input", "steps_workspace": "sws", "steps_workspace_bytes": ctx.shapes["sws"][0],
              "workspace": None, "workspace_bytes": 0}
        nf = lib.pde_adi_mixed_forward_input_workspace_bytes(C.byref(d), sps)
        assert (nf == 0) == bool(p["one_launch"]), (nf, p)      # the one-launch forward needs no scratch
        if nf:
            fa.update(workspace="fiws", workspace_bytes=ctx.ws("fiws", nf))
        ni = ctx.ws("iws", lib.pde_adi_mixed_backward_input_workspace_bytes(C.byref(d), sps))
        assert ni > 0
        calls.append(("pde_adi_mixed_forward_input", fa))
        calls.append(("pde_adi_mixed_backward_input", {"gu": "gu_input", "steps_workspace": "sws", "workspace": "iws",
                                                       "workspace_bytes": ni}))

    def _steps(self, ctx, p, calls):
        shape, dt, K = (p["B"], p["C"], p["H"], p["W"]), BC.IO[p["io"]][1], p["steps"]
        for k in reversed(range(K)):
            ctx.out(f"gi{k}", shape, dt)
            calls.append(("pde_adi_backward_input_step", {"step": k, "gy": f"gi{k + 1}" if k + 1 < K else "gK", "gu": f"gi{k}",
                                                          "steps_workspace": "sws"}))

    def _mix(self, ctx, p, calls):
        lib = BC.lib()
        shape, dt = (p["B"], p["C"], p["HW"]), BC.IO[p["io"]][1]
        ctx.out("gu_input", shape, dt)
        if p["io"] == "f64":
            calls.append(("pde_channel_mix_f64_backward_input", {"gu": "gu_input"}))
            return
        a = {"gu": "gu_input", "workspace": None, "workspace_bytes": 0}
        n = lib.pde_channel_mix_backward_input_workspace_bytes(p["B"], p["C"], p["HW"])
        assert (n > 0) == (p["C"] == 128 and p["HW"] % 4 == 0), (n, p)
        if n:
            a.update(workspace="iws", workspace_bytes=ctx.ws("iws", n))
        calls.append(("pde_channel_mix_backward_input", a))

    def _blend(self, ctx, p, calls):
        dt = BC.IO[p["io"]][1]
        ctx.out("g_u0_input", (p["n"],), dt)
        ctx.out("g_u_input", (p["n"],), dt)
        f = "pde_skip_blend_f64_backward_input" if p["io"] == "f64" else "pde_skip_blend_backward_input"
        calls.append((f, {"g_u0": "g_u0_input", "g_u": "g_u_input"}))


def twins(case):
    out = list(TWINS[case.family])
    if case.family == "steps":
        out += [(f"gi{k}", f"g{k}") for k in range(case.p["steps"])]
    return out


def _mixed(Cc, N, io, mode, one=0, B=3):
    return InputCase(f"mixed-input-c{Cc}-n{N}-b{B}-{io}-m{mode}", "mixed",
                     dict(B=B, C=Cc, H=N, W=N, io=io, steps=2, mode=mode, one_launch=one))


def _cases():
    out = []
    # per-step route: the scalar operator (C = 5) in the three tensor types, the three-piece kernel (32 / 64 / 96 fp32), the
    # fused fp32-MFMA kernel (128 fp32 with its fragment table; 32 / 96 on 16-bit tensors), the 16-bit matrix cores (64 / 128)
    for io in BC.IO3:
        out.append(_mixed(5, 8, io, 1))
        out.append(_mixed(5, 8, io, 2, B=2))
    for Cc, mode in ((32, 1), (64, 2), (96, 1), (128, 2)):
        out.append(_mixed(Cc, 8, "f32", mode))
    for io in ("bf16", "f16"):
        out.append(_mixed(32, 8, io, 2))
        out.append(_mixed(96, 8, io, 1))
        out.append(_mixed(64, 8, io, 1))
        out.append(_mixed(128, 8, io, 2, B=1))
    # the one-launch forward (keep = 0); 28 x 28 leaves the three-piece backward a ragged last 64-pixel tile
    out.append(_mixed(32, 28, "f32", 1, one=1))
    out.append(_mixed(64, 28, "f32", 2, one=1, B=2))
    for io in BC.IO3:
        out.append(InputCase(f"steps-input-n16-c5-{io}", "steps", dict(B=3, C=5, H=16, W=16, io=io, steps=2, ckpt=0)))
    out.append(InputCase("steps-input-n32-c2-f32", "steps", dict(B=3, C=2, H=32, W=32, io="f32", steps=2, ckpt=0)))
    mix = [(1, 1, 1, "f32", "scalar", "scalar"), (33, 2, 49, "bf16", "scalar", "scalar"), (160, 1, 49, "f16", "scalar", "scalar"),
           (160, 2, 196, "f32", "scalar", "scalar"),
           (32, 3, 196, "f32", "mfma32", "split3"), (64, 1, 64, "f32", "mfma32", "split3"), (64, 5, 196, "f32", "mfma32", "split3"),
           (96, 2, 196, "f32", "mfma32", "split3"),
           (128, 1, 64, "f32", "mfma32", "fused"), (128, 3, 196, "f32", "mfma32", "fused"),
           (32, 2, 64, "bf16", "mfma32", "fused"), (64, 5, 196, "bf16", "mfma32", "fused"), (96, 2, 64, "f16", "mfma32", "fused"),
           (128, 3, 196, "f16", "mfma32", "fused"),
           (64, 1, 64, "bf16", "mfma16", "mfma16"), (64, 3, 128, "f16", "mfma16", "mfma16"), (128, 1, 64, "f16", "mfma16", "mfma16"),
           (128, 2, 128, "bf16", "mfma16", "mfma16"),
           (128, 2, 1, "f16", "scalar", "scalar")]
    for Cc, B, HW, io, fp, bp in mix:
        out.append(InputCase(f"mix-input-c{Cc}-b{B}-hw{HW}-{io}", "mix", dict(B=B, C=Cc, HW=HW, io=io, fwd_path=fp, bwd_path=bp)))
    for Cc, B, HW in ((1, 1, 1), (33, 2, 49), (128, 3, 196)):
        out.append(InputCase(f"mix-input-c{Cc}-b{B}-hw{HW}-f64", "mix", dict(B=B, C=Cc, HW=HW, io="f64")))
    for n in (1, 255, 256 * 512 + 3):
        for io in BC.IO3 + ("f64",):
            out.append(InputCase(f"blend-input-n{n}-{io}", "blend", dict(n=n, io=io)))
    return out


CASES = _cases()


def header_functions():
    """``bounds_cases.header_functions()`` with the functions of include/pdecnn_mixed_input.h added."""
    import os
    import re
    out = dict(BC.header_functions())
    src = open(os.path.join(BC.ROOT, "include", "pdecnn_mixed_input.h")).read()
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
