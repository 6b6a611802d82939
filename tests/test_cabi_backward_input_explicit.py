"""The input-only backward of the explicit 5-point and the Jacobi layers (include/pdecnn_explicit_input.h) on a machine
without a GPU: the third header is included by pdecnn.h, header, ctypes table and exports agree, the workspace queries are
0 where the header says so, and every refusal the header names is answered on the host with the code it states.  Addresses
are made up; the refusal codes are checked in a child interpreter that sees no device, so that a refusal that is missing
ends in PDE_E_LAUNCH instead of a kernel on made-up addresses."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

from test_cabi import declared_functions

NEW = ["pde_explicit5_backward_input_workspace_bytes", "pde_explicit5_backward_input", "pde_explicit5_backward_input_states",
       "pde_explicit5_f64_backward_input_workspace_bytes", "pde_explicit5_f64_backward_input",
       "pde_explicit5_f64_backward_input_states", "pde_jacobi_io_backward_input_workspace_bytes", "pde_jacobi_io_backward_input",
       "pde_jacobi_io_backward_input_states", "pde_jacobi_f64_backward_input", "pde_jacobi_f64_backward_input_states"]
BADARG, SWEEPS, LAUNCH, WORKSPACE = -1, -3, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_in_the_new_header():
    src = open(os.path.join(ROOT, "include", "pdecnn_explicit_input.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): len([q for q in m.group(2).split(",") if q.strip() not in ("", "void")])
            for m in re.finditer(r"\b(pde_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}


def test_the_symbols_exist_and_are_bound():
    """Declared in include/pdecnn_explicit_input.h, which pdecnn.h includes; bound in ``_lib.SIGNATURES_EXPLICIT_INPUT``."""
    from cnn_with_pde_amd import _lib
    assert '#include "pdecnn_explicit_input.h"' in open(os.path.join(ROOT, "include", "pdecnn.h")).read()
    hdr = declared_in_the_new_header()
    assert sorted(hdr) == sorted(NEW) == sorted(_lib.SIGNATURES_EXPLICIT_INPUT)
    assert sorted(_lib.SIGNATURES) == declared_functions()          # pdecnn.h itself declares what it declared
    others = set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SMALL_INPUT) | set(_lib.SIGNATURES_MIXED_INPUT)
    assert not set(NEW) & others
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n), f"{n} not exported"
    bound = _lib.load()
    sig = dict(_lib.SIGNATURES, **_lib.SIGNATURES_EXPLICIT_INPUT)
    for n in NEW:
        assert getattr(bound, n).argtypes == sig[n][1]
        assert len(sig[n][1]) == hdr[n], n
    # the plain call is the _states call without (cotangents of the emitted states, emit_mask); the _states call is the full
    # one without u, [states,] and the two parameter gradients
    for fam, dropped in (("pde_explicit5_", 4), ("pde_explicit5_f64_", 4), ("pde_jacobi_io_", 3)):
        assert len(sig[fam + "backward_input_states"][1]) == len(sig[fam + "backward_input"][1]) + 2
        assert len(sig[fam + "backward_input_states"][1]) == len(sig[fam + "backward_states"][1]) - dropped
        assert sig[fam + "backward_input_workspace_bytes"][1] == sig[fam + "backward_workspace_bytes"][1]
    assert len(sig["pde_jacobi_f64_backward_input_states"][1]) == len(sig["pde_jacobi_f64_backward_input"][1]) + 2
    assert len(sig["pde_jacobi_f64_backward_input_states"][1]) == len(sig["pde_jacobi_f64_backward_states"][1]) - 5   # no workspace


def test_workspace_queries():
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    up = lambda n: -(-n // 256) * 256                                                                     # noqa: E731
    ex, ex64, jac = (lib.pde_explicit5_backward_input_workspace_bytes, lib.pde_explicit5_f64_backward_input_workspace_bytes,
                     lib.pde_jacobi_io_backward_input_workspace_bytes)
    for io in (_lib.PDE_IO_F32, _lib.PDE_IO_BF16, _lib.PDE_IO_F16):
        for N in (16, 32, 64):
            for steps in (1, 3, 130):
                assert ex(5, 3, N, N, io, steps) == 0                        # register planes
        for H, W in ((5, 7), (12, 20), (60, 64)):
            assert ex(5, 3, H, W, io, 1) == 0                                # one step: gout straight to gu
            for steps in (2, 3, 130):
                assert ex(5, 3, H, W, io, steps) == 2 * up(5 * 3 * H * W * 4)
                assert ex(5, 3, H, W, io, steps) < lib.pde_explicit5_backward_workspace_bytes(5, 3, H, W, io, steps)
        for H, W in ((4, 4), (5, 9), (48, 48), (64, 64)):
            for nt in (0, 1, 10, 130):
                assert jac(3, H, W, nt, io) == 0                             # plane path 1
        for H, W in ((65, 4), (4, 65), (224, 224), (1024, 1024)):
            for nt in (0, 1, 10, 11, 130):
                assert lib.pde_jacobi_plane_path(H, W) == 2
                assert jac(3, H, W, nt, io) == 2 * up(3 * (H + 2) * (W + 2) * 4)
                assert jac(3, H, W, nt, io) < lib.pde_jacobi_io_backward_workspace_bytes(3, H, W, nt, io)
    assert ex64(5, 3, 16, 16, 1) == 0 and ex64(5, 3, 5, 7, 1) == 0
    assert ex64(5, 3, 16, 16, 3) == 2 * up(5 * 3 * 16 * 16 * 8)
    assert ex64(5, 3, 16, 16, 3) < lib.pde_explicit5_f64_backward_workspace_bytes(5, 3, 16, 16, 3)
    # what the calls refuse
    assert ex(0, 3, 5, 7, 0, 3) == 0 and ex(5, 3, 5, 0, 0, 3) == 0 and ex(5, 3, 5, 7, 0, 0) == 0
    assert ex64(5, 0, 5, 7, 3) == 0
    assert jac(3, 65, 3, 3, 0) == 0 and jac(3, 65, 1025, 3, 0) == 0 and jac(3, 65, 65, -1, 0) == 0 and jac(3, 65, 65, 3, 9) == 0


CHILD = r"""
import ctypes as C, json, sys
sys.path[:0] = [%(root)r, %(here)r]
import torch
assert not torch.cuda.is_available(), "the refusals must be answered without a device"
from cnn_with_pde_amd import _lib
import test_cabi_backward_input_explicit as T
json.dump(T.refusals(_lib.load(), _lib), open(sys.argv[1], "w"))
"""


def refusals(lib, L):
    """{what: (answer, expected)} — run in the child."""
    BIG = 1 << 40
    p = C.c_void_p(1 << 41)
    p2 = C.c_void_p((1 << 41) + (1 << 32))
    w = C.c_void_p((1 << 41) + (1 << 33))
    out = {}

    def put(what, got, want):
        assert what not in out
        out[what] = (got, want)

    def off(q, n):
        return C.c_void_p(q.value + n)

    def mask(*bits):
        v = sum(1 << b for b in bits)
        return (C.c_uint64 * 2)(v & (2 ** 64 - 1), v >> 64)

    F32, BF16 = L.PDE_IO_F32, L.PDE_IO_BF16

    def ex(B=2, Cc=2, H=5, W=7, io=F32, gout=p, a=p, s=p, steps=3, gu=p2, ws=w, n=BIG):
        return lib.pde_explicit5_backward_input(B, Cc, H, W, io, gout, a, s, 0.01, 1e-6, 0.15, 0.1, steps, gu, ws, n, None)

    def ex_s(B=2, Cc=2, H=5, W=7, io=F32, gout=p, gtraj=p, em=mask(0), a=p, s=p, steps=3, gu=p2, ws=w, n=BIG):
        return lib.pde_explicit5_backward_input_states(B, Cc, H, W, io, gout, gtraj, em, a, s, 0.01, 1e-6, 0.15, 0.1, steps, gu,
                                                       ws, n, None)

    def ex64(B=2, Cc=2, H=5, W=7, gout=p, a=p, s=p, steps=3, gu=p2, ws=w, n=BIG):
        return lib.pde_explicit5_f64_backward_input(B, Cc, H, W, gout, a, s, 0.01, 1e-6, 0.15, 0.1, steps, gu, ws, n, None)

    def ex64_s(B=2, Cc=2, H=5, W=7, gout=p, gtraj=p, em=mask(0), a=p, s=p, steps=3, gu=p2, ws=w, n=BIG):
        return lib.pde_explicit5_f64_backward_input_states(B, Cc, H, W, gout, gtraj, em, a, s, 0.01, 1e-6, 0.15, 0.1, steps, gu,
                                                           ws, n, None)

    def jac(B=2, H=65, W=8, nt=3, io=F32, gout=p, a=p, b=p, gu=p2, ws=w, n=BIG):
        return lib.pde_jacobi_io_backward_input(B, H, W, nt, io, gout, a, b, gu, ws, n, None)

    def jac_s(B=2, H=65, W=8, nt=3, io=F32, gout=p, gs=p, em=mask(0), a=p, b=p, gu=p2, ws=w, n=BIG):
        return lib.pde_jacobi_io_backward_input_states(B, H, W, nt, io, gout, gs, em, a, b, gu, ws, n, None)

    def jac64(B=2, H=5, W=9, nt=3, gout=p, a=p, b=p, gu=p2):
        return lib.pde_jacobi_f64_backward_input(B, H, W, nt, gout, a, b, gu, None)

    def jac64_s(B=2, H=5, W=9, nt=3, gout=p, gs=p, em=mask(0), a=p, b=p, gu=p2):
        return lib.pde_jacobi_f64_backward_input_states(B, H, W, nt, gout, gs, em, a, b, gu, None)

    calls = {"ex": ex, "ex_s": ex_s, "ex64": ex64, "ex64_s": ex64_s, "jac": jac, "jac_s": jac_s, "jac64": jac64, "jac64_s": jac64_s}
    # a well-formed call gets past validation: with no device its launch fails
    for k, f in calls.items():
        put(f"{k} well-formed", f(), LAUNCH)
    put("ex register plane without a workspace", ex(H=16, W=16, ws=None, n=0), LAUNCH)
    put("ex one step without a workspace", ex(steps=1, ws=None, n=0), LAUNCH)
    put("ex 130 steps", ex(steps=130), LAUNCH)
    put("ex_s NULL mask and no gtraj", ex_s(gtraj=None, em=None), LAUNCH)
    put("ex_s empty mask and no gtraj", ex_s(gtraj=None, em=mask()), LAUNCH)
    put("ex_s empty mask, 130 steps", ex_s(gtraj=None, em=mask(), steps=130), LAUNCH)
    put("ex_s 128 steps, bit 126", ex_s(em=mask(126), steps=128), LAUNCH)
    put("ex64 one step without a workspace", ex64(steps=1, ws=None, n=0), LAUNCH)
    put("jac plane path 1 without a workspace", jac(H=5, W=9, ws=None, n=0), LAUNCH)
    put("jac nt = 0", jac(nt=0), LAUNCH)
    put("jac_s NULL mask and no gstates", jac_s(gs=None, em=None), LAUNCH)
    put("jac_s path 1, bf16", jac_s(H=5, W=9, io=BF16, ws=None, n=0), LAUNCH)
    put("jac64_s NULL mask and no gstates", jac64_s(gs=None, em=None), LAUNCH)
    # NULL required pointers
    for k, f in calls.items():
        put(f"{k} no gout", f(gout=None), BADARG)
        put(f"{k} no gu", f(gu=None), BADARG)
        put(f"{k} no first parameter", f(a=None), BADARG)
        if k.startswith("ex"):
            put(f"{k} no channel_scaling", f(s=None), BADARG)
        else:
            put(f"{k} no b_col", f(b=None), BADARG)
    # dimensions
    for k in ("ex", "ex_s", "ex64", "ex64_s"):
        f = calls[k]
        put(f"{k} B = 0", f(B=0), BADARG)
        put(f"{k} C = 0", f(Cc=0), BADARG)
        put(f"{k} H = 0", f(H=0), BADARG)
        put(f"{k} W = 0", f(W=0), BADARG)
        put(f"{k} no steps", f(steps=0), BADARG)
    for k in ("jac", "jac_s", "jac64", "jac64_s"):
        f = calls[k]
        put(f"{k} B = 0", f(B=0), BADARG)
        put(f"{k} W = 0", f(W=0), BADARG)
        put(f"{k} H = 0", f(H=0), BADARG)
        put(f"{k} nt < 0", f(nt=-1), BADARG)
    put("jac H = 3", jac(H=3), BADARG)
    put("jac W above the tiled limit", jac(W=L.PDE_JACOBI_MAX_HW + 1), BADARG)
    put("jac64 above 64 x 64", jac64(H=65), BADARG)
    put("jac64_s above 64 x 64", jac64_s(W=65), BADARG)
    for k in ("ex", "ex_s", "jac", "jac_s"):
        put(f"{k} float64 tensors", calls[k](io=L.PDE_IO_F64), BADARG)
        put(f"{k} unknown tensor type", calls[k](io=7), BADARG)
    # the emission mask: three steps, so bits 0 and 1 only
    for k, g in (("ex_s", "gtraj"), ("ex64_s", "gtraj"), ("jac_s", "gs"), ("jac64_s", "gs")):
        f = calls[k]
        steps = "steps" if k.startswith("ex") else "nt"
        put(f"{k} mask without the cotangents", f(**{g: None}), BADARG)
        put(f"{k} bit nt-1", f(em=mask(2)), BADARG)
        put(f"{k} bit above nt-1", f(em=mask(5)), BADARG)
        put(f"{k} bit 64", f(em=mask(64)), BADARG)
        put(f"{k} bits 0 and 1", f(em=mask(0, 1)), LAUNCH)
        put(f"{k} one step and a mask", f(em=mask(0), **{steps: 1}), BADARG)
        put(f"{k} 130 steps and a mask", f(em=mask(0), **{steps: 130}), SWEEPS)
        put(f"{k} 129 steps and a mask", f(em=mask(127), **{steps: 129}), SWEEPS)
        put(f"{k} 128 steps, bit 127", f(em=mask(127), **{steps: 128}), BADARG)
        put(f"{k} BADARG comes before the mask", f(gu=None, em=mask(0), **{steps: 130}), BADARG)
    # alignment: float4 rows ask 16 bytes of fp32 tensors and 8 of 16-bit ones, other planes and Jacobi an element
    put("ex float4 rows, gout off by 4", ex(H=12, W=20, gout=off(p, 4)), BADARG)
    put("ex float4 rows, gu off by 8", ex(H=12, W=20, gu=off(p2, 8)), BADARG)
    put("ex float4 rows bf16, gu off by 8 is in order", ex(H=12, W=20, io=BF16, gu=off(p2, 8)), LAUNCH)
    put("ex float4 rows bf16, gu off by 4", ex(H=12, W=20, io=BF16, gu=off(p2, 4)), BADARG)
    put("ex_s float4 rows, gtraj off by 4", ex_s(H=12, W=20, gtraj=off(p, 4)), BADARG)
    put("ex columns, gout off by 4 is in order", ex(gout=off(p, 4)), LAUNCH)
    put("ex columns, gout off by 2", ex(gout=off(p, 2)), BADARG)
    put("ex alpha_base off by 2", ex(a=off(p, 2)), BADARG)
    put("ex channel_scaling off by 1", ex(s=off(p, 1)), BADARG)
    put("ex64 gu off by 4", ex64(gu=off(p2, 4)), BADARG)
    put("ex64_s gtraj off by 4", ex64_s(gtraj=off(p, 4)), BADARG)
    put("ex64 alpha_base off by 4", ex64(a=off(p, 4)), BADARG)
    put("jac gout off by 2", jac(gout=off(p, 2)), BADARG)
    put("jac bf16 gout off by 2 is in order", jac(io=BF16, gout=off(p, 2)), LAUNCH)
    put("jac bf16 gu off by 1", jac(io=BF16, gu=off(p2, 1)), BADARG)
    put("jac a_row off by 2", jac(a=off(p, 2)), BADARG)
    put("jac_s gstates off by 2", jac_s(gs=off(p, 2)), BADARG)
    put("jac64 gu off by 4", jac64(gu=off(p2, 4)), BADARG)
    put("jac64_s gstates off by 4", jac64_s(gs=off(p, 4)), BADARG)
    put("jac64 b_col off by 4", jac64(b=off(p, 4)), BADARG)
    # workspaces
    need = lib.pde_explicit5_backward_input_workspace_bytes(2, 2, 5, 7, F32, 3)
    need64 = lib.pde_explicit5_f64_backward_input_workspace_bytes(2, 2, 5, 7, 3)
    needj = lib.pde_jacobi_io_backward_input_workspace_bytes(2, 65, 8, 3, F32)
    assert need > 0 and need64 > 0 and needj > 0
    for k, nb in (("ex", need), ("ex_s", need), ("ex64", need64), ("ex64_s", need64), ("jac", needj), ("jac_s", needj)):
        f = calls[k]
        put(f"{k} exact workspace", f(n=nb), LAUNCH)
        put(f"{k} short workspace", f(n=nb - 1), WORKSPACE)
        put(f"{k} no workspace", f(ws=None, n=0), WORKSPACE)
        put(f"{k} no workspace but a size", f(ws=None), WORKSPACE)
        put(f"{k} workspace off by 4", f(ws=off(w, 4)), WORKSPACE)
        put(f"{k} BADARG comes before WORKSPACE", f(gu=None, ws=None, n=0), BADARG)
    put("ex register plane, unused workspace off by 4", ex(H=16, W=16, ws=off(w, 4)), WORKSPACE)
    put("jac path 1, unused workspace off by 4", jac(H=5, W=9, ws=off(w, 4)), WORKSPACE)
    put("ex_s the mask comes before the workspace", ex_s(em=mask(2), ws=None, n=0), BADARG)
    put("jac_s the mask comes before the workspace", jac_s(em=mask(2), ws=None, n=0), BADARG)
    put("jac_s 130 steps and a mask come before the workspace", jac_s(nt=130, ws=None, n=0), SWEEPS)
    return out


def test_refusal_codes_without_gpu(tmp_path):
    report = str(tmp_path / "report.json")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": os.path.dirname(here), "here": here}, report], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rep = json.load(open(report))
    assert len(rep) > 150
    wrong = {k: v for k, v in rep.items() if v[0] != v[1]}
    assert not wrong, f"(answer, expected): {wrong}"
    assert sum(1 for v in rep.values() if v[1] == LAUNCH) >= 30       # calls that got past validation
