"""The tangent-linear pass of the explicit 5-point and the Jacobi layers (include/pdecnn_explicit_tangent.h) on a machine
without a GPU: the header is included by pdecnn.h, header, ctypes table and exports agree, the workspace queries return the
documented sums, and every refusal the header names is answered on the host with the forward's code.  Addresses are made
up; the refusal codes are checked in a child interpreter that sees no device, so that a refusal that is missing ends in
PDE_E_LAUNCH instead of a kernel on made-up addresses."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

from test_cabi import declared_functions

NEW = ["pde_explicit5_tangent_workspace_bytes", "pde_explicit5_tangent", "pde_explicit5_f64_tangent_workspace_bytes",
       "pde_explicit5_f64_tangent", "pde_jacobi_io_tangent_workspace_bytes", "pde_jacobi_io_tangent", "pde_jacobi_f64_tangent"]
BADARG, LAUNCH, WORKSPACE = -1, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_in_the_new_header():
    src = open(os.path.join(ROOT, "include", "pdecnn_explicit_tangent.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): len([q for q in m.group(2).split(",") if q.strip() not in ("", "void")])
            for m in re.finditer(r"\b(pde_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}


def test_the_symbols_exist_and_are_bound():
    """Declared in include/pdecnn_explicit_tangent.h, which pdecnn.h includes; bound in ``_lib.SIGNATURES_EXPLICIT_TANGENT``."""
    from cnn_with_pde_amd import _lib
    assert '#include "pdecnn_explicit_tangent.h"' in open(os.path.join(ROOT, "include", "pdecnn.h")).read()
    hdr = declared_in_the_new_header()
    assert len(NEW) == 7 and sorted(hdr) == sorted(NEW) == sorted(_lib.SIGNATURES_EXPLICIT_TANGENT)
    assert sorted(_lib.SIGNATURES) == declared_functions()          # pdecnn.h itself declares what it declared
    assert len(_lib.SIGNATURES_TANGENT) == 8
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SMALL_INPUT) | set(_lib.SIGNATURES_MIXED_INPUT) |
              set(_lib.SIGNATURES_EXPLICIT_INPUT) | set(_lib.SIGNATURES_TANGENT))
    assert not set(NEW) & others
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n), f"{n} not exported"
    bound = _lib.load()
    for n in NEW:
        res, args = _lib.SIGNATURES_EXPLICIT_TANGENT[n]
        assert getattr(bound, n).argtypes == args and getattr(bound, n).restype == res
        assert len(args) == hdr[n], n
    T, S = _lib.SIGNATURES_EXPLICIT_TANGENT, _lib.SIGNATURES
    # the forward's leading arguments; the forward's query arguments
    assert T["pde_explicit5_tangent"][1][:5] == S["pde_explicit5_forward"][1][:5]
    assert T["pde_explicit5_tangent_workspace_bytes"] == S["pde_explicit5_backward_workspace_bytes"]
    assert T["pde_explicit5_f64_tangent_workspace_bytes"] == S["pde_explicit5_f64_backward_workspace_bytes"]
    assert T["pde_jacobi_io_tangent"][1][:5] == S["pde_jacobi_io_forward"][1][:5]
    assert T["pde_jacobi_io_tangent_workspace_bytes"] == S["pde_jacobi_io_backward_workspace_bytes"]
    assert _lib.PDE_JACOBI_TANGENT_TILED_K == _lib.PDE_JACOBI_TILED_K
    assert re.search(r"#define\s+PDE_JACOBI_TANGENT_TILED_K\s+PDE_JACOBI_TILED_K\b",
                     open(os.path.join(ROOT, "include", "pdecnn_explicit_tangent.h")).read())
    tiled = open(os.path.join(ROOT, "cnn-with-pde_amd", "csrc", "pde_jacobi_tiled.h")).read()
    assert re.search(r"constexpr int kJTanK = kJK;", tiled)           # the steps per launch, recorded beside the kernel


def test_workspace_queries():
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    up = lambda n: -(-n // 256) * 256                                                                     # noqa: E731
    K = L.PDE_JACOBI_TANGENT_TILED_K
    for B, Cc in ((1, 1), (3, 2), (700, 3)):
        for H, W in ((1, 1), (1, 4), (5, 7), (8, 12), (16, 16), (32, 32), (64, 64), (33, 33), (64, 32), (128, 128)):
            wave = (H, W) in ((16, 16), (32, 32), (64, 64))
            for nt in (1, 2, 3, 10):
                for io in (L.PDE_IO_F32, L.PDE_IO_BF16, L.PDE_IO_F16):
                    want = 0 if (nt == 1 or wave) else 4 * up(B * Cc * H * W * 4)
                    assert lib.pde_explicit5_tangent_workspace_bytes(B, Cc, H, W, io, nt) == want, (B, Cc, H, W, io, nt)
                want = 0 if nt == 1 else 4 * up(B * Cc * H * W * 8)
                assert lib.pde_explicit5_f64_tangent_workspace_bytes(B, Cc, H, W, nt) == want, (B, Cc, H, W, nt)
    for B in (1, 3, 40):
        for H, W in ((4, 4), (5, 9), (64, 64), (65, 4), (4, 65), (65, 65), (130, 67), (1024, 1024)):
            tiled = max(H, W) > 64
            for nt in (0, 1, K - 1, K, K + 1, 2 * K, 2 * K + 1):
                for io in (L.PDE_IO_F32, L.PDE_IO_BF16, L.PDE_IO_F16):
                    want = 4 * up(B * H * W * 4) if (tiled and nt > K) else 0
                    assert lib.pde_jacobi_io_tangent_workspace_bytes(B, H, W, nt, io) == want, (B, H, W, nt, io)
    # what the calls refuse
    for a in ((0, 2, 5, 7, 0, 3), (2, 0, 5, 7, 0, 3), (2, 2, 0, 7, 0, 3), (2, 2, 5, 0, 0, 3), (2, 2, 5, 7, 0, 0), (2, 2, 5, 7, 7, 3),
              (2, 2, 5, 7, L.PDE_IO_F64, 3), (-1, 2, 5, 7, 0, 3)):
        assert lib.pde_explicit5_tangent_workspace_bytes(*a) == 0, a
    for a in ((0, 2, 5, 7, 3), (2, 0, 5, 7, 3), (2, 2, 0, 7, 3), (2, 2, 5, 0, 3), (2, 2, 5, 7, 0), (65536, 2, 5, 7, 3), (2, 65536, 5, 7, 3)):
        assert lib.pde_explicit5_f64_tangent_workspace_bytes(*a) == 0, a
    for a in ((0, 65, 8, 12, 0), (2, 65, 3, 12, 0), (2, 3, 65, 12, 0), (2, 65, L.PDE_JACOBI_MAX_HW + 1, 12, 0), (2, 65, 8, 12, 7),
              (2, 65, 8, 12, L.PDE_IO_F64), (2, 65, 8, -1, 0)):
        assert lib.pde_jacobi_io_tangent_workspace_bytes(*a) == 0, a


CHILD = r"""
import ctypes as C, json, sys
sys.path[:0] = [%(root)r, %(here)r]
import torch
assert not torch.cuda.is_available(), "the refusals must be answered without a device"
from cnn_with_pde_amd import _lib
import test_cabi_explicit_tangent as T
json.dump(T.refusals(_lib.load(), _lib), open(sys.argv[1], "w"))
"""


def refusals(lib, L):
    """{what: (answer, expected)} — run in the child."""
    BIG = 1 << 40
    p = C.c_void_p(1 << 41)
    p1 = C.c_void_p((1 << 41) + (1 << 31))
    p2 = C.c_void_p((1 << 41) + (1 << 32))
    p3 = C.c_void_p((1 << 41) + (1 << 33))
    w = C.c_void_p((1 << 41) + (1 << 34))
    out = {}

    def put(what, got, want):
        assert what not in out
        out[what] = (got, want)

    def off(q, n):
        return C.c_void_p(q.value + n)

    def ex(B=2, Cc=3, H=5, W=8, io=L.PDE_IO_F32, u=p, du=p1, a=p, s=p, da=p, ds=p, nt=3, y=p2, dy=p3, ws=w, n=BIG):
        return lib.pde_explicit5_tangent(B, Cc, H, W, io, u, du, a, s, da, ds, 0.01, 1e-6, 0.15, 0.1, nt, y, dy, ws, n, None)

    def ex64(B=2, Cc=3, H=5, W=8, u=p, du=p1, a=p, s=p, da=p, ds=p, nt=3, y=p2, dy=p3, ws=w, n=BIG):
        return lib.pde_explicit5_f64_tangent(B, Cc, H, W, u, du, a, s, da, ds, 0.01, 1e-6, 0.15, 0.1, nt, y, dy, ws, n, None)

    def jac(B=2, H=9, W=12, nt=3, io=L.PDE_IO_F32, u=p, du=p1, a=p, b=p, da=p, db=p, y=p2, dy=p3, ws=w, n=BIG):
        return lib.pde_jacobi_io_tangent(B, H, W, nt, io, u, du, a, b, da, db, y, dy, ws, n, None)

    def jac64(B=2, H=9, W=12, nt=3, u=p, du=p1, a=p, b=p, da=p, db=p, y=p2, dy=p3):
        return lib.pde_jacobi_f64_tangent(B, H, W, nt, u, du, a, b, da, db, y, dy, None)

    for k, f, el in (("ex", ex, 4), ("ex64", ex64, 8), ("jac", jac, 4), ("jac64", jac64, 8)):
        P1, P2 = ("a", "s") if k.startswith("ex") else ("a", "b")
        D1, D2 = "d" + P1, "d" + P2
        # calls that get past validation: with no device the first launch fails
        put(f"{k} well-formed", f(), LAUNCH)
        put(f"{k} no du", f(du=None), LAUNCH)
        put(f"{k} du alone", f(**{D1: None, D2: None}), LAUNCH)
        put(f"{k} one parameter tangent alone", f(du=None, **{D1: None}), LAUNCH)
        put(f"{k} the other parameter tangent alone", f(du=None, **{D2: None}), LAUNCH)
        put(f"{k} no y", f(y=None), LAUNCH)
        # the tangents, the outputs, the required inputs
        put(f"{k} all three tangents NULL", f(du=None, **{D1: None, D2: None}), BADARG)
        put(f"{k} no dy", f(dy=None), BADARG)
        put(f"{k} no u", f(u=None), BADARG)
        put(f"{k} no {P1}", f(**{P1: None}), BADARG)
        put(f"{k} no {P2}", f(**{P2: None}), BADARG)
        # sizes
        put(f"{k} B = 0", f(B=0), BADARG)
        put(f"{k} B < 0", f(B=-3), BADARG)
        put(f"{k} H = 0", f(H=0), BADARG)
        put(f"{k} W = 0", f(W=0), BADARG)
        put(f"{k} W < 0", f(W=-4), BADARG)
        if k.startswith("ex"):
            put(f"{k} C = 0", f(Cc=0), BADARG)
            put(f"{k} num_steps = 0", f(nt=0), BADARG)
            put(f"{k} 1 x 1", f(H=1, W=1), LAUNCH)
            put(f"{k} one step takes no workspace", f(nt=1, ws=None, n=0), LAUNCH)
        else:
            put(f"{k} nt < 0", f(nt=-1), BADARG)
            put(f"{k} nt = 0", f(nt=0), LAUNCH)
            put(f"{k} 64 x 64", f(H=64, W=64), LAUNCH)
        if k == "jac":
            put("jac H = 3", f(H=3), BADARG)
            put("jac W = 3", f(W=3), BADARG)
            put("jac 4 x 4", f(H=4, W=4), LAUNCH)
            put("jac 65 x 4 (tiled)", f(H=65, W=4), LAUNCH)
            put("jac 1024 x 1024", f(B=1, H=L.PDE_JACOBI_MAX_HW, W=L.PDE_JACOBI_MAX_HW), LAUNCH)
            put("jac H = 1025", f(H=L.PDE_JACOBI_MAX_HW + 1), BADARG)
            put("jac W = 1025", f(W=L.PDE_JACOBI_MAX_HW + 1), BADARG)
            put("jac sizes come before the pointers", f(H=3, dy=None), BADARG)
        if k == "jac64":
            put("jac64 H = 65", f(H=65), BADARG)
            put("jac64 W = 65", f(W=65), BADARG)
            put("jac64 H = 1", f(H=1), BADARG)
            put("jac64 2 x 2 (the float64 forward's lower end)", f(H=2, W=2), LAUNCH)
        if k == "ex64":
            put("ex64 B = 65536", f(B=65536), BADARG)
            put("ex64 C = 65536", f(Cc=65536), BADARG)
        # the tensor type
        if k in ("ex", "jac"):
            put(f"{k} unknown tensor type", f(io=7), BADARG)
            put(f"{k} float64 tensors belong to the f64 call", f(io=L.PDE_IO_F64), BADARG)
            put(f"{k} negative tensor type", f(io=-1), BADARG)
            put(f"{k} bf16", f(io=L.PDE_IO_BF16), LAUNCH)
            put(f"{k} fp16", f(io=L.PDE_IO_F16), LAUNCH)
        # alignment.  ex at W = 8: tensors on four elements; everything else on the element
        four = k == "ex"
        for name, q in (("u", p), ("du", p1), ("y", p2), ("dy", p3)):
            put(f"{k} {name} off by half an element", f(**{name: off(q, el // 2)}), BADARG)
            put(f"{k} {name} off by one element", f(**{name: off(q, el)}), BADARG if four else LAUNCH)
            put(f"{k} {name} off by three elements", f(**{name: off(q, 3 * el)}), BADARG if four else LAUNCH)
            put(f"{k} {name} off by four elements is in order", f(**{name: off(q, 4 * el)}), LAUNCH)
        for name in (P1, P2, D1, D2):
            put(f"{k} {name} off by half an element", f(**{name: off(p, el // 2)}), BADARG)
            put(f"{k} {name} off by one element is in order", f(**{name: off(p, el)}), LAUNCH)
        if four:
            for name, q in (("u", p), ("du", p1), ("y", p2), ("dy", p3)):
                put(f"ex W = 7: {name} off by one element is in order", f(W=7, **{name: off(q, 4)}), LAUNCH)
                put(f"ex W = 7: {name} off by half an element", f(W=7, **{name: off(q, 2)}), BADARG)
                put(f"ex 16x16: {name} off by one element", f(H=16, W=16, **{name: off(q, 4)}), BADARG)
                put(f"ex bf16: {name} off by 8 bytes is in order", f(io=L.PDE_IO_BF16, **{name: off(q, 8)}), LAUNCH)
                put(f"ex fp16: {name} off by 2 bytes", f(io=L.PDE_IO_F16, **{name: off(q, 2)}), BADARG)
                put(f"ex fp16 W = 7: {name} off by 2 bytes is in order", f(io=L.PDE_IO_F16, W=7, **{name: off(q, 2)}), LAUNCH)
                put(f"ex fp16 W = 7: {name} off by 1 byte", f(io=L.PDE_IO_F16, W=7, **{name: off(q, 1)}), BADARG)
        if k == "jac":
            put("jac fp16 u off by 2 is in order", f(io=L.PDE_IO_F16, u=off(p, 2)), LAUNCH)
            put("jac fp16 dy off by 1", f(io=L.PDE_IO_F16, dy=off(p3, 1)), BADARG)
            put("jac bf16 du off by 1", f(io=L.PDE_IO_BF16, du=off(p1, 1)), BADARG)
        # the workspace
        if k == "jac64":
            continue
        if k == "ex":
            need = lib.pde_explicit5_tangent_workspace_bytes(2, 3, 5, 8, L.PDE_IO_F32, 3)
            tight = {}
        elif k == "ex64":
            need = lib.pde_explicit5_f64_tangent_workspace_bytes(2, 3, 5, 8, 3)
            tight = {}
        else:
            tight = dict(H=65, W=12, nt=L.PDE_JACOBI_TANGENT_TILED_K + 1)
            need = lib.pde_jacobi_io_tangent_workspace_bytes(2, 65, 12, tight["nt"], L.PDE_IO_F32)
        assert need > 0
        put(f"{k} exact workspace", f(n=need, **tight), LAUNCH)
        put(f"{k} workspace short by one byte", f(n=need - 1, **tight), WORKSPACE)
        put(f"{k} no workspace where one is needed", f(ws=None, n=0, **tight), WORKSPACE)
        put(f"{k} workspace off by 4", f(ws=off(w, 4), **tight), WORKSPACE)
        put(f"{k} workspace off by 8", f(ws=off(w, 8), **tight), WORKSPACE)
        put(f"{k} BADARG comes before WORKSPACE", f(dy=None, n=0, **tight), BADARG)
        put(f"{k} alignment comes before WORKSPACE", f(u=off(p, 1), n=0, **tight), BADARG)
        put(f"{k} the tangents come before WORKSPACE", f(du=None, n=0, **{D1: None, D2: None}, **tight), BADARG)
        if k == "jac":
            put("jac one launch takes no workspace", f(H=65, W=12, nt=L.PDE_JACOBI_TANGENT_TILED_K, ws=None, n=0), LAUNCH)
            put("jac small planes take no workspace", f(ws=None, n=0), LAUNCH)
            put("jac a misaligned workspace is refused even where none is needed", f(ws=off(w, 4)), WORKSPACE)
        if k == "ex":
            put("ex register planes take no workspace", f(H=32, W=32, ws=None, n=0), LAUNCH)
    return out


def test_refusal_codes_without_gpu(tmp_path):
    report = str(tmp_path / "report.json")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": os.path.dirname(here), "here": here}, report], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rep = json.load(open(report))
    assert len(rep) > 200
    wrong = {k: v for k, v in rep.items() if v[0] != v[1]}
    assert not wrong, f"(answer, expected): {wrong}"
    assert sum(1 for v in rep.values() if v[1] == LAUNCH) >= 60      # calls that got past validation
