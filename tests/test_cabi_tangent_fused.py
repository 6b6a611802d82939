"""The tangent-linear pass on the fused two-sided solver (include/pdecnn_tangent_fused.h) on a machine without a GPU: the
header is included by pdecnn.h and declares exactly the two calls, header, ctypes table and exports agree, the workspace
query is the header's formula, and every refusal the header names is answered on the host with the code it states, in the
order it states.  Addresses are made up; the refusal codes are checked in a child interpreter that sees no device, so that a
refusal that is missing ends in PDE_E_LAUNCH instead of a kernel on made-up addresses."""
import ctypes as C
import json
import os
import subprocess
import sys

from test_cabi import declared_functions
from test_cabi_tangent import _descs

NEW = ["pde_adi_tangent_fused_workspace_bytes", "pde_adi_tangent_fused"]
BADARG, UNSUPPORTED_N, SWEEPS, LAUNCH, WORKSPACE = -1, -2, -3, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = (8, 12, 16, 20, 24, 28, 32)
DCO_BYTES = 32 * 36 * 4                     # one line image of floats per (sweep, channel)


def declared_in_the_new_header():
    import re
    src = open(os.path.join(ROOT, "include", "pdecnn_tangent_fused.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): len([q for q in m.group(2).split(",") if q.strip() not in ("", "void")])
            for m in re.finditer(r"\b(pde_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}


def test_the_symbols_exist_and_are_bound():
    from cnn_with_pde_amd import _lib
    assert '#include "pdecnn_tangent_fused.h"' in open(os.path.join(ROOT, "include", "pdecnn.h")).read()
    hdr = declared_in_the_new_header()
    assert sorted(hdr) == sorted(NEW) == sorted(_lib.SIGNATURES_TANGENT_FUSED)
    assert sorted(_lib.SIGNATURES) == declared_functions()          # pdecnn.h itself declares what it declared
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SMALL_INPUT) | set(_lib.SIGNATURES_MIXED_INPUT) |
              set(_lib.SIGNATURES_EXPLICIT_INPUT) | set(_lib.SIGNATURES_TANGENT) | set(_lib.SIGNATURES_EXPLICIT_TANGENT))
    assert not set(NEW) & others
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n), f"{n} not exported"
    bound = _lib.load()
    for n in NEW:
        res, args = _lib.SIGNATURES_TANGENT_FUSED[n]
        assert getattr(bound, n).argtypes == args and getattr(bound, n).restype == res
        assert len(args) == hdr[n], n
    # the arguments of pde_adi_tangent
    assert _lib.SIGNATURES_TANGENT_FUSED["pde_adi_tangent_fused"] == _lib.SIGNATURES_TANGENT["pde_adi_tangent"]
    assert _lib.SIGNATURES_TANGENT_FUSED["pde_adi_tangent_fused_workspace_bytes"] == \
        _lib.SIGNATURES_TANGENT["pde_adi_tangent_workspace_bytes"]


def test_the_switch_is_read_from_the_environment():
    code = ("import sys; sys.path.insert(0, %r); from cnn_with_pde_amd import _lib; "
            "print(int(_lib.tangent_fused_enabled()))" % ROOT)
    for val, want in ((None, "1"), ("1", "1"), ("0", "0")):
        env = {k: v for k, v in os.environ.items() if k != "PDE_TANGENT_FUSED"}
        if val is not None:
            env["PDE_TANGENT_FUSED"] = val
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip() == want, (val, r.stdout, r.stderr[-2000:])


def test_workspace_query():
    from cnn_with_pde_amd import _lib as L, functional as F_
    lib = L.load()
    up = lambda n: -(-n // 256) * 256                                                                     # noqa: E731
    for N in (8, 12, 28, 32):
        for B, Cc, S in ((1, 1, 1), (3, 2, 6), (700, 3, 3)):
            for io in (L.PDE_IO_F32, L.PDE_IO_BF16, L.PDE_IO_F16):
                d = _descs(L, F_, B, Cc, N, N, S, io=io)
                fwd = lib.pde_adi_forward_workspace_bytes(C.byref(d))
                assert fwd > 0
                got = lib.pde_adi_tangent_fused_workspace_bytes(C.byref(d))
                assert got == fwd + up(S * Cc * DCO_BYTES), (N, B, Cc, S, got, fwd)
    for kw in (dict(H=10, W=10), dict(H=33, W=33), dict(H=36, W=36), dict(H=128, W=128), dict(H=16, W=16, S=0),
               dict(H=16, W=16, B=0), dict(H=16, W=16, Cc=0), dict(H=16, W=16, io=7), dict(H=16, W=16, io=L.PDE_IO_F64)):
        assert lib.pde_adi_tangent_fused_workspace_bytes(C.byref(_descs(L, F_, **kw))) == 0, kw
    d = _descs(L, F_, H=16, W=16, S=3)
    d.num_sweeps = L.PDE_MAX_SWEEPS + 1
    assert lib.pde_adi_tangent_fused_workspace_bytes(C.byref(d)) == 0
    assert lib.pde_adi_tangent_fused_workspace_bytes(None) == 0


CHILD = r"""
import ctypes as C, json, sys
sys.path[:0] = [%(root)r, %(here)r]
import torch
assert not torch.cuda.is_available(), "the refusals must be answered without a device"
from cnn_with_pde_amd import _lib, functional
import test_cabi_tangent_fused as T
json.dump(T.refusals(_lib.load(), _lib, functional), open(sys.argv[1], "w"))
"""


def refusals(lib, L, F_):
    """{what: (answer, expected)} — run in the child."""
    BIG = 1 << 40
    p = C.c_void_p(1 << 41)
    p2 = C.c_void_p((1 << 41) + (1 << 32))
    p3 = C.c_void_p((1 << 41) + (1 << 33))
    w = C.c_void_p((1 << 41) + (1 << 34))
    out = {}

    def put(what, got, want):
        assert what not in out
        out[what] = (got, want)

    def off(q, n):
        return C.c_void_p(q.value + n)

    def f(u=p, du=p, ab=p, bb=p, asl=p, bsl=p, dab=p, dbb=p, das=p, dbs=p, y=p2, dy=p3, ws=w, n=BIG, d=None, **kw):
        if d is None:
            kw.setdefault("H", 16)
            kw["W"] = kw["H"]
            d = _descs(L, F_, **kw)
        return lib.pde_adi_tangent_fused(C.byref(d), u, du, ab, bb, asl, bsl, dab, dbb, das, dbs, y, dy, ws, n, None)

    # calls that get past validation: with no device the first launch fails
    put("well-formed", f(), LAUNCH)
    put("no du", f(du=None), LAUNCH)
    put("du alone", f(dab=None, dbb=None, das=None, dbs=None), LAUNCH)
    put("one parameter tangent alone", f(du=None, dab=None, dbb=None, dbs=None), LAUNCH)
    put("no y", f(y=None), LAUNCH)
    put("96 sweeps", f(S=L.PDE_MAX_SWEEPS), LAUNCH)
    for N in FUSED:
        put(f"N = {N}", f(H=N), LAUNCH)
    for io in (L.PDE_IO_BF16, L.PDE_IO_F16):
        put(f"io {io}", f(io=io), LAUNCH)
    # the five tangents, the outputs, the required inputs
    put("all five tangents NULL", f(du=None, dab=None, dbb=None, das=None, dbs=None), BADARG)
    put("no dy", f(dy=None), BADARG)
    put("no u", f(u=None), BADARG)
    for name in ("ab", "bb", "asl", "bsl"):
        put(f"no {name}", f(**{name: None}), BADARG)
    put("no descriptor", lib.pde_adi_tangent_fused(None, p, p, p, p, p, p, p, p, p, p, p2, p3, w, BIG, None), BADARG)
    # the descriptor
    put("B = 0", f(B=0), BADARG)
    put("C = 0", f(Cc=0), BADARG)
    put("S = 0", f(S=0), BADARG)
    d = _descs(L, F_, H=16, W=16)
    d.num_sweeps = L.PDE_MAX_SWEEPS + 1
    put("S = 97", f(d=d), SWEEPS)
    d = _descs(L, F_, H=16, W=16)
    d.sweep[1].axis = 2
    put("bad axis", f(d=d), BADARG)
    put("unknown tensor type", f(io=7), BADARG)
    put("float64 tensors", f(io=L.PDE_IO_F64), BADARG)
    for N in (2, 5, 10, 33, 36, 128, 129):
        put(f"N = {N} is off the fused list", f(H=N), UNSUPPORTED_N)
    put("the descriptor comes before the pointers", f(S=0, dy=None), BADARG)
    d = _descs(L, F_, H=10, W=10)
    d.num_sweeps = L.PDE_MAX_SWEEPS + 1
    put("N comes before the sweeps", f(d=d), UNSUPPORTED_N)
    put("N comes before the pointers", f(H=10, u=None), UNSUPPORTED_N)
    # alignment: 16 bytes for every tensor, parameter and tangent
    for name, q in (("u", p), ("du", p), ("y", p2), ("dy", p3), ("ab", p), ("bb", p), ("asl", p), ("bsl", p), ("dab", p),
                    ("dbb", p), ("das", p), ("dbs", p)):
        for n in (4, 8):
            put(f"{name} off by {n}", f(**{name: off(q, n)}), BADARG)
        put(f"{name} off by 16 is in order", f(**{name: off(q, 16)}), LAUNCH)
    put("bf16 u off by one element", f(io=L.PDE_IO_BF16, u=off(p, 2)), BADARG)
    put("fp16 dy off by one element", f(io=L.PDE_IO_F16, dy=off(p3, 2)), BADARG)
    put("the pointers come before alignment", f(u=off(p, 4), dy=None), BADARG)
    # the workspace
    d = _descs(L, F_, H=16, W=16)
    need = lib.pde_adi_tangent_fused_workspace_bytes(C.byref(d))
    assert need > 0
    put("exact workspace", f(n=need), LAUNCH)
    put("short workspace", f(n=need - 1), WORKSPACE)
    put("the forward's workspace is short", f(n=lib.pde_adi_forward_workspace_bytes(C.byref(d))), WORKSPACE)
    put("no workspace", f(ws=None, n=0), BADARG)                 # a required pointer, as in the forward
    put("workspace off by 4", f(ws=off(w, 4)), WORKSPACE)
    put("workspace off by 8", f(ws=off(w, 8)), WORKSPACE)
    put("BADARG comes before WORKSPACE", f(dy=None, n=0), BADARG)
    put("alignment comes before WORKSPACE", f(u=off(p, 4), n=0), BADARG)
    put("all five NULL comes before WORKSPACE", f(du=None, dab=None, dbb=None, das=None, dbs=None, n=0), BADARG)
    return out


def test_refusal_codes_without_gpu(tmp_path):
    report = str(tmp_path / "report.json")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": os.path.dirname(here), "here": here}, report], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rep = json.load(open(report))
    assert len(rep) > 80
    wrong = {k: v for k, v in rep.items() if v[0] != v[1]}
    assert not wrong, f"(answer, expected): {wrong}"
    assert sum(1 for v in rep.values() if v[1] == LAUNCH) >= 25      # calls that got past validation
