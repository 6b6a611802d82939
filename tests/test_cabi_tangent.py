"""The tangent-linear pass of the four ADI families (include/pdecnn_tangent.h) on a machine without a GPU: the header is
included by pdecnn.h, header, ctypes table and exports agree, the workspace query holds what the header lists, and every
refusal the header names is answered on the host with the code it states.  Addresses are made up; the refusal codes are
checked in a child interpreter that sees no device, so that a refusal that is missing ends in PDE_E_LAUNCH instead of a
kernel on made-up addresses."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

from test_cabi import declared_functions

FAMILIES = ("pde_adi_", "pde_adi_f64_", "pde_adi_rect_", "pde_adi_rect_f64_")
NEW = [f + n for f in FAMILIES for n in ("tangent_workspace_bytes", "tangent")]
BADARG, UNSUPPORTED_N, SWEEPS, LAUNCH, WORKSPACE = -1, -2, -3, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_in_the_new_header():
    src = open(os.path.join(ROOT, "include", "pdecnn_tangent.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): len([q for q in m.group(2).split(",") if q.strip() not in ("", "void")])
            for m in re.finditer(r"\b(pde_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}


def test_the_symbols_exist_and_are_bound():
    """Declared in include/pdecnn_tangent.h, which pdecnn.h includes; bound in ``_lib.SIGNATURES_TANGENT`` by ``load()``."""
    from cnn_with_pde_amd import _lib
    assert '#include "pdecnn_tangent.h"' in open(os.path.join(ROOT, "include", "pdecnn.h")).read()
    hdr = declared_in_the_new_header()
    assert len(NEW) == 8 and sorted(hdr) == sorted(NEW) == sorted(_lib.SIGNATURES_TANGENT)
    assert sorted(_lib.SIGNATURES) == declared_functions()          # pdecnn.h itself declares what it declared
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SMALL_INPUT) | set(_lib.SIGNATURES_MIXED_INPUT) |
              set(_lib.SIGNATURES_EXPLICIT_INPUT))
    assert not set(NEW) & others
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n), f"{n} not exported"
    bound = _lib.load()
    for n in NEW:
        res, args = _lib.SIGNATURES_TANGENT[n]
        assert getattr(bound, n).argtypes == args and getattr(bound, n).restype == res
        assert len(args) == hdr[n], n
    for f in FAMILIES:
        # descriptor, u, du, four parameters, four tangents, y, dy, workspace, its size, stream
        assert len(_lib.SIGNATURES_TANGENT[f + "tangent"][1]) == 16
        assert _lib.SIGNATURES_TANGENT[f + "tangent_workspace_bytes"] == (C.c_size_t, _lib.SIGNATURES[f + "forward_workspace_bytes"][1])
        assert _lib.SIGNATURES_TANGENT[f + "tangent"][1][0] == _lib.SIGNATURES[f + "forward"][1][0]


def _descs(L, F_, B=2, Cc=3, H=5, W=5, S=3, io=None, f64=False):
    sweeps = tuple(F_.Sweep(s % 2, 0.1, 1.0, 0.05 * s) for s in range(S))
    rect = H != W
    cls = {(False, False): L.PdeAdiDesc, (True, False): L.PdeAdiRectDesc, (False, True): L.PdeAdiDescF64,
           (True, True): L.PdeAdiRectDescF64}[rect, f64]
    d = cls()
    if rect:
        d.H, d.W = H, W
    else:
        d.N = H
    d.B, d.C, d.num_sweeps = B, Cc, S
    d.io_dtype = (L.PDE_IO_F64 if f64 else L.PDE_IO_F32) if io is None else io
    d.smooth3, d.has_clamp_max, d.clamp_max, d.eps = 1, 1, 2.0, 1e-6
    for i, s in enumerate(sweeps[:L.PDE_MAX_SWEEPS]):
        d.sweep[i].axis, d.sweep[i].delta, d.sweep[i].h2, d.sweep[i].t = s.axis, s.delta, s.h2, s.t
    return d


def test_workspace_queries():
    from cnn_with_pde_amd import _lib as L, functional as F_
    lib = L.load()
    up = lambda n: -(-n // 256) * 256                                                                     # noqa: E731
    for f64 in (False, True):
        size = 8 if f64 else 4
        for H, W in ((2, 2), (5, 5), (28, 28), (32, 32), (100, 100), (128, 128), (2, 128), (5, 12), (101, 100)):
            for B, Cc, S in ((1, 1, 1), (3, 2, 6), (700, 3, 3)):
                d = _descs(L, F_, B, Cc, H, W, S, f64=f64)
                fam = "pde_adi_" + ("rect_" if H != W else "") + ("f64_" if f64 else "")
                fwd = getattr(lib, fam + "forward_workspace_bytes")(C.byref(d))
                if not f64 and H == W and H in (28, 32):
                    # the fused sizes run on the any-size kernels here: their factorisation, not the fused records
                    fwd = up(S * Cc * 4 * H * W * size) + up(16 * L.PDE_MAX_SWEEPS)
                got = getattr(lib, fam + "tangent_workspace_bytes")(C.byref(d))
                need = fwd + up(S * Cc * H * W * size)                  # factorisation + schedule, then dco
                if 2 * H * (W + 1) * size > 160 * 1024:                # the primal planes in the workspace
                    G = min(B, max(1, -(-256 // Cc)))
                    need += up(G * Cc * H * (W + 1) * size)
                assert got == need, (fam, H, W, B, Cc, S, got, need)
    # what the calls refuse
    for kw in (dict(H=1, W=1), dict(H=129, W=129), dict(S=0), dict(B=0), dict(Cc=0), dict(io=7), dict(H=1, W=5), dict(H=5, W=129)):
        for f64 in (False, True):
            d = _descs(L, F_, f64=f64, **kw)
            fam = "pde_adi_" + ("rect_" if kw.get("H", 5) != kw.get("W", 5) else "") + ("f64_" if f64 else "")
            assert getattr(lib, fam + "tangent_workspace_bytes")(C.byref(d)) == 0, (fam, kw)
    d = _descs(L, F_, S=3)
    d.num_sweeps = L.PDE_MAX_SWEEPS + 1
    assert lib.pde_adi_tangent_workspace_bytes(C.byref(d)) == 0
    assert lib.pde_adi_tangent_workspace_bytes(None) == 0


CHILD = r"""
import ctypes as C, json, sys
sys.path[:0] = [%(root)r, %(here)r]
import torch
assert not torch.cuda.is_available(), "the refusals must be answered without a device"
from cnn_with_pde_amd import _lib, functional
import test_cabi_tangent as T
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

    def family(name, f64, rect):
        def call(u=p, du=p, ab=p, bb=p, asl=p, bsl=p, dab=p, dbb=p, das=p, dbs=p, y=p2, dy=p3, ws=w, n=BIG, d=None, **kw):
            if d is None:
                if rect:
                    kw.setdefault("H", 5)
                    kw.setdefault("W", 9)
                d = _descs(L, F_, f64=f64, **kw)
            return getattr(lib, name + "tangent")(C.byref(d), u, du, ab, bb, asl, bsl, dab, dbb, das, dbs, y, dy, ws, n, None)
        return call

    calls = {"sq": family("pde_adi_", False, False), "sq64": family("pde_adi_f64_", True, False),
             "rect": family("pde_adi_rect_", False, True), "rect64": family("pde_adi_rect_f64_", True, True)}
    for k, f in calls.items():
        f64 = k.endswith("64")
        el = 8 if f64 else 4
        # calls that get past validation: with no device the first launch fails
        put(f"{k} well-formed", f(), LAUNCH)
        put(f"{k} no du", f(du=None), LAUNCH)
        put(f"{k} du alone", f(dab=None, dbb=None, das=None, dbs=None), LAUNCH)
        put(f"{k} one parameter tangent alone", f(du=None, dab=None, dbb=None, dbs=None), LAUNCH)
        put(f"{k} no y", f(y=None), LAUNCH)
        put(f"{k} 96 sweeps", f(S=L.PDE_MAX_SWEEPS), LAUNCH)
        # the five tangents, the outputs, the required inputs
        put(f"{k} all five tangents NULL", f(du=None, dab=None, dbb=None, das=None, dbs=None), BADARG)
        put(f"{k} no dy", f(dy=None), BADARG)
        put(f"{k} no u", f(u=None), BADARG)
        for name in ("ab", "bb", "asl", "bsl"):
            put(f"{k} no {name}", f(**{name: None}), BADARG)
        put(f"{k} no descriptor", getattr(lib, {"sq": "pde_adi_", "sq64": "pde_adi_f64_", "rect": "pde_adi_rect_",
                                              "rect64": "pde_adi_rect_f64_"}[k] + "tangent")(
            None, p, p, p, p, p, p, p, p, p, p, p2, p3, w, BIG, None), BADARG)
        # the descriptor
        put(f"{k} B = 0", f(B=0), BADARG)
        put(f"{k} C = 0", f(Cc=0), BADARG)
        put(f"{k} S = 0", f(S=0), BADARG)
        d = _descs(L, F_, f64=f64, **(dict(H=5, W=9) if "rect" in k else {}))
        d.num_sweeps = L.PDE_MAX_SWEEPS + 1
        put(f"{k} S = 97", f(d=d), SWEEPS)
        d = _descs(L, F_, f64=f64, **(dict(H=5, W=9) if "rect" in k else {}))
        d.sweep[1].axis = 2
        put(f"{k} bad axis", f(d=d), BADARG)
        put(f"{k} unknown tensor type", f(io=7), BADARG)
        put(f"{k} tensors of the other family", f(io=L.PDE_IO_F32 if f64 else L.PDE_IO_F64), BADARG)
        if "rect" in k:
            put(f"{k} H = 1", f(H=1, W=9), UNSUPPORTED_N)
            put(f"{k} W = 129", f(H=5, W=129), UNSUPPORTED_N)
            put(f"{k} 2 x 128", f(H=2, W=128), LAUNCH)
        else:
            put(f"{k} N = 1", f(H=1, W=1), UNSUPPORTED_N)
            put(f"{k} N = 129", f(H=129, W=129), UNSUPPORTED_N)
            put(f"{k} N = 2", f(H=2, W=2), LAUNCH)
            put(f"{k} N = 128", f(H=128, W=128), LAUNCH)
            put(f"{k} N = 28 (a fused size)", f(H=28, W=28), LAUNCH)
        put(f"{k} the descriptor comes before the pointers", f(S=0, dy=None), BADARG)
        put(f"{k} N comes before the sweeps", f(d=(lambda q: (setattr(q, "num_sweeps", 97), q)[1])(
            _descs(L, F_, f64=f64, **(dict(H=1, W=9) if "rect" in k else dict(H=1, W=1))))), UNSUPPORTED_N)
        # alignment: the element, tensors and parameters alike
        for name, q in (("u", p), ("du", p), ("y", p2), ("dy", p3)):
            put(f"{k} {name} off by half an element", f(**{name: off(q, el // 2)}), BADARG)
            put(f"{k} {name} off by one element is in order", f(**{name: off(q, el)}), LAUNCH)
        for name in ("ab", "bsl", "dab", "dbs"):
            put(f"{k} {name} off by half an element", f(**{name: off(p, el // 2)}), BADARG)
            put(f"{k} {name} off by one element is in order", f(**{name: off(p, el)}), LAUNCH)
        if not f64:
            put(f"{k} bf16 u off by 2 is in order", f(io=L.PDE_IO_BF16, u=off(p, 2)), LAUNCH)
            put(f"{k} fp16 dy off by 1", f(io=L.PDE_IO_F16, dy=off(p3, 1)), BADARG)
        # the workspace
        d = _descs(L, F_, f64=f64, **(dict(H=5, W=9) if "rect" in k else {}))
        need = getattr(lib, {"sq": "pde_adi_", "sq64": "pde_adi_f64_", "rect": "pde_adi_rect_",
                             "rect64": "pde_adi_rect_f64_"}[k] + "tangent_workspace_bytes")(C.byref(d))
        assert need > 0
        put(f"{k} exact workspace", f(n=need), LAUNCH)
        put(f"{k} short workspace", f(n=need - 1), WORKSPACE)
        put(f"{k} no workspace", f(ws=None, n=0), BADARG)             # a required pointer, as in the family's forward
        put(f"{k} workspace off by 4", f(ws=off(w, 4)), WORKSPACE)
        put(f"{k} workspace off by 8", f(ws=off(w, 8)), WORKSPACE)
        put(f"{k} BADARG comes before WORKSPACE", f(dy=None, n=0), BADARG)
        put(f"{k} alignment comes before WORKSPACE", f(u=off(p, 1), n=0), BADARG)
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
