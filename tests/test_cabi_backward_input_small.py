"""The input-only backward of the one-launch C <= 4 layers (pde_adi_small_forward_input, pde_adi_small_backward_input[_states],
pde_adi_multi_backward_input and their workspace query) on a machine without a GPU: header, ctypes table and exports
agree, the query is 0 exactly where the path is refused, and every refusal the header names is answered on the host with
the code it states.  Addresses are made up; the refusal codes are checked in a child interpreter that sees no device, so
that a refusal that is missing ends in PDE_E_LAUNCH instead of a kernel on made-up addresses."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from test_cabi import declared_functions

NEW = ["pde_adi_small_backward_input_workspace_bytes", "pde_adi_small_forward_input", "pde_adi_small_backward_input",
       "pde_adi_small_backward_input_states", "pde_adi_multi_backward_input"]
BADARG, LAUNCH, WORKSPACE = -1, -4, -5


def declared_in_the_new_header():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pdecnn_small_input.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pde_[a-z0-9_]+)\s*\(", src)))


def test_the_five_symbols_exist_and_are_bound():
    """Declared in include/pdecnn_small_input.h, which pdecnn.h includes; bound in ``_lib.SIGNATURES_SMALL_INPUT`` by ``load()``."""
    from cnn_with_pde_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert '#include "pdecnn_small_input.h"' in open(os.path.join(root, "include", "pdecnn.h")).read()
    assert declared_in_the_new_header() == sorted(NEW) == sorted(_lib.SIGNATURES_SMALL_INPUT)
    assert sorted(_lib.SIGNATURES) == declared_functions()          # pdecnn.h itself declares what it declared
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n), f"{n} not exported"
    bound = _lib.load()
    sig = dict(_lib.SIGNATURES, **_lib.SIGNATURES_SMALL_INPUT)
    for n in NEW:
        assert getattr(bound, n).argtypes == sig[n][1]
    # forward_input is the forward without `states`; the plain input backward is the _states call without (gtraj, emit_mask)
    # and with the skip weight
    fwd, fin = sig["pde_adi_small_forward"][1], sig["pde_adi_small_forward_input"][1]
    assert len(fin) == len(fwd) - 1 and fin[:5] == fwd[:5] and fin[5:] == fwd[6:]
    assert len(sig["pde_adi_small_backward_input_states"][1]) == len(sig["pde_adi_small_backward_input"][1]) + 1
    assert len(sig["pde_adi_multi_backward_input"][1]) == len(sig["pde_adi_multi_backward"][1]) - 1      # no u


def _desc(N=16, B=3, Cc=3, K=2, sps=3, io=None):
    from cnn_with_pde_amd import _lib
    d = _lib.PdeAdiDesc()
    d.N, d.B, d.C, d.num_sweeps = N, B, Cc, K * sps
    d.io_dtype = _lib.PDE_IO_F32 if io is None else io
    d.eps = 1e-6
    for s in range(K * sps):
        d.sweep[s].axis = 1 if s % sps == 1 else 0
        d.sweep[s].delta, d.sweep[s].h2, d.sweep[s].t = (0.01 if sps == 3 and s % 3 != 1 else 0.02), 1.0, 0.02 * (s // sps)
    return d


def test_workspace_query():
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    q = lib.pde_adi_small_backward_input_workspace_bytes
    assert q(None, 3) == 0
    assert q(C.byref(_desc(Cc=5)), 3) == 0                      # C = 5
    assert q(C.byref(_desc(N=20)), 3) == 0                      # N = 20: no one-launch kernels
    assert q(C.byref(_desc()), 1) == 0                          # sweeps_per_step = 1
    assert q(C.byref(_desc()), 2) == 0                          # x,y,x steps asked for as x,y
    for d, sps in ((_desc(Cc=5), 3), (_desc(N=20), 3), (_desc(), 1), (_desc(), 2)):
        assert lib.pde_adi_small_supported(C.byref(d), sps) == 0
    for N in (16, 28, 32):
        for Cc in (1, 3, 4):
            for io, item in ((_lib.PDE_IO_F32, 4), (_lib.PDE_IO_BF16, 2), (_lib.PDE_IO_F16, 2)):
                d = _desc(N=N, Cc=Cc, B=5, io=io)
                assert lib.pde_adi_small_supported(C.byref(d), 3) == 1
                want = -(-(5 * Cc * N * N * item) // 256) * 256          # one tensor: the slab of a side-by-side group
                assert q(C.byref(d), 3) == want
                assert want < lib.pde_adi_small_backward_workspace_bytes(C.byref(d), 3, 0)
    assert q(C.byref(_desc(sps=2)), 2) > 0                      # Lie steps


CHILD = r"""
import ctypes as C, json, sys
sys.path[:0] = [%(root)r, %(here)r]
import torch
assert not torch.cuda.is_available(), "the refusals must be answered without a device"
from cnn_with_pde_amd import _lib
import test_cabi_backward_input_small as T
json.dump(T.refusals(_lib.load(), _lib), open(sys.argv[1], "w"))
"""


def refusals(lib, L):
    """{what: (answer, expected)} — run in the child."""
    BIG = 1 << 40
    p = C.c_void_p(1 << 41)
    p2 = C.c_void_p((1 << 41) + (1 << 32))
    odd = C.c_void_p((1 << 41) + 4)
    out = {}

    def put(what, got, want):
        assert what not in out
        out[what] = (got, want)

    plain, states, fin = lib.pde_adi_small_backward_input, lib.pde_adi_small_backward_input_states, lib.pde_adi_small_forward_input
    multi = lib.pde_adi_multi_backward_input
    d = _desc()
    em0, em1, em_hi = (C.c_uint64 * 2)(0, 0), (C.c_uint64 * 2)(1, 0), (C.c_uint64 * 2)(2, 0)

    def bwd(d=d, sps=3, mode=2, gy=p, M=p, sk=None, gu=p, sws=p, ws=None, n=0):
        return plain(None if d is None else C.byref(d), sps, mode, gy, M, sk, gu, sws, ws, n, None)

    def bwd_states(d=d, sps=3, mode=1, gy=p, gtraj=p, em=em1, M=p, gu=p, sws=p, ws=None, n=0):
        return states(None if d is None else C.byref(d), sps, mode, gy, gtraj, em, M, gu, sws, ws, n, None)

    def fwd(d=d, sps=3, mode=2, u=p, y=p2, M=p, sk=None, co=(p, p, p, p), sws=p, n=BIG):
        return fin(None if d is None else C.byref(d), sps, mode, u, y, M, sk, *co, None, None, None, sws, n, None)

    # a well-formed call gets past validation: with no device its launch fails
    put("bwd well-formed", bwd(), LAUNCH)
    put("bwd well-formed, skip blend", bwd(sk=p), LAUNCH)
    put("bwd well-formed, unused workspace given", bwd(ws=p, n=16), LAUNCH)
    put("states well-formed", bwd_states(), LAUNCH)
    put("states well-formed, empty mask and no gtraj", bwd_states(gtraj=None, em=em0), LAUNCH)
    put("states well-formed, NULL mask", bwd_states(gtraj=None, em=None), LAUNCH)
    put("fwd well-formed", fwd(), LAUNCH)
    # NULL required pointers
    put("bwd no descriptor", bwd(d=None), BADARG)
    put("bwd no gy", bwd(gy=None), BADARG)
    put("bwd no M", bwd(M=None), BADARG)
    put("bwd no gu", bwd(gu=None), BADARG)
    put("states no gy", bwd_states(gy=None), BADARG)
    put("states no M", bwd_states(M=None), BADARG)
    put("states no gu", bwd_states(gu=None), BADARG)
    put("fwd no descriptor", fwd(d=None), BADARG)
    put("fwd no u", fwd(u=None), BADARG)
    put("fwd no y", fwd(y=None), BADARG)
    put("fwd no M", fwd(M=None), BADARG)
    for i in range(4):
        co = [p] * 4
        co[i] = None
        put(f"fwd no coefficient {i}", fwd(co=co), BADARG)
    put("fwd no steps workspace", fwd(sws=None), BADARG)         # as pde_adi_small_forward answers it
    put("fwd short steps workspace", fwd(n=16), WORKSPACE)
    # descriptors the path refuses
    for what, dd, sps in (("C = 5", _desc(Cc=5), 3), ("N = 20", _desc(N=20), 3), ("sps = 1", _desc(), 1),
                          ("Strang as Lie", _desc(), 2), ("B = 0", _desc(B=0), 3)):
        put(f"bwd {what}", bwd(d=dd, sps=sps), BADARG)
        put(f"states {what}", bwd_states(d=dd, sps=sps), BADARG)
        put(f"fwd {what}", fwd(d=dd, sps=sps), BADARG)
    put("bwd mode 0", bwd(mode=0), BADARG)
    put("bwd mode 3", bwd(mode=3), BADARG)
    put("bwd skip_weight in mode 1", bwd(mode=1, sk=p), BADARG)
    put("fwd skip_weight in mode 1", fwd(mode=1, sk=p), BADARG)
    # the emission mask: K = 2, so only bit 0 may be set
    put("states mask without gtraj", bwd_states(gtraj=None), BADARG)
    put("states bit K-1", bwd_states(em=em_hi), BADARG)
    put("states bit 64", bwd_states(em=(C.c_uint64 * 2)(0, 1)), BADARG)
    # alignment of the tensors (16 bytes) and of the skip weight (an element)
    put("bwd gy off by 4", bwd(gy=odd), BADARG)
    put("bwd gu off by 4", bwd(gu=odd), BADARG)
    put("bwd M off by 4", bwd(M=odd), BADARG)
    put("bwd skip_weight off by 1", bwd(sk=C.c_void_p(p.value + 1)), BADARG)
    put("bwd skip_weight off by 4 is in order", bwd(sk=odd), LAUNCH)
    put("states gtraj off by 4", bwd_states(gtraj=odd), BADARG)
    put("fwd y off by 4", fwd(y=odd), BADARG)
    # workspaces
    put("bwd no steps workspace", bwd(sws=None), WORKSPACE)
    put("bwd steps workspace off by 4", bwd(sws=odd), WORKSPACE)
    put("bwd workspace off by 4", bwd(ws=odd, n=BIG), WORKSPACE)
    put("states no steps workspace", bwd_states(sws=None), WORKSPACE)
    put("states workspace off by 4", bwd_states(ws=odd, n=BIG), WORKSPACE)
    put("BADARG comes before WORKSPACE", bwd(M=None, sws=None), BADARG)

    # the shared-input call: an array of PdeSmallLayer
    def layers(n, B=3, **kw):
        arr = (L.PdeSmallLayer * n)()
        keep = []
        need = 0
        for i in range(n):
            dd = _desc(B=B, K=1 + i)
            keep.append(dd)
            a = arr[i]
            a.desc, a.sweeps_per_step, a.mode = C.pointer(dd), 3, 1
            a.M = p.value + (i << 20)
            a.steps_workspace = p2.value + (i << 24)
            need = lib.pde_adi_small_backward_input_workspace_bytes(C.byref(dd), 3)
            a.workspace, a.workspace_bytes = p2.value + (1 << 30) + (i << 24), need
            a.weight = 0.5
        for k, (i, v) in kw.items():
            setattr(arr[i], k, v)
        return arr, keep, need

    def mcall(n, arr, gy=p, gu=p):
        return multi(n, arr, gy, gu, None)

    arr, keep, need = layers(3)
    put("multi well-formed, side by side", mcall(3, arr), LAUNCH)
    put("multi well-formed, gys only", mcall(3, layers(3, gys=(1, p.value))[0], gy=None), LAUNCH)
    arr, keep, _ = layers(2, B=1025)
    for a in arr:
        a.workspace, a.workspace_bytes = None, 0
    put("multi well-formed, one after the other without slabs", mcall(2, arr), LAUNCH)
    arr, keep, _ = layers(1)
    arr[0].workspace, arr[0].workspace_bytes = None, 0
    put("multi well-formed, one layer without a slab", mcall(1, arr), LAUNCH)
    put("multi no layers", multi(3, None, p, p, None), BADARG)
    put("multi zero layers", mcall(0, layers(1)[0]), BADARG)
    put("multi five layers", mcall(5, layers(5)[0]), BADARG)
    put("multi no gu", mcall(3, layers(3)[0], gu=None), BADARG)
    put("multi gu off by 4", mcall(3, layers(3)[0], gu=odd), BADARG)
    put("multi no M", mcall(3, layers(3, M=(1, None))[0]), BADARG)
    put("multi no desc", mcall(3, layers(3, desc=(2, None))[0]), BADARG)
    put("multi mode 2 with several layers", mcall(3, layers(3, mode=(1, 2))[0]), BADARG)
    put("multi skip_weight in mode 1", mcall(3, layers(3, skip_weight=(0, p.value))[0]), BADARG)
    put("multi sweeps_per_step disagree", mcall(3, layers(3, sweeps_per_step=(2, 2))[0]), BADARG)
    for what, dd in (("B", _desc(B=4)), ("C", _desc(Cc=4)), ("N", _desc(N=28)), ("io", _desc(io=L.PDE_IO_BF16))):
        arr, keep, _ = layers(3)
        arr[1].desc = C.pointer(dd)
        put(f"multi layers disagree in {what}", mcall(3, arr), BADARG)
    arr, keep, _ = layers(3)
    arr[2].desc = C.pointer(_desc(Cc=5))
    put("multi unsupported descriptor", mcall(3, arr), BADARG)
    # every non-NULL device pointer of the struct at its alignment, the ones the call does not read too
    for f in ("M", "alpha_base", "beta_base", "alpha_slope", "beta_slope", "states", "gys", "g_plane_sums", "g_alpha_base",
              "g_beta_base", "g_alpha_slope", "g_beta_slope", "gM"):
        put(f"multi {f} off by 4", mcall(3, layers(3, **{f: (1, odd.value)})[0]), BADARG)
    for f in ("skip_weight", "weight_ptr", "plane_sums", "kappa_max", "kappa_max_host", "g_skip_weight", "g_weight"):
        arr, keep, _ = layers(1)
        arr[0].mode = 2
        setattr(arr[0], f, p.value + 2)
        put(f"multi {f} off by 2", mcall(1, arr), BADARG)
    put("multi no steps workspace", mcall(3, layers(3, steps_workspace=(1, None))[0]), WORKSPACE)
    put("multi steps workspace off by 4", mcall(3, layers(3, steps_workspace=(1, odd.value))[0]), WORKSPACE)
    put("multi no slab side by side", mcall(3, layers(3, workspace=(2, None))[0]), WORKSPACE)
    put("multi short slab", mcall(3, layers(3, workspace_bytes=(0, need - 1))[0]), WORKSPACE)
    put("multi slab off by 4", mcall(3, layers(3, workspace=(0, odd.value))[0]), WORKSPACE)
    arr, keep, _ = layers(2, B=1025)
    arr[1].workspace = odd.value
    put("multi unused slab off by 4", mcall(2, arr), WORKSPACE)
    return out


def test_refusal_codes_without_gpu(tmp_path):
    report = str(tmp_path / "report.json")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": os.path.dirname(here), "here": here}, report], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    import json
    rep = json.load(open(report))
    assert len(rep) > 100
    wrong = {k: v for k, v in rep.items() if v[0] != v[1]}
    assert not wrong, f"(answer, expected): {wrong}"
    assert sum(1 for v in rep.values() if v[1] == LAUNCH) >= 12      # calls that got past validation
