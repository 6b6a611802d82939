"""The tangent-linear pass on the fused two-sided solver: include/pdecnn_tangent_fused.h (adi_factor_tangent_kernel and
adi_tangent_kernel of csrc/pde_adi_tangent_dev.h), and the route functional._tangent_call gives it at N = 8 .. 32.

Reference for every value: ``torch.autograd.forward_ad`` through the float64 oracle, with the input generator, the oracle
JVP and the gate of tests/test_gpu_tangent.py: max|err| / max|ref| <= max(1e-5, 4 min(o32, 1e-4)) with o32 the error of the
oracle's own forward AD in fp32; 1e-5 of the scale for duality.  Inputs are built away from the clamp's kinks (no raw
coefficient within 1e-4 of a bound), with at least a fifth of the entries clamped in some sweep and a mask that moves between
sweeps; the generator asserts that.

Shapes are the smallest at which this kernel can go wrong: every fused N once (N = 8: 24 idle lines, N = 12: half rows that
are no multiple of four, N = 32: no idle line), one plane, a ragged second chunk (B = 17 at sixteen planes per workgroup
iteration), records resident (S = 2, 3) and through the ring (S = 30: it turns over ten times), a hand-made schedule whose
axes run y, x, x, y (the axis comes from the table)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.autograd.forward_ad as fwad

import test_gpu_tangent as T
from oracle import pde_oracle as O
from test_gpu_tangent import MODES, gate, make_inputs, oracle_jvp

pytestmark = pytest.mark.gpu

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
EPS = T.EPS
NAMES = T.NAMES
rel = T.rel

#: (N, B, C, split, steps, smooth3, clamp_max, mode); split "yxxy": sweeps 1 .. 4 of two Strang steps
CASES = [
    (8, 3, 3, "strang", 1, True, 1.5, "both"),
    (12, 1, 1, "lie", 1, False, None, "params"),
    (16, 17, 1, "strang", 1, True, None, "single"),
    (20, 3, 3, "lie", 2, False, 1.5, "single_a"),
    (24, 3, 1, "strang", 2, True, 1.5, "du"),
    (28, 3, 3, "strang", 1, False, None, "both"),
    (32, 1, 3, "lie", 1, True, 1.5, "params"),
    (32, 3, 1, "strang", 10, False, 1.5, "both"),
    (12, 17, 3, "strang", 10, True, None, "both"),
    (16, 3, 3, "yxxy", 2, True, 1.5, "both"),
    (28, 1, 1, "yxxy", 2, False, None, "params"),
]
IDS = ["n%d_b%dc%d_%s%d_%s%s%s" % (c[0], c[1], c[2], c[3], c[4], c[7], "_smooth" if c[5] else "", "_max" if c[6] else "")
       for c in CASES]
PARAM_CASES = [i for i, c in enumerate(CASES) if MODES[c[7]][1]]


def _spec(case):
    N, B, Cc, split, K, smooth3, cmax, mode = case
    return O.AdiSpec(N, Cc, 0.4, 1.0, 1.3, K, "strang" if split == "yxxy" else split, smooth3, cmax, "none", False, EPS)


def _schedules(case):
    """(the oracle's [(axis, delta, t)], the library's sweeps) of a case"""
    spec = _spec(case)
    osched, sweeps = O.sweep_schedule(spec), T._sweeps(spec)
    if case[3] == "yxxy":
        osched, sweeps = osched[1:5], sweeps[1:5]
        assert [s[0] for s in osched] == [1, 0, 0, 1] and [s.axis for s in sweeps] == [1, 0, 0, 1]
    return spec, osched, sweeps


def _oracle_fn(spec, osched):
    def fn(a, p):
        for axis, delta, t in osched:
            base, slope = (p["alpha_base"], p["alpha_time_coeff"]) if axis == 0 else (p["beta_base"], p["beta_time_coeff"])
            a = O._implicit_sweep(a, O.coefficient_at(base, slope, t, spec), axis, delta, spec.dx if axis == 0 else spec.dy, spec)
        return a
    return fn


def _condition(params, spec, osched):
    """tests/test_gpu_tangent.py's condition on the inputs, for the sweeps this case runs"""
    near, share, masks = float("inf"), 0.0, {0: [], 1: []}
    for ax, _, t in osched:
        raw = ((params["alpha_base"] + params["alpha_time_coeff"] * t) if ax == 0 else
               (params["beta_base"] + params["beta_time_coeff"] * t)).double()
        near = min(near, float((raw - spec.eps).abs().min()))
        clamped = raw < spec.eps
        if spec.clamp_max is not None:
            near = min(near, float((raw - spec.clamp_max).abs().min()))
            clamped = clamped | (raw > spec.clamp_max)
        share = max(share, float(clamped.double().mean()))
        masks[ax].append(clamped)
    moves = any(bool((m != ms[0]).any()) for ms in masks.values() for m in ms[1:]) or bool((masks[0][0] != masks[1][0]).any())
    return near, share, moves


def _desc(u, sweeps, smooth3, cmax):
    import cnn_with_pde_amd._lib as L
    import cnn_with_pde_amd.functional as F_
    B, Cc, H, W = u.shape
    return F_._desc(L.PdeAdiDesc, B, Cc, H, W, F_._io_dtype(u), sweeps, smooth3, cmax, EPS)


def c_call(name, u, du, p, dp, sweeps, smooth3, cmax, want_y=True):
    """``pde_adi_tangent_fused`` or ``pde_adi_tangent`` (the any-size kernels) straight through the C ABI"""
    import cnn_with_pde_amd._lib as L
    import cnn_with_pde_amd.functional as F_
    lib = L.load()
    d = _desc(u, sweeps, smooth3, cmax)
    n = getattr(lib, name + "_workspace_bytes")(C.byref(d))
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device=u.device)
    y = torch.empty_like(u) if want_y else None
    dy = torch.empty_like(u)
    ptr = F_._ptr
    L.check(getattr(lib, name)(C.byref(d), ptr(u), ptr(du), *[ptr(t) for t in p], *[ptr(t) for t in dp], ptr(y), ptr(dy),
                               ptr(ws), n, F_._stream()), name)
    return y, dy


def fused(u, du, p, dp, sweeps, smooth3, cmax, want_y=True):
    return c_call("pde_adi_tangent_fused", u, du, p, dp, sweeps, smooth3, cmax, want_y)


def _function(r, u=None, du=None, dp=None):
    import cnn_with_pde_amd.functional as F_
    N, B, Cc, split, K, smooth3, cmax, mode = r["case"]
    dp = r["dp"] if dp is None else dp
    return F_.adi_diffuse_tangent(r["u"] if u is None else u, *r["p"], r["sweeps"], du=r["du"] if du is None else du,
                                  d_alpha_base=dp[0], d_beta_base=dp[1], d_alpha_time_coeff=dp[2], d_beta_time_coeff=dp[3],
                                  smooth3=smooth3, clamp_max=cmax, eps=EPS)


@functools.lru_cache(maxsize=None)
def run(i):
    """Everything the tests of case ``i`` share: the reference (computed once, never changed) and the library's results."""
    case = CASES[i]
    N, B, Cc, split, K, smooth3, cmax, mode = case
    spec, osched, sweeps = _schedules(case)
    with_du, names = MODES[mode]
    u, du, params, dparams = make_inputs(B, Cc, N, N, spec, 2000 + 17 * i, F32)
    near, share, moves = _condition(params, spec, osched)
    assert near >= 1e-4 and share >= 0.2 and moves, (near, share, moves)
    du = du if with_du else None
    dparams = {n: (dparams[n] if n in names else None) for n in NAMES}
    fn = _oracle_fn(spec, osched)
    y_ref, yd_ref = oracle_jvp(fn, u, du, params, dparams)
    o32 = rel(oracle_jvp(fn, u, du, params, dparams, F32)[1], yd_ref)
    dev = lambda t: None if t is None else t.to(F32).cuda()                                               # noqa: E731
    r = dict(case=(N, N, B, Cc, F32), spec=spec, sweeps=sweeps, y_ref=y_ref, yd_ref=yd_ref, o32=o32, u=dev(u), du=dev(du),
             p=[dev(params[n]) for n in NAMES], dp=[dev(dparams[n]) for n in NAMES])
    r["y"], r["yd"] = fused(r["u"], r["du"], r["p"], r["dp"], sweeps, smooth3, cmax)
    torch.cuda.synchronize()
    r["gate"] = gate(r)
    r["case"] = case
    return r


# ---- value ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_value_against_the_float64_oracle(i):
    r = run(i)
    errs = {"y": rel(r["y"], r["y_ref"]), "ydot": rel(r["yd"], r["yd_ref"])}
    print(IDS[i], errs, "o32", r["o32"], "gate", r["gate"])
    assert torch.isfinite(r["yd"]).all()
    assert errs["ydot"] <= r["gate"] and errs["y"] <= r["gate"], (errs, "o32", r["o32"])


# ---- bitwise identities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_identities(i):
    import cnn_with_pde_amd.functional as F_
    r = run(i)
    N, B, Cc, split, K, smooth3, cmax, mode = r["case"]
    kw = dict(smooth3=smooth3, clamp_max=cmax, eps=EPS)
    args = (r["sweeps"], smooth3, cmax)
    with torch.no_grad():
        assert torch.equal(r["y"], F_.adi_diffuse(r["u"], *r["p"], r["sweeps"], **kw))          # the fused forward
        du = r["du"] if r["du"] is not None else torch.randn_like(r["u"])
        y0, yd0 = fused(r["u"], du, r["p"], [None] * 4, *args)
        assert torch.equal(yd0, F_.adi_diffuse(du, *r["p"], r["sweeps"], **kw)) and torch.equal(y0, r["y"])
    _, yd2 = fused(r["u"], None if r["du"] is None else 2 * r["du"], r["p"], [None if t is None else 2 * t for t in r["dp"]],
                   *args, want_y=False)
    assert torch.equal(yd2, 2 * r["yd"])                                                        # and dy without y stored
    _, yd1 = fused(r["u"], r["du"], r["p"], r["dp"], *args, want_y=False)
    assert torch.equal(yd1, r["yd"])


# ---- duality with the library's own (fused) backward ----------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_duality_with_the_backward(i):
    import cnn_with_pde_amd.functional as F_
    r = run(i)
    N, B, Cc, split, K, smooth3, cmax, mode = r["case"]
    g = torch.randn(r["u"].shape, generator=torch.Generator().manual_seed(5 + i), dtype=F64).float().cuda()
    u = r["u"].clone().requires_grad_(True)
    p = [t.clone().requires_grad_(True) for t in r["p"]]
    y = F_.adi_diffuse(u, *p, r["sweeps"], smooth3=smooth3, clamp_max=cmax, eps=EPS)
    y.backward(g)
    dot = lambda a, b: float((a.double() * b.double()).sum())                                             # noqa: E731
    lhs = dot(r["yd"], g)
    rhs = (0.0 if r["du"] is None else dot(r["du"], u.grad)) + sum(dot(t, q.grad) for t, q in zip(r["dp"], p) if t is not None)
    scale = float(r["yd"].double().norm() * g.double().norm())
    print(IDS[i], "duality", abs(lhs - rhs) / scale)
    assert abs(lhs - rhs) <= 1e-5 * scale, (lhs, rhs, scale)


# ---- the route ------------------------------------------------------------------------------------------------------------
def test_the_function_and_forward_ad_take_the_fused_call():
    """Fails on a build without the route: there both return pde_adi_tangent's bits."""
    import cnn_with_pde_amd.functional as F_
    differs = 0
    for i in range(len(CASES)):
        r = run(i)
        N, B, Cc, split, K, smooth3, cmax, mode = r["case"]
        fy, fyd = _function(r)
        assert torch.equal(fy, r["y"]) and torch.equal(fyd, r["yd"]), IDS[i]
        with fwad.dual_level():
            u = r["u"] if r["du"] is None else fwad.make_dual(r["u"], r["du"])
            p = [t if dt is None else fwad.make_dual(t, dt) for t, dt in zip(r["p"], r["dp"])]
            y, yd = fwad.unpack_dual(F_.adi_diffuse(u, *p, r["sweeps"], smooth3=smooth3, clamp_max=cmax, eps=EPS))
            assert yd is not None and torch.equal(y, r["y"]) and torch.equal(yd, r["yd"]), IDS[i]
        if i in PARAM_CASES:
            ay, ayd = c_call("pde_adi_tangent", r["u"], r["du"], r["p"], r["dp"], r["sweeps"], smooth3, cmax)
            assert rel(ayd, r["yd_ref"]) <= r["gate"]
            differs += int(not torch.equal(ayd, r["yd"]))
    assert differs >= 1                    # the any-size recurrences are another order of operations


# ---- 16-bit tensors: fp32 arithmetic, one rounding on the store ---------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("i", [1, 6], ids=[IDS[1], IDS[6]])
def test_16_bit_tensors_round_the_fp32_result_once(i, dtype):
    r = run(i)
    N, B, Cc, split, K, smooth3, cmax, mode = r["case"]
    u16, du16 = r["u"].to(dtype), torch.randn_like(r["u"]).to(dtype)
    y16, yd16 = fused(u16, du16, r["p"], r["dp"], r["sweeps"], smooth3, cmax)
    y32, yd32 = fused(u16.float(), du16.float(), r["p"], r["dp"], r["sweeps"], smooth3, cmax)
    assert y16.dtype == dtype and yd16.dtype == dtype
    assert torch.equal(yd16, yd32.to(dtype)) and torch.equal(y16, y32.to(dtype))
    if dtype == BF16:                                    # bf16 tensors with fp32 parameters are a route of the function's own
        fy, fyd = _function(r, u=u16, du=du16)
        assert torch.equal(fy, y16) and torch.equal(fyd, yd16)


# ---- several chunks per workgroup ---------------------------------------------------------------------------------------
def test_workgroups_that_walk_several_chunks():
    """C = 64 leaves a channel at most 512 / 64 = 8 workgroups, a workgroup iteration takes at most 8 x 4 planes: with
    B = 600 every workgroup walks at least three chunks, and the last chunk is ragged."""
    import cnn_with_pde_amd.functional as F_
    B, Cc, N = 600, 64, 8
    g = torch.Generator().manual_seed(9)
    u, du = torch.randn(B, Cc, N, N, generator=g).cuda(), torch.randn(B, Cc, N, N, generator=g).cuda()
    assert u.numel() * 4 < 10 << 20
    p = [(0.2 + torch.rand(Cc, N, N, generator=g)).cuda() for _ in range(2)] + [torch.randn(Cc, N, N, generator=g).cuda() for _ in range(2)]
    dp = [torch.randn(Cc, N, N, generator=g).cuda() for _ in range(4)]
    sweeps = tuple(s for st in F_.adi_schedule(0.4, 1.0, 1.3, 1, "strang") for s in st)
    y, yd = fused(u, du, p, dp, sweeps, True, 1.0)
    for lo, hi in ((0, 1), (31, 97), (599, 600)):
        yb, ydb = fused(u[lo:hi].contiguous(), du[lo:hi].contiguous(), p, dp, sweeps, True, 1.0)
        assert torch.equal(y[lo:hi], yb) and torch.equal(yd[lo:hi], ydb), (lo, hi)
    with torch.no_grad():
        assert torch.equal(y, F_.adi_diffuse(u, *p, sweeps, smooth3=True, clamp_max=1.0, eps=EPS))


# ---- misaligned views ---------------------------------------------------------------------------------------------------
def test_misaligned_views_are_copied():
    r = run(5)

    def shifted(t):                                      # the same values, 4 bytes off a 16-byte boundary
        buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    dp = list(r["dp"])
    dp[1] = shifted(dp[1])
    fy, fyd = _function(r, u=shifted(r["u"]), du=shifted(r["du"]), dp=dp)
    assert torch.equal(fy, r["y"]) and torch.equal(fyd, r["yd"])


# ---- layers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4], ids=[T.LAYER_IDS[k] for k in (1, 2, 3, 4)])
def test_layer_jvp_against_the_oracle(k):
    """FashionDiffusionLayer(28), SvhnDiffusionLayer(12, 3), EnhancedDiffusionLayer(12, 3) and (12, 8), two steps each: the
    check of tests/test_gpu_tangent.py at its gate, on layers whose every sweep now runs the fused tangent kernel."""
    import cnn_with_pde_amd._lib as L
    assert L.tangent_fused_enabled() and T._layers()[k][4][0] in T.FUSED
    T.test_layer_jvp_against_the_oracle(k)


# ---- graph capture ------------------------------------------------------------------------------------------------------
def test_graph_capture_of_the_tangent_call():
    r = run(9)
    assert r["case"][0] == 16
    dp = [torch.randn_like(t) for t in r["p"]]
    su, sdu = r["u"].clone(), torch.randn_like(r["u"])
    call = lambda: _function(r, u=su, du=sdu, dp=dp)                                                      # noqa: E731
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                            # warm-up: the per-kernel LDS attribute is set outside capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gy, gyd = call()
    su.copy_(torch.randn_like(su))
    sdu.copy_(torch.randn_like(sdu))
    graph.replay()
    torch.cuda.synchronize()
    ey, eyd = call()
    assert torch.equal(gy, ey) and torch.equal(gyd, eyd)


# ---- the switch -----------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(here)r]
import torch
import test_gpu_tangent_fused as TF
from cnn_with_pde_amd import _lib
assert not _lib.tangent_fused_enabled()
r = TF.run(5)
N, B, Cc, split, K, smooth3, cmax, mode = r["case"]
assert N == 28
fy, fyd = TF._function(r)
ay, ayd = TF.c_call("pde_adi_tangent", r["u"], r["du"], r["p"], r["dp"], r["sweeps"], smooth3, cmax)
assert torch.equal(fy, ay) and torch.equal(fyd, ayd), "PDE_TANGENT_FUSED=0 does not give pde_adi_tangent's bits"
assert not torch.equal(fyd, r["yd"])
print("any-size route")
"""


def test_the_switch_restores_the_any_size_route():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PDE_TANGENT_FUSED="0")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": os.path.dirname(here), "here": here}], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "any-size route" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
