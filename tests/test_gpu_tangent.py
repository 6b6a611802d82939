"""The tangent-linear (forward-mode) pass of the implicit layers: include/pdecnn_tangent.h (gen_factor_tangent_kernel and
gen_tangent_kernel of csrc/pde_adi_gen.hip), functional.adi_diffuse_tangent, the ``jvp`` of the ctypes nodes and
layers.layer_jvp.

Reference for every value: ``torch.autograd.forward_ad`` through the float64 oracle (oracle/pde_oracle.py), whose forward
AD matches central differences and its own reverse mode.  Gates, as max|err| / max|ref|: float64 1e-11 (the float64 gate of
tests/test_gpu_f64.py); fp32 max(1e-5, 4 min(o32, 1e-4)) with o32 the same error of the oracle's own forward AD in fp32
(the window rule of tests/test_gpu_fuzz.py); 16-bit tensors bitwise the rounding of the fp32 call on the up-cast inputs.
Inputs are built away from the clamp's kinks (no raw coefficient within 1e-4 of a bound, asserted), with at least a fifth
of the entries clamped in some sweep and a mask that moves between sweeps."""
import functools

import pytest
import torch
import torch.autograd.forward_ad as fwad

from oracle import pde_oracle as O
from test_gpu_parity import quiet

pytestmark = pytest.mark.gpu

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
EPS = 1e-6
NAMES = ("alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff")


def rel(a, ref):
    ref = ref.double().cpu()
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


# ---- inputs -----------------------------------------------------------------------------------------------------------
def _raw_coefficients(params, spec):
    """base + slope t of every sweep, [(axis, t, raw)]"""
    return [(ax, t, (params["alpha_base"] + params["alpha_time_coeff"] * t) if ax == 0 else
             (params["beta_base"] + params["beta_time_coeff"] * t)) for ax, _, t in O.sweep_schedule(spec)]


def _condition(params, spec):
    """(distance of the nearest raw coefficient to a clamp bound, largest clamped share of a sweep, whether a mask moves)"""
    near, share, masks = float("inf"), 0.0, {0: [], 1: []}
    for ax, _, raw in _raw_coefficients(params, spec):
        raw = raw.double()
        near = min(near, float((raw - spec.eps).abs().min()))
        clamped = raw < spec.eps
        if spec.clamp_max is not None:
            near = min(near, float((raw - spec.clamp_max).abs().min()))
            clamped = clamped | (raw > spec.clamp_max)
        share = max(share, float(clamped.double().mean()))
        masks[ax].append(clamped)
    if max(len(ms) for ms in masks.values()) > 1:      # a parameter's own mask at two times
        moves = any(bool((m != ms[0]).any()) for ms in masks.values() for m in ms[1:])
    else:                                               # one sweep per axis: the two sweeps' masks
        moves = bool((masks[0][0] != masks[1][0]).any())
    return near, share, moves


def _draw_pair(n, hi, dt, clamped_low, g):
    return (-clamped_low * hi + (1.3 + clamped_low) * hi * torch.rand(n, generator=g, dtype=F64),
            (hi / dt) * torch.randn(n, generator=g, dtype=F64))


def make_params(C, H, W, spec, g, dtype):
    """The four parameters (float64 values that ``dtype`` holds exactly): bases across both clamp bounds, slopes that carry
    entries over them during the schedule; an entry whose raw coefficient comes within 2e-4 of a bound in any sweep is
    drawn again."""
    hi = 2.0 if spec.clamp_max is None else spec.clamp_max
    low = 0.5 if spec.clamp_max is None else 0.3
    times = {0: sorted({t for ax, _, t in O.sweep_schedule(spec) if ax == 0}),
             1: sorted({t for ax, _, t in O.sweep_schedule(spec) if ax == 1})}
    params = {}
    for ax, (bn, sn) in ((0, ("alpha_base", "alpha_time_coeff")), (1, ("beta_base", "beta_time_coeff"))):
        base, slope = _draw_pair(C * H * W, hi, spec.dt, low, g)
        for _ in range(200):
            base, slope = base.to(dtype).double(), slope.to(dtype).double()
            bad = torch.zeros(C * H * W, dtype=torch.bool)
            for t in times[ax]:
                raw = base + slope * t
                bad |= (raw - spec.eps).abs() < 2e-4
                if spec.clamp_max is not None:
                    bad |= (raw - spec.clamp_max).abs() < 2e-4
            if not bool(bad.any()):
                break
            base[bad], slope[bad] = _draw_pair(int(bad.sum()), hi, spec.dt, low, g)
        params[bn], params[sn] = base.view(C, H, W), slope.view(C, H, W)
    return params


def make_inputs(B, C, H, W, spec, seed, dtype=F64):
    """u, du, the four parameters and their tangents (float64 values that ``dtype`` holds exactly, CPU) from the first seed
    at or after ``seed`` that meets the condition on the inputs; the condition is asserted."""
    for s in range(seed, seed + 100):
        g = torch.Generator().manual_seed(s)
        params = make_params(C, H, W, spec, g, dtype)
        near, share, moves = _condition(params, spec)
        if near >= 1e-4 and share >= 0.2 and moves:
            break
    near, share, moves = _condition(params, spec)
    assert near >= 1e-4 and share >= 0.2 and moves, (near, share, moves)
    q = lambda t: t.to(dtype).double()
    u = q(torch.randn(B, C, H, W, generator=g, dtype=F64))
    du = q(torch.randn(B, C, H, W, generator=g, dtype=F64))
    dparams = {n: q(torch.randn(C, H, W, generator=g, dtype=F64) * (1.0 if n.endswith("base") else 1.0 / spec.dt)) for n in NAMES}
    return u, du, params, dparams


def oracle_jvp(fn, u, du, params, dparams, dtype=F64):
    """(y, ydot) of ``fn(u, params)`` by forward AD in ``dtype`` on the CPU; absent tangents are None."""
    with fwad.dual_level():
        x = u.to(dtype) if du is None else fwad.make_dual(u.to(dtype), du.to(dtype))
        p = {k: (v.to(dtype) if dparams.get(k) is None else fwad.make_dual(v.to(dtype), dparams[k].to(dtype)))
             for k, v in params.items()}
        y, yd = fwad.unpack_dual(fn(x, p))
        return y.detach(), (torch.zeros_like(y) if yd is None else yd.detach())


# which tangents a case carries
MODES = {"both": (True, NAMES), "du": (True, ()), "params": (False, NAMES), "single": (False, ("beta_time_coeff",)),
         "single_a": (True, ("alpha_base",))}

#: (H, W, B, C, dtype, split, steps, smooth3, clamp_max, mode): the kernel's edges — the shortest lines, the kGenBatch boundary
#: and remainder (9, 10, 17), the fused sizes (28, 32), one past them, the second wave (65), the longest line, thin and
#: odd rectangles, and float64 on both sides of the LDS limit (101 x 101: the primal plane in the workspace)
CASES = [
    (2, 2, 3, 3, F32, "strang", 1, True, 1.5, "both"),
    (3, 3, 1, 3, F32, "lie", 2, False, 1.5, "params"),
    (9, 9, 3, 1, F32, "strang", 1, False, 1.5, "single"),
    (10, 10, 1, 1, F32, "lie", 2, True, None, "both"),
    (17, 17, 3, 3, F32, "strang", 1, True, 1.5, "du"),
    (28, 28, 3, 1, F32, "strang", 1, True, None, "both"),
    (32, 32, 1, 3, F32, "lie", 2, False, 1.5, "params"),
    (33, 33, 1, 3, F32, "strang", 1, False, 1.5, "single_a"),
    (65, 65, 3, 1, F32, "lie", 2, True, 1.5, "both"),
    (128, 128, 1, 1, F32, "strang", 1, False, 1.5, "both"),
    (2, 128, 3, 1, F32, "lie", 2, False, 1.5, "both"),
    (128, 3, 1, 3, F32, "strang", 1, True, 1.5, "params"),
    (5, 12, 3, 3, F32, "lie", 2, True, 1.5, "both"),
    (101, 101, 1, 1, F64, "lie", 1, False, 1.5, "both"),
    (20, 20, 3, 3, F64, "strang", 1, True, 1.5, "both"),
    (6, 10, 1, 3, F64, "lie", 2, False, 1.5, "single"),
]
IDS = ["%dx%d_b%dc%d_%s_%s%d_%s" % (c[0], c[1], c[2], c[3], str(c[4]).split(".")[1], c[5], c[6], c[9]) for c in CASES]
FUSED = (8, 12, 16, 20, 24, 28, 32)


def _spec(case):
    H, W, B, C, dtype, split, K, smooth3, cmax, mode = case
    return O.AdiSpec(H, C, 0.4, 1.0, 1.3, K, split, smooth3, cmax, "none", False, EPS)


def _sweeps(spec):
    import cnn_with_pde_amd.functional as F_
    return tuple(s for st in F_.adi_schedule(spec.dt, spec.dx, spec.dy, spec.num_steps, spec.split) for s in st)


def cabi_tangent(u, du, p, dp, sweeps, smooth3, cmax, want_y=True):
    """One pde_adi*_tangent call on device tensors: u, du in the tensors' type, parameters (C,H,W) in float / double."""
    import cnn_with_pde_amd._lib as L
    import cnn_with_pde_amd.functional as F_
    B, C, H, W = u.shape
    f64 = u.dtype == F64
    fam, cls, _ = F_._ADI_FAMILY[H != W, f64]
    d = F_._desc(cls, B, C, H, W, L.PDE_IO_F64 if f64 else F_._io_dtype(u), sweeps, smooth3, cmax, EPS)
    return F_._tangent_call(L.load(), fam, d, u, du, p, dp, want_y)


@functools.lru_cache(maxsize=None)
def run(i):
    """Everything the tests of case ``i`` share: the reference (computed once, never changed) and the library's results."""
    import cnn_with_pde_amd.functional as F_
    case = CASES[i]
    H, W, B, C, dtype, split, K, smooth3, cmax, mode = case
    spec, (with_du, names) = _spec(case), MODES[mode]
    u, du, params, dparams = make_inputs(B, C, H, W, spec, 1000 + 17 * i, dtype)
    du = du if with_du else None
    dparams = {n: (dparams[n] if n in names else None) for n in NAMES}
    fn = lambda a, p: O.adi_forward(a, p, spec)
    y_ref, yd_ref = oracle_jvp(fn, u, du, params, dparams)
    o32 = None
    if dtype == F32:
        o32 = rel(oracle_jvp(fn, u, du, params, dparams, F32)[1], yd_ref)
    dev = lambda t: None if t is None else t.to(dtype).cuda()
    r = dict(case=case, spec=spec, sweeps=_sweeps(spec), y_ref=y_ref, yd_ref=yd_ref, o32=o32, u=dev(u), du=dev(du),
             p=[dev(params[n]) for n in NAMES], dp=[dev(dparams[n]) for n in NAMES])
    r["y"], r["yd"] = cabi_tangent(r["u"], r["du"], r["p"], r["dp"], r["sweeps"], smooth3, cmax)
    r["fy"], r["fyd"] = F_.adi_diffuse_tangent(r["u"], *r["p"], r["sweeps"], du=r["du"], d_alpha_base=r["dp"][0],
                                               d_beta_base=r["dp"][1], d_alpha_time_coeff=r["dp"][2],
                                               d_beta_time_coeff=r["dp"][3], smooth3=smooth3, clamp_max=cmax, eps=EPS)
    torch.cuda.synchronize()
    return r


def gate(r):
    if r["case"][4] == F64:
        return 1e-11
    return max(1e-5, 4.0 * min(r["o32"], 1e-4))


# ---- value ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_value_against_the_float64_oracle(i):
    r = run(i)
    errs = {"y": rel(r["y"], r["y_ref"]), "ydot": rel(r["yd"], r["yd_ref"])}
    print(IDS[i], errs, "o32", r["o32"], "gate", gate(r))
    assert torch.isfinite(r["yd"]).all()
    assert errs["ydot"] <= gate(r) and errs["y"] <= gate(r), (errs, "o32", r["o32"])
    # the public function makes the same call
    assert torch.equal(r["fy"], r["y"]) and torch.equal(r["fyd"], r["yd"])


# ---- bitwise identities (the operations are gen_fwd_kernel's, in its order) ---------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_identities_with_the_forward(i):
    import cnn_with_pde_amd.functional as F_
    r = run(i)
    H, W, B, C, dtype, split, K, smooth3, cmax, mode = r["case"]
    kw = dict(smooth3=smooth3, clamp_max=cmax, eps=EPS)
    with torch.no_grad():
        y_fwd = F_.adi_diffuse(r["u"], *r["p"], r["sweeps"], **kw)
        if H == W and H in FUSED and dtype == F32:
            # the plain forward is the fused kernel there: another order of operations
            assert rel(r["y"], y_fwd) <= 1e-5
        else:
            assert torch.equal(r["y"], y_fwd)
            du = r["du"] if r["du"] is not None else torch.randn_like(r["u"])
            _, yd0 = cabi_tangent(r["u"], du, r["p"], [None] * 4, r["sweeps"], smooth3, cmax, want_y=False)
            assert torch.equal(yd0, F_.adi_diffuse(du, *r["p"], r["sweeps"], **kw))
    _, yd2 = cabi_tangent(r["u"], None if r["du"] is None else 2 * r["du"], r["p"],
                          [None if t is None else 2 * t for t in r["dp"]], r["sweeps"], smooth3, cmax, want_y=False)
    assert torch.equal(yd2, 2 * r["yd"])


# ---- duality with the library's own backward ----------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_duality_with_the_backward(i):
    import cnn_with_pde_amd.functional as F_
    r = run(i)
    H, W, B, C, dtype, split, K, smooth3, cmax, mode = r["case"]
    g = torch.randn(r["u"].shape, generator=torch.Generator().manual_seed(5 + i), dtype=F64).to(dtype).cuda()
    u = r["u"].clone().requires_grad_(True)
    p = [t.clone().requires_grad_(True) for t in r["p"]]
    y = F_.adi_diffuse(u, *p, r["sweeps"], smooth3=smooth3, clamp_max=cmax, eps=EPS)
    y.backward(g)
    dot = lambda a, b: float((a.double() * b.double()).sum())
    lhs = dot(r["yd"], g)
    rhs = (0.0 if r["du"] is None else dot(r["du"], u.grad)) + sum(dot(t, q.grad) for t, q in zip(r["dp"], p) if t is not None)
    scale = float(r["yd"].double().norm() * g.double().norm())
    print(IDS[i], "duality", abs(lhs - rhs) / scale)
    assert abs(lhs - rhs) <= (1e-11 if dtype == F64 else 1e-5) * scale, (lhs, rhs, scale)


# ---- 16-bit tensors: fp32 arithmetic, one rounding on the store ---------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("i", [4, 9, 12], ids=[IDS[4], IDS[9], IDS[12]])
def test_16_bit_tensors_round_the_fp32_result_once(i, dtype):
    import cnn_with_pde_amd.functional as F_
    r = run(i)
    H, W, B, C, _, split, K, smooth3, cmax, mode = r["case"]
    u16 = r["u"].to(dtype)
    du16 = (r["du"] if r["du"] is not None else torch.ones_like(r["u"])).to(dtype)
    y16, yd16 = cabi_tangent(u16, du16, r["p"], r["dp"], r["sweeps"], smooth3, cmax)
    y32, yd32 = cabi_tangent(u16.float(), du16.float(), r["p"], r["dp"], r["sweeps"], smooth3, cmax)
    assert y16.dtype == dtype and yd16.dtype == dtype
    assert torch.equal(yd16, yd32.to(dtype)) and torch.equal(y16, y32.to(dtype))
    if dtype == BF16:                                    # bf16 tensors with fp32 parameters are a route of the function's own
        fy, fyd = F_.adi_diffuse_tangent(u16, *r["p"], r["sweeps"], du=du16, d_alpha_base=r["dp"][0], d_beta_base=r["dp"][1],
                                         d_alpha_time_coeff=r["dp"][2], d_beta_time_coeff=r["dp"][3], smooth3=smooth3,
                                         clamp_max=cmax, eps=EPS)
        assert torch.equal(fy, y16) and torch.equal(fyd, yd16)


def test_function_refuses_a_call_without_tangents():
    import cnn_with_pde_amd.functional as F_
    r = run(1)
    with pytest.raises(ValueError):
        F_.adi_diffuse_tangent(r["u"], *r["p"], r["sweeps"])


# ---- torch.autograd.forward_ad through the nodes ------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 4, 6, 12, 14], ids=[IDS[k] for k in (0, 4, 6, 12, 14)])
def test_forward_ad_through_adi_diffuse(i):
    """Raises torch's NotImplementedError ("You must implement the jvp function") without the node's jvp."""
    import cnn_with_pde_amd.functional as F_
    r = run(i)
    H, W, B, C, dtype, split, K, smooth3, cmax, mode = r["case"]
    with fwad.dual_level():
        u = r["u"] if r["du"] is None else fwad.make_dual(r["u"], r["du"])
        p = [t if dt is None else fwad.make_dual(t, dt) for t, dt in zip(r["p"], r["dp"])]
        y, yd = fwad.unpack_dual(F_.adi_diffuse(u, *p, r["sweeps"], smooth3=smooth3, clamp_max=cmax, eps=EPS))
        assert yd is not None
        errs = {"y": rel(y, r["y_ref"]), "ydot": rel(yd, r["yd_ref"])}
    print(IDS[i], errs, "o32", r["o32"])
    assert max(errs.values()) <= gate(r), (errs, "o32", r["o32"])
    if any(t is not None for t in r["dp"]):
        assert torch.equal(yd, r["yd"])                  # one *_tangent call: the same launches


@pytest.mark.parametrize("dtype", [F32, F64])
def test_forward_ad_through_channel_mix_and_skip_blend(dtype):
    import cnn_with_pde_amd.functional as F_
    g = torch.Generator().manual_seed(11)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    u, ut, u0, u0t, M, Mt, w, wt = mk(3, 5, 6, 7), mk(3, 5, 6, 7), mk(3, 5, 6, 7), mk(3, 5, 6, 7), mk(5, 5), mk(5, 5), mk(1), mk(1)
    tol = 1e-11 if dtype == F64 else 1e-5
    d = lambda t: t.to(dtype).cuda()
    mix = lambda a, m: torch.einsum("ij,bjhw->bihw", m, a)
    blend = lambda a, b, s: torch.sigmoid(s) * a + (1 - torch.sigmoid(s)) * b
    for tu, tm in ((ut, Mt), (ut, None), (None, Mt)):
        with fwad.dual_level():
            y_ref, yd_ref = fwad.unpack_dual(mix(u if tu is None else fwad.make_dual(u, tu),
                                                 M if tm is None else fwad.make_dual(M, tm)))
            y, yd = fwad.unpack_dual(F_.channel_mix(d(u) if tu is None else fwad.make_dual(d(u), d(tu)),
                                                    d(M) if tm is None else fwad.make_dual(d(M), d(tm))))
            assert rel(y, y_ref) <= tol and rel(yd, yd_ref) <= tol
    for t0, t1, tw in ((u0t, ut, wt), (u0t, None, None), (None, None, wt), (None, ut, wt)):
        with fwad.dual_level():
            dual = lambda a, t, f=(lambda z: z): f(a) if t is None else fwad.make_dual(f(a), f(t))
            y_ref, yd_ref = fwad.unpack_dual(blend(dual(u0, t0), dual(u, t1), dual(w, tw)))
            y, yd = fwad.unpack_dual(F_.skip_blend(dual(u0, t0, d), dual(u, t1, d), dual(w, tw, d)))
            assert rel(y, y_ref) <= tol and rel(yd, yd_ref) <= tol


def _layers():
    import cnn_with_pde_amd as P
    return [
        ("mnist9", lambda: quiet(P.MnistDiffusionLayer, 9, 0.4, 1.0, 1.3, 2), O.mnist_spec(9, 0.4, 1.0, 1.3, 2), 1, (9, 9), F32),
        ("fashion28", lambda: quiet(P.FashionDiffusionLayer, 28, 0.4, 1.0, 2), O.fashion_spec(28, 0.4, 1.0, 2), 1, (28, 28), F32),
        ("svhn12c3", lambda: quiet(P.SvhnDiffusionLayer, 12, 3, 0.4, 1.0, 2), O.svhn_spec(12, 3, 0.4, 1.0, 2), 3, (12, 12), F32),
        ("enhanced12c3", lambda: quiet(P.EnhancedDiffusionLayer, 12, 3, 0.4, 1.0, 1.3, 2), O.cifar10_spec(12, 3, 0.4, 1.0, 1.3, 2),
         3, (12, 12), F32),
        ("enhanced12c8", lambda: quiet(P.EnhancedDiffusionLayer, 12, 8, 0.4, 1.0, 1.3, 2), O.cifar10_spec(12, 8, 0.4, 1.0, 1.3, 2),
         8, (12, 12), F32),
        ("learnable12c3", lambda: quiet(P.LearnableDiffusionLayer, 12, 3, 0.4, 1.0, 1.3, 2), O.cifar2_spec(12, 3, 0.4, 1.0, 1.3, 2),
         3, (12, 12), F32),
        ("enhanced_rect6x10", lambda: quiet(P.EnhancedDiffusionLayer, (6, 10), 3, 0.4, 1.0, 1.3, 2),
         O.cifar10_spec(6, 3, 0.4, 1.0, 1.3, 2), 3, (6, 10), F32),
        ("enhanced12c3_f64", lambda: quiet(P.EnhancedDiffusionLayer, 12, 3, 0.4, 1.0, 1.3, 2), O.cifar10_spec(12, 3, 0.4, 1.0, 1.3, 2),
         3, (12, 12), F64),
    ]


LAYER_IDS = ["mnist9", "fashion28", "svhn12c3", "enhanced12c3", "enhanced12c8", "learnable12c3", "enhanced_rect6x10",
             "enhanced12c3_f64"]


@pytest.mark.parametrize("k", range(len(LAYER_IDS)), ids=LAYER_IDS)
def test_layer_jvp_against_the_oracle(k):
    """Raises torch's NotImplementedError without the nodes' jvp."""
    import cnn_with_pde_amd as P
    name, make, spec, C, (H, W), dtype = _layers()[k]
    g = torch.Generator().manual_seed(300 + k)
    ly = make()
    drawn = make_params(C, H, W, spec, g, dtype)
    with torch.no_grad():
        for n, p in ly.named_parameters():
            if n in NAMES:
                p.copy_(drawn[n].view_as(p))
            if n in ("channel_mixing", "channel_coupling"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            if n == "skip_weight":
                p.fill_(0.3)
    ly = ly.to(dtype)
    params = {n: p.detach().clone().double() for n, p in ly.named_parameters()}
    near, _, _ = _condition({n: (v if v.dim() == 3 else v.unsqueeze(0)) for n, v in params.items() if n in NAMES}, spec)
    assert near >= 1e-4, near
    q = lambda t: t.to(dtype).double()
    u, du = q(torch.randn(3, C, H, W, generator=g, dtype=F64)), q(torch.randn(3, C, H, W, generator=g, dtype=F64))
    dparams = {n: q(torch.randn(p.shape, generator=g, dtype=F64) * (1.0 / spec.dt if n.endswith("time_coeff") else 1.0))
               for n, p in params.items()}
    fn = lambda a, p: O.adi_forward(a, p, spec)
    ly = ly.cuda()
    for use_du, names in ((True, tuple(params)), (True, ()), (False, ("alpha_time_coeff",))):
        dp = {n: dparams[n] for n in names}
        y_ref, yd_ref = oracle_jvp(fn, u, du if use_du else None, params, dp)
        y, yd = P.layer_jvp(ly, u.to(dtype).cuda(), du.to(dtype).cuda() if use_du else None,
                            {n: t.to(dtype).cuda() for n, t in dp.items()})
        if dtype == F64:
            tol, o32 = 1e-11, None
        else:
            o32 = rel(oracle_jvp(fn, u, du if use_du else None, params, dp, F32)[1], yd_ref)
            tol = max(1e-5, 4.0 * min(o32, 1e-4))
        errs = {"y": rel(y, y_ref), "ydot": rel(yd, yd_ref)}
        print(name, names, errs, "o32", o32)
        assert y.dtype == dtype and max(errs.values()) <= tol, (errs, "o32", o32)
        with torch.no_grad():
            assert torch.equal(y, ly(u.to(dtype).cuda())) or rel(y, ly(u.to(dtype).cuda())) <= 1e-5


def test_layer_jvp_refuses_the_explicit_layers():
    import cnn_with_pde_amd as P
    pl = quiet(P.PDELayer, 16, 16)
    with pytest.raises(TypeError):
        P.layer_jvp(pl, torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))
    il = quiet(P.ImprovedDiffusionLayer, 16, 2)
    with pytest.raises(TypeError):
        P.layer_jvp(il, torch.zeros(1, 2, 16, 16), torch.zeros(1, 2, 16, 16))


def test_gradcheck_with_forward_ad():
    import cnn_with_pde_amd.functional as F_
    g = torch.Generator().manual_seed(21)
    spec = O.AdiSpec(4, 2, 0.4, 1.0, 1.3, 1, "strang", True, 1.5, "none", False, EPS)
    u, _, params, _ = make_inputs(2, 2, 4, 4, spec, 77)
    sweeps = _sweeps(spec)
    ins = [t.cuda().requires_grad_(True) for t in (u, *[params[n] for n in NAMES])]
    fn = lambda a, ab, bb, asl, bsl: F_.adi_diffuse(a, ab, bb, asl, bsl, sweeps, smooth3=True, clamp_max=1.5, eps=EPS)
    assert torch.autograd.gradcheck(fn, ins, eps=1e-6, atol=1e-6, rtol=1e-5, check_forward_ad=True, check_backward_ad=True,
                                    check_undefined_grad=False, check_batched_grad=False)


# ---- nothing else moves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 3, 16, 16), (2, 3, 10, 10), (2, 2, 6, 9)])
def test_no_tangent_no_change(shape):
    """Inside a dual level without a tangent the routes, the results and what the frozen node keeps are those outside."""
    import cnn_with_pde_amd.functional as F_
    B, C, H, W = shape
    g = torch.Generator().manual_seed(3)
    u = torch.randn(shape, generator=g).cuda().requires_grad_(True)
    p = [(0.5 + torch.rand(C, H, W, generator=g)).cuda() for _ in range(2)] + [torch.randn(C, H, W, generator=g).cuda() for _ in range(2)]
    sweeps = tuple(s for st in F_.adi_schedule(0.3, 1.0, 1.0, 2) for s in st)
    y0 = F_.adi_diffuse(u, *p, sweeps, clamp_max=2.0)
    with fwad.dual_level():
        y1 = F_.adi_diffuse(u, *p, sweeps, clamp_max=2.0)
        assert fwad.unpack_dual(y1).tangent is None
    assert torch.equal(y0, y1) and type(y0.grad_fn) is type(y1.grad_fn)
    if hasattr(y1.grad_fn, "saved_tensors"):             # the ctypes node on its frozen route: the four coefficient views alone
        kept = [t for t in y1.grad_fn.saved_tensors if t is not None]
        assert len(kept) == 4 and all(tuple(t.shape) == (C, H, W) for t in kept)
    gy = torch.randn(shape, generator=g).cuda()
    (g0,), (g1,) = torch.autograd.grad(y0, u, gy), torch.autograd.grad(y1, u, gy)
    assert torch.equal(g0, g1)


def test_trajectory_under_a_dual_level_is_refused():
    import cnn_with_pde_amd.functional as F_
    r = run(1)
    H, W, B, C, dtype, split, K, smooth3, cmax, mode = r["case"]
    with fwad.dual_level():
        u = fwad.make_dual(r["u"], torch.ones_like(r["u"]))
        with pytest.raises(NotImplementedError, match="trajectory"):
            F_.adi_diffuse_states(u, *r["p"], r["sweeps"], [0], smooth3=smooth3, clamp_max=cmax, eps=EPS)


def test_graph_capture_of_the_tangent_call():
    import cnn_with_pde_amd.functional as F_
    r = run(4)
    H, W, B, C, dtype, split, K, smooth3, cmax, mode = r["case"]
    dp = [torch.randn_like(t) for t in r["p"]]
    su, sdu = r["u"].clone(), torch.randn_like(r["u"])
    call = lambda: F_.adi_diffuse_tangent(su, *r["p"], r["sweeps"], du=sdu, d_alpha_base=dp[0], d_beta_base=dp[1],
                                          d_alpha_time_coeff=dp[2], d_beta_time_coeff=dp[3], smooth3=smooth3,
                                          clamp_max=cmax, eps=EPS)
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


def test_workgroups_that_walk_several_planes():
    """float64 beyond the LDS limit with more planes than workgroups (C = 64: four groups for five samples): a workgroup
    reuses its slice of the workspace for its next plane.  Bitwise the same call made sample by sample, and y bitwise the
    forward's."""
    import cnn_with_pde_amd.functional as F_
    B, C, H, W = 5, 64, 81, 128
    g = torch.Generator().manual_seed(9)
    u, du = torch.randn(B, C, H, W, generator=g, dtype=F64).cuda(), torch.randn(B, C, H, W, generator=g, dtype=F64).cuda()
    p = [(0.2 + torch.rand(C, H, W, generator=g, dtype=F64)).cuda() for _ in range(2)] + \
        [torch.randn(C, H, W, generator=g, dtype=F64).cuda() for _ in range(2)]
    dp = [torch.randn(C, H, W, generator=g, dtype=F64).cuda() for _ in range(4)]
    sweeps = tuple(s for st in F_.adi_schedule(0.4, 1.0, 1.3, 1, "lie") for s in st)
    y, yd = cabi_tangent(u, du, p, dp, sweeps, False, 1.0)
    for b in range(B):
        yb, ydb = cabi_tangent(u[b:b + 1].contiguous(), du[b:b + 1].contiguous(), p, dp, sweeps, False, 1.0)
        assert torch.equal(y[b:b + 1], yb) and torch.equal(yd[b:b + 1], ydb), b
    with torch.no_grad():
        assert torch.equal(y, F_.adi_diffuse(u, *p, sweeps, clamp_max=1.0, eps=EPS))
