"""The tangent-linear (forward-mode) pass of the explicit 5-point and the Jacobi layers: include/pdecnn_explicit_tangent.h
(explicit5_tangent_wave, explicit5_tangent[_col]_kernel, jacobi_tangent_kernel, jacobi_tiled_tangent_kernel and the
float64 forms), functional.explicit5_tangent / jacobi_diffuse_tangent, the ``jvp`` of the two ctypes nodes and
layers.explicit_layer_jvp.

Reference for every value: ``torch.autograd.forward_ad`` in float64 on the CPU through the oracle as it stands
(``O.tiny_forward``, ``O.jacobi_forward``, ``O.emotion_coefficients``), the ``oracle_jvp`` idiom of tests/test_gpu_tangent.py.
Gates, as max|err| / max|ref|, are that file's: float64 1e-11; fp32 max(1e-5, 4 min(o32, 1e-4)) with o32 the same error of
the oracle's own forward AD in fp32; 16-bit tensors bitwise the rounding of the fp32 call on the up-cast inputs.

The scalars of the explicit step (dt, eps, max_coeff, relax) are values fp32 holds exactly, so the float64 oracle and the
fp32 kernels clamp at the same bounds: every explicit case has a channel below eps, one exactly max_coeff (where the
derivative passes, in the kernels as in torch's clamp) and one inside where C allows."""
import functools

import pytest
import torch
import torch.autograd.forward_ad as fwad

from oracle import pde_oracle as O
from test_gpu_parity import quiet
from test_gpu_tangent import oracle_jvp, rel

pytestmark = pytest.mark.gpu

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16


def f32(x):
    return float(torch.tensor(x, dtype=F32))


DT, EPS, MAXC, RELAX = f32(0.5), f32(1e-6), f32(0.15), f32(0.625)
EX_NAMES = ("alpha_base", "channel_scaling")
JAC_NAMES = ("a_row", "b_col")
#: which tangents a case carries: (du, parameter tangents by position)
MODES = {"both": (True, (0, 1)), "du": (True, ()), "params": (False, (0, 1)), "single": (False, (1,)), "single_a": (True, (0,))}
MODE_ORDER = ("both", "params", "single", "single_a", "du")

#: (path, B, C, H, W, num_steps, dtype).  Wave: plane counts that are no multiple of 4 leave the last workgroup partly filled.
EX_CASES = [("wave", 1, 3, 16, 16, 1, F32), ("wave", 5, 1, 32, 32, 3, F32), ("wave", 1, 5, 64, 64, 2, F32),
            ("float4", 2, 3, 1, 4, 2, F32), ("float4", 1, 2, 8, 12, 3, F32), ("float4", 3, 1, 20, 4, 1, F32),
            ("col", 2, 3, 1, 1, 2, F32), ("col", 1, 2, 5, 7, 3, F32), ("col", 1, 1, 33, 33, 2, F32), ("col", 2, 1, 3, 2, 1, F32),
            ("f64", 2, 3, 5, 7, 3, F64), ("f64", 1, 2, 16, 16, 2, F64)]
#: (path, B, H, W, nt, dtype).  Tiled: ring and folded row in different tiles (65), both sides of the 10 steps of one launch.
JAC_CASES = [("one", 3, 4, 4, 1, F32), ("one", 1, 5, 9, 3, F32), ("one", 2, 48, 48, 10, F32), ("one", 1, 64, 64, 2, F32),
             ("tiled", 1, 65, 65, 1, F32), ("tiled", 2, 64, 130, 10, F32), ("tiled", 1, 130, 67, 11, F32),
             ("tiled", 1, 70, 66, 21, F32), ("f64", 1, 4, 7, 3, F64), ("f64", 2, 64, 64, 2, F64)]
#: where the cycle below eps / exactly max_coeff / inside / above starts in the cases with fewer than three channels
ROT = {1: 1, 5: 0, 8: 2, 9: 1, 4: 0, 7: 1, 11: 1}
EX_MODE = [MODE_ORDER[i % 5] for i in range(len(EX_CASES))]
JAC_MODE = [MODE_ORDER[(i + 1) % 5] for i in range(len(JAC_CASES))]
EX_IDS = ["%s_b%dc%d_%dx%d_k%d_%s_%s" % (c[0], c[1], c[2], c[3], c[4], c[5], str(c[6]).split(".")[1], m)
          for c, m in zip(EX_CASES, EX_MODE)]
JAC_IDS = ["%s_b%d_%dx%d_nt%d_%s_%s" % (c[0], c[1], c[2], c[3], c[4], str(c[5]).split(".")[1], m)
           for c, m in zip(JAC_CASES, JAC_MODE)]


def make_alpha(C, rot, g, dtype=F32):
    """alpha_base (float64 values that ``dtype`` holds exactly): channel c is below eps, exactly max_coeff, inside or above
    max_coeff in turn, starting at ``rot``."""
    kinds = (-0.02, MAXC, None, 0.3)
    vals = [kinds[(c + rot) % 4] for c in range(C)]
    a = torch.tensor([0.03 + 0.09 * float(torch.rand((), generator=g, dtype=F64)) if v is None else v for v in vals], dtype=F64)
    a = a.to(dtype).double()
    assert all(float(a[c]) == MAXC for c in range(C) if (c + rot) % 4 == 1)
    return a


def gate(dtype, o32):
    return 1e-11 if dtype == F64 else max(1e-5, 4.0 * min(o32, 1e-4))


def _pick(mode, du, dps):
    with_du, idx = MODES[mode]
    return (du if with_du else None), [dps[k] if k in idx else None for k in range(len(dps))]


def cabi_explicit(u, du, p, dp, K, want_y=True, cfg=None):
    """One pde_explicit5[_f64]_tangent call on device tensors."""
    import cnn_with_pde_amd._lib as L
    import cnn_with_pde_amd.functional as F_
    return F_._explicit5_tangent_call(L.load(), u.dtype == F64, u, du, p[0], p[1], dp[0], dp[1],
                                      cfg or (DT, EPS, MAXC, RELAX, K), want_y)


def cabi_jacobi(u, du, p, dp, nt, want_y=True):
    """One pde_jacobi_io_tangent / pde_jacobi_f64_tangent call on device tensors."""
    import cnn_with_pde_amd._lib as L
    import cnn_with_pde_amd.functional as F_
    return F_._jacobi_tangent_call(L.load(), u.dtype == F64, u, du, p[0], p[1], dp[0], dp[1], nt, want_y)


def ex_fn(K):
    return lambda a, p: O.tiny_forward(a, p, DT, K, EPS, MAXC, RELAX)


def jac_fn(nt):
    return lambda a, p: O.jacobi_forward(a, p["a_row"], p["b_col"], nt)


@functools.lru_cache(maxsize=None)
def run_ex(i):
    """Everything the tests of explicit case ``i`` share: the reference (computed once, never changed) and the results."""
    import cnn_with_pde_amd.functional as F_
    path, B, C, H, W, K, dtype = EX_CASES[i]
    g = torch.Generator().manual_seed(4000 + 31 * i)
    q = lambda t: t.to(dtype).double()
    params = {"alpha_base": make_alpha(C, ROT.get(i, 0), g, dtype),
              "channel_scaling": q(1.0 + 0.3 * torch.randn(C, generator=g, dtype=F64))}
    u, du = q(torch.randn(B, C, H, W, generator=g, dtype=F64)), q(torch.randn(B, C, H, W, generator=g, dtype=F64))
    dps = [q(0.1 * torch.randn(C, generator=g, dtype=F64)), q(torch.randn(C, generator=g, dtype=F64))]
    du, dps = _pick(EX_MODE[i], du, dps)
    dparams = dict(zip(EX_NAMES, dps))
    y_ref, yd_ref = oracle_jvp(ex_fn(K), u, du, params, dparams)
    o32 = rel(oracle_jvp(ex_fn(K), u, du, params, dparams, F32)[1], yd_ref) if dtype == F32 else None
    dev = lambda t: None if t is None else t.to(dtype).cuda()
    r = dict(case=EX_CASES[i], K=K, dtype=dtype, y_ref=y_ref, yd_ref=yd_ref, o32=o32, u=dev(u), du=dev(du),
             p=[dev(params[n]) for n in EX_NAMES], dp=[dev(t) for t in dps])
    r["y"], r["yd"] = cabi_explicit(r["u"], r["du"], r["p"], r["dp"], K)
    r["fy"], r["fyd"] = F_.explicit5_tangent(r["u"], *r["p"], du=r["du"], d_alpha_base=r["dp"][0], d_channel_scaling=r["dp"][1],
                                             dt=DT, eps=EPS, max_coeff=MAXC, relax=RELAX, num_steps=K)
    torch.cuda.synchronize()
    return r


@functools.lru_cache(maxsize=None)
def run_jac(i):
    import cnn_with_pde_amd.functional as F_
    path, B, H, W, nt, dtype = JAC_CASES[i]
    g = torch.Generator().manual_seed(5000 + 31 * i)
    q = lambda t: t.to(dtype).double()
    params = {"a_row": q(0.05 + 0.15 * torch.rand(H, generator=g, dtype=F64)),
              "b_col": q(0.05 + 0.15 * torch.rand(W, generator=g, dtype=F64))}
    u, du = q(torch.randn(B, H, W, generator=g, dtype=F64)), q(torch.randn(B, H, W, generator=g, dtype=F64))
    dps = [q(0.1 * torch.randn(H, generator=g, dtype=F64)), q(0.1 * torch.randn(W, generator=g, dtype=F64))]
    du, dps = _pick(JAC_MODE[i], du, dps)
    dparams = dict(zip(JAC_NAMES, dps))
    y_ref, yd_ref = oracle_jvp(jac_fn(nt), u, du, params, dparams)
    o32 = rel(oracle_jvp(jac_fn(nt), u, du, params, dparams, F32)[1], yd_ref) if dtype == F32 else None
    dev = lambda t: None if t is None else t.to(dtype).cuda()
    r = dict(case=JAC_CASES[i], nt=nt, dtype=dtype, y_ref=y_ref, yd_ref=yd_ref, o32=o32, u=dev(u), du=dev(du),
             p=[dev(params[n]) for n in JAC_NAMES], dp=[dev(t) for t in dps])
    r["y"], r["yd"] = cabi_jacobi(r["u"], r["du"], r["p"], r["dp"], nt)
    r["fy"], r["fyd"] = F_.jacobi_diffuse_tangent(r["u"], *r["p"], nt, du=r["du"], d_a_row=r["dp"][0], d_b_col=r["dp"][1])
    torch.cuda.synchronize()
    return r


# ---- value ------------------------------------------------------------------------------------------------------------
def _check_value(tag, r):
    errs = {"y": rel(r["y"], r["y_ref"]), "ydot": rel(r["yd"], r["yd_ref"])}
    tol = gate(r["dtype"], r["o32"])
    print(tag, errs, "o32", r["o32"], "gate", tol)
    assert torch.isfinite(r["yd"]).all() and float(r["yd_ref"].abs().max()) > 0
    assert errs["ydot"] <= tol and errs["y"] <= tol, (errs, "o32", r["o32"])
    # the public function makes the same call
    assert torch.equal(r["fy"], r["y"]) and torch.equal(r["fyd"], r["yd"])


@pytest.mark.parametrize("i", range(len(EX_CASES)), ids=EX_IDS)
def test_explicit_value_against_the_float64_oracle(i):
    _check_value(EX_IDS[i], run_ex(i))


@pytest.mark.parametrize("i", range(len(JAC_CASES)), ids=JAC_IDS)
def test_jacobi_value_against_the_float64_oracle(i):
    _check_value(JAC_IDS[i], run_jac(i))


def test_the_drawn_alphas_meet_every_side_of_the_clamp():
    for i, (path, B, C, H, W, K, dtype) in enumerate(EX_CASES):
        a = run_ex(i)["p"][0].double().cpu()
        kinds = {"below": bool((a < EPS).any()), "at_max": bool((a == MAXC).any()), "inside": bool(((a > EPS) & (a < MAXC)).any())}
        assert sum(kinds.values()) == min(C, 3), (EX_IDS[i], a, kinds)
        assert C >= 3 or i in ROT
    seen = set()
    for i in range(len(EX_CASES)):
        a = run_ex(i)["p"][0].double().cpu()
        seen |= {"below"} if bool((a < EPS).any()) else set()
        seen |= {"at_max"} if bool((a == MAXC).any()) else set()
        seen |= {"inside"} if bool(((a > EPS) & (a < MAXC)).any()) else set()
        seen |= {"above"} if bool((a > MAXC).any()) else set()
    assert seen == {"below", "at_max", "inside", "above"}


# ---- bitwise identities (the operations are the forward kernels', in their order) ---------------------------------------
def _scaled(t, k):
    return None if t is None else k * t


@pytest.mark.parametrize("i", range(len(EX_CASES)), ids=EX_IDS)
def test_explicit_identities_with_the_forward(i):
    import cnn_with_pde_amd.functional as F_
    r = run_ex(i)
    K = r["K"]
    kw = dict(dt=DT, eps=EPS, max_coeff=MAXC, relax=RELAX, num_steps=K)
    with torch.no_grad():
        assert torch.equal(r["y"], F_.explicit5_step(r["u"], *r["p"], **kw))
        du = r["du"] if r["du"] is not None else torch.randn_like(r["u"])
        _, yd0 = cabi_explicit(r["u"], du, r["p"], [None, None], K, want_y=False)
        assert torch.equal(yd0, F_.explicit5_step(du, *r["p"], **kw))
    _, yd4 = cabi_explicit(r["u"], _scaled(r["du"], 4), r["p"], [_scaled(t, 4) for t in r["dp"]], K, want_y=False)
    assert torch.equal(yd4, 4 * r["yd"])
    y2, yd2 = cabi_explicit(r["u"], r["du"], r["p"], r["dp"], K)
    assert torch.equal(y2, r["y"]) and torch.equal(yd2, r["yd"])


@pytest.mark.parametrize("i", range(len(JAC_CASES)), ids=JAC_IDS)
def test_jacobi_identities_with_the_forward(i):
    import cnn_with_pde_amd.functional as F_
    r = run_jac(i)
    nt = r["nt"]
    with torch.no_grad():
        assert torch.equal(r["y"], F_.jacobi_diffuse(r["u"], *r["p"], nt))
        du = r["du"] if r["du"] is not None else torch.randn_like(r["u"])
        _, yd0 = cabi_jacobi(r["u"], du, r["p"], [None, None], nt, want_y=False)
        assert torch.equal(yd0, F_.jacobi_diffuse(du, *r["p"], nt))
    _, yd4 = cabi_jacobi(r["u"], _scaled(r["du"], 4), r["p"], [_scaled(t, 4) for t in r["dp"]], nt, want_y=False)
    assert torch.equal(yd4, 4 * r["yd"])
    y2, yd2 = cabi_jacobi(r["u"], r["du"], r["p"], r["dp"], nt)
    assert torch.equal(y2, r["y"]) and torch.equal(yd2, r["yd"])


# ---- duality with the library's own backward ----------------------------------------------------------------------------
def _duality(tag, r, y, u, p, seed):
    dtype = r["dtype"]
    g = torch.randn(r["u"].shape, generator=torch.Generator().manual_seed(seed), dtype=F64).to(dtype).cuda()
    y.backward(g)
    dot = lambda a, b: float((a.double() * b.double()).sum())
    lhs = dot(r["yd"], g)
    rhs = (0.0 if r["du"] is None else dot(r["du"], u.grad)) + sum(dot(t, q.grad) for t, q in zip(r["dp"], p) if t is not None)
    scale = float(r["yd"].double().norm() * g.double().norm())
    print(tag, "duality", abs(lhs - rhs) / scale)
    # float64: the gate the feature was asked to meet.  The fp32 kernel paths are an EXTRA check beside it, at the bound
    # tests/test_gpu_tangent.py holds its fp32 cases to (both sides come from fp32 kernels; 1e-11 is not theirs to meet)
    assert abs(lhs - rhs) <= (1e-11 if dtype == F64 else 1e-5) * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("i", [10, 11, 0, 4, 7], ids=[EX_IDS[k] for k in (10, 11, 0, 4, 7)])
def test_explicit_duality_with_the_backward(i):
    """<gy, ydot> = <gu, du> + <gtheta, dtheta>: the float64 kernels to 1e-11; extra, once per fp32 kernel path, to 1e-5."""
    import cnn_with_pde_amd.functional as F_
    r = run_ex(i)
    u = r["u"].clone().requires_grad_(True)
    p = [t.clone().requires_grad_(True) for t in r["p"]]
    y = F_.explicit5_step(u, *p, dt=DT, eps=EPS, max_coeff=MAXC, relax=RELAX, num_steps=r["K"])
    _duality(EX_IDS[i], r, y, u, p, 50 + i)


@pytest.mark.parametrize("i", [8, 9, 2, 6], ids=[JAC_IDS[k] for k in (8, 9, 2, 6)])
def test_jacobi_duality_with_the_backward(i):
    import cnn_with_pde_amd.functional as F_
    r = run_jac(i)
    u = r["u"].clone().requires_grad_(True)
    p = [t.clone().requires_grad_(True) for t in r["p"]]
    y = F_.jacobi_diffuse(u, *p, r["nt"])
    _duality(JAC_IDS[i], r, y, u, p, 70 + i)


# ---- 16-bit tensors: fp32 arithmetic, one rounding on the store, fp32 between the launches --------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("i", [0, 1, 2, 4, 7], ids=[EX_IDS[k] for k in (0, 1, 2, 4, 7)])
def test_explicit_16_bit_tensors_round_the_fp32_result_once(i, dtype):
    """Every kernel path that takes the type, the three register sizes each: the 16 x 16 wave kernel is the one whose step
    fuses the other product, in all three tensor types.  y is also the 16-bit forward's y, bit for bit."""
    import cnn_with_pde_amd.functional as F_
    r = run_ex(i)
    K = r["K"]
    u16 = r["u"].to(dtype)
    du16 = (r["du"] if r["du"] is not None else torch.ones_like(r["u"])).to(dtype)
    y16, yd16 = cabi_explicit(u16, du16, r["p"], r["dp"], K)
    y32, yd32 = cabi_explicit(u16.float(), du16.float(), r["p"], r["dp"], K)
    assert y16.dtype == dtype and yd16.dtype == dtype
    assert torch.equal(yd16, yd32.to(dtype)) and torch.equal(y16, y32.to(dtype))
    if dtype == BF16:                                    # bf16 tensors with fp32 parameters are a route of the function's own
        fy, fyd = F_.explicit5_tangent(u16, *r["p"], du=du16, d_alpha_base=r["dp"][0], d_channel_scaling=r["dp"][1], dt=DT,
                                       eps=EPS, max_coeff=MAXC, relax=RELAX, num_steps=K)
        assert torch.equal(fy, y16) and torch.equal(fyd, yd16)
        with torch.no_grad():
            y_fwd = F_.explicit5_step(u16, *r["p"], dt=DT, eps=EPS, max_coeff=MAXC, relax=RELAX, num_steps=K)
        assert y_fwd.dtype == BF16 and torch.equal(y16, y_fwd)
    else:                                                # the float16 route: every parameter fp16 too
        ph = [t.half() for t in r["p"]]
        fy, fyd = F_.explicit5_tangent(u16, *ph, du=du16, d_alpha_base=r["dp"][0], d_channel_scaling=r["dp"][1], dt=DT,
                                       eps=EPS, max_coeff=MAXC, relax=RELAX, num_steps=K)
        ey, eyd = cabi_explicit(u16, du16, [t.float() for t in ph], r["dp"], K)
        assert fy.dtype == F16 and torch.equal(fy, ey) and torch.equal(fyd, eyd)
        with torch.no_grad():
            y_fwd = F_.explicit5_step(u16, *ph, dt=DT, eps=EPS, max_coeff=MAXC, relax=RELAX, num_steps=K)
        assert y_fwd.dtype == F16 and torch.equal(ey, y_fwd)


@pytest.mark.parametrize("i", [2, 6], ids=[JAC_IDS[k] for k in (2, 6)])
def test_jacobi_fp16_tensors_round_the_fp32_result_once(i):
    import cnn_with_pde_amd.functional as F_
    r = run_jac(i)
    nt = r["nt"]
    u16 = r["u"].half()
    du16 = (r["du"] if r["du"] is not None else torch.ones_like(r["u"])).half()
    y16, yd16 = cabi_jacobi(u16, du16, r["p"], r["dp"], nt)
    y32, yd32 = cabi_jacobi(u16.float(), du16.float(), r["p"], r["dp"], nt)
    assert y16.dtype == F16 and yd16.dtype == F16
    assert torch.equal(yd16, yd32.half()) and torch.equal(y16, y32.half())
    ph = [t.half() for t in r["p"]]
    fy, fyd = F_.jacobi_diffuse_tangent(u16, *ph, nt, du=du16, d_a_row=r["dp"][0], d_b_col=r["dp"][1])
    ey, eyd = cabi_jacobi(u16, du16, [t.float() for t in ph], r["dp"], nt)
    assert fy.dtype == F16 and torch.equal(fy, ey) and torch.equal(fyd, eyd)


def test_functions_refuse_a_call_without_tangents():
    import cnn_with_pde_amd.functional as F_
    r, j = run_ex(3), run_jac(1)
    with pytest.raises(ValueError):
        F_.explicit5_tangent(r["u"], *r["p"], num_steps=2)
    with pytest.raises(ValueError):
        F_.jacobi_diffuse_tangent(j["u"], *j["p"], 3)


# ---- torch.autograd.forward_ad through the nodes ------------------------------------------------------------------------
def _dual(t, dt):
    return t if dt is None else fwad.make_dual(t, dt)


@pytest.mark.parametrize("i", range(len(EX_CASES)), ids=EX_IDS)
def test_forward_ad_through_explicit5_step(i):
    """Raises torch's NotImplementedError ("You must implement the jvp function") without the node's jvp."""
    import cnn_with_pde_amd.functional as F_
    r = run_ex(i)
    with fwad.dual_level():
        out = F_.explicit5_step(_dual(r["u"], r["du"]), *[_dual(t, dt) for t, dt in zip(r["p"], r["dp"])], dt=DT, eps=EPS,
                                max_coeff=MAXC, relax=RELAX, num_steps=r["K"])
        y, yd = fwad.unpack_dual(out)
        assert yd is not None
        y, yd = y.detach().clone(), yd.detach().clone()
    errs = {"y": rel(y, r["y_ref"]), "ydot": rel(yd, r["yd_ref"])}
    print(EX_IDS[i], errs, "o32", r["o32"])
    assert max(errs.values()) <= gate(r["dtype"], r["o32"]), (errs, "o32", r["o32"])
    assert torch.equal(y, r["y"]) and torch.equal(yd, r["yd"])      # the C call's tensors (du alone: the forward at du, its bits)


@pytest.mark.parametrize("i", range(len(JAC_CASES)), ids=JAC_IDS)
def test_forward_ad_through_jacobi_diffuse(i):
    import cnn_with_pde_amd.functional as F_
    r = run_jac(i)
    with fwad.dual_level():
        out = F_.jacobi_diffuse(_dual(r["u"], r["du"]), *[_dual(t, dt) for t, dt in zip(r["p"], r["dp"])], r["nt"])
        y, yd = fwad.unpack_dual(out)
        assert yd is not None
        y, yd = y.detach().clone(), yd.detach().clone()
    errs = {"y": rel(y, r["y_ref"]), "ydot": rel(yd, r["yd_ref"])}
    print(JAC_IDS[i], errs, "o32", r["o32"])
    assert max(errs.values()) <= gate(r["dtype"], r["o32"]), (errs, "o32", r["o32"])
    assert torch.equal(y, r["y"]) and torch.equal(yd, r["yd"])


# ---- layers.explicit_layer_jvp ---------------------------------------------------------------------------------------------
def _improved(size, channels, num_steps):
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(size + channels)
    ly = quiet(P.ImprovedDiffusionLayer, size, channels, num_steps=num_steps)
    with torch.no_grad():
        ly.alpha_base.copy_(make_alpha(channels, 0, g))
        ly.channel_scaling.copy_(1.0 + 0.3 * torch.randn(channels, generator=g))
    cfg = (f32(ly.dt), f32(ly.stability_eps), f32(ly.max_coeff), f32(ly._relax))
    fn = lambda a, p: O.tiny_forward(a, p, cfg[0], num_steps, cfg[1], cfg[2], cfg[3])
    return ly, fn, (3, channels, size, size)


def _pde_layer(Nx, Ny, scalars):
    import cnn_with_pde_amd as P
    ly = quiet(P.PDELayer, Nx=Nx, Ny=Ny)
    with torch.no_grad():
        for n, v in scalars.items():
            getattr(ly, n).fill_(v)

    def fn(a, p):
        A, Bc = O.emotion_coefficients(p, Nx, Ny, ly.Lx, ly.Ly, ly.dt, a.dtype)
        return O.jacobi_forward(a.squeeze(1), A, Bc, ly.Nt).unsqueeze(1)
    return ly, fn, (2, 1, Ny, Nx)


#: coefficients of the 70 x 66 plane kept inside the explicit scheme's stability bound (a_i + b_j < 1/2)
SMALL = dict(alpha_w1=0.03, alpha_w2=0.01, alpha_w3=0.01, beta_w1=0.03, beta_w2=0.01, beta_w3=0.01)
LAYERS = {"improved16c3k2": lambda: _improved(16, 3, 2), "improved10c2": lambda: _improved(10, 2, 1),
          "pde16": lambda: _pde_layer(16, 16, {}), "pde70x66": lambda: _pde_layer(70, 66, SMALL)}


@pytest.mark.parametrize("name", list(LAYERS))
def test_explicit_layer_jvp_against_the_oracle(name):
    """Every named parameter perturbed in turn, then all of them with du.  Raises torch's NotImplementedError without the
    nodes' jvp."""
    import cnn_with_pde_amd as P
    ly, fn, shape = LAYERS[name]()
    g = torch.Generator().manual_seed(len(name))
    params = {n: p.detach().clone().double() for n, p in ly.named_parameters()}
    q = lambda t: t.float().double()
    u, du = q(torch.randn(shape, generator=g, dtype=F64)), q(torch.randn(shape, generator=g, dtype=F64))
    dparams = {n: q(0.1 * torch.randn(p.shape, generator=g, dtype=F64)) for n, p in params.items()}
    ly = ly.cuda()
    with torch.no_grad():
        y_plain = ly(u.float().cuda())
    for use_du, names in [(False, (n,)) for n in params] + [(True, tuple(params))]:
        dp = {n: dparams[n] for n in names}
        y, yd = P.explicit_layer_jvp(ly, u.float().cuda(), du.float().cuda() if use_du else None,
                                     {n: t.float().cuda() for n, t in dp.items()})
        assert y.dtype == F32 and y.shape == shape and torch.equal(y, y_plain)
        if names == ("beta_base",):                        # the layer does not use it: exactly zero
            assert int(torch.count_nonzero(yd)) == 0
            continue
        y_ref, yd_ref = oracle_jvp(fn, u, du if use_du else None, params, dp)
        o32 = rel(oracle_jvp(fn, u, du if use_du else None, params, dp, F32)[1], yd_ref)
        tol = gate(F32, o32)
        errs = {"y": rel(y, y_ref), "ydot": rel(yd, yd_ref)}
        print(name, names, errs, "o32", o32)
        assert float(yd_ref.abs().max()) > 0 and max(errs.values()) <= tol, (names, errs, "o32", o32)


def test_explicit_layer_jvp_refusals():
    import cnn_with_pde_amd as P
    il = quiet(P.ImprovedDiffusionLayer, 16, 2).cuda()
    u = torch.zeros(1, 2, 16, 16).cuda()
    with pytest.raises(KeyError):
        P.explicit_layer_jvp(il, u, None, {"no_such_parameter": torch.zeros(2).cuda()})
    with pytest.raises(ValueError):
        P.explicit_layer_jvp(il, u, None, {"alpha_base": torch.zeros(3).cuda()})
    with pytest.raises(ValueError):
        P.explicit_layer_jvp(il, u, torch.zeros(1, 2, 16, 8).cuda())
    with pytest.raises(TypeError):
        P.explicit_layer_jvp(quiet(P.MnistDiffusionLayer, 9, 0.4, 1.0, 1.3, 2), torch.zeros(1, 1, 9, 9).cuda())
    with pytest.raises(TypeError):
        P.explicit_layer_jvp(torch.nn.Linear(2, 2), torch.zeros(1, 2))


def test_gradcheck_with_forward_ad():
    import cnn_with_pde_amd.functional as F_
    g = torch.Generator().manual_seed(23)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    # away from the clamp's kinks: one channel clamped from below, one from above, one inside
    ins = [t.cuda().requires_grad_(True) for t in (mk(2, 3, 4, 5), torch.tensor([-0.05, 0.3, 0.07], dtype=F64), 1.0 + 0.3 * mk(3))]
    fn = lambda a, ab, s: F_.explicit5_step(a, ab, s, dt=0.5, eps=1e-6, max_coeff=0.15, relax=0.625, num_steps=2)
    assert torch.autograd.gradcheck(fn, ins, eps=1e-6, atol=1e-6, rtol=1e-5, check_forward_ad=True, check_backward_ad=True,
                                    check_undefined_grad=False, check_batched_grad=False)
    ins = [t.cuda().requires_grad_(True) for t in (mk(2, 4, 4), 0.05 + 0.15 * torch.rand(4, generator=g, dtype=F64),
                                                   0.05 + 0.15 * torch.rand(4, generator=g, dtype=F64))]
    fn = lambda a, ar, bc: F_.jacobi_diffuse(a, ar, bc, 3)
    assert torch.autograd.gradcheck(fn, ins, eps=1e-6, atol=1e-6, rtol=1e-5, check_forward_ad=True, check_backward_ad=True,
                                    check_undefined_grad=False, check_batched_grad=False)


def test_trajectory_under_a_dual_level_is_refused():
    import cnn_with_pde_amd.functional as F_
    r, j = run_ex(4), run_jac(1)
    with fwad.dual_level():
        u = fwad.make_dual(r["u"], torch.ones_like(r["u"]))
        with pytest.raises(NotImplementedError, match="trajectory"):
            F_.explicit5_states(u, *r["p"], dt=DT, eps=EPS, max_coeff=MAXC, relax=RELAX, steps=(1, 3))
        a = fwad.make_dual(j["p"][0], torch.ones_like(j["p"][0]))
        with pytest.raises(NotImplementedError, match="trajectory"):
            F_.jacobi_diffuse_states(j["u"], a, j["p"][1], (1, 3))


# ---- nothing else moves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["explicit_wave", "explicit_generic", "jacobi", "jacobi_tiled"])
def test_no_tangent_no_change(kind):
    """Inside a dual level without a tangent the routes, the results and what the frozen node keeps are those outside."""
    import cnn_with_pde_amd.functional as F_
    g = torch.Generator().manual_seed(3)
    if kind.startswith("explicit"):
        shape = (2, 3, 16, 16) if kind == "explicit_wave" else (2, 3, 5, 7)
        p = [(0.02 + 0.1 * torch.rand(3, generator=g)).cuda(), (1 + 0.1 * torch.randn(3, generator=g)).cuda()]
        call = lambda a: F_.explicit5_step(a, *p, num_steps=2)
        kept_shapes = [(3,), (3,)]
    else:
        shape = (2, 9, 12) if kind == "jacobi" else (1, 66, 70)
        p = [(0.05 + 0.15 * torch.rand(shape[1], generator=g)).cuda(), (0.05 + 0.15 * torch.rand(shape[2], generator=g)).cuda()]
        call = lambda a: F_.jacobi_diffuse(a, *p, 12)
        kept_shapes = [(shape[1],), (shape[2],)]
    u = torch.randn(shape, generator=g).cuda().requires_grad_(True)
    y0 = call(u)
    with fwad.dual_level():
        y1 = call(u)
        assert fwad.unpack_dual(y1).tangent is None
    assert torch.equal(y0, y1) and type(y0.grad_fn) is type(y1.grad_fn)
    for y in (y0, y1):                                   # the frozen route: the two parameter vectors alone
        kept = [t for t in y.grad_fn.saved_tensors if t is not None]
        assert [tuple(t.shape) for t in kept] == kept_shapes
    gy = torch.randn(shape, generator=g).cuda()
    (g0,), (g1,) = torch.autograd.grad(y0, u, gy), torch.autograd.grad(y1, u, gy)
    assert torch.equal(g0, g1)


# ---- graph capture --------------------------------------------------------------------------------------------------------
def _capture(call, statics):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                            # warm-up: the per-kernel LDS attribute is set outside capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gy, gyd = call()
    for t in statics:
        t.copy_(torch.randn_like(t))
    graph.replay()
    torch.cuda.synchronize()
    ey, eyd = call()
    assert torch.equal(gy, ey) and torch.equal(gyd, eyd)


def test_graph_capture_of_the_wave_call():
    import cnn_with_pde_amd.functional as F_
    r = run_ex(1)
    su, sdu = r["u"].clone(), torch.randn_like(r["u"])
    da, ds = torch.randn_like(r["p"][0]), torch.randn_like(r["p"][1])
    _capture(lambda: F_.explicit5_tangent(su, *r["p"], du=sdu, d_alpha_base=da, d_channel_scaling=ds, dt=DT, eps=EPS,
                                          max_coeff=MAXC, relax=RELAX, num_steps=r["K"]), (su, sdu))


def test_graph_capture_of_the_chained_tiled_launches():
    import cnn_with_pde_amd.functional as F_
    r = run_jac(6)                                        # 130 x 67, nt = 11: two launches through the workspace images
    su, sdu = r["u"].clone(), torch.randn_like(r["u"])
    da, db = 0.1 * torch.randn_like(r["p"][0]), 0.1 * torch.randn_like(r["p"][1])
    _capture(lambda: F_.jacobi_diffuse_tangent(su, *r["p"], r["nt"], du=sdu, d_a_row=da, d_b_col=db), (su, sdu))
