"""The epilogue kernels against fp64 at their edges, through the public wrappers (functional.skip_blend, gate_combine,
bn_pool) and so through the C ABI: the SVHN skip blend (pde_blend.hip, blend64_* of pde_f64.hip), the attention gates with
the weighted combination (pde_gate.hip), BatchNorm2d with the 4x4 average and max pooling (pde_tail.hip).

Exact cases (tests/epilogue_util.py; proved exact on the CPU by tests/test_epilogue_cases.py) are compared with
``torch.equal``.  General cases keep the bounds of the older tests of these kernels (test_gpu_parity.py, test_gpu_models.py,
test_gpu_tail.py); 16-bit tensors must be within 1 ulp of the fp64 result rounded to their type.  A gradient that autograd
hands back in fp16 (the float16 route needs fp16 parameters) is held to the same bound before that last rounding: it must
lie between the rounded ends of the allowed interval.  Every tensor is its own contiguous allocation."""
import pytest
import torch

import epilogue_util as E
import golden_util as G
from test_gpu_f16 import max_ulps

pytestmark = pytest.mark.gpu

IO3 = ("f32", "bf16", "f16")


def _ulps(a, b):
    return max_ulps(a, b) if a.dtype == torch.float16 else E.ulps16(a, b)


def _dev(t, dtype, grad=False):
    """a fresh contiguous device tensor of the values of ``t``"""
    d = t.to(dtype).contiguous().cuda()
    return d.requires_grad_(True) if grad else d


def _within_after_rounding(got, ref, tol):
    """``got`` (fp16 or bf16) is the rounding of some value within ``tol`` of the fp64 ``ref``: rounding is monotone, so it
    lies between the roundings of ref - tol and ref + tol."""
    ref = ref.double().cpu().reshape(got.shape)
    lo, hi = (ref - tol).to(got.dtype).double(), (ref + tol).to(got.dtype).double()
    g = got.detach().double().cpu()
    return bool(((lo <= g) & (g <= hi)).all())


def _param_dtype(name):
    """weights and gates: fp32, except on the float16 route, which a call takes only with every parameter in fp16"""
    return {"f16": torch.float16, "f64": torch.float64}.get(name, torch.float32)


# --------------------------------------------------------------------------------------------------- skip blend
def _run_blend(u0, u, g, w):
    from cnn_with_pde_amd import functional as F_
    out = F_.skip_blend(u0, u, w)
    out.backward(g)
    return out.detach()


def _blend_exact(n, name):
    dt, wdt = E.DTYPES[name], _param_dtype(name)
    c = E.blend_exact_case(n)
    u0, u, g = _dev(c["u0"], dt, True), _dev(c["u"], dt, True), _dev(c["g"], dt)
    w = torch.zeros((), dtype=wdt, device="cuda", requires_grad=True)          # s = 1/2 exactly
    out = _run_blend(u0, u, g, w)
    assert out.dtype == dt and u0.grad.dtype == dt and u.grad.dtype == dt and w.grad.dtype == wdt
    assert torch.equal(out, _dev(c["out"], dt)), "out"
    assert torch.equal(u0.grad, _dev(c["g_u0"], dt)), "g_u0"
    assert torch.equal(u.grad, _dev(c["g_u"], dt)), "g_u"
    want = torch.tensor(c["g_w"], dtype=torch.float64).to(torch.float64 if name == "f64" else torch.float32).to(wdt)
    assert float(w.grad) == float(want), (float(w.grad), float(want))


@pytest.mark.parametrize("name", IO3)
@pytest.mark.parametrize("n", E.BLEND_SIZES)
def test_blend_exact(n, name):
    """Integers at skip_weight = 0: every element, tail and trip of the grid-stride loop, tolerance 0."""
    _blend_exact(n, name)


@pytest.mark.parametrize("n", E.BLEND64_SIZES)
def test_blend64_exact(n):
    _blend_exact(n, "f64")


def _blend_general(u0, u, g, wval, name):
    dt, wdt = E.DTYPES[name], _param_dtype(name)
    u0, u, g = u0.to(dt), u.to(dt), g.to(dt)
    wv = torch.tensor(wval, dtype=torch.float64).to(wdt)
    ref = E.blend_ref(u0, u, wv, g)
    a, b, w = _dev(u0, dt, True), _dev(u, dt, True), _dev(wv, wdt, True)
    out = _run_blend(a, b, _dev(g, dt), w)
    assert out.dtype == dt and w.grad.dtype == wdt
    got = {"out": out.cpu(), "g_u0": a.grad.cpu(), "g_u": b.grad.cpu()}
    tol_w = 2e-5 * max(1.0, abs(ref["g_w"]))
    if name in ("bf16", "f16"):
        for k, v in got.items():
            ulps = _ulps(v, ref[k].to(dt))
            print(f"blend {name} w={wval} n={u0.numel()} {k}: {ulps} ulp")
            assert ulps <= 1, k
    else:
        # fp64: s, 1 - s and each product within a few roundings of 1.1e-16; 1 - s formed by subtraction keeps the absolute
        # error of s, at skip_weight = 6 (1 - s = 2.5e-3) a relative 4.5e-14 per rounding: 1e-12 covers twenty of them
        tol = 1e-6 if name == "f32" else 1e-12
        for k, v in got.items():
            err = G.rel_err(v, ref[k])
            print(f"blend {name} w={wval} n={u0.numel()} {k}: {err:.3e}")
            assert err <= tol, k
        if name == "f64":
            tol_w = 1e-12 * max(1.0, float((g.double() * (u0.double() - u.double())).abs().sum()))
    print(f"blend {name} w={wval} n={u0.numel()} g_w: {float(w.grad)!r} vs {ref['g_w']!r}")
    if name == "f16":
        assert _within_after_rounding(w.grad, torch.tensor(ref["g_w"], dtype=torch.float64), tol_w)
    else:
        assert abs(float(w.grad) - ref["g_w"]) <= tol_w


@pytest.mark.parametrize("name", IO3 + ("f64",))
@pytest.mark.parametrize("wval", [-4.0, 0.9, 6.0])
def test_blend_general(wval, name):
    """A sigmoid near 0, the model's initial one and one near 1 (1 - s = 2.5e-3), at a ragged size."""
    _blend_general(*E.blend_general_case(21501), wval, name)


def test_blend_cancelling_sum():
    """u = u0 + 1e-3 noise: the weight's gradient is a sum of 2^20 differences of nearly equal numbers."""
    _blend_general(*E.blend_general_case((1 << 20) + 3, 1e-3), 0.9, "f32")


def test_blend_mixed_types_follow_u():
    """The contract of INTEGRATION.md for a call the layers never make (they route their input once, so u0 and u always
    share a type): with u in bf16 and u0 in fp32 the blend runs in bf16, u0 rounded first, and every gradient comes back
    in its own tensor's type."""
    from cnn_with_pde_amd import functional as F_
    u0, u, g = E.blend_general_case(2049)
    a, b = _dev(u0, torch.float32, True), _dev(u, torch.bfloat16, True)
    w = torch.tensor(0.9, device="cuda", requires_grad=True)
    out = F_.skip_blend(a, b, w)
    out.backward(_dev(g, torch.bfloat16))
    a2, b2 = _dev(u0, torch.bfloat16, True), _dev(u, torch.bfloat16, True)
    w2 = torch.tensor(0.9, device="cuda", requires_grad=True)
    out2 = F_.skip_blend(a2, b2, w2)
    out2.backward(_dev(g, torch.bfloat16))
    assert out.dtype == torch.bfloat16 and a.grad.dtype == torch.float32 and b.grad.dtype == torch.bfloat16
    assert torch.equal(out, out2) and torch.equal(a.grad, a2.grad.float()) and torch.equal(b.grad, b2.grad)
    assert float(w.grad) == float(w2.grad)


# --------------------------------------------------------------------------------------------------- gate and combination
def _run_gate(ys, gates, w, g):
    import cnn_with_pde_amd as P
    out = P.gate_combine(ys, gates, w)
    out.backward(g)
    return out.detach()


@pytest.mark.parametrize("name", IO3)
@pytest.mark.parametrize("L,hw,bc,gate4d", E.gate_exact_cases(), ids=E.gate_case_id)
def test_gate_exact(L, hw, bc, gate4d, name):
    """Integers, weights 1/2, 1, 2, -1: output, every gy_i, every gate gradient and the weight gradient, tolerance 0."""
    dt, pdt = E.DTYPES[name], _param_dtype(name)
    c = E.gate_exact_case(L, hw, bc)
    ref, (B, Cc) = c["ref"], bc
    gshape = (B, Cc, 1, 1) if gate4d else (B, Cc)
    ys = [_dev(y, dt, True) for y in c["ys"]]
    gates = [_dev(t.reshape(gshape), pdt, True) for t in c["gates"]]
    w = _dev(c["w"], pdt, True)
    out = _run_gate(ys, gates, w, _dev(c["g"], dt))
    assert out.dtype == dt and torch.equal(out, _dev(ref["out"], dt)), "out"
    for i in range(L):
        assert ys[i].grad.dtype == dt and torch.equal(ys[i].grad, _dev(ref["gy"][i], dt)), f"gy{i}"
        assert gates[i].grad.dtype == pdt and gates[i].grad.shape == gshape
        assert torch.equal(gates[i].grad, _dev(ref["ggate"][i].float().reshape(gshape), pdt)), f"ggate{i}"
    assert w.grad.dtype == pdt and torch.equal(w.grad, _dev(ref["gw"].float(), pdt)), "gw"


def test_gate_refusals_through_the_wrapper():
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(L.PdeError):
        P.gate_combine([z(2, 3, 5, 5)], [z(2, 3)], z(1))                       # HW = 25 is no multiple of 4
    with pytest.raises(L.PdeError):
        P.gate_combine([z(2, 3, 4, 4) for _ in range(5)], [z(2, 3) for _ in range(5)], z(5))


@pytest.mark.parametrize("name", IO3)
def test_gate_general(name):
    dt, pdt = E.DTYPES[name], _param_dtype(name)
    ys, gates, w, g = E.gate_general_case()
    ys, g, gates, w = [y.to(dt) for y in ys], g.to(dt), [t.to(pdt) for t in gates], w.to(pdt)
    ref = E.gate_ref(ys, gates, w, g)
    yd, gd, wd = [_dev(y, dt, True) for y in ys], [_dev(t, pdt, True) for t in gates], _dev(w, pdt, True)
    out = _run_gate(yd, gd, wd, _dev(g, dt))
    assert out.dtype == dt
    pairs = [("out", out.cpu(), ref["out"])] + [(f"gy{i}", yd[i].grad.cpu(), ref["gy"][i]) for i in range(len(ys))]
    for k, got, want in pairs:
        if name == "f32":
            err = G.rel_err(got, want)
            print(f"gate f32 {k}: {err:.3e}")
            assert err <= 1e-6, k
        else:
            ulps = _ulps(got, want.to(dt))
            print(f"gate {name} {k}: {ulps} ulp")
            assert ulps <= 1, k
    dots = [(f"ggate{i}", gd[i].grad, ref["ggate"][i]) for i in range(len(ys))] + [("gw", wd.grad, ref["gw"])]
    for k, got, want in dots:
        assert got.dtype == pdt
        if name == "f16":
            assert _within_after_rounding(got, want, 1e-5 * float(want.abs().max())), k
        else:
            err = G.rel_err(got.cpu(), want)
            print(f"gate {name} {k}: {err:.3e}")
            assert err <= 1e-5, k


# --------------------------------------------------------------------------------------------------- BatchNorm + pooling
_TAIL = [(*s, None, t) for s in E.TAIL_SHAPES for t in (True, False)] + \
        [(*s, v, t) for v, s in E.TAIL_VARIANTS.items() for t in (True, False)]


@pytest.mark.parametrize("B,Cc,N,variant,training", _TAIL)
def test_tail_vs_fp64(B, Cc, N, variant, training):
    """x = k/64 with exact ties in the windows, weights 1.25, -0.75, 0, 2, 0.5 per channel, against torch's modules in fp64.
    Bounds: those of test_gpu_tail.py, or twice the error of torch's own fp32 modules on the GPU on the same inputs
    against the same reference where that is larger (the +100 case: fp32 rounds beta - mean*scale to 1.5e-6 of max|z|)."""
    from cnn_with_pde_amd import functional as F_
    case = E.tail_case(B, Cc, N, variant)
    ref = E.tail_reference(B, Cc, N, variant, training)
    plain = E.tail_torch(case, training, torch.float32, "cuda")
    bn = case.module(torch.float32, "cuda", training)
    x = _dev(case.x, torch.float32, True)
    assert F_.bn_pool_supported(x, bn)
    got = E.tail_collect(bn, x, F_.bn_pool(x, bn), _dev(case.gout, torch.float32))
    tol = 2e-5 if (training or not case.track) else 1e-6               # batch statistics / running statistics
    base = {"out": tol, "dx": 5 * tol, "dweight": 5 * tol, "dbias": 5 * tol, "running_mean": 1e-5, "running_var": 1e-5}
    bad = []
    for k, b in base.items():
        if ref[k] is None:
            assert got[k] is None and plain[k] is None, k
            continue
        fused, pl = G.rel_err(got[k], ref[k]), G.rel_err(plain[k], ref[k])
        bound = max(b, 2 * pl)
        print(f"tail B={B} C={Cc} N={N} {variant or 'plain'} {'train' if training else 'eval'} {k}: "
              f"fused {fused:.3e} plain {pl:.3e} bound {bound:.3e}")
        if not fused <= bound:
            bad.append((k, fused, bound))
    assert not bad, bad
    assert got["num_batches_tracked"] == ref["num_batches_tracked"] == plain["num_batches_tracked"]
