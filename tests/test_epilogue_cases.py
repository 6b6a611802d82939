"""The ground tests/test_gpu_epilogues.py stands on, checked without a GPU: the hand-written fp64 references of the skip
blend and of the gate combination against torch autograd; that every "exact" case is exact (inputs, intermediates and
results representable in its I/O type, sums independent of their order); that the BatchNorm + pooling inputs hold exact
ties and no near-ties, and that torch's fp64 CPU modules resolve a tie as the kernel does; that the 1-ulp criterion of the
general 16-bit cases is within reach of fp32 arithmetic on their inputs; and the refusals of the three C-ABI families that
return before any launch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import epilogue_util as E

IO16_32 = ("f32", "bf16", "f16")


def _fits(x, dtype):
    """every element of the fp64 / int64 tensor is a value of ``dtype``"""
    x = x.double()
    return bool(torch.equal(x.to(dtype).double(), x))


def _sum_f32_two_orders(terms):
    """Sequential fp32 sums of the terms along the last axis, first to last and last to first."""
    t = np.ascontiguousarray(terms.double().numpy().astype(np.float32))
    fwd = np.add.accumulate(t, axis=-1, dtype=np.float32)[..., -1]
    bwd = np.add.accumulate(t[..., ::-1], axis=-1, dtype=np.float32)[..., -1]
    return torch.from_numpy(fwd.astype(np.float64)), torch.from_numpy(bwd.astype(np.float64))


# --------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("w", [-4.0, 0.0, 0.9, 6.0])
def test_blend_reference_vs_autograd(w):
    gen = torch.Generator().manual_seed(1)
    u0, u, g = (torch.randn(1001, generator=gen, dtype=torch.float64) for _ in range(3))
    a, b, ww = u0.clone().requires_grad_(True), u.clone().requires_grad_(True), torch.tensor(w, dtype=torch.float64, requires_grad=True)
    s = torch.sigmoid(ww)
    out = s * a + (1 - s) * b
    out.backward(g)
    ref = E.blend_ref(u0, u, w, g)
    for got, want in ((ref["out"], out.detach()), (ref["g_u0"], a.grad), (ref["g_u"], b.grad),
                      (torch.tensor(ref["g_w"], dtype=torch.float64), ww.grad)):
        assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("L,gate4d", [(1, False), (3, True), (4, False)])
def test_gate_reference_vs_autograd(L, gate4d):
    gen = torch.Generator().manual_seed(2)
    B, Cc, H, W = 3, 5, 6, 10
    ys = [torch.randn(B, Cc, H, W, generator=gen, dtype=torch.float64) for _ in range(L)]
    gates = [torch.randn(B, Cc, generator=gen, dtype=torch.float64) for _ in range(L)]
    w = torch.randn(L, generator=gen, dtype=torch.float64)
    g = torch.randn(B, Cc, H, W, generator=gen, dtype=torch.float64)
    yr = [y.clone().requires_grad_(True) for y in ys]
    gr = [(t.view(B, Cc, 1, 1) if gate4d else t).clone().requires_grad_(True) for t in gates]
    wr = w.clone().requires_grad_(True)
    out = sum(wr[i] * gr[i].view(B, Cc, 1, 1) * yr[i] for i in range(L))
    out.backward(g)
    ref = E.gate_ref(ys, gr, w, g)
    pairs = [(ref["out"], out.detach()), (ref["gw"], wr.grad)]
    pairs += [(ref["gy"][i], yr[i].grad) for i in range(L)] + [(ref["ggate"][i], gr[i].grad.view(B, Cc)) for i in range(L)]
    for got, want in pairs:
        got = got.detach()
        assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))


# --------------------------------------------------------------------------------------------------- exact cases are exact
@pytest.mark.parametrize("n", sorted(set(E.BLEND_SIZES + E.BLEND64_SIZES)))
def test_blend_exact_cases_are_exact(n):
    c = E.blend_exact_case(n)
    assert 1.0 / (1.0 + math.exp(-0.0)) == 0.5 and float(np.float32(1) / (np.float32(1) + np.exp(np.float32(-0.0)))) == 0.5
    for v in (c["u0"], c["u"], c["g"]):
        assert int(v.abs().max()) <= 32
    if n >= E.BLEND_SMALL_RANGE_FROM:
        assert int(c["g"].abs().max()) <= 3 and int((c["u0"] - c["u"]).abs().max()) <= 3
    # inputs, the two products of the forward, the outputs and the gradients: values of every I/O type
    tensors = (c["u0"], c["u"], c["g"], 0.5 * c["u0"].double(), 0.5 * c["u"].double(), c["out"], c["g_u0"], c["g_u"])
    for name in IO16_32:
        assert all(_fits(t, E.DTYPES[name]) for t in tensors), name
    assert torch.equal(c["out"], E.blend_ref(c["u0"], c["u"], 0.0, c["g"])["out"])
    # the sum behind the weight's gradient: int64 = fp32 in two orders; a quarter of it is an fp32 value, finite in fp16
    fwd, bwd = _sum_f32_two_orders(c["g"] * (c["u0"] - c["u"]))
    assert float(fwd) == float(bwd) == float(c["sum"])
    assert abs(c["sum"]) < 2 ** 24 and float(np.float32(c["g_w"])) == c["g_w"] == E.blend_ref(c["u0"], c["u"], 0.0, c["g"])["g_w"]
    if n in E.BLEND_SIZES:
        assert math.isfinite(float(torch.tensor(c["g_w"]).to(torch.float16)))


@pytest.mark.parametrize("L,hw,bc,gate4d", E.gate_exact_cases(), ids=E.gate_case_id)
def test_gate_exact_cases_are_exact(L, hw, bc, gate4d):
    c = E.gate_exact_case(L, hw, bc)
    ref, w = c["ref"], c["w"]
    assert max(int(y.abs().max()) for y in c["ys"]) <= 3 and int(c["g"].abs().max()) <= 3
    assert max(int(t.abs().max()) for t in c["gates"]) <= 2 and bc[0] * bc[1] <= 67
    assert float(ref["out"].abs().max()) <= 48
    f = [w[i] * c["gates"][i].double() for i in range(L)]
    for name in IO16_32:
        dt = E.DTYPES[name]
        assert all(_fits(t, dt) for t in (*c["ys"], c["g"], *c["gates"], w, *f, ref["out"], *ref["gy"])), name
    # every partial sum of the forward, in the kernel's order of the inputs and in the opposite one, is a multiple of 1/2
    # below 64: fp32 holds it whatever the order
    terms = torch.stack([f[i][:, :, None, None] * c["ys"][i].double() for i in range(L)], dim=-1)
    fwd, bwd = _sum_f32_two_orders(terms)
    assert torch.equal(fwd, ref["out"]) and torch.equal(bwd, ref["out"])
    for i in range(L):
        B, Cc = bc
        prod = (c["g"] * c["ys"][i]).reshape(B, Cc, -1)
        dot = prod.sum(-1)                                                          # int64
        fwd, bwd = _sum_f32_two_orders(prod)
        assert torch.equal(fwd, dot.double()) and torch.equal(bwd, dot.double())
        assert int(prod.abs().sum(-1).max()) < 2 ** 24
        assert torch.equal(ref["ggate"][i], w[i] * dot.double()) and _fits(ref["ggate"][i], torch.float32)
        gw_terms = (c["gates"][i] * dot).reshape(-1)
        fwd, bwd = _sum_f32_two_orders(gw_terms)
        assert float(fwd) == float(bwd) == float(gw_terms.sum()) == float(ref["gw"][i])
        assert int(gw_terms.abs().sum()) < 2 ** 24
        # the float16 route returns these two in fp16: rounded once from the exact value, never to infinity
        assert bool(torch.isfinite(ref["ggate"][i].to(torch.float16)).all())
    assert bool(torch.isfinite(ref["gw"].to(torch.float16)).all())


def test_gate_exact_cases_cover_every_factor():
    cases = E.gate_exact_cases()
    assert {c[0] for c in cases} == {1, 2, 3, 4}
    assert {c[1] for c in cases} == set(E.GATE_PLANES)
    assert {c[2][0] * c[2][1] for c in cases} == {1, 3, 4, 5, 67} and {c[2] for c in cases} == set(E.GATE_BC)
    assert {c[1][0] * c[1][1] for c in cases if c[0] == 4} >= {4, 260, 4096}
    assert {c[3] for c in cases} == {False, True}


# --------------------------------------------------------------------------------------------------- BatchNorm + pooling
def _tail_cases():
    return [(B, Cc, N, None) for B, Cc, N in E.TAIL_SHAPES] + [(*shape, v) for v, shape in E.TAIL_VARIANTS.items()]


@pytest.mark.parametrize("B,Cc,N,variant", _tail_cases())
def test_tail_inputs_tie_exactly_or_differ_by_2_to_minus_6(B, Cc, N, variant):
    c = E.tail_case(B, Cc, N, variant)
    win = N // 4
    assert _fits(c.x, torch.float32) and _fits(c.gout, torch.float32) and _fits(c.weight, torch.float32)
    assert _fits(c.bias, torch.float32) and _fits(c.running_mean, torch.float32) and _fits(c.running_var, torch.float32)
    assert bool((c.gout != 0).all()) and _fits(4 * c.gout, torch.int16)
    windows = c.x.unfold(2, win, win).unfold(3, win, win).reshape(B, Cc, 16, win * win)
    d = windows.sort(dim=-1).values.diff(dim=-1)
    assert bool(((d == 0) | (d >= 2.0 ** -6)).all())
    if win > 1:
        assert bool((d == 0).any()), "no tie in any window"
    if Cc >= 3:
        assert float(c.weight.min()) < 0 and bool((c.weight == 0).any())


def test_fp64_cpu_max_pool_takes_the_first_maximum():
    z = torch.zeros(1, 1, 8, 8, dtype=torch.float64)
    z[0, 0, 1, 1] = z[0, 0, 0, 1] = z[0, 0, 1, 0] = 2.0              # window (0,0): maxima at 1, 8, 9 -> 1
    z[0, 0, 3, 7] = z[0, 0, 2, 7] = 5.0                              # window (1,3): 23, 31 -> 23
    _, idx = nn.functional.adaptive_max_pool2d(z, 4, return_indices=True)
    assert int(idx[0, 0, 0, 0]) == 1 and int(idx[0, 0, 1, 3]) == 23
    assert int(idx[0, 0, 3, 3]) == 6 * 8 + 6                         # an all-equal window: its first element


@pytest.mark.parametrize("B,Cc,N,variant", _tail_cases())
@pytest.mark.parametrize("training", [True, False])
def test_tail_reference_resolves_ties_by_position(B, Cc, N, variant, training):
    """Through the fp64 BatchNorm equal inputs stay equal, so the reference's arg-max is the first maximum (weight > 0),
    the first minimum (weight < 0) or the first element (weight 0) of x in every window."""
    c = E.tail_case(B, Cc, N, variant)
    win = N // 4
    bn = c.module(torch.float64, "cpu", training)
    with torch.no_grad():
        _, idx = nn.functional.adaptive_max_pool2d(bn(c.x), 4, return_indices=True)
    wgt = c.weight if c.affine else torch.ones(Cc, dtype=torch.float64)
    key = c.x * torch.sign(wgt).view(1, Cc, 1, 1)
    pos = torch.arange(N * N).view(1, 1, N, N).expand(B, Cc, N, N)
    kw = key.unfold(2, win, win).unfold(3, win, win).reshape(B, Cc, 4, 4, win * win)
    pw = pos.unfold(2, win, win).unfold(3, win, win).reshape(B, Cc, 4, 4, win * win)
    is_max = kw == kw.max(dim=-1, keepdim=True).values
    first = torch.where(is_max, pw, torch.full_like(pw, N * N)).min(dim=-1).values
    assert torch.equal(idx, first)


# --------------------------------------------------------------------------------------------------- the 1-ulp criterion
def _f32_eval(terms):
    """sum of fp32 products: each product and each partial sum rounded to fp32, and the products kept exact (fused)"""
    plain = torch.zeros_like(terms[0][1], dtype=torch.float32)
    fused = torch.zeros_like(plain)
    for f, v in terms:
        plain = plain + f.float() * v.float()
        fused = (f.float().double() * v.float().double() + fused.double()).float()
    return plain, fused


@pytest.mark.parametrize("name", ["bf16", "f16"])
@pytest.mark.parametrize("w", [-4.0, 0.9, 6.0])
def test_blend_general_inputs_allow_one_ulp(w, name):
    """fp32 arithmetic rounded once to the 16-bit type is within 1 ulp of the rounded fp64 result on the inputs of the
    general blend case (a result that cancels to far below its terms would not be)."""
    dt = E.DTYPES[name]
    u0, u, g = (x.to(dt) for x in E.blend_general_case(21501))
    wv = torch.tensor(w).to(dt if name == "f16" else torch.float32)
    ref = E.blend_ref(u0, u, wv, g)
    s = torch.tensor(1.0 / (1.0 + math.exp(-float(wv))), dtype=torch.float32)
    t = torch.tensor(1.0 / (1.0 + math.exp(float(wv))), dtype=torch.float32)
    for ev in _f32_eval([(s, u0), (t, u)]):
        assert E.ulps16(ev.to(dt), ref["out"].to(dt)) <= 1
    assert E.ulps16((s.float() * g.float()).to(dt), ref["g_u0"].to(dt)) <= 1
    assert E.ulps16((t.float() * g.float()).to(dt), ref["g_u"].to(dt)) <= 1


@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_gate_general_inputs_allow_one_ulp(name):
    dt = E.DTYPES[name]
    pdt = dt if name == "f16" else torch.float32
    ys, gates, w, g = E.gate_general_case()
    ys, g, gates, w = [y.to(dt) for y in ys], g.to(dt), [t.to(pdt) for t in gates], w.to(pdt)
    ref = E.gate_ref(ys, gates, w, g)
    f = [(w[i].float() * gates[i].float())[:, :, None, None] for i in range(len(ys))]
    for ev in _f32_eval(list(zip(f, ys))):
        assert E.ulps16(ev.to(dt), ref["out"].to(dt)) <= 1
    for i in range(len(ys)):
        assert E.ulps16((f[i] * g.float()).to(dt), ref["gy"][i].to(dt)) <= 1


# --------------------------------------------------------------------------------------------------- refusals before a launch
# Every call below fails a check that its entry point makes before its first launch; the pointers are never dereferenced.
_P = C.c_void_p(4096)


def _lib():
    from cnn_with_pde_amd import _lib as L
    return L, L.load()


def test_blend_refusals():
    L, lib = _lib()
    assert lib.pde_skip_blend_forward(0, L.PDE_IO_F32, _P, _P, _P, _P, None) == -1
    assert lib.pde_skip_blend_backward(0, L.PDE_IO_F32, _P, _P, _P, _P, _P, _P, _P, _P, 1 << 20, None) == -1
    assert lib.pde_skip_blend_backward_workspace_bytes(0) == 0
    for io in (L.PDE_IO_F64, 4, -1):                                     # float64 has its own entry points
        assert lib.pde_skip_blend_forward(16, io, _P, _P, _P, _P, None) == -1
        assert lib.pde_skip_blend_backward(16, io, _P, _P, _P, _P, _P, _P, _P, _P, 1 << 20, None) == -1
    need = lib.pde_skip_blend_backward_workspace_bytes(5000)
    assert need == 3 * 8
    assert lib.pde_skip_blend_backward(5000, L.PDE_IO_F32, _P, _P, _P, _P, _P, _P, _P, _P, need - 1, None) == -5
    assert lib.pde_skip_blend_f64_forward(0, _P, _P, _P, _P, None) == -1
    assert lib.pde_skip_blend_f64_backward(0, _P, _P, _P, _P, _P, _P, _P, _P, 1 << 20, None) == -1
    need = lib.pde_skip_blend_f64_backward_workspace_bytes(257)
    assert need >= 2 * 8
    assert lib.pde_skip_blend_f64_backward(257, _P, _P, _P, _P, _P, _P, _P, _P, need - 1, None) == -5


@pytest.mark.parametrize("L_,B,Cc,HW", [(0, 2, 3, 16), (5, 2, 3, 16), (2, 2, 3, 6), (2, 0, 3, 16)])
def test_gate_refusals(L_, B, Cc, HW):
    L, lib = _lib()
    arr = (C.c_void_p * 5)(*([4096] * 5))
    for io in (L.PDE_IO_F32, L.PDE_IO_BF16, L.PDE_IO_F16):
        assert lib.pde_gate_combine_forward(L_, B, Cc, HW, io, arr, arr, _P, _P, None) == -1
        assert lib.pde_gate_combine_backward(L_, B, Cc, HW, io, _P, arr, arr, _P, arr, arr, None) == -1


def test_bn_pool_refusals():
    L, lib = _lib()
    big = 1 << 20

    def fwd(B, Cc, N, training=1, rm=_P, rv=_P, ws=big):
        return lib.pde_bn_pool_forward(B, Cc, N, _P, _P, _P, 1e-5, training, 0.1, rm, rv, _P, _P, _P, _P, _P, ws, None)

    def bwd(B, Cc, N, ws=big):
        return lib.pde_bn_pool_backward(B, Cc, N, _P, _P, _P, _P, _P, _P, 1, _P, _P, _P, _P, ws, None)

    for N in (2, 30, 68):
        assert fwd(2, 3, N) == -1 and bwd(2, 3, N) == -1
    assert fwd(0, 3, 8) == -1 and bwd(0, 3, 8) == -1
    assert fwd(2, 3, 8, training=0, rm=None) == -1 and fwd(2, 3, 8, training=0, rv=None) == -1
    need = lib.pde_bn_pool_workspace_bytes(2, 3)
    assert need == 2 * 3 * 2 * 4 and lib.pde_bn_pool_workspace_bytes(0, 3) == 0
    assert fwd(2, 3, 8, ws=need - 1) == -5 and bwd(2, 3, 8, ws=need - 1) == -5
    assert fwd(2, 3, 8, training=0, ws=need - 1) == -5
