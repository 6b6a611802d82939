"""The implicit diffusion layers on rectangular planes (H != W): the pde_adi_rect_* entry points — the any-size kernels of
csrc/pde_adi_gen.hip generalised from one N to (H, W) — through every layer class, against oracle.pde_oracle (whose
sweeps are shape-generic; tests/test_oracle_rect.py pins it on rectangles against dense solves).  Tolerances are those
of the square tests, taken by import: fp32 1e-5 (test_gpu_parity.TOL), bf16 2e-2 (test_gpu_anysize.test_bf16_tensors),
the fp16 windows of test_gpu_f16.py, float64 test_gpu_f64.TOL.

Two tests hold the SQUARE any-size path in place bit for bit: the rectangle entry points with H = W = N against the
square ones, and a fixture written on the GPU from the commit before the generalisation
(tests/golden/adi_gen_square_path/results.npz, tools/gen_adi_gen_square_golden.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import golden_util as G
import rect_util as R
import test_gpu_f16 as T16
from oracle import pde_oracle as O
from test_gpu_f64 import TOL as TOL64
from test_gpu_f64 import _check as _check64
from test_gpu_f64 import _perturb as _perturb64
from test_gpu_parity import TOL, _compare, _perturb, quiet

pytestmark = pytest.mark.gpu

#: both orientations, a fused line length on one side only (20, 28, 32), both sides of the LDS limits named in
#: test_gpu_anysize.test_longest_lines (82, 100, 128), the shortest side the library takes (2)
PLANES = [(5, 9), (9, 5), (3, 7), (20, 36), (28, 32), (32, 28), (48, 64), (2, 128), (128, 2), (100, 128), (128, 82)]
_ids = lambda hw: f"{hw[0]}x{hw[1]}"                                                        # noqa: E731


def _layer(kind, hw, Cc, g):
    """(layer, spec) of one layer family on the plane ``hw``; the oracle reads the plane from its input."""
    import cnn_with_pde_amd as P
    H = hw[0]
    if kind == "mnist":                  # one channel, smoothed coefficients, Strang, dx != dy
        ly, spec = quiet(P.MnistDiffusionLayer, hw, 0.01, 1.0, 1.3, 3), O.mnist_spec(H, 0.01, 1.0, 1.3, 3)
        _perturb(ly, g, 0.2, 0.4)
    elif kind == "cifar10":              # clamp to [eps, 10], channel mixing before every step
        ly, spec = quiet(P.EnhancedDiffusionLayer, hw, Cc, dt=0.02, num_steps=3), O.cifar10_spec(H, Cc, dt=0.02, num_steps=3)
        _perturb(ly, g, 0.2, 0.5)
        with torch.no_grad():
            ly.channel_mixing.copy_(torch.eye(Cc) + 0.1 * torch.randn(Cc, Cc, generator=g))
    elif kind == "fashion":              # the mnist layer with dy == dx at dt = 0.3: coefficients that need checkpoints
        ly, spec = P.FashionDiffusionLayer(hw, 0.3, 1.0, 2), O.fashion_spec(H, 0.3, 1.0, 2)
        _perturb(ly, g, 0.2, 0.3)
    elif kind == "cifar2":               # Lie split
        ly, spec = quiet(P.LearnableDiffusionLayer, hw, Cc, 0.03, 1.0, 1.2, 3), O.cifar2_spec(H, Cc, 0.03, 1.0, 1.2, 3)
        _perturb(ly, g, 0.2, 0.4)
    else:                                # SVHN: smoothed, coupling after every step, skip blend
        ly, spec = P.SvhnDiffusionLayer(hw, Cc, 0.05, 1.0, 2), O.svhn_spec(H, Cc, 0.05, 1.0, 2)
        _perturb(ly, g, 0.2, 0.3)
        with torch.no_grad():
            ly.channel_coupling.copy_(torch.eye(Cc) + 0.05 * torch.randn(Cc, Cc, generator=g))
            ly.skip_weight.fill_(0.2)
    return ly, spec


@pytest.mark.parametrize("hw", PLANES, ids=_ids)
def test_every_layer_class_vs_oracle(hw):
    """Forward, input gradient and every parameter gradient of every implicit layer class."""
    g = torch.Generator().manual_seed(1000 + 131 * hw[0] + hw[1])
    for kind, Cc, B in (("mnist", 1, 4), ("cifar10", 3, 3), ("cifar10", 5, 2), ("cifar2", 2, 3), ("svhn", 4, 2), ("fashion", 1, 3)):
        ly, spec = _layer(kind, hw, Cc, g)
        assert ly.size == hw and tuple(ly.alpha_base.shape[-2:]) == hw
        u, gy = torch.randn(B, Cc, *hw, generator=g), torch.randn(B, Cc, *hw, generator=g)
        want = {"g_alpha_base", "g_beta_base", "g_alpha_time_coeff", "g_beta_time_coeff"}
        if kind == "svhn":
            # Everything but the skip weight's gradient with the plain cotangent.  That gradient is ONE scalar,
            # s(1-s) sum gy (u0 - u_S): with gy independent of u the terms cancel like a random walk; on the 2 x 128 plane
            # (2048 terms) a draw left |sum| = 7e-4 sum|terms|, where the fp32 oracle itself is 3.8e-5 from the fp64 one —
            # the bound would test the draw, not the kernels.  So the skip weight is frozen for this pass (_compare checks
            # the gradients that exist) and checked in a second pass, below.
            ly.skip_weight.requires_grad_(False)
            errs = _compare(ly, lambda a, p: O.adi_forward(a, p, spec), u, gy)
            assert want | {"g_channel_coupling"} <= set(errs) and "g_skip_weight" not in errs, errs
            print(kind, Cc, hw, "plain cotangent", {k: f"{v:.2e}" for k, v in errs.items()})
            # u0 - u_S is the part of u0 the diffusion removed, and <u0, u0 - u_S> > 0 (a sum of squared differences to
            # first order): a cotangent with a component along u keeps the scalar's sum well conditioned whatever the draw
            ly = ly.cpu()                                  # _compare moved it to the device
            ly.skip_weight.requires_grad_(True)
            ly.zero_grad(set_to_none=True)
            gy = gy + 0.5 * u
            want = want | {"g_skip_weight"}
        errs = _compare(ly, lambda a, p: O.adi_forward(a, p, spec), u, gy)
        print(kind, Cc, hw, {k: f"{v:.2e}" for k, v in errs.items()})
        assert want <= set(errs), (kind, errs)


@pytest.mark.parametrize("hw", [(36, 20), (24, 40)], ids=_ids)
def test_clamp_masks_that_move_in_time(hw):
    """Coefficients that cross both clamp bounds during the schedule: the pass-through mask is per sweep."""
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(5)
    ly = quiet(P.EnhancedDiffusionLayer, hw, 2, dt=0.5, num_steps=3, channel_mixing_enabled=False)
    with torch.no_grad():
        ly.channel_mixing.copy_(torch.eye(2))
        ly.alpha_base.copy_(9.0 + 2.0 * torch.rand(2, *hw, generator=g))          # around clamp_max = 10
        ly.alpha_time_coeff.copy_(2.0 * torch.randn(2, *hw, generator=g))
        ly.beta_base.copy_(0.3 * torch.randn(2, *hw, generator=g))                 # around the floor
        ly.beta_time_coeff.copy_(torch.randn(2, *hw, generator=g))
    u, gy = torch.randn(6, 2, *hw, generator=g), torch.randn(6, 2, *hw, generator=g)
    _compare(ly, lambda a, p: O.adi_forward(a, p, O.cifar10_spec(hw[0], 2, dt=0.5, num_steps=3)), u, gy, tol=2e-5)


@pytest.mark.parametrize("policy", ["auto", "lagged"])
def test_checkpoint_modes_agree_and_match_oracle(policy):
    """Fashion-size coefficients (0.27 / 0.54): rebuilding the state backwards amplifies rounding, the checkpoint plan
    must hold 1e-5 — "auto" / "lagged" (the maxima through the pinned ring), all states, and a sparse mask (1e-3, as for
    squares)."""
    import cnn_with_pde_amd as P
    hw = (40, 28)
    g = torch.Generator().manual_seed(6)
    spec = O.mnist_spec(hw[0], 0.3, 1.0, 1.0, 4)
    u, gy = torch.randn(4, 1, *hw, generator=g), torch.randn(4, 1, *hw, generator=g)
    outs = {}
    for ck in (policy, (1 << 11) - 1, 0b010010010010):
        ly = quiet(P.MnistDiffusionLayer, hw, 0.3, 1.0, 1.0, 4)
        _perturb(ly, torch.Generator().manual_seed(8), 0.2, 0.3)
        ly.checkpoint_policy = ck
        outs[ck] = _compare(ly, lambda a, p: O.adi_forward(a, p, spec), u, gy, tol=TOL if ck != 0b010010010010 else 1e-3)
    assert outs[policy]["y"] == outs[(1 << 11) - 1]["y"]
    # the plan "auto" made is the one freeze_checkpoint_plan pins (same coefficients, the conservative budget)
    ly = quiet(P.MnistDiffusionLayer, hw, 0.3, 1.0, 1.0, 4).cuda()
    mask = ly.freeze_checkpoint_plan()
    assert isinstance(mask, int) and mask != 0 and ly.checkpoint_policy == mask


def test_kappa_max_on_a_rectangle():
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import functional as F_
    hw = (28, 44)
    g = torch.Generator().manual_seed(31)
    ly = quiet(P.MnistDiffusionLayer, hw, 0.05, 1.0, 1.5, 3)
    _perturb(ly, g, 0.3, 0.5)
    ly = ly.cuda()
    km = F_.kappa_max_async(torch.empty(1, 1, *hw, device="cuda"), ly.alpha_base, ly.beta_base, ly.alpha_time_coeff,
                            ly.beta_time_coeff, ly._schedule().flat, smooth3=True, clamp_max=None, eps=ly.stability_eps)
    km.event.synchronize()
    spec = O.mnist_spec(hw[0], 0.05, 1.0, 1.5, 3)
    want = []
    for axis, delta, t in O.sweep_schedule(spec):
        base, slope, h = ((ly.alpha_base, ly.alpha_time_coeff, spec.dx) if axis == 0 else (ly.beta_base, ly.beta_time_coeff, spec.dy))
        th = O.coefficient_at(base.detach().cpu(), slope.detach().cpu(), t, spec)
        th = O._smooth3(th if axis == 0 else th.t().contiguous())
        want.append(float((th * delta / h ** 2).max()))
    got = km.host.tolist()[:len(want)]
    assert max(abs(a - b) / b for a, b in zip(got, want)) < 1e-6, (got, want)


def test_bf16_tensors():
    import cnn_with_pde_amd as P
    hw = (48, 36)
    g = torch.Generator().manual_seed(21)
    ly = quiet(P.EnhancedDiffusionLayer, hw, 3, dt=0.02, num_steps=2, channel_mixing_enabled=False)
    _perturb(ly, g, 0.1, 0.2)
    with torch.no_grad():
        ly.channel_mixing.copy_(torch.eye(3))
    u = torch.randn(5, 3, *hw, generator=g).bfloat16().float()
    gy = torch.randn(5, 3, *hw, generator=g).bfloat16().float()
    _compare(ly, lambda a, p: O.adi_forward(a, p, O.cifar10_spec(hw[0], 3, dt=0.02, num_steps=2)), u, gy, tol=2e-2,
             dtype=torch.bfloat16)


@pytest.mark.parametrize("kind,hw", [("mnist", (28, 36)), ("mnist", (36, 20)), ("enhanced", (20, 32))],
                         ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_f16_whole_schedule_layers(kind, hw):
    """``layer.half()``: 1 ulp of the fp32 route on the same fp16-exact values, parameter gradients inside the fp16 window
    (test_gpu_f16.test_whole_schedule_layers on a rectangle)."""
    import cnn_with_pde_amd as P

    def make():
        if kind == "mnist":
            return quiet(P.MnistDiffusionLayer, size=hw, num_steps=4), O.mnist_spec(size=hw[0], num_steps=4)
        return (quiet(P.EnhancedDiffusionLayer, hw, 2, num_steps=4, channel_mixing_enabled=False),
                O.AdiSpec(hw[0], 2, 0.001, 1.0, 1.0, 4, "strang", False, 10.0, "none", False))
    gen = torch.Generator().manual_seed(hw[0] * 7 + hw[1])
    l32, spec = make()
    T16._perturb(l32, gen)
    T16._half_exact(l32)
    Cc = 2 if kind == "enhanced" else 1
    u = torch.randn(3, Cc, *hw, generator=gen).half()
    gy = torch.randn(3, Cc, *hw, generator=gen).half()
    l32 = l32.cuda()
    y32, gu32, _ = T16._run(l32, u.float().cuda(), gy.float().cuda())
    l16 = make()[0].half().cuda()
    l16.load_state_dict(l32.state_dict())
    y, gu, gp = T16._run(l16, u.cuda(), gy.cuda())
    assert y.dtype == torch.float16 and gu.dtype == torch.float16
    assert T16.max_ulps(y, y32.half()) <= 1 and T16.max_ulps(gu, gu32.half()) <= 1
    params = {k: v.detach().double().cpu() for k, v in l32.named_parameters()}
    _, _, gp_ref = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec), u.double(), params, gy.double())
    for n, g_ in gp.items():
        assert g_.dtype == torch.float16, n
        err = G.rel_err(g_.float().cpu().reshape(gp_ref[n].shape), gp_ref[n])
        print(kind, hw, n, f"{err:.2e}")
        assert err <= T16.TOL_PGRAD, n


@pytest.mark.parametrize("kind", ["cifar10", "svhn"])
def test_f16_channel_layers_vs_oracle(kind):
    """fp16 layers with a channel operator (composed per step on a rectangle) against the fp64 oracle with fp16 states:
    the windows of test_gpu_f16.test_channel_layers_vs_oracle."""
    import cnn_with_pde_amd as P
    hw, Cc = (16, 24), 3
    gen = torch.Generator().manual_seed(3)
    if kind == "cifar10":
        layer, spec = quiet(P.EnhancedDiffusionLayer, hw, Cc, num_steps=3), O.cifar10_spec(hw[0], Cc, num_steps=3)
    else:
        layer, spec = P.SvhnDiffusionLayer(hw, Cc, num_steps=3), O.svhn_spec(hw[0], Cc, num_steps=3)
    T16._perturb(layer, gen)
    if kind == "svhn":
        with torch.no_grad():
            layer.skip_weight.fill_(0.3)
    layer = T16._half_exact(layer).half()
    u = torch.randn(4, Cc, *hw, generator=gen).half().double()
    gy = torch.randn(4, Cc, *hw, generator=gen).half().double()
    params = {k: v.detach().double() for k, v in layer.named_parameters()}
    cast = lambda t: t.half().to(t.dtype)                                                   # noqa: E731
    for sc, tol, tol_skip in ((cast, T16.TOL_CAST, T16.TOL_SKIP), (None, T16.TOL_PLAIN, T16.TOL_PLAIN)):
        y_ref, gu_ref, gp_ref = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec, sc), u, params, gy)
        y, gu, gp = T16._run(layer.cuda(), u.half().cuda(), gy.half().cuda())
        assert y.dtype == torch.float16 and gu.dtype == torch.float16
        errs = {"y": G.rel_err(y.float().cpu(), y_ref), "gu": G.rel_err(gu.float().cpu(), gu_ref)}
        for n, g_ in gp.items():
            assert g_.dtype == torch.float16, n
            errs["g_" + n] = G.rel_err(g_.float().cpu().reshape(gp_ref[n].shape), gp_ref[n])
        print(kind, "state_cast" if sc else "plain", {k: f"{v:.3e}" for k, v in errs.items()})
        bad = {k: v for k, v in errs.items() if not v <= (tol_skip if k == "g_skip_weight" else tol)}
        assert not bad, (bad, errs)


@pytest.mark.parametrize("hw", [(5, 9), (36, 20), (28, 32), (100, 128), (128, 100), (128, 2)], ids=_ids)
@pytest.mark.parametrize("kind", ["mnist", "cifar10", "cifar2", "svhn"])
def test_f64_layers_vs_oracle(kind, hw):
    """``layer.double()``: double end to end (pde_adi_rect_f64_*); 100 x 128 / 128 x 100 keep the state plane of the
    backward in global memory (two double planes pass the LDS limit)."""
    import cnn_with_pde_amd as P
    gen = torch.Generator().manual_seed(hw[0] * 3 + hw[1])
    Cc = 1 if kind == "mnist" else 2
    if kind == "mnist":
        layer, spec = quiet(P.MnistDiffusionLayer, size=hw, num_steps=2), O.mnist_spec(size=hw[0], num_steps=2)
    elif kind == "cifar10":
        layer, spec = quiet(P.EnhancedDiffusionLayer, hw, Cc, num_steps=2), O.cifar10_spec(hw[0], Cc, num_steps=2)
    elif kind == "cifar2":
        layer, spec = quiet(P.LearnableDiffusionLayer, hw, Cc, num_steps=2), O.cifar2_spec(hw[0], Cc, num_steps=2)
    else:
        layer, spec = P.SvhnDiffusionLayer(hw, Cc, num_steps=2), O.svhn_spec(hw[0], Cc, num_steps=2)
    layer = layer.double()
    _perturb64(layer, gen, slope=0.5)
    u = torch.randn(3, Cc, *hw, generator=gen, dtype=torch.float64)
    gy = torch.randn(u.shape, generator=gen, dtype=torch.float64)
    params = {k: v.detach().clone() for k, v in layer.named_parameters()}
    ref = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec), u, params, gy)
    layer = layer.cuda()
    ud = u.cuda().requires_grad_(True)
    y = layer(ud)
    assert y.dtype == torch.float64
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    _check64(layer, ud, gy, y, ref, tol=TOL64)


def test_constant_input_and_repeatability():
    """Exact properties that need no oracle: every line system has row sums 1 + eps, so a constant plane comes back as
    c / (1 + eps)^S (to rounding); two calls give the same bits."""
    import cnn_with_pde_amd as P
    hw = (20, 52)
    g = torch.Generator().manual_seed(41)
    ly = quiet(P.MnistDiffusionLayer, hw, 0.05, 1.0, 1.5, 3)
    _perturb(ly, g, 0.3, 0.5)
    ly = ly.cuda()
    S = len(ly._schedule().flat)
    with torch.no_grad():
        y = ly(torch.full((2, 1, *hw), 3.0, device="cuda"))
    want = 3.0 / (1.0 + ly.stability_eps) ** S
    # every sweep rounds each entry a few times (fp32, 2^-24 relative each): 1e-5 is the suite's fp32 bound
    assert float((y.double() - want).abs().max()) / want < TOL
    u = torch.randn(9, 1, *hw, generator=g).cuda()
    gy = torch.randn(9, 1, *hw, generator=g).cuda()
    res = []
    for _ in range(2):
        for p in ly.parameters():
            p.grad = None
        x = u.clone().requires_grad_(True)
        y = ly(x)
        y.backward(gy)
        res.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in ly.parameters()])
        torch.empty(1 << 22, device="cuda").normal_()
    assert all(torch.equal(a, b) for a, b in zip(*res))


def _lib():
    from cnn_with_pde_amd import _lib as L
    L.load()
    return C.CDLL(L.LIB_PATH)


@pytest.mark.parametrize("N", [36, 100])
def test_square_through_rect_entry_is_bitwise_the_square_entry(N):
    """pde_adi_rect_forward / _backward with H = W = N against pde_adi_forward / _backward at a line length on the any-size
    path: the same kernels on the same work."""
    lib = _lib()
    case = R.adi_case(3, 2, N, N, 500 + N)
    old, new = R.run_entry(lib, case, rect=False), R.run_entry(lib, case, rect=True)
    for k in old:
        assert torch.equal(old[k], new[k]), k


def test_square_through_rect_entry_matches_fused_kernels():
    """N = 32: the square entry runs the fused register-resident kernels, the rectangle entry the any-size ones — another
    order of operations, the same mathematics (1e-5).  Every state is kept (mask of all sweeps but the last): the case's
    coefficients (up to 0.3) would amplify rounding in states rebuilt backwards, which is not what is compared here."""
    lib = _lib()
    case = R.adi_case(3, 2, 32, 32, 532, ckpt=0b11111)
    old, new = R.run_entry(lib, case, rect=False), R.run_entry(lib, case, rect=True)
    errs = {k: G.rel_err(new[k].cpu(), old[k].cpu()) for k in old}
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("N", sorted(R.SQUARE_PATH_CASES))
def test_square_any_size_path_did_not_move(N):
    """The square entry points at N = 30 (partial sums in LDS), 64 and 128 give, bit for bit, what they gave at the commit
    before the kernels were generalised to (H, W)."""
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adi_gen_square_path", "results.npz"))
    got = R.run_entry(_lib(), R.square_path_case(N), rect=False)
    for k, t in got.items():
        assert torch.equal(t.cpu(), torch.from_numpy(want[f"{k}_{N}"])), (k, N)


@pytest.mark.parametrize("kind", ["mnist", "svhn"])
def test_graphed_step_replays_eager_bits(kind):
    """Forward + backward of a rectangular layer with a frozen plan as ONE hipGraph."""
    import cnn_with_pde_amd as P
    hw = (24, 40)
    g = torch.Generator().manual_seed(19)
    if kind == "mnist":
        layer, Cc = quiet(P.MnistDiffusionLayer, hw, 0.3, 1.0, 1.0, 4), 1        # fashion-size coefficients: checkpoints
    else:
        layer, Cc = P.SvhnDiffusionLayer(hw, 3, dt=0.01, num_steps=3), 3
        with torch.no_grad():
            layer.channel_coupling.copy_(torch.eye(3) + 0.05 * torch.randn(3, 3, generator=g))
    layer = layer.cuda()
    x = torch.randn(6, Cc, *hw, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(6, Cc, *hw, generator=g).cuda()
    mask = layer.freeze_checkpoint_plan()
    assert (mask != 0) == (kind == "mnist")
    params = list(layer.parameters())

    def fn():
        y = layer(x)
        return (y,) + torch.autograd.grad(y, [x] + params, gy)

    step = P.GraphedStep(fn)
    for _ in range(2):
        eager = [t.clone() for t in fn()]
        got = step()
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert torch.equal(a, b)
        with torch.no_grad():
            x.copy_(torch.randn(x.shape, generator=g))


def test_refusals_through_the_module():
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd._lib import PdeError
    for hw in ((1, 8), (8, 129)):
        for layer in (quiet(P.MnistDiffusionLayer, hw).cuda(), quiet(P.EnhancedDiffusionLayer, hw, 3).cuda(),
                      P.SvhnDiffusionLayer(hw, 3).cuda(), quiet(P.MnistDiffusionLayer, hw).double().cuda()):
            Cc = 1 if layer.alpha_base.dim() == 2 else 3
            with pytest.raises(PdeError):
                layer(torch.zeros(2, Cc, *hw, device="cuda", dtype=layer.alpha_base.dtype))
    layer = quiet(P.FashionDiffusionLayer, (20, 36)).cuda()
    for shape in ((2, 1, 20, 30), (2, 1, 36, 20), (2, 1, 36, 36)):
        with pytest.raises(PdeError):
            layer(torch.zeros(*shape, device="cuda"))
    from cnn_with_pde_amd import functional as F_
    u = torch.zeros(2, 3, 20, 36, device="cuda")
    ok, bad = torch.ones(3, 20, 36, device="cuda"), torch.ones(3, 36, 20, device="cuda")
    with pytest.raises(PdeError):
        F_.adi_diffuse(u, ok, bad, ok, ok, F_.adi_schedule(0.01, 1.0, 1.0, 1)[0])


@pytest.mark.parametrize("name", ["mnist_20x36", "cifar10_c3_24x40"])
def test_layers_match_reference_vectors_on_rectangles(name):
    """The reference's own classes run on rectangular parameters (tests/golden/rect, tools/make_golden.py rect): the
    product's class with ``size=(H, W)`` loads those parameters and gives the reference's y and gradients to 1e-5."""
    import cnn_with_pde_amd as P
    g = G.Golden(name, directory=os.path.join(G.GOLDEN_DIR, "rect"))
    hw = tuple(g.meta["plane"])
    cls = {"mnist_test": P.MnistDiffusionLayer, "cifar10": P.EnhancedDiffusionLayer}[g.script]
    layer = quiet(cls, **dict(g.ctor, size=hw))
    layer.load_state_dict(g.params)
    layer = layer.cuda()
    ud = g.u.cuda().requires_grad_(True)
    y = layer(ud)
    y.backward(g.gy.cuda())
    torch.cuda.synchronize()
    errs = {"y": G.rel_err(y.detach().cpu(), g.y), "gu": G.rel_err(ud.grad.cpu(), g.gu)}
    for n, p in layer.named_parameters():
        errs["g_" + n] = G.rel_err(p.grad.cpu(), g.grads[n])
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL, errs


def test_state_dict_round_trip():
    import cnn_with_pde_amd as P
    a = P.SvhnDiffusionLayer((12, 20), 3).cuda()
    b = P.SvhnDiffusionLayer((12, 20), 3).cuda()
    b.load_state_dict(a.state_dict())
    assert a.size == b.size == (12, 20) and quiet(P.MnistDiffusionLayer, 28).size == 28
    u = torch.randn(2, 3, 12, 20, device="cuda")
    with torch.no_grad():
        assert torch.equal(a(u), b(u))
