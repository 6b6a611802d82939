"""``layer.trajectory`` / ``functional.adi_diffuse_states``: the states after chosen time steps out of the launches the
plain forward makes, and a backward that takes an upstream gradient for every one of them (the pde_adi*_forward_states /
pde_adi*_backward_states entry points: emitting variants of the fused kernels and of the any-size kernels).

Reference of every case: the oracle as it stands.  The state after step k of a K-step layer is the output of the same
layer built with ``num_steps=k`` and no skip blend, so the reference is a stack of ``O.adi_forward`` calls, differentiated
with a random cotangent of the stacked shape; the metric is ``golden_util.rel_err`` on the states, the input gradient
and every parameter gradient, as ``test_gpu_parity._compare`` does.  Tolerances are the project's own, by import: fp32
``test_gpu_parity.TOL``, bf16 2e-2 (``test_gpu_anysize.test_bf16_tensors``), the fp16 windows of ``test_gpu_f16.py``,
float64 ``test_gpu_f64.TOL``; the checkpointed sparse-mask case keeps the 1e-3 its plain twin has in
``test_gpu_rect.py``."""
import dataclasses

import pytest
import torch

import golden_util as G
import test_gpu_f16 as T16
from oracle import pde_oracle as O
from test_gpu_f64 import TOL as TOL64
from test_gpu_f64 import _perturb as _perturb64
from test_gpu_parity import TOL, _perturb, quiet

pytestmark = pytest.mark.gpu
TOL_BF16 = 2e-2


def _stack_fn(spec, sel):
    return lambda a, p: torch.stack([O.adi_forward(a, p, dataclasses.replace(spec, num_steps=k, skip=False)) for k in sel])


def _traj(layer, spec, u, gy=None, steps=None, tol=TOL, dtype=torch.float32, seed=0):
    """Forward + backward of ``layer.trajectory`` against the oracle; every figure is printed before it is asserted."""
    sel = list(range(1, spec.num_steps + 1)) if steps is None else list(steps)
    if gy is None:
        gy = torch.randn((len(sel),) + tuple(u.shape), generator=torch.Generator().manual_seed(977 + seed), dtype=u.dtype)
        if dtype in (torch.bfloat16, torch.float16):
            gy = gy.to(dtype).to(u.dtype)
    params = {k: v.detach().clone() for k, v in layer.named_parameters()}
    y_ref, gu_ref, gp_ref = O.value_and_grads(_stack_fn(spec, sel), u, params, gy)
    dl = layer.cuda()
    dl.zero_grad(set_to_none=True)
    ud = u.to(dtype).cuda().requires_grad_(True)
    y = dl.trajectory(ud, steps)
    assert y.dtype == dtype and tuple(y.shape) == (len(sel),) + tuple(u.shape)
    assert all(y[i].is_contiguous() for i in range(len(sel)))
    y.backward(gy.to(dtype).cuda())
    torch.cuda.synchronize()
    errs = {"y": G.rel_err(y.detach().cpu(), y_ref), "gu": G.rel_err(ud.grad.cpu(), gu_ref)}
    for i in range(len(sel)):
        errs[f"y[{sel[i]}]"] = G.rel_err(y[i].detach().cpu(), y_ref[i])
    for n, p in dl.named_parameters():
        if gp_ref.get(n) is not None:
            assert p.grad is not None, n
            errs["g_" + n] = G.rel_err(p.grad.cpu().reshape(gp_ref[n].shape), gp_ref[n])
        else:
            assert p.grad is None, n
    print({k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v <= tol}
    assert not bad, (bad, errs)
    return errs, y.detach(), ud.grad, {n: p.grad for n, p in dl.named_parameters() if p.grad is not None}


def _enhanced(hw, Cc, steps, g, dt=0.01, slope=0.5, lie=False):
    import cnn_with_pde_amd as P
    N = hw if isinstance(hw, int) else hw[0]
    if lie:
        ly = quiet(P.LearnableDiffusionLayer, hw, Cc, dt, 1.0, 1.2, steps, channel_mixing_enabled=False)
        spec = dataclasses.replace(O.cifar2_spec(N, Cc, dt, 1.0, 1.2, steps), mix="none")
    else:
        ly = quiet(P.EnhancedDiffusionLayer, hw, Cc, dt=dt, num_steps=steps, channel_mixing_enabled=False)
        spec = dataclasses.replace(O.cifar10_spec(N, Cc, dt=dt, num_steps=steps), mix="none")
    _perturb(ly, g, 0.15, slope)
    return ly, spec


def _uv(g, B, Cc, hw, dtype=torch.float32):
    hw = (hw, hw) if isinstance(hw, int) else hw
    return torch.randn(B, Cc, *hw, generator=g, dtype=dtype)


# ---- fused family -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["strang_32", "n28_cut", "single_plane", "lie", "twelve_steps"])
def test_fused_family_vs_oracle(case):
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(11)
    if case == "strang_32":              # a ragged batch against the planes per workgroup pass, slopes != 0, all steps
        ly, spec = _enhanced(32, 5, 4, g)
        _traj(ly, spec, _uv(g, 13, 5, 32))
    elif case == "n28_cut":              # the schedule is cut at step 3 of 4
        ly, spec = _enhanced(28, 2, 4, g)
        _traj(ly, spec, _uv(g, 7, 2, 28), steps=[1, 3])
    elif case == "single_plane":
        ly, spec = quiet(P.MnistDiffusionLayer, 32, 0.01, 1.0, 1.3, 2), O.mnist_spec(32, 0.01, 1.0, 1.3, 2)
        _perturb(ly, g, 0.2, 0.4)
        _traj(ly, spec, _uv(g, 1, 1, 32))
    elif case == "lie":
        ly, spec = _enhanced(32, 3, 3, g, dt=0.03, slope=0.4, lie=True)
        _traj(ly, spec, _uv(g, 9, 3, 32))
    else:                                # a schedule longer than stays resident in the forward's ring
        ly, spec = _enhanced(32, 2, 12, g)
        _traj(ly, spec, _uv(g, 5, 2, 32))


@pytest.mark.parametrize("N", [12, 20])
def test_fused_other_line_lengths(N):
    """The emitting instantiations at line lengths whose half rows are no multiple of four values (N = 12: 6, N = 20: 10)
    and whose planes are no multiple of a wave's 16-byte accesses: Strang and Lie, a ragged batch."""
    g = torch.Generator().manual_seed(300 + N)
    ly, spec = _enhanced(N, 3, 3, g, dt=0.02)
    _traj(ly, spec, _uv(g, 11, 3, N))
    ly, spec = _enhanced(N, 2, 3, g, dt=0.03, slope=0.4, lie=True)
    _traj(ly, spec, _uv(g, 9, 2, N), steps=[1, 3])


def _moving_masks(hw, g):
    """The coefficients of test_gpu_rect.test_clamp_masks_that_move_in_time: they cross both clamp bounds during the
    schedule, so the clamp's pass-through mask is per sweep (the backward's masked body)."""
    import cnn_with_pde_amd as P
    ly = quiet(P.EnhancedDiffusionLayer, hw, 2, dt=0.5, num_steps=3, channel_mixing_enabled=False)
    p2 = (hw, hw) if isinstance(hw, int) else hw
    with torch.no_grad():
        ly.channel_mixing.copy_(torch.eye(2))
        ly.alpha_base.copy_(9.0 + 2.0 * torch.rand(2, *p2, generator=g))          # around clamp_max = 10
        ly.alpha_time_coeff.copy_(2.0 * torch.randn(2, *p2, generator=g))
        ly.beta_base.copy_(0.3 * torch.randn(2, *p2, generator=g))                 # around the floor
        ly.beta_time_coeff.copy_(torch.randn(2, *p2, generator=g))
    return ly, dataclasses.replace(O.cifar10_spec(p2[0], 2, dt=0.5, num_steps=3), mix="none")


@pytest.mark.parametrize("hw", [32, (36, 20)], ids=str)
def test_masked_body(hw):
    g = torch.Generator().manual_seed(5)
    ly, spec = _moving_masks(hw, g)
    _traj(ly, spec, _uv(g, 6, 2, hw))


def test_checkpoint_modes():
    """A default FashionDiffusionLayer (coefficients 0.27 / 0.54) needs checkpoints: "auto", "lagged" and the all-states
    mask are exact and agree at the fp32 tolerance; a sparse mask holds 1e-3."""
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(6)
    u = _uv(g, 6, 1, 28)
    spec = O.fashion_spec(28)
    S = 3 * spec.num_steps
    res = {}
    for ck in ("auto", "lagged", (1 << (S - 1)) - 1, 0b010010010010 & ((1 << (S - 1)) - 1)):
        ly = P.FashionDiffusionLayer()
        ly.checkpoint_policy = ck
        sparse = ck == 0b010010010010 & ((1 << (S - 1)) - 1)
        res[ck] = _traj(ly, spec, u, tol=1e-3 if sparse else TOL)
    base = res[(1 << (S - 1)) - 1]
    for ck in ("auto", "lagged"):
        assert torch.equal(res[ck][1], base[1])
        assert G.rel_err(res[ck][2].cpu(), base[2].cpu()) <= TOL
        for n in base[3]:
            assert G.rel_err(res[ck][3][n].cpu(), base[3][n].cpu()) <= TOL, (ck, n)


def test_launch_groups():
    """34 Strang steps = 102 sweeps: two launch groups, states out of both."""
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(34)
    ly, spec = quiet(P.MnistDiffusionLayer, size=8, num_steps=34), O.mnist_spec(size=8, num_steps=34)
    _perturb(ly, g, 0.2, 0.4)
    _traj(ly, spec, _uv(g, 3, 1, 8))


# ---- any-size family, float64, 16-bit tensors --------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [36, 5, (20, 36), (36, 20), (128, 2)], ids=str)
def test_anysize_family_vs_oracle(hw):
    g = torch.Generator().manual_seed(100 + (hw if isinstance(hw, int) else hw[0] * 131 + hw[1]))
    ly, spec = _enhanced(hw, 3, 3, g, dt=0.02)
    _traj(ly, spec, _uv(g, 3, 3, hw), steps=None if isinstance(hw, int) else [1, 3])


@pytest.mark.parametrize("hw", [(5, 9), 32, (100, 128)], ids=str)
def test_float64(hw):
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(64)
    N = hw if isinstance(hw, int) else hw[0]
    ly = quiet(P.EnhancedDiffusionLayer, hw, 2, dt=0.01, num_steps=3, channel_mixing_enabled=False).double()
    _perturb64(ly, g, slope=0.5)
    with torch.no_grad():
        ly.channel_mixing.copy_(torch.eye(2))
    spec = dataclasses.replace(O.cifar10_spec(N, 2, dt=0.01, num_steps=3), mix="none")
    _traj(ly, spec, _uv(g, 2, 2, hw, torch.float64), tol=TOL64, dtype=torch.float64)


@pytest.mark.parametrize("hw", [32, (24, 40)], ids=str)
def test_bf16_tensors(hw):
    g = torch.Generator().manual_seed(21)
    ly, spec = _enhanced(hw, 3, 3, g, dt=0.02, slope=0.2)
    u = _uv(g, 5, 3, hw).bfloat16().float()
    _traj(ly, spec, u, tol=TOL_BF16, dtype=torch.bfloat16)


def test_model_half():
    """``layer.half()`` on 28 x 28: the states and the input gradient are those of the fp32 route on the same fp16-exact
    values rounded once (1 ulp), and inside the fp16 windows against the oracle; parameter gradients inside TOL_PGRAD."""
    gen = torch.Generator().manual_seed(28)
    l32, spec = T16._whole("enhanced", 28)
    T16._perturb(l32, gen)
    T16._half_exact(l32)
    u = torch.randn(3, 2, 28, 28, generator=gen).half()
    gy = torch.randn(4, 3, 2, 28, 28, generator=gen).half()
    l32 = l32.cuda()
    ud = u.float().cuda().requires_grad_(True)
    y32 = l32.trajectory(ud)
    y32.backward(gy.float().cuda())
    l16 = quiet(lambda: T16._whole("enhanced", 28)[0]).half().cuda()
    l16.load_state_dict(l32.state_dict())
    uh = u.cuda().requires_grad_(True)
    y = l16.trajectory(uh)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    assert y.dtype == torch.float16 and uh.grad.dtype == torch.float16
    ulps = T16.max_ulps(y.detach(), y32.detach().half()), T16.max_ulps(uh.grad, ud.grad.half())
    print("ulps against the fp32 route", ulps)
    assert max(ulps) <= 1
    params = {k: v.detach().double().cpu() for k, v in l32.named_parameters()}
    y_ref, gu_ref, gp_ref = O.value_and_grads(_stack_fn(spec, [1, 2, 3, 4]), u.double(), params, gy.double())
    errs = {"y": G.rel_err(y.detach().cpu(), y_ref), "gu": G.rel_err(uh.grad.cpu(), gu_ref)}
    for n, p in l16.named_parameters():
        if gp_ref.get(n) is not None:
            assert p.grad is not None and p.grad.dtype == torch.float16, n
            errs["g_" + n] = G.rel_err(p.grad.float().cpu().reshape(gp_ref[n].shape), gp_ref[n])
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["y"] <= T16.TOL_PLAIN and errs["gu"] <= T16.TOL_PLAIN, errs
    assert all(v <= T16.TOL_PGRAD for k, v in errs.items() if k.startswith("g_")), errs


# ---- layers with a channel operator ------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [None, [2, 3]], ids=["all", "2_3"])
@pytest.mark.parametrize("kind", ["svhn", "enhanced_c3", "enhanced_wide"])
def test_operator_layers(kind, steps):
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(7)
    if kind == "svhn":
        ly, spec, shape = P.SvhnDiffusionLayer(32, 3, 0.05, 1.0, 3), O.svhn_spec(32, 3, 0.05, 1.0, 3), (4, 3, 32, 32)
        with torch.no_grad():
            ly.channel_coupling.copy_(torch.eye(3) + 0.05 * torch.randn(3, 3, generator=g))
            ly.skip_weight.fill_(0.2)
    elif kind == "enhanced_c3":
        ly, spec, shape = (quiet(P.EnhancedDiffusionLayer, 32, 3, dt=0.01, num_steps=3), O.cifar10_spec(32, 3, dt=0.01, num_steps=3),
                           (4, 3, 32, 32))
    else:                                # C = 32: the wide-operator path of the plain forward
        ly, spec, shape = (quiet(P.EnhancedDiffusionLayer, 16, 32, dt=0.01, num_steps=3), O.cifar10_spec(16, 32, dt=0.01, num_steps=3),
                           (2, 32, 16, 16))
    _perturb(ly, g, 0.2, 0.3)
    u = torch.randn(*shape, generator=g)
    _, y, _, grads = _traj(ly, spec, u, steps=steps)
    if kind == "svhn":                   # no blend: the last state is the 3-step layer without its skip, and the weight is unused
        assert ly.skip_weight.grad is None and "skip_weight" not in grads
        with torch.no_grad():
            blended = ly(u.cuda())
        assert not torch.equal(blended, y[-1])


# ---- invariants --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw", [32, 28, 36, (20, 36)], ids=str)
def test_last_state_is_bitwise_the_forward_and_calls_repeat(hw, dtype):
    g = torch.Generator().manual_seed(3)
    ly, _ = _enhanced(hw, 3, 10 if hw == 32 else 4, g)
    ly = ly.cuda()
    u = _uv(g, 9, 3, hw).to(dtype).cuda()
    K = ly.num_steps
    gy = torch.randn((K,) + tuple(u.shape), generator=g).to(dtype).cuda()
    with torch.no_grad():
        assert torch.equal(ly.trajectory(u)[-1], ly(u))
        assert torch.equal(ly.trajectory(u, [2, K])[-1], ly(u))
    runs = []
    for _ in range(2):
        ly.zero_grad(set_to_none=True)
        x = u.clone().requires_grad_(True)
        y = ly.trajectory(x)
        y.backward(gy)
        runs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in ly.parameters() if p.grad is not None])
        torch.empty(1 << 20, device="cuda").normal_()
    assert len(runs[0]) == 6 and all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw", [(96, 72), (128, 128)], ids=str)
def test_long_lines_with_the_device_full(hw, dtype):
    """A side above 64 makes the any-size workgroup two waves, and 2048 planes keep every CU busy with several of them:
    a state copied out while the other wave is already in the next sweep would show here.  Every emitted state must be
    bit for bit the plain forward of the same layer cut to that many steps (which stores nothing mid-loop), and two calls
    must agree bit for bit."""
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(65)
    ly, _ = _enhanced(hw, 8, 3, g, dt=0.02)
    ly = ly.cuda()
    u = _uv(g, 256, 8, hw).to(dtype).cuda()
    with torch.no_grad():
        a, b = ly.trajectory(u), ly.trajectory(u)
        assert torch.equal(a, b)
        for k in (1, 2, 3):
            cut = quiet(P.EnhancedDiffusionLayer, hw, 8, dt=0.02, num_steps=k, channel_mixing_enabled=False).cuda()
            cut.load_state_dict(ly.state_dict())
            assert torch.equal(a[k - 1], cut(u)), k


def test_one_sweep_launch_per_pass():
    """The library's launch counters: forward + backward of ``trajectory`` (all 10 states) counts what forward + backward
    of the layer itself counts — one sweep launch per pass, not one per step."""
    from cnn_with_pde_amd import functional as F_
    g = torch.Generator().manual_seed(4)
    ly, _ = _enhanced(32, 4, 10, g)
    ly = ly.cuda()
    u = _uv(g, 8, 4, 32).cuda()
    counts = []
    for fn in (lambda x: ly(x).sum(), lambda x: ly.trajectory(x).sum()):
        fn(u.clone().requires_grad_(True)).backward()          # warm: nothing one-off inside the counted pass
        torch.cuda.synchronize()
        F_.timing_enable(True)
        try:
            fn(u.clone().requires_grad_(True)).backward()
            torch.cuda.synchronize()
            _, nf, _, nb = F_.timing_read()
        finally:
            F_.timing_enable(False)
        counts.append((nf, nb))
    print("launches (forward, backward): layer", counts[0], "trajectory", counts[1])
    assert counts[0] == counts[1] == (1, 1)


def test_functional_emit_indices():
    """``adi_diffuse_states`` with sweep indices that are no step boundaries (the table-driven kernels), against the
    composition of plain calls; the last sweep is always included."""
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import functional as F_
    g = torch.Generator().manual_seed(12)
    for N in (32, 36):
        names = ["alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff"]
        ps = [(1.0 + 0.2 * torch.rand(2, N, N, generator=g)).cuda() for _ in range(2)] + \
             [(0.3 * torch.randn(2, N, N, generator=g)).cuda() for _ in range(2)]
        sweeps = [s for st in P.adi_schedule(0.02, 1.0, 1.0, 2) for s in st][:5]        # x y x x y: no step pattern
        u = torch.randn(4, 2, N, N, generator=g).cuda()
        out = F_.adi_diffuse_states(u, *ps, sweeps, [0, 3], clamp_max=10.0)
        assert tuple(out.shape) == (3, 4, 2, N, N)
        for i, s in enumerate((0, 3, 4)):
            want = P.adi_diffuse(u, *ps, sweeps[:s + 1], clamp_max=10.0)
            assert G.rel_err(out[i].cpu(), want.cpu()) <= TOL, (N, s, names)
    with pytest.raises(ValueError):
        F_.adi_diffuse_states(u, *ps, sweeps, [3, 1], clamp_max=10.0)
    with pytest.raises(ValueError):
        F_.adi_diffuse_states(u, *ps, sweeps, [5], clamp_max=10.0)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd._lib import PdeError
    ly = quiet(P.EnhancedDiffusionLayer, 32, 2, num_steps=4, channel_mixing_enabled=False).cuda()
    u = torch.zeros(2, 2, 32, 32, device="cuda")
    for bad in ([0], [3, 2], [5], [], [1, 1], [1.5]):
        with pytest.raises(ValueError):
            ly.trajectory(u, bad)
    with pytest.raises(PdeError):
        quiet(P.EnhancedDiffusionLayer, 32, 2, num_steps=4, channel_mixing_enabled=False).trajectory(torch.zeros(2, 2, 32, 32))
    with pytest.raises(PdeError):
        quiet(P.EnhancedDiffusionLayer, 32, 2, num_steps=4).trajectory(torch.zeros(2, 2, 32, 32))
    wide = quiet(P.MnistDiffusionLayer, (8, 129)).cuda()
    with pytest.raises(PdeError):
        wide(torch.zeros(2, 1, 8, 129, device="cuda"))
    with pytest.raises(PdeError):
        wide.trajectory(torch.zeros(2, 1, 8, 129, device="cuda"))
    with pytest.raises(ValueError):
        wide.trajectory(torch.zeros(2, 3, 8, 129, device="cuda"))
