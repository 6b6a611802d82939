"""GPU: the backward of the layers with a channel operator above C = 4 when no parameter takes a gradient
(include/pdecnn_mixed_input.h behind ``adi_diffuse_mixed``, ``channel_mix`` and ``skip_blend``).

The contract: every piece of the adjoint — M^T g on each path of the channel operator, the transposed solves of a step, the
skip split — is formed with the arithmetic the full backward has, so gu is BITWISE the gu of the same call with parameters
that require grad, on both mirrors of the node (csrc/host_ext.cpp and functional.py), and y is bitwise the y of the forward
that keeps its states, under ``no_grad`` too.  Beside that: the PDE_MIX_* arrangements and PDE_BWD_INPUT=0 in child
interpreters, fp32 against the fp64 oracle, the adjoint identity in float64, which C symbols the nodes call, what they keep
alive, and the frozen layer classes against their trainable twins.

Run as a script this file is the child of the switch tests: ``python test_gpu_backward_input_mixed.py both <cases>``
compares frozen and trainable calls inside a process started with a PDE_MIX_* switch; ``... save <out.pt>`` writes the
frozen gu of CHILD_CASES, started with PDE_BWD_INPUT=0 where a frozen call must take the full backward.

After a fault of the device nothing more is started on it, as in tests/test_gpu_backward_input_small.py: every test runs
inside ``_guarded``, and a child that ends with a fault code, its time limit or fault text on stderr ends the session."""
import contextlib
import copy
import ctypes as C
import functools
import io
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_bounds as TB  # noqa: E402

pytestmark = pytest.mark.gpu

FAULT_CODES = (3, -6, -11, 134, 139, 124, 137)
FAULT_TEXT = ("illegal memory access", "Memory access fault", "HIP error", "hipError", "HSA_STATUS_ERROR")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
DT = 0.02
CLAMP = 1.0                   # with _tensors(moving=True): reached inside the time window at some points of channel 0


def _guarded(fn):
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            out = fn(*a, **k)
            TB._sync()
            return out
        except RuntimeError as e:
            if not TB._is_fault(e):
                raise
            pytest.exit(f"GPU fault in {fn.__name__}: {e}", returncode=3)
    return run


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _gen(*key):
    return torch.Generator().manual_seed(90001 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _steps(K, split, dt=DT):
    import cnn_with_pde_amd as P
    return P.adi_schedule(dt, 1.0, 1.0, K, split)


def _tensors(g, B, Cc, N, dtype, K, moving=False):
    """u, gy, the four coefficient tensors, M — all of the tensors' type on the float16 and float64 routes, fp32 otherwise.
    ``moving``: the clamp mask of channel 0 moves in time (tests/test_gpu_backward_input_small.py)."""
    pt = dtype if dtype in (torch.float16, torch.float64) else torch.float32
    u = torch.randn(B, Cc, N, N, generator=g).to(dtype).cuda()
    gy = torch.randn(B, Cc, N, N, generator=g).to(dtype).cuda()
    T = K * DT
    ps = [0.8 * (1 + 0.1 * torch.randn(Cc, N, N, generator=g)) for _ in range(2)]
    ps += [0.5 * torch.randn(Cc, N, N, generator=g) for _ in range(2)]
    if moving:
        low = torch.rand(Cc, N, N, generator=g) < 0.25
        low[1:] = False
        for i in range(2):
            ps[i] = torch.where(low, CLAMP - 0.5 * T * (0.1 + 0.8 * torch.rand(Cc, N, N, generator=g)), ps[i])
            ps[i + 2] = torch.where(low, torch.ones(Cc, N, N), ps[i + 2])
        first, last = ps[0] + ps[2] * 0.0, ps[0] + ps[2] * (T - DT / 2)
        assert bool(((first < CLAMP) & (last > CLAMP))[0].any()), "the clamp mask of channel 0 must move"
    M = (torch.eye(Cc) + 0.3 / Cc ** 0.5 * torch.randn(Cc, Cc, generator=g)).to(pt).cuda()
    return u, gy, [p.to(pt).cuda() for p in ps], M


def _mixed(u, gy, ps, M, steps, mode, frozen, **kw):
    import cnn_with_pde_amd.functional as F
    ud = u.clone().requires_grad_(True)
    pp = [p.clone().requires_grad_(not frozen) for p in ps]
    y = F.adi_diffuse_mixed(ud, *pp, M.clone().requires_grad_(not frozen), steps, mode, **kw)
    (gu,) = torch.autograd.grad(y, ud, gy)
    return y.detach(), gu


def _both(u, gy, ps, M, steps, mode, full_ck=(0,), **kw):
    """Frozen against trainable, and the call under no_grad: y and gu bit for bit."""
    import cnn_with_pde_amd.functional as F
    y1, only = _mixed(u, gy, ps, M, steps, mode, True, checkpoints="auto", **kw)
    assert bool(torch.isfinite(only.double()).all()) and float(only.double().abs().max()) > 0
    with torch.no_grad():
        y2 = F.adi_diffuse_mixed(u, *ps, M, steps, mode, **kw)
    assert torch.equal(y2, y1), f"{int((y2 != y1).sum())} of {y1.numel()} elements of y differ under no_grad"
    for ck in full_ck:
        y0, full = _mixed(u, gy, ps, M, steps, mode, False, checkpoints=ck, **kw)
        assert torch.equal(y0, y1), f"{int((y0 != y1).sum())} of {y0.numel()} elements of y differ (full checkpoints={ck})"
        assert torch.equal(only, full), f"{int((only != full).sum())} of {full.numel()} elements of gu differ (checkpoints={ck})"
    return only


@pytest.fixture(params=["native", "ctypes"])
def node(request, monkeypatch):
    """The autograd node ``adi_diffuse_mixed`` takes: the native one (csrc/host_ext.cpp) or the Python one."""
    from cnn_with_pde_amd import _lib as L
    L.load()
    assert L.host_ext() is not None, "the native host path was not built"
    if request.param == "ctypes":
        monkeypatch.setattr(L, "_host", False)
        assert L.host_ext() is None
    return request.param


# ---------------------------------------------------------------------------------------------------- 1. the layer call
#: (B, C, N, tensors): scalar operator with fused and any-size sweeps; the three-piece kernel (28 x 28: a ragged last tile);
#: the fused fp32-MFMA kernel (C = 128 fp32; 32 / 96 on 16-bit tensors); the 16-bit matrix cores (64 / 128)
SHAPES = [(2, 5, 8, "f32"), (2, 5, 8, "bf16"), (2, 5, 8, "f16"), (2, 5, 10, "f32"),
          (2, 32, 28, "f32"), (2, 64, 8, "f32"), (2, 96, 8, "f32"), (1, 128, 8, "f32"),
          (2, 32, 8, "bf16"), (2, 32, 8, "f16"), (2, 96, 8, "bf16"), (2, 96, 8, "f16"),
          (2, 64, 8, "bf16"), (2, 64, 8, "f16"), (1, 128, 8, "bf16"), (1, 128, 8, "f16")]


@pytest.mark.parametrize("B,Cc,N,dt", SHAPES, ids=[f"b{b}c{c}n{n}-{d}" for b, c, n, d in SHAPES])
def test_frozen_gu_and_y_are_bitwise_the_trainable_calls(B, Cc, N, dt, node):
    K = 2
    for split in ("strang", "lie"):
        for mode in ("pre", "post"):
            u, gy, ps, M = _tensors(_gen(B, Cc, N, len(split), len(mode)), B, Cc, N, DTYPES[dt], K)
            _both(u, gy, ps, M, _steps(K, split), mode, clamp_max=10.0)


@pytest.mark.parametrize("Cc,N,dt", [(5, 8, "f32"), (32, 28, "f32"), (64, 8, "bf16")])
def test_moving_clamp_masks_and_parked_states_on_the_full_side(Cc, N, dt, node):
    """Coefficients whose clamp mask moves in time (the full backward runs its masked body on that channel), and on the full
    side once no checkpoint, once the state after the first sweep of every step parked, once the plan from the maxima."""
    K = 3
    for mode in ("pre", "post"):
        u, gy, ps, M = _tensors(_gen(Cc, N, len(mode), 3), 2, Cc, N, DTYPES[dt], K, moving=True)
        _both(u, gy, ps, M, _steps(K, "strang"), mode, full_ck=(0, 1, "auto"), clamp_max=CLAMP)


def test_a_visible_eps_scales_as_the_full_backward_does():
    """eps = 1e-2: every step's adjoint carries (1+eps)^-3, applied where pde_adi_backward_step applies it."""
    for mode in ("pre", "post"):
        u, gy, ps, M = _tensors(_gen(7, len(mode)), 2, 5, 16, torch.float32, 3)
        _both(u, gy, ps, M, _steps(3, "strang"), mode, clamp_max=10.0, eps=1e-2)


def test_no_call_takes_a_one_launch_reverse_walk():
    """pde_adi_mixed_backward_input_one_launch: no one-launch kernel is built, the composed route serves every shape."""
    import cnn_with_pde_amd.functional as F
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    for Cc, N, io, split in ((32, 28, L.PDE_IO_F32, "strang"), (64, 32, L.PDE_IO_F32, "lie"), (16, 32, L.PDE_IO_F32, "strang"),
                             (64, 32, L.PDE_IO_BF16, "strang")):
        st = _steps(2, split)
        d = F._make_desc(2, Cc, N, io, [s for x in st for s in x], False, 10.0, 1e-6)
        assert lib.pde_adi_mixed_backward_input_one_launch(C.byref(d), len(st[0])) == 0


# ---------------------------------------------------------------------------------------------------- 2. switches
SWITCH_CASES = {
    # fp32 at C = 32 / 64 / 96 on the fused fp32-MFMA kernel
    "PDE_MIX_NO_SPLIT": [(2, 32, 28, "f32"), (2, 64, 8, "f32"), (2, 96, 8, "f32")],
    # the transposed apply kernel alone: fp32 at C = 128, 16-bit tensors at C = 32
    "PDE_MIX_UNFUSED": [(1, 128, 8, "f32"), (2, 32, 8, "bf16"), (2, 96, 8, "f16")],
    # the composed forward at the shapes the one-launch forward serves
    "PDE_WIDE": [(2, 32, 28, "f32"), (2, 64, 32, "f32")],
}
CHILD_CASES = [(2, 5, 8, "f32", "pre"), (2, 32, 28, "f32", "post"), (2, 64, 8, "bf16", "pre"), (1, 128, 8, "f16", "post")]


def _run_child(args, env, timeout=300):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired as e:       # a hang: nothing more may start on this device
        pytest.exit(f"the child ran into its time limit: {str(e.stderr)[-1500:]}", returncode=3)
    if r.returncode in FAULT_CODES or (r.returncode != 0 and any(t in r.stderr for t in FAULT_TEXT)):
        pytest.exit(f"GPU fault in the child (exit {r.returncode}): {r.stderr[-1500:]}", returncode=3)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r


@pytest.mark.parametrize("switch", sorted(SWITCH_CASES))
def test_bitwise_behind_a_switch(switch):
    """The other arrangements of the channel operator's backward (reached as tests/test_gpu_mix_paths.py reaches them) and
    the per-step forward at the wide shapes: frozen against trainable inside a child started with the switch."""
    env = dict(os.environ, **{switch: "0" if switch == "PDE_WIDE" else "1"})
    r = _run_child(["both", switch], env)
    assert f"{len(SWITCH_CASES[switch]) * 2} comparisons" in r.stdout, r.stdout[-500:]


def _child_case(case):
    B, Cc, N, dt, mode = case
    u, gy, ps, M = _tensors(_gen(B, Cc, N, 5), B, Cc, N, DTYPES[dt], 2)
    return u, gy, ps, M, _steps(2, "strang"), mode


def test_the_switch_restores_the_full_calls(tmp_path):
    out = str(tmp_path / "gu.pt")
    _run_child(["save", out], dict(os.environ, PDE_BWD_INPUT="0"))
    got = torch.load(out)
    assert len(got) == len(CHILD_CASES)
    for case, (y, gu) in zip(CHILD_CASES, got):
        u, gy, ps, M, steps, mode = _child_case(case)
        y1, mine = _mixed(u, gy, ps, M, steps, mode, True, clamp_max=10.0)
        assert torch.equal(mine.cpu(), gu) and torch.equal(y1.cpu(), y), case


# ---------------------------------------------------------------------------------------------------- 3. operator, blend
MIX_SHAPES = [(2, 5, 8, "f32"), (2, 5, 10, "bf16"), (2, 32, 28, "f32"), (2, 64, 8, "f32"), (2, 96, 8, "f32"), (1, 128, 8, "f32"),
              (2, 32, 8, "bf16"), (2, 96, 8, "f16"), (2, 64, 8, "bf16"), (1, 128, 8, "f16"), (2, 5, 8, "f64"), (2, 33, 7, "f64")]


@pytest.mark.parametrize("B,Cc,N,dt", MIX_SHAPES, ids=[f"b{b}c{c}n{n}-{d}" for b, c, n, d in MIX_SHAPES])
def test_channel_mix_with_a_frozen_operator(B, Cc, N, dt):
    import cnn_with_pde_amd.functional as F
    u, gy, _, M = _tensors(_gen(B, Cc, N, 11), B, Cc, N, DTYPES[dt], 1)
    res = []
    for frozen in (True, False):
        ud = u.clone().requires_grad_(True)
        Mm = M.clone().requires_grad_(not frozen)
        y = F.channel_mix(ud, Mm)
        big = [t for t in y.grad_fn.saved_tensors if t is not None and t.numel() == u.numel()]
        assert bool(big) != frozen, [tuple(t.shape) for t in y.grad_fn.saved_tensors if t is not None]
        y.backward(gy)
        assert (Mm.grad is None) == frozen
        res.append((y.detach(), ud.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert bool(torch.isfinite(res[0][1].double()).all()) and float(res[0][1].double().abs().max()) > 0


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("shape", [(2, 5, 8, 8), (3, 7, 5, 5), (2, 64, 32, 32)], ids=lambda s: "x".join(map(str, s)))
def test_skip_blend_with_a_frozen_weight(shape, dt):
    """(3, 7, 5, 5): 525 elements, a tail of 5 behind the 8-wide accesses."""
    import cnn_with_pde_amd.functional as F
    g = _gen(*shape, 12)
    dtype = DTYPES[dt]
    u0, u, gy = (torch.randn(shape, generator=g).to(dtype).cuda() for _ in range(3))
    w = torch.tensor(0.3).to(dtype if dt in ("f16", "f64") else torch.float32).cuda()
    res = []
    for frozen in (True, False):
        a, b = u0.clone().requires_grad_(True), u.clone().requires_grad_(True)
        ww = w.clone().requires_grad_(not frozen)
        y = F.skip_blend(a, b, ww)
        big = [t for t in y.grad_fn.saved_tensors if t is not None and t.numel() == u.numel()]
        assert bool(big) != frozen
        y.backward(gy)
        assert (ww.grad is None) == frozen
        res.append((y.detach(), a.grad, b.grad))
    for x, z in zip(*res):
        assert torch.equal(x, z)
    # only one of the two tensors needs a gradient: the other comes back as None, the first unchanged
    a = u0.clone().requires_grad_(True)
    (ga,) = torch.autograd.grad(F.skip_blend(a, u, w), a, gy)
    assert torch.equal(ga, res[0][1])


# ---------------------------------------------------------------------------------------------------- 4. the layers
def _randomise(layer, g):
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if n in ("alpha_base", "beta_base"):
                p.mul_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif n in ("alpha_time_coeff", "beta_time_coeff"):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif n in ("channel_mixing", "channel_coupling"):
                c = p.shape[0]
                p.copy_(torch.eye(c) + (0.4 / c ** 0.5) * torch.randn(c, c, generator=g))
            elif n == "skip_weight":
                p.fill_(0.3)


def _make(kind, C_, N, steps, dt):
    import cnn_with_pde_amd as P
    from oracle import pde_oracle as O
    if kind == "cifar10":
        return quiet(P.EnhancedDiffusionLayer, N, C_, dt=dt, num_steps=steps), O.cifar10_spec(N, C_, dt=dt, num_steps=steps)
    if kind == "cifar2":
        return quiet(P.LearnableDiffusionLayer, N, C_, dt=dt, num_steps=steps), O.cifar2_spec(N, C_, dt=dt, num_steps=steps)
    return quiet(P.SvhnDiffusionLayer, N, C_, dt=dt, dx=1.0, num_steps=steps), O.svhn_spec(N, C_, dt=dt, dx=1.0, num_steps=steps)


def _freeze(layer):
    for p in layer.parameters():
        p.requires_grad_(False)
    return layer


@pytest.mark.parametrize("kind,C_,N", [("cifar10", 5, 8), ("cifar10", 32, 28), ("cifar2", 64, 8), ("svhn", 5, 16), ("svhn", 32, 28),
                                       ("svhn", 5, 10)])
def test_frozen_layers_give_their_trainable_twins_input_gradient(kind, C_, N, node):
    g = _gen(len(kind), C_, N)
    layer = _make(kind, C_, N, 3, 0.02)[0]
    _randomise(layer, g)
    layer = layer.cuda()
    twin = copy.deepcopy(layer)
    _freeze(layer)
    x = torch.randn(2, C_, N, N, generator=g).cuda()
    gy = torch.randn(2, C_, N, N, generator=g).cuda()
    res = []
    for m in (layer, twin):
        xd = x.clone().requires_grad_(True)
        y = m(xd)
        (gx,) = torch.autograd.grad(y, xd, gy)
        res.append((y.detach(), gx))
    with torch.no_grad():
        assert torch.equal(layer(x), res[0][0])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert all(p.grad is None for p in layer.parameters())


# ---------------------------------------------------------------------------------------------------- 5. against fp64
@pytest.mark.parametrize("kind,C_,N,steps,dt,B", [
    ("cifar10", 64, 32, 3, 0.02, 3), ("cifar10", 32, 28, 2, 0.05, 5), ("cifar2", 64, 28, 3, 0.03, 2), ("cifar2", 32, 32, 4, 0.02, 3),
    ("svhn", 64, 32, 3, 0.02, 2), ("svhn", 32, 28, 2, 0.05, 1)])            # the six shapes of tests/test_gpu_wide.py
def test_frozen_fp32_gu_against_the_fp64_oracle(kind, C_, N, steps, dt, B):
    import golden_util as G
    from oracle import pde_oracle as O
    from test_gpu_wide import CASES, TOL
    assert (kind, C_, N, steps, dt, B) in CASES and TOL == 1e-5
    g = torch.Generator().manual_seed(4000 + C_ + N + steps)
    layer, spec = _make(kind, C_, N, steps, dt)
    _randomise(layer, g)
    u = torch.randn(B, C_, N, N, generator=g)
    gy = torch.randn(B, C_, N, N, generator=g)
    params = {k: v.detach().clone() for k, v in layer.named_parameters()}
    y_ref, gu_ref, _ = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec), u, params, gy)
    dl = _freeze(layer.cuda())
    ud = u.cuda().requires_grad_(True)
    y = dl(ud)
    y.backward(gy.cuda())
    errs = {"y": G.rel_err(y.detach().cpu(), y_ref), "gu": G.rel_err(ud.grad.cpu(), gu_ref)}
    print(f"{kind} C={C_} N={N}: rel err vs the fp64 oracle {errs}")
    assert all(v <= TOL for v in errs.values()), errs


@pytest.mark.parametrize("Cc,N,mode", [(5, 8, "pre"), (5, 10, "post"), (33, 7, "pre")])
def test_adjoint_identity_in_float64(Cc, N, mode):
    """<F v, g> = <v, F^T g> on the float64 per-step route (channel_mix + adi_diffuse, both on their input-only backward):
    within 1e-11 of |F v| |g|, the bound tests/test_gpu_backward_input.py holds the same identity to."""
    import cnn_with_pde_amd.functional as F
    v, g, ps, M = _tensors(_gen(Cc, N, len(mode), 64), 3, Cc, N, torch.float64, 3)
    steps = _steps(3, "strang")
    with torch.no_grad():
        Fv = F.adi_diffuse_mixed(v, *ps, M, steps, mode, clamp_max=10.0)
    assert Fv.dtype == torch.float64
    _, Ftg = _mixed(v, g, ps, M, steps, mode, True, clamp_max=10.0)
    lhs, rhs = float((Fv * g).sum()), float((v * Ftg).sum())
    scale = float(Fv.norm() * g.norm())
    print(f"C={Cc} N={N} {mode}: <F v, g> = {lhs:.15e}  <v, F^T g> = {rhs:.15e}  |diff| / scale = {abs(lhs - rhs) / scale:.2e}")
    assert abs(lhs - rhs) <= 1e-11 * scale
    _, full = _mixed(v, g, ps, M, steps, mode, False, clamp_max=10.0)
    assert torch.equal(Ftg, full)


# ---------------------------------------------------------------------------------------------------- 6. the nodes
class _Counted:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


def test_which_calls_the_python_node_makes(monkeypatch):
    import cnn_with_pde_amd.functional as F
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    monkeypatch.setattr(L, "_host", False)
    ticket_waits = _Counted(F._KmaxTicket.wait)
    monkeypatch.setattr(F._KmaxTicket, "wait", lambda self: ticket_waits(self))
    names = ["pde_adi_mixed_forward", "pde_adi_mixed_forward_input", "pde_adi_mixed_backward", "pde_adi_mixed_backward_input",
             "pde_adi_param_grads", "pde_channel_mix_backward_steps"]
    c = {n: _Counted(getattr(lib, n)) for n in names}
    for n, v in c.items():
        monkeypatch.setattr(lib, n, v)

    def calls():
        got = {k.replace("pde_adi_mixed_", ""): v.calls for k, v in c.items() if v.calls}
        for v in c.values():
            v.calls = 0
        return got

    u, gy, ps, M = _tensors(_gen(6), 2, 5, 8, torch.float32, 2)
    steps = _steps(2, "strang")
    for ck in ("auto", 0, 1):                                     # `checkpoints` is ignored on the frozen route
        _mixed(u, gy, ps, M, steps, "pre", True, checkpoints=ck)
        assert calls() == {"forward_input": 1, "backward_input": 1}, ck
    with torch.no_grad():
        F.adi_diffuse_mixed(u, *ps, M, steps, "post")
    assert calls() == {"forward_input": 1}
    assert ticket_waits.calls == 0                                # no wait for coefficient maxima anywhere above ...
    sink = []
    ud = u.clone().requires_grad_(True)
    F.adi_diffuse_mixed(ud, *ps, M, steps, "pre", kmax_sink=sink)
    assert calls() == {"forward_input": 1} and len(sink) == 1 and len(sink[0].wait()) == 6       # ... but a sink gets them
    ticket_waits.calls = 0
    _mixed(u, gy, ps, M, steps, "pre", False, checkpoints="auto")
    assert calls() == {"forward": 1, "backward": 1} and ticket_waits.calls == 1
    # the operator alone needs a gradient: the full route
    ud = u.clone().requires_grad_(True)
    y = F.adi_diffuse_mixed(ud, *ps, M.clone().requires_grad_(True), steps, "pre", checkpoints=0)
    y.backward(gy)
    assert calls() == {"forward": 1, "backward": 1}


def test_what_the_nodes_keep(node):
    """Frozen: no tensor of u's size is saved by either mirror, and across the forward of a ten-step (4, 32, 28, 28) call the
    memory held grows by less than two tensors of the input's size; the trainable call keeps 2K - 1 states beside y (2K
    tensors).  Both figures are counted beside the steps workspace — the factorisation, which both routes keep for their
    backward and which does not depend on the batch: 38 MB here, 95 tensors of this small batch's size."""
    import cnn_with_pde_amd.functional as F
    from cnn_with_pde_amd import _lib as L
    K, B, Cc, N = 10, 4, 32, 28
    u, gy, ps, M = _tensors(_gen(8), B, Cc, N, torch.float32, K)
    steps = _steps(K, "strang", 0.001)
    tensor = u.numel() * u.element_size()
    d = F._make_desc(B, Cc, N, L.PDE_IO_F32, [s for st in steps for s in st], False, 10.0, 1e-6)
    sws = L.load().pde_adi_steps_workspace_bytes(C.byref(d), 3)
    held = {}
    for frozen in (True, False):
        torch.cuda.synchronize()
        ud = u.clone().requires_grad_(True)
        pp = [p.clone().requires_grad_(not frozen) for p in ps]
        Mm = M.clone().requires_grad_(not frozen)
        before = torch.cuda.memory_allocated()
        y = F.adi_diffuse_mixed(ud, *pp, Mm, steps, "pre", clamp_max=10.0, checkpoints=0)
        torch.cuda.synchronize()
        held[frozen] = torch.cuda.memory_allocated() - before
        if node == "ctypes":
            big = [t for t in y.grad_fn.saved_tensors if t is not None and t.numel() >= u.numel()]
            assert bool(big) != frozen, [tuple(t.shape) for t in y.grad_fn.saved_tensors if t is not None]
        y.backward(gy)
        assert ud.grad is not None and all((p.grad is None) == frozen for p in pp)
        del y, ud, pp
    print(f"held beside the inputs: frozen {held[True]} B, trainable {held[False]} B, of which the steps workspace {sws} B; "
          f"one tensor {tensor} B")
    assert held[True] - sws < 2 * tensor, (held, sws, tensor)
    assert held[False] - sws >= 2 * K * tensor, (held, sws, tensor)


def test_the_per_step_route_keeps_nothing_either():
    """C = 5 (no one-launch forward): the two scratch tensors of the forward are gone when it returns."""
    import cnn_with_pde_amd.functional as F
    from cnn_with_pde_amd import _lib as L
    u, gy, ps, M = _tensors(_gen(9), 8, 5, 32, torch.float32, 10)
    steps = _steps(10, "strang", 0.001)
    tensor = u.numel() * u.element_size()
    torch.cuda.synchronize()
    ud = u.clone().requires_grad_(True)
    before = torch.cuda.memory_allocated()
    y = F.adi_diffuse_mixed(ud, *ps, M, steps, "post", clamp_max=10.0)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before
    d = F._make_desc(8, 5, 32, L.PDE_IO_F32, [s for st in steps for s in st], False, 10.0, 1e-6)
    sws = L.load().pde_adi_steps_workspace_bytes(C.byref(d), 3)
    assert held - sws < 2 * tensor, (held, sws, tensor)            # y alone, beside the factorisation
    y.backward(gy)


# ---------------------------------------------------------------------------------------------------- the child
def _child_both(switch):
    assert os.environ.get(switch) == ("0" if switch == "PDE_WIDE" else "1")
    from cnn_with_pde_amd import _lib as L
    n = 0
    for host in (None, False):                                    # the native node, then the ctypes node
        L._host = host
        for B, Cc, N, dt in SWITCH_CASES[switch]:
            for mode in ("pre", "post"):
                u, gy, ps, M = _tensors(_gen(B, Cc, N, len(mode), 21), B, Cc, N, DTYPES[dt], 2)
                _both(u, gy, ps, M, _steps(2, "strang"), mode, clamp_max=10.0)
                n += 1
    torch.cuda.synchronize()
    print(f"{n // 2} comparisons per node")


def _child_save(out):
    assert os.environ.get("PDE_BWD_INPUT") == "0"
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    outs = []
    names = ("pde_adi_mixed_forward_input", "pde_adi_mixed_backward_input", "pde_adi_mixed_backward")
    L._host = False                       # the ctypes node: its calls can be counted
    for case in CHILD_CASES:
        cnt = {n: _Counted(getattr(lib, n)) for n in names}
        for n, c in cnt.items():
            setattr(lib, n, c)
        u, gy, ps, M, steps, mode = _child_case(case)
        y, gu = _mixed(u, gy, ps, M, steps, mode, True, clamp_max=10.0)
        assert [cnt[n].calls for n in names] == [0, 0, 1], (case, [cnt[n].calls for n in names])
        for n, c in cnt.items():
            setattr(lib, n, c.fn)
        outs.append((y.cpu(), gu.cpu()))
    L._host = None
    assert L.host_ext() is not None       # and the native node under the same switch: bitwise the ctypes node's
    for case, (y0, g0) in zip(CHILD_CASES, outs):
        u, gy, ps, M, steps, mode = _child_case(case)
        y, gu = _mixed(u, gy, ps, M, steps, mode, True, clamp_max=10.0)
        assert torch.equal(gu.cpu(), g0) and torch.equal(y.cpu(), y0), case
    torch.cuda.synchronize()
    torch.save(outs, out)


# every test of this file behind the guard (see the head of the file)
for _name, _fn in list(globals().items()):
    if _name.startswith("test_") and callable(_fn):
        globals()[_name] = _guarded(_fn)


if __name__ == "__main__":
    try:
        if sys.argv[1] == "both":
            _child_both(sys.argv[2])
        else:
            assert sys.argv[1] == "save"
            _child_save(sys.argv[2])
    except RuntimeError as e:
        if not TB._is_fault(e):
            raise
        print(f"GPU fault: {e}", file=sys.stderr)
        sys.exit(3)
