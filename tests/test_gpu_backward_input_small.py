"""GPU: the backward of the one-launch C <= 4 layers when no parameter takes a gradient (pde_adi_small_forward_input,
pde_adi_small_backward_input[_states], pde_adi_multi_backward_input behind ``adi_diffuse_small``, ``adi_diffuse_small_states``
and ``adi_diffuse_multi``).

The contract: per plane the operations on the adjoint are the full kernel's in its order, so gu is BITWISE the gu of the
same call with parameters that require grad — every N, C, both step patterns, both positions of the channel operator,
the skip blend, smoothing, clamp masks that move in time, 16-bit tensors, rebuilt or parked states on the full side,
a grid that walks two samples, both launch arrangements of a shared-input group — and y is bitwise the y of the forward
that keeps its states.  Beside that: the trajectory call, fp32 against the fp64 oracle, which C symbol the backward
calls and what the node keeps alive, the layers and models of the reference, repeatability with dirty LDS and hipGraph
capture.

Run as a script (``python test_gpu_backward_input_small.py child <out.pt>``) this file computes the frozen gu of
CHILD_CASES and of one attack step through two models and writes them to a file: the parent starts it with
PDE_BWD_INPUT=0, where a frozen call must take the full backward, and compares bitwise.

After a fault of the device nothing more is started on it, as in tests/test_gpu_bounds.py: every test of this file runs
inside ``_guarded`` (applied to all of them at the end of the file), which ends the whole pytest session on a
``RuntimeError`` from torch that is not the library's own ``PdeError``; the child exits with 3 on such an error, and a child
that ends with 3, an abort, a segmentation fault, its time limit or fault text on stderr ends the session too."""
import contextlib
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

#: how a child that met a fault, an abort, a segmentation fault or a time limit ends, and what a fault leaves on stderr
FAULT_CODES = (3, -6, -11, 134, 139, 124, 137)
FAULT_TEXT = ("illegal memory access", "Memory access fault", "HIP error", "hipError", "HSA_STATUS_ERROR")


def _guarded(fn):
    """``fn`` with the session ended on a fault of the device (the asynchronous ones surface at the closing synchronize)."""
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


DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DT = 0.02
CLAMP = 1.0                   # with _tensors(moving=True): reached inside the time window at some points of channel 0


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _gen(*key):
    return torch.Generator().manual_seed(70001 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _steps(K, split, dt=DT):
    import cnn_with_pde_amd as P
    return P.adi_schedule(dt, 1.0, 1.0, K, split)


def _tensors(g, B, C, N, dtype, K, moving=True):
    """u, gy, the four coefficient tensors, M.  ``moving``: at a quarter of the points of channel 0 alpha and beta start just
    under CLAMP and rise with slope 1, so that they reach the clamp inside the window of K steps: that channel's clamp mask
    moves in time (the full backward then runs its masked body there; the adjoint never looks)."""
    pt = torch.float16 if dtype == torch.float16 else torch.float32       # (fp16 route: every parameter fp16 too)
    u = torch.randn(B, C, N, N, generator=g).to(dtype).cuda()
    gy = torch.randn(B, C, N, N, generator=g).to(dtype).cuda()
    T = K * DT
    ps = [0.8 * (1 + 0.1 * torch.randn(C, N, N, generator=g)) for _ in range(2)]
    ps += [0.5 * torch.randn(C, N, N, generator=g) for _ in range(2)]
    if moving:
        low = torch.rand(C, N, N, generator=g) < 0.25
        low[1:] = False
        for i in range(2):
            ps[i] = torch.where(low, CLAMP - 0.5 * T * (0.1 + 0.8 * torch.rand(C, N, N, generator=g)), ps[i])
            ps[i + 2] = torch.where(low, torch.ones(C, N, N), ps[i + 2])
        first, last = ps[0] + ps[2] * 0.0, ps[0] + ps[2] * (T - DT / 2)
        assert bool(((first < CLAMP) & (last > CLAMP))[0].any()), "the clamp mask of channel 0 must move"
    M = (torch.eye(C) + 0.2 * torch.randn(C, C, generator=g)).cuda()
    return u, gy, [p.to(pt).cuda() for p in ps], M


def _small(u, gy, ps, M, steps, mode, frozen, skip=None, emit=None, gtraj=None, **kw):
    import cnn_with_pde_amd.functional as F
    ud = u.clone().requires_grad_(True)
    pp = [p.clone().requires_grad_(not frozen) for p in ps]
    Mm = M.clone().requires_grad_(not frozen)
    kw.setdefault("clamp_max", CLAMP)
    if emit is None:
        sk = None if skip is None else skip.clone().requires_grad_(not frozen)
        y = F.adi_diffuse_small(ud, *pp, Mm, steps, mode, skip_weight=sk, **kw)
        (gu,) = torch.autograd.grad(y, ud, gy)
    else:
        y = F.adi_diffuse_small_states(ud, *pp, Mm, steps, mode, emit, **kw)
        (gu,) = torch.autograd.grad(y, ud, gtraj)
    return y.detach(), gu


def _both(u, gy, ps, M, steps, mode, full_ck=(0,), **kw):
    y1, only = _small(u, gy, ps, M, steps, mode, True, checkpoints=0, **kw)
    assert bool(torch.isfinite(only.double()).all())
    for ck in full_ck:
        y0, full = _small(u, gy, ps, M, steps, mode, False, checkpoints=ck, **kw)
        assert torch.equal(y0, y1), f"{int((y0 != y1).sum())} of {y0.numel()} elements of y differ (full checkpoints={ck})"
        assert torch.equal(only, full), f"{int((only != full).sum())} of {full.numel()} elements of gu differ (checkpoints={ck})"
    return only


@pytest.fixture(params=["native", "ctypes"])
def node(request, monkeypatch):
    """The autograd node ``adi_diffuse_small`` / ``adi_diffuse_multi`` take: the native one (csrc/host_ext.cpp) or the Python one."""
    from cnn_with_pde_amd import _lib as L
    L.load()
    assert L.host_ext() is not None, "the native host path was not built"
    if request.param == "ctypes":
        monkeypatch.setattr(L, "_host", False)
        assert L.host_ext() is None
    return request.param


MODES = [("pre", False), ("post", False), ("post", True)]


# ---------------------------------------------------------------------------------------------------- 1. one layer
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("N", [16, 28, 32])
def test_frozen_gu_and_y_are_bitwise_the_trainable_calls(N, C, dt, node):
    """The full side once with no checkpoint and once with a mask that parks the state after the first sweep of every step."""
    for B in (1, 5):
        for K in (1, 3):
            for split in ("strang", "lie"):
                for mode, skip in MODES:
                    for smooth3 in (False, True):
                        u, gy, ps, M = _tensors(_gen(N, C, B, K, len(split), smooth3), B, C, N, DTYPES[dt], K)
                        sk = torch.tensor(0.3).cuda() if skip else None
                        _both(u, gy, ps, M, _steps(K, split), mode, full_ck=(0, 1), skip=sk, smooth3=smooth3)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("mode,skip", MODES)
def test_a_grid_that_walks_two_samples(mode, skip, dt, node):
    """B = 1027: the grid is capped at 1024 workgroups, three of them walk two samples, and two workgroups share a CU."""
    u, gy, ps, M = _tensors(_gen(1027, len(mode), skip), 1027, 3, 16, DTYPES[dt], 2)
    sk = torch.tensor(-0.4).cuda() if skip else None
    _both(u, gy, ps, M, _steps(2, "strang"), mode, full_ck=(0, 1), skip=sk)


def test_two_workgroups_on_a_cu_do_not_disturb_each_other():
    """Several times the chip's CUs in workgroups, N = 32: every sample's gu is the gu of the same sample in a batch of five."""
    u, gy, ps, M = _tensors(_gen(900), 900, 3, 32, torch.float32, 3)
    steps = _steps(3, "strang")
    _, big = _small(u, gy, ps, M, steps, "pre", True)
    for i in (0, 300, 895):
        _, few = _small(u[i:i + 5], gy[i:i + 5], ps, M, steps, "pre", True)
        assert torch.equal(big[i:i + 5], few)
    for _ in range(2):
        assert torch.equal(_small(u, gy, ps, M, steps, "pre", True)[1], big)


# ---------------------------------------------------------------------------------------------------- 2. trajectory
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("mode", ["pre", "post"])
def test_trajectory_with_a_cotangent_on_every_slice(mode, dt):
    K = 4
    for split in ("strang", "lie"):
        for emit in ([0, 1, 2], [0], []):
            g = _gen(K, len(mode), len(emit), len(split))
            u, gy, ps, M = _tensors(g, 5, 3, 16, DTYPES[dt], K)
            gtraj = torch.randn(len(emit) + 1, *u.shape, generator=g).to(u.dtype).cuda()
            _both(u, gy, ps, M, _steps(K, split), mode, full_ck=(0, 1), emit=emit, gtraj=gtraj)


# ---------------------------------------------------------------------------------------------------- 3. shared input
def _multi(u, base, w, frozen, checkpoints=0):
    import cnn_with_pde_amd as P
    ud = u.clone().requires_grad_(True)
    layers = []
    for ps, M, st in base:
        pp = [p.clone().requires_grad_(not frozen) for p in ps]
        layers.append(dict(alpha_base=pp[0], beta_base=pp[1], alpha_time_coeff=pp[2], beta_time_coeff=pp[3],
                           M=M.clone().requires_grad_(not frozen), steps=st, clamp_max=CLAMP))
    out, ys, sums = P.adi_diffuse_multi(ud, layers, weights=w.clone().requires_grad_(not frozen), plane_sums=True,
                                        checkpoints=checkpoints)
    loss = (out.float() * 0.7).sum() + (ys[1].float() ** 2).sum() + (sums[len(base) - 1].float() * 0.3).sum()
    (gu,) = torch.autograd.grad(loss, ud)
    return out.detach(), [y.detach() for y in ys], gu


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("B", [3, 1025], ids=["side-by-side", "one-after-the-other"])
@pytest.mark.parametrize("L", [2, 3])
def test_shared_input_group_bitwise(L, B, dt, node):
    g = _gen(L, B)
    u = torch.randn(B, 3, 16, 16, generator=g).to(DTYPES[dt]).cuda()
    base = []
    for ldt, k in ((0.02, 2), (0.04, 3), (0.05, 1))[:L]:
        _, _, ps, M = _tensors(g, 1, 3, 16, DTYPES[dt], k)
        base.append((ps, M, _steps(k, "strang", ldt)))
    w = torch.softmax(torch.randn(L, generator=g), 0).cuda()
    out1, ys1, only = _multi(u, base, w, True)
    for ck in (0, 1):
        out0, ys0, full = _multi(u, base, w, False, ck)
        assert torch.equal(out0, out1) and all(torch.equal(a, b) for a, b in zip(ys0, ys1))
        assert torch.equal(only, full), f"{int((only != full).sum())} of {full.numel()} elements of gu differ (checkpoints={ck})"


# ---------------------------------------------------------------------------------------------------- 4. fresh process
CHILD_CASES = [(16, 3, "strang", "pre", False, "f32"), (28, 1, "lie", "post", True, "bf16"), (32, 4, "strang", "post", True, "f16"),
               (32, 3, "strang", "pre", False, "f32")]


def _child_case(case):
    N, C, split, mode, skip, dt = case
    u, gy, ps, M = _tensors(_gen(N, C, len(split), 5), 5, C, N, DTYPES[dt], 3)
    return u, gy, ps, M, _steps(3, split), mode, (torch.tensor(0.3).cuda() if skip else None)


def _models():
    import cnn_with_pde_amd as P
    out = []
    for cls, seed in ((P.SvhnPDEClassifier, 31), (P.CIFAR10PDENoConv, 32)):
        torch.manual_seed(seed)
        m = quiet(cls).cuda().eval()
        for p in m.parameters():
            p.requires_grad_(False)
        out.append(m)
    return out


def _attack_step(model):
    """One FGSM step: the gradient of the loss with respect to the image, on a batch of two."""
    g = _gen(len(type(model).__name__))
    x = torch.rand(2, 3, 32, 32, generator=g).cuda().requires_grad_(True)
    target = torch.tensor([3, 7]).cuda()
    loss = torch.nn.functional.cross_entropy(model(x), target)
    (gx,) = torch.autograd.grad(loss, x)
    return gx


def test_the_switch_restores_the_full_backward(tmp_path):
    out = str(tmp_path / "gu.pt")
    env = dict(os.environ, PDE_BWD_INPUT="0")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", out], env=env, capture_output=True, text=True,
                           timeout=300)
    except subprocess.TimeoutExpired as e:       # a hang: nothing more may start on this device
        pytest.exit(f"the child ran into its time limit: {str(e.stderr)[-1500:]}", returncode=3)
    if r.returncode in FAULT_CODES or (r.returncode != 0 and any(t in r.stderr for t in FAULT_TEXT)):
        pytest.exit(f"GPU fault in the child (exit {r.returncode}): {r.stderr[-1500:]}", returncode=3)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = torch.load(out)
    assert len(got) == len(CHILD_CASES) + 2
    for case, theirs in zip(CHILD_CASES, got):
        u, gy, ps, M, steps, mode, sk = _child_case(case)
        _, mine = _small(u, gy, ps, M, steps, mode, True, skip=sk)
        assert torch.equal(mine.cpu(), theirs), case
    for model, theirs in zip(_models(), got[len(CHILD_CASES):]):
        gx = _attack_step(model)
        assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
        assert torch.equal(gx.cpu(), theirs), type(model).__name__


# ---------------------------------------------------------------------------------------------------- 5. against fp64
@pytest.mark.parametrize("mode,skip,split", [("pre", False, "lie"), ("post", True, "strang")])
def test_fp32_gu_against_the_fp64_oracle(mode, skip, split, node):
    """The oracle's own input gradient (autograd through its float64 forward) is the reference; the project's 1e-5."""
    import golden_util as G
    from oracle import pde_oracle as O
    from test_gpu_parity import TOL
    N, C, K = 16, 3, 3
    u, gy, ps, M = _tensors(_gen(N, K, len(mode)), 5, C, N, torch.float32, K, moving=False)
    sk = torch.tensor(0.3).cuda() if skip else None
    _, gu = _small(u, gy, ps, M, _steps(K, split), mode, True, skip=sk, clamp_max=10.0)
    spec = O.AdiSpec(N, C, DT, 1.0, 1.0, K, split, False, 10.0, mode, skip, 1e-6)
    params = {k: p.double().cpu() for k, p in zip(("alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff"), ps)}
    params["channel_mixing" if mode == "pre" else "channel_coupling"] = M.double().cpu()
    if skip:
        params["skip_weight"] = sk.double().cpu()
    ud = u.double().cpu().requires_grad_(True)
    (ref,) = torch.autograd.grad(O.adi_forward(ud, params, spec), ud, gy.double().cpu())
    err = G.rel_err(gu.cpu(), ref)
    print(f"{mode} skip={skip} {split}: rel err of gu vs the fp64 oracle {err:.2e}")
    assert err <= TOL, err


# ---------------------------------------------------------------------------------------------------- 6. the node
class _Counted:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


def _count(monkeypatch, lib, names):
    out = {}
    for n in names:
        out[n] = _Counted(getattr(lib, n))
        monkeypatch.setattr(lib, n, out[n])
    return out


def test_which_call_the_python_nodes_make(monkeypatch):
    import cnn_with_pde_amd.functional as F
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    monkeypatch.setattr(L, "_host", False)
    waits = _Counted(F._wait_event)
    monkeypatch.setattr(F, "_wait_event", waits)
    ticket_waits = _Counted(F._KmaxTicket.wait)
    monkeypatch.setattr(F._KmaxTicket, "wait", lambda self: ticket_waits(self))
    c = _count(monkeypatch, lib, ["pde_adi_small_forward", "pde_adi_small_forward_input", "pde_adi_small_backward",
                                  "pde_adi_small_backward_input", "pde_adi_small_forward_states", "pde_adi_small_backward_states",
                                  "pde_adi_small_backward_input_states", "pde_adi_multi_backward", "pde_adi_multi_backward_input"])
    u, gy, ps, M = _tensors(_gen(6), 5, 3, 16, torch.float32, 3)
    steps = _steps(3, "strang")

    def calls():
        got = {k.replace("pde_adi_", ""): v.calls for k, v in c.items() if v.calls}
        for v in c.values():
            v.calls = 0
        return got

    for ck in ("auto", 0, 1):                                     # `checkpoints` is ignored on the frozen route
        _small(u, gy, ps, M, steps, "pre", True, checkpoints=ck)
        assert calls() == {"small_forward_input": 1, "small_backward_input": 1}, ck
    _small(u, gy, ps, M, steps, "pre", False, checkpoints=0)
    assert calls() == {"small_forward": 1, "small_backward": 1}
    g4 = torch.randn(3, *u.shape, generator=_gen(7)).cuda()
    _small(u, gy, ps, M, steps, "post", True, emit=[0, 1], gtraj=g4, checkpoints="auto")
    assert calls() == {"small_forward_states": 1, "small_backward_input_states": 1}
    _small(u, gy, ps, M, steps, "post", True, emit=[], gtraj=g4[:1], checkpoints="auto")
    assert calls() == {"small_forward_input": 1, "small_backward_input_states": 1}
    _small(u, gy, ps, M, steps, "post", False, emit=[0, 1], gtraj=g4, checkpoints=0)
    assert calls() == {"small_forward_states": 1, "small_backward_states": 1}
    base = [(ps, M, steps), (ps, M, _steps(2, "strang", 0.04))]
    w = torch.tensor([0.4, 0.6]).cuda()
    _multi(u, base, w, True, "auto")
    assert calls() == {"multi_backward_input": 1}
    assert waits.calls == 0 and ticket_waits.calls == 0           # no wait for coefficient maxima anywhere above ...
    _multi(u, base, w, False, "auto")
    assert calls() == {"multi_backward": 1} and waits.calls == 1  # ... where the trainable group waits once


def test_what_the_nodes_keep(node):
    """Frozen: no tensor of u's shape is saved, and for K = 10, B = 64, C = 3, N = 32 the memory held with only y alive is
    below the trainable call's by at least K - 1 tensors of u's size (it holds K states and u)."""
    import cnn_with_pde_amd.functional as F
    K, B, C, N = 10, 64, 3, 32
    u, gy, ps, M = _tensors(_gen(8), B, C, N, torch.float32, K)
    steps = _steps(K, "strang")
    sk = torch.tensor(0.3).cuda()
    held = {}
    for frozen in (True, False):
        torch.cuda.synchronize()
        ud = u.clone().requires_grad_(True)
        pp = [p.clone().requires_grad_(not frozen) for p in ps]
        before = torch.cuda.memory_allocated()
        y = F.adi_diffuse_small(ud, *pp, M.clone().requires_grad_(not frozen), steps, "post",
                                skip_weight=sk.clone().requires_grad_(not frozen), clamp_max=CLAMP, checkpoints=0)
        torch.cuda.synchronize()
        held[frozen] = torch.cuda.memory_allocated() - before
        if node == "ctypes":
            big = [t for t in y.grad_fn.saved_tensors if t is not None and tuple(t.shape[-4:]) == tuple(u.shape)]
            assert bool(big) != frozen, [tuple(t.shape) for t in y.grad_fn.saved_tensors if t is not None]
        y.backward(gy)
        assert ud.grad is not None and all((p.grad is None) == frozen for p in pp)
        del y, ud, pp
    tensor = u.numel() * u.element_size()
    print(f"held beside the inputs: frozen {held[True]} B, trainable {held[False]} B, one tensor {tensor} B")
    assert held[False] - held[True] >= (K - 1) * tensor, held


# ---------------------------------------------------------------------------------------------------- 7. layers, models
@pytest.mark.parametrize("which", ["svhn", "enhanced"])
def test_frozen_layers_give_their_trainable_twins_input_gradient(which, monkeypatch):
    """... and reach the input-only calls: on the ctypes node, where the bound functions can be counted."""
    import copy
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    monkeypatch.setattr(L, "_host", False)
    c = _count(monkeypatch, lib, ["pde_adi_small_forward", "pde_adi_small_forward_input", "pde_adi_small_backward",
                                  "pde_adi_small_backward_input"])
    g = _gen(len(which), 9)
    cls = P.SvhnDiffusionLayer if which == "svhn" else P.EnhancedDiffusionLayer
    layer = quiet(cls, 32, 3, num_steps=3).cuda()
    with torch.no_grad():
        layer.alpha_base.mul_((1 + 0.2 * torch.randn(layer.alpha_base.shape, generator=g)).cuda())
        layer.beta_time_coeff.copy_((0.5 * torch.randn(layer.beta_time_coeff.shape, generator=g)).cuda())
    twin = copy.deepcopy(layer)
    for p in layer.parameters():
        p.requires_grad_(False)
    x = torch.randn(5, 3, 32, 32, generator=g).cuda()
    gy = torch.randn(5, 3, 32, 32, generator=g).cuda()
    res = []
    for m in (layer, twin):
        for v in c.values():
            v.calls = 0
        xd = x.clone().requires_grad_(True)
        y = m(xd)
        (gx,) = torch.autograd.grad(y, xd, gy)
        res.append((y.detach(), gx))
        got = {k.replace("pde_adi_small_", ""): v.calls for k, v in c.items() if v.calls}
        assert got == ({"forward_input": 1, "backward_input": 1} if m is layer else {"forward": 1, "backward": 1}), got
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert all(p.grad is None for p in layer.parameters())


# ---------------------------------------------------------------------------------------------------- 8. repeat, capture
def _dirty():
    """Kernels that use LDS and leave arbitrary bit patterns (NaN payloads included) behind (tests/test_gpu_determinism.py)."""
    x = torch.randn(1 << 16, device="cuda")
    x[::7] = float("nan")
    x.sort()
    torch.cumsum(x, 0)
    (x.view(256, 256) @ x.view(256, 256)).sum()
    torch.softmax(x.view(64, -1), 1)


@pytest.mark.parametrize("N,dt", [(16, "f32"), (28, "bf16"), (32, "f16")])
def test_repeatable_whatever_is_left_in_lds(N, dt):
    """Lanes beyond the plane exist for N < 32 and read the wave's image: a run must not depend on what it finds there."""
    u, gy, ps, M = _tensors(_gen(N, 14), 33, 3, N, DTYPES[dt], 3)
    first = None
    for _ in range(3):
        _dirty()
        _, gu = _small(u, gy, ps, M, _steps(3, "strang"), "post", True, skip=torch.tensor(0.3).cuda())
        assert bool(torch.isfinite(gu.float()).all())
        first = gu if first is None else first
        assert torch.equal(gu, first)


def test_frozen_svhn_layer_captured_in_a_graph():
    """Forward + backward of a frozen layer are launches only — no wait for coefficient maxima, no plan — under the
    default checkpoint policy: captured as they are, the replay equals the eager call bitwise, twice."""
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(21)
    layer = quiet(P.SvhnDiffusionLayer, 32, 3, num_steps=3).cuda()
    with torch.no_grad():
        layer.alpha_base.mul_((1 + 0.2 * torch.randn(layer.alpha_base.shape, generator=g)).cuda())
    for p in layer.parameters():
        p.requires_grad_(False)
    x = torch.randn(33, 3, 32, 32, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(33, 3, 32, 32, generator=g).cuda()

    def fn():
        y = layer(x)
        return (y,) + torch.autograd.grad(y, [x], gy)

    step = P.GraphedStep(fn)
    eager = [t.clone() for t in fn()]
    for _ in range(2):
        got = step()
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert torch.equal(a, b)


def _child_main():
    assert sys.argv[1] == "child" and os.environ.get("PDE_BWD_INPUT") == "0"
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    L._host = False                       # the ctypes node: its calls can be counted
    outs = []
    names = ("pde_adi_small_backward_input", "pde_adi_small_forward_input", "pde_adi_small_backward")
    for case in CHILD_CASES:
        cnt = {n: _Counted(getattr(lib, n)) for n in names}
        for n, c in cnt.items():
            setattr(lib, n, c)
        u, gy, ps, M, steps, mode, sk = _child_case(case)
        _, gu = _small(u, gy, ps, M, steps, mode, True, skip=sk)
        assert [cnt[n].calls for n in names] == [0, 0, 1], (case, [cnt[n].calls for n in names])
        for n, c in cnt.items():
            setattr(lib, n, c.fn)
        outs.append(gu.cpu())
    L._host = None
    assert L.host_ext() is not None       # and the native node under the same switch: bitwise the ctypes node's
    for case, want in zip(CHILD_CASES, outs):
        u, gy, ps, M, steps, mode, sk = _child_case(case)
        _, gu = _small(u, gy, ps, M, steps, mode, True, skip=sk)
        assert torch.equal(gu.cpu(), want), case
    for model in _models():
        outs.append(_attack_step(model).cpu())
    torch.cuda.synchronize()
    torch.save(outs, sys.argv[2])


# every test of this file behind the guard (see the head of the file)
for _name, _fn in list(globals().items()):
    if _name.startswith("test_") and callable(_fn):
        globals()[_name] = _guarded(_fn)


if __name__ == "__main__":
    try:
        _child_main()
    except RuntimeError as e:
        if not TB._is_fault(e):
            raise
        print(f"GPU fault: {e}", file=sys.stderr)
        sys.exit(3)
