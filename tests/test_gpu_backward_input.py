"""GPU: the backward of an implicit layer whose coefficients take no gradient (the *_backward_input entry points).

With frozen coefficients the autograd nodes of ``adi_diffuse`` / ``adi_diffuse_states`` run gu = F^T gy alone.  The
contract: per plane the operations that produce gu are the full backward's in its order, so gu is BITWISE the gu of the
same call with coefficients that require grad — HIP or assembly full backward, rebuilt or parked states, moving clamp
masks, 16-bit tensors, float64, rectangles.  Beside that: the adjoint identity on the float64 route, fp32 against the
fp64 oracle, the trajectory call, what the node keeps alive and which C symbol its backward calls, repeatability with
dirty LDS and hipGraph capture.

Run as a script (``python test_gpu_backward_input.py child <out.pt>``) this file computes gu of CHILD_CASES with frozen
coefficients and writes them to a file: the parent starts it with PDE_BWD_INPUT=0, where the frozen call must take the
full backward, and compares bitwise."""
import contextlib
import ctypes
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

pytestmark = pytest.mark.gpu

FUSED = [(8, 8), (28, 28), (32, 32)]
ANY = [(6, 6), (50, 50), (128, 128)]
RECT = [(3, 7), (5, 128)]
BATCHES = (1, 33)             # 33: one plane over a 32-plane chunk at N = 32, ragged at the others
CH = 3                        # odd: the XCD-ordered block map has a remainder
SCHEDULES = ("one", "lie2", "strang3", "strang12")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _sweeps(kind, dt=0.02):
    import cnn_with_pde_amd as P
    if kind == "one":
        return [P.Sweep(0, dt / 2, 1.0, 0.0)]
    steps, split = {"lie2": (2, "lie"), "strang3": (3, "strang"), "strang12": (12, "strang")}[kind]
    return [s for st in P.adi_schedule(dt, 1.0, 1.0, steps, split) for s in st]


def _gen(*key):
    return torch.Generator().manual_seed(90001 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _tensors(g, B, H, W, dtype, C=CH, base=1.0, slope=0.5):
    pt = dtype if dtype in (torch.float64, torch.float16) else torch.float32     # (fp16 route: every parameter fp16 too)
    u = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).to(dtype).cuda()
    gy = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).to(dtype).cuda()
    ps = [(base * (1 + 0.15 * torch.randn(C, H, W, generator=g, dtype=torch.float64))).to(pt).cuda() for _ in range(2)]
    ps += [(slope * torch.randn(C, H, W, generator=g, dtype=torch.float64)).to(pt).cuda() for _ in range(2)]
    return u, gy, ps


def _gu(u, gy, ps, sweeps, frozen, emit=None, gtraj=None, **kw):
    """(output, gu, parameter tensors) of one call whose coefficients require grad or not."""
    import cnn_with_pde_amd as P
    ud = u.clone().requires_grad_(True)
    pp = [p.clone().requires_grad_(not frozen) for p in ps]
    kw.setdefault("clamp_max", 10.0)
    if emit is None:
        y = P.adi_diffuse(ud, *pp, sweeps, **kw)
        (gu,) = torch.autograd.grad(y, ud, gy)
    else:
        y = P.adi_diffuse_states(ud, *pp, sweeps, emit, **kw)
        (gu,) = torch.autograd.grad(y, ud, gtraj)
    assert all(p.grad is None for p in pp)
    return y.detach(), gu, pp


def _both(u, gy, ps, sweeps, **kw):
    y0, full, _ = _gu(u, gy, ps, sweeps, False, **kw)
    y1, only, _ = _gu(u, gy, ps, sweeps, True, **kw)
    assert torch.equal(y0, y1)
    assert bool(torch.isfinite(only.double()).all())
    assert torch.equal(only, full), f"{int((only != full).sum())} of {full.numel()} elements of gu differ"
    return only


@pytest.fixture(params=["native", "ctypes"])
def node(request, monkeypatch):
    """The autograd node a square fp32 / bf16 / fp16 call takes: the native one (csrc/host_ext.cpp) or ``_AdiFn``."""
    from cnn_with_pde_amd import _lib as L
    L.load()
    assert L.host_ext() is not None, "the native host path was not built"
    if request.param == "ctypes":
        monkeypatch.setattr(L, "_host", False)
        assert L.host_ext() is None
    return request.param


# ---------------------------------------------------------------------------------------------------- 1. bitwise
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("hw", FUSED + ANY, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frozen_gu_is_bitwise_the_full_backwards(hw, dt, node):
    H, W = hw
    for B in BATCHES:
        for kind in SCHEDULES:
            if H == 128 and kind == "strang12" and B == 33:
                continue                                            # (the same kernel path as B = 1, 36 sweeps of 99 big planes)
            u, gy, ps = _tensors(_gen(H, B, len(kind)), B, H, W, DTYPES[dt])
            _both(u, gy, ps, _sweeps(kind), checkpoints=0)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("hw", RECT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rectangles_bitwise(hw, dt):
    H, W = hw
    for B in BATCHES:
        for kind in SCHEDULES:
            u, gy, ps = _tensors(_gen(H, W, B, len(kind)), B, H, W, DTYPES[dt])
            _both(u, gy, ps, _sweeps(kind), checkpoints=0)


@pytest.mark.parametrize("hw", FUSED + ANY[:2] + [(128, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_float64_bitwise(hw):
    H, W = hw
    for B in BATCHES:
        for kind in SCHEDULES if H < 128 else ("one", "lie2"):
            u, gy, ps = _tensors(_gen(H, B, len(kind), 64), B, H, W, torch.float64)
            _both(u, gy, ps, _sweeps(kind), checkpoints=0)


def _desc(B, C, N, sweeps, **kw):
    from cnn_with_pde_amd import _lib as L
    from cnn_with_pde_amd import functional as F_
    return F_._build_desc(B, C, N, L.PDE_IO_F32, sweeps, kw.get("smooth3", False), kw.get("clamp_max", 10.0), kw.get("eps", 1e-6))


def test_against_the_assembly_backward(node):
    """N = 32, fp32, Strang steps, no checkpoints: the full backward's fast body is the hand-scheduled assembly kernel."""
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    for B in BATCHES:
        sweeps = _sweeps("strang3")
        d = _desc(B, CH, 32, sweeps)
        assert lib.pde_adi_backward_kernel(ctypes.byref(d), 0) == 1
        assert lib.pde_adi_backward_input_kernel(ctypes.byref(d)) == 0
        u, gy, ps = _tensors(_gen(32, B, 1), B, 32, 32, torch.float32)
        _both(u, gy, ps, sweeps, checkpoints=0)


@pytest.mark.parametrize("N", [28, 32])
def test_moving_clamp_masks_on_two_of_four_channels(N, node):
    """base + slope t crosses the clamp floor inside the time window on channels 0 and 1: the full backward hands those
    channels to its masked body (one plane per lane, masks per sweep).  The mask only enters the parameter gradients."""
    g = _gen(N, 4, 4)
    sweeps = _sweeps("strang3", dt=0.05)
    T = 3 * 0.05
    u, gy, ps = _tensors(g, 33, N, N, torch.float32, C=4)
    low = torch.rand(4, N, N, generator=g) < 0.25
    low[2:] = False
    for base, slope in ((ps[0], ps[2]), (ps[1], ps[3])):
        base.copy_(torch.where(low, 0.5 * T * torch.rand(4, N, N, generator=g), base.cpu()).cuda())
        slope.copy_(torch.where(low, -torch.ones(4, N, N), slope.cpu()).cuda())
    _both(u, gy, ps, sweeps, checkpoints=0)
    # the clamp floor is reached on channels 0 and 1 only, and only later in the time window: their masks move
    late = (ps[0] + ps[2] * sweeps[-1].t) < 1e-6
    early = (ps[0] + ps[2] * sweeps[0].t) < 1e-6
    assert bool(late[:2].any()) and not bool(late[2:].any()) and not bool(early.any())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_fashion_sized_coefficients_whose_full_backward_parks_states(dt, node):
    """dt = 0.3 with coefficients near 1: rebuilding states backwards would amplify rounding error, so the full backward
    runs a forward pre-pass and parks states (plan_checkpoints gives a non-empty mask).  The adjoint never reads a state."""
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import functional as F_
    sweeps = [s for st in P.adi_schedule(0.3, 1.0, 1.0, 4) for s in st]
    for B in BATCHES:
        u, gy, ps = _tensors(_gen(28, B, 3), B, 28, 28, DTYPES[dt], C=1, slope=0.05)
        km = F_.kappa_max_async(u, *ps, sweeps, smooth3=True)
        km.event.synchronize()
        assert P.plan_checkpoints(km.host.tolist()) != 0
        _both(u, gy, ps, sweeps, smooth3=True, clamp_max=None, checkpoints="auto")


@pytest.mark.parametrize("hw", [(32, 32), (28, 28), (50, 50), (5, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_visible_eps_scaling(hw, node):
    """eps = 1e-2: the adjoint of the fused kernels carries one factor (1+eps) per undone sweep (3 % per Strang step) and
    resolves it with one multiply at the end, where the full backward does."""
    H, W = hw
    for kind in ("lie2", "strang3", "strang12"):
        u, gy, ps = _tensors(_gen(H, W, len(kind), 2), 33, H, W, torch.float32)
        _both(u, gy, ps, _sweeps(kind), checkpoints=0, eps=1e-2)


CHILD_CASES = [(32, 32, "strang3", "f32"), (28, 28, "lie2", "bf16"), (8, 8, "strang12", "f16"), (50, 50, "strang3", "f32"),
               (3, 7, "lie2", "f32"), (6, 6, "strang3", "f64")]


def _child_case(case):
    H, W, kind, dt = case
    u, gy, ps = _tensors(_gen(H, W, len(kind), 5), 33, H, W, DTYPES[dt])
    return u, gy, ps, _sweeps(kind)


def test_the_switch_restores_the_full_backward(tmp_path):
    out = str(tmp_path / "gu.pt")
    env = dict(os.environ, PDE_BWD_INPUT="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = torch.load(out)
    assert len(got) == len(CHILD_CASES)
    for case, theirs in zip(CHILD_CASES, got):
        u, gy, ps, sweeps = _child_case(case)
        _, mine, _ = _gu(u, gy, ps, sweeps, True, checkpoints=0)
        assert torch.equal(mine.cpu(), theirs), case


# ---------------------------------------------------------------------------------------------------- 2. against fp64
@pytest.mark.parametrize("hw", FUSED + ANY + RECT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_adjoint_identity_in_float64(hw):
    """<F(v), g> = <v, F^T g> with F the library's float64 forward.  Both sides are sums of n products of doubles, each
    side's rounding error bounded by a small multiple of eps64 |F(v)| |g|; held at test_gpu_f64.TOL relative to that scale."""
    import cnn_with_pde_amd as P
    from test_gpu_f64 import TOL
    H, W = hw
    for B in BATCHES:
        for kind in SCHEDULES:
            v, g, ps = _tensors(_gen(H, W, B, len(kind), 8), B, H, W, torch.float64)
            sweeps = _sweeps(kind)
            with torch.no_grad():
                Fv = P.adi_diffuse(v, *ps, sweeps, clamp_max=10.0)
            _, Ftg, _ = _gu(v, g, ps, sweeps, True)
            lhs, rhs = float((Fv * g).sum()), float((v * Ftg).sum())
            scale = float(Fv.norm() * g.norm())
            print(f"{H}x{W} B={B} {kind}: <F v, g> = {lhs:.15e}  <v, F^T g> = {rhs:.15e}  |diff| / scale = {abs(lhs - rhs) / scale:.2e}")
            assert abs(lhs - rhs) <= TOL * scale, (hw, B, kind, lhs, rhs)


@pytest.mark.parametrize("split,steps", [("strang", 3), ("lie", 2)])
@pytest.mark.parametrize("hw", FUSED + [(6, 6), (3, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fp32_gu_against_the_fp64_oracle(hw, split, steps, node):
    import cnn_with_pde_amd as P
    import golden_util as G
    from oracle import pde_oracle as O
    from test_gpu_parity import TOL
    H, W = hw
    dt = 0.02
    u, gy, ps = _tensors(_gen(H, W, steps, 9), 5, H, W, torch.float32)
    sweeps = [s for st in P.adi_schedule(dt, 1.0, 1.0, steps, split) for s in st]
    _, gu, _ = _gu(u, gy, ps, sweeps, True)
    spec = O.AdiSpec(H, CH, dt, 1.0, 1.0, steps, split, False, 10.0, "none", False, 1e-6)
    params = {k: p.double().cpu() for k, p in zip(("alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff"), ps)}
    ud = u.double().cpu().requires_grad_(True)
    (ref,) = torch.autograd.grad(O.adi_forward(ud, params, spec), ud, gy.double().cpu())
    err = G.rel_err(gu.cpu(), ref)
    print(f"{H}x{W} {split}: rel err of gu vs fp64 oracle {err:.2e}")
    assert err <= TOL, err


# ---------------------------------------------------------------------------------------------------- 3. trajectory
@pytest.mark.parametrize("dt", ["f32", "bf16", "f64"])
@pytest.mark.parametrize("hw", [(8, 8), (32, 32), (50, 50), (5, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_trajectory_with_a_cotangent_on_every_state(hw, dt):
    H, W = hw
    for kind in ("lie2", "strang3", "strang12"):
        sweeps = _sweeps(kind)
        S = len(sweeps)
        for emit in ([0], list(range(S - 1)), list(range(0, S - 1, 3))):
            g = _gen(H, W, S, len(emit), 3)
            u, gy, ps = _tensors(g, 33, H, W, DTYPES[dt])
            K = len(emit) + 1                                             # (the last sweep's state is always returned)
            gtraj = torch.randn(K, *u.shape, generator=g, dtype=torch.float64).to(u.dtype).cuda()
            _both(u, gy, ps, sweeps, emit=emit, gtraj=gtraj, checkpoints=0, eps=1e-3)


@pytest.mark.parametrize("hw", [(28, 28), (6, 6), (3, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_trajectory_of_the_last_state_alone_is_the_plain_call(hw):
    H, W = hw
    sweeps = _sweeps("strang3")
    u, gy, ps = _tensors(_gen(H, W, 11), 33, H, W, torch.float32)
    _, plain, _ = _gu(u, gy, ps, sweeps, True)
    _, traj, _ = _gu(u, gy, ps, sweeps, True, emit=[], gtraj=gy[None])
    assert torch.equal(plain, traj)


# ---------------------------------------------------------------------------------------------------- 4. the node
class _Counted:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


@pytest.mark.parametrize("fam,hw,dt", [("pde_adi_", (28, 28), "f32"), ("pde_adi_", (50, 50), "bf16"),
                                       ("pde_adi_rect_", (3, 7), "f32"), ("pde_adi_f64_", (8, 8), "f64"),
                                       ("pde_adi_rect_f64_", (5, 128), "f64")])
@pytest.mark.parametrize("emit", [None, [0, 2]], ids=["plain", "states"])
def test_what_the_python_node_keeps_and_calls(fam, hw, dt, emit, monkeypatch):
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    monkeypatch.setattr(L, "_host", False)                                # the ctypes node for squares too
    H, W = hw
    sweeps = _sweeps("strang3")
    u, gy, ps = _tensors(_gen(H, W, 12), 5, H, W, DTYPES[dt])
    new, old = _Counted(getattr(lib, fam + "backward_input_states")), _Counted(getattr(lib, fam + "backward_states"))
    monkeypatch.setattr(lib, fam + "backward_input_states", new)
    monkeypatch.setattr(lib, fam + "backward_states", old)
    for frozen in (True, False):
        new.calls = old.calls = 0
        ud = u.clone().requires_grad_(True)
        pp = [p.clone().requires_grad_(not frozen) for p in ps]
        if emit is None:
            y = P.adi_diffuse(ud, *pp, sweeps, clamp_max=10.0)
            g = gy
        else:
            y = P.adi_diffuse_states(ud, *pp, sweeps, emit, clamp_max=10.0)
            g = torch.ones_like(y)
        saved = [t for t in y.grad_fn.saved_tensors if t is not None]
        big = [t for t in saved if tuple(t.shape[-4:]) == tuple(u.shape)]
        if frozen:
            assert not big, [tuple(t.shape) for t in saved]               # neither y nor u (nor the trajectory)
            assert len(saved) == 4
        else:
            assert big
        y.backward(g)
        assert (new.calls, old.calls) == ((1, 0) if frozen else (0, 1))
        assert ud.grad is not None and all((p.grad is None) == frozen for p in pp)


def test_the_native_node_keeps_neither_y_nor_u(monkeypatch):
    """The C++ node saves the four coefficient views on the frozen path (six tensors otherwise), takes no coefficient-maxima
    slot under the default policy, and still hands the lagged call's ticket out."""
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L
    from cnn_with_pde_amd import functional as F_
    H_ = L.host_ext()
    assert H_ is not None
    sweeps = _sweeps("strang3")
    u, gy, ps = _tensors(_gen(28, 13), 5, 28, 28, torch.float32)
    for frozen in (True, False):
        ud = u.clone().requires_grad_(True)
        pp = [p.clone().requires_grad_(not frozen) for p in ps]
        y = P.adi_diffuse(ud, *pp, sweeps, clamp_max=10.0)
        assert "AdiFn" in y.grad_fn.name()
        y.backward(gy)
        assert ud.grad is not None and all((p.grad is None) == frozen for p in pp)
    ud = u.clone().requires_grad_(True)
    sink = []
    y = P.adi_diffuse(ud, *ps, sweeps, clamp_max=10.0, checkpoints=0, kmax_sink=sink)
    assert len(sink) == 1                                                 # the lagged call hands its ticket out
    sink[0].event.synchronize()
    km = sink[0].host
    km = km() if callable(km) else km
    ref = F_.kappa_max_async(u, *ps, sweeps, clamp_max=10.0)
    ref.event.synchronize()
    assert torch.allclose(torch.as_tensor(km).float().cpu(), ref.host.cpu(), rtol=1e-6, atol=0)
    (gu,) = torch.autograd.grad(y, ud, gy)
    _, want, _ = _gu(u, gy, ps, sweeps, False, checkpoints=0)
    assert torch.equal(gu, want)


# ---------------------------------------------------------------------------------------------------- 5. repeat, capture
def _dirty():
    """Kernels that use LDS and leave arbitrary bit patterns (NaN payloads included) behind (tests/test_gpu_determinism.py)."""
    x = torch.randn(1 << 16, device="cuda")
    x[::7] = float("nan")
    x.sort()
    torch.cumsum(x, 0)
    (x.view(256, 256) @ x.view(256, 256)).sum()
    torch.softmax(x.view(64, -1), 1)


@pytest.mark.parametrize("hw,dt", [((8, 8), "f32"), ((12, 12), "bf16"), ((20, 20), "f32"), ((28, 28), "f16"), ((32, 32), "f32"),
                                   ((50, 50), "f32"), ((3, 7), "f32")], ids=lambda s: str(s))
def test_repeatable_whatever_is_left_in_lds(hw, dt):
    """Lanes beyond the plane exist for N < 32 and read the wave's image: a run must not depend on what it finds there."""
    H, W = hw
    for kind, emit in (("strang12", None), ("lie2", [0, 2])):
        sweeps = _sweeps(kind)
        g = _gen(H, W, 14)
        u, gy, ps = _tensors(g, 33, H, W, DTYPES[dt])
        gtraj = None if emit is None else torch.randn(len(emit) + 1, *u.shape, generator=g).to(u.dtype).cuda()
        first = None
        for _ in range(3):
            _dirty()
            _, gu, _ = _gu(u, gy, ps, sweeps, True, emit=emit, gtraj=gtraj)
            assert bool(torch.isfinite(gu.float()).all())
            first = gu if first is None else first
            assert torch.equal(gu, first)


def test_frozen_mnist_layer_captured_in_a_graph():
    """Forward + backward of a frozen layer are launches only — no wait for coefficient maxima, no plan — under the
    default checkpoint policy: captured as they are, the replay equals the eager call bitwise."""
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(21)
    layer = quiet(P.MnistDiffusionLayer, 28).cuda()
    with torch.no_grad():
        layer.alpha_base.mul_((1 + 0.2 * torch.randn(layer.alpha_base.shape, generator=g)).cuda())
        layer.beta_time_coeff.copy_((0.5 * torch.randn(layer.beta_time_coeff.shape, generator=g)).cuda())
    for p in layer.parameters():
        p.requires_grad_(False)
    x = torch.randn(33, 1, 28, 28, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(33, 1, 28, 28, generator=g).cuda()

    def fn():
        y = layer(x)
        return (y,) + torch.autograd.grad(y, [x], gy)

    step = P.GraphedStep(fn)
    eager = [t.clone() for t in fn()]
    got = step()
    torch.cuda.synchronize()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    assert all(p.grad is None for p in layer.parameters())


if __name__ == "__main__":
    assert sys.argv[1] == "child" and os.environ.get("PDE_BWD_INPUT") == "0"
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    L._host = False                       # the ctypes node: its calls can be counted
    outs = []
    for case in CHILD_CASES:
        H, W, kind, dt = case
        fam = "pde_adi_" + ("rect_" if H != W else "") + ("f64_" if dt == "f64" else "")
        new, old = _Counted(getattr(lib, fam + "backward_input_states")), _Counted(getattr(lib, fam + "backward_states"))
        setattr(lib, fam + "backward_input_states", new)
        setattr(lib, fam + "backward_states", old)
        u, gy, ps, sweeps = _child_case(case)
        _, gu, _ = _gu(u, gy, ps, sweeps, True, checkpoints=0)
        assert (new.calls, old.calls) == (0, 1), (case, new.calls, old.calls)
        setattr(lib, fam + "backward_input_states", new.fn)
        setattr(lib, fam + "backward_states", old.fn)
        outs.append(gu.cpu())
    L._host = None
    H_ = L.host_ext()                     # and the native node under the same switch: bitwise the ctypes node's
    for case, want in zip(CHILD_CASES, outs):
        if case[0] == case[1] and case[3] != "f64":
            u, gy, ps, sweeps = _child_case(case)
            _, gu, _ = _gu(u, gy, ps, sweeps, True, checkpoints=0)
            assert torch.equal(gu.cpu(), want), case
    torch.cuda.synchronize()
    torch.save(outs, sys.argv[2])
