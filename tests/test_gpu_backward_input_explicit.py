"""GPU: the backward of an explicit 5-point or a Jacobi layer whose parameters take no gradient (the entry points of
include/pdecnn_explicit_input.h).

With frozen alpha_base / channel_scaling (a_row / b_col) the nodes of ``explicit5_step`` / ``explicit5_states`` and
``jacobi_diffuse`` / ``jacobi_diffuse_states`` run the adjoint walk alone.  The contract: what happens to the adjoint is
what the full backward does to it, in its order, so gu is BITWISE the gu of the same call with parameters that require
grad — register planes, float4 and scalar columns, the one-workgroup and the tiled Jacobi kernels, 16-bit tensors,
float64, plain and trajectory calls.  Beside that: the adjoint identity on the float64 route, fp32 against autograd
through the fp64 oracle, what the node keeps alive and which C symbols it calls, the switch, repeatability with dirty
LDS and hipGraph capture.

Run as a script (``python test_gpu_backward_input_explicit.py child <out.pt>``) this file computes gu of CHILD_CASES with
frozen parameters and writes them to a file: the parent starts it with PDE_BWD_INPUT=0, where the frozen call must take
the full backward, and compares bitwise."""
import contextlib
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

WAVE = [(2, 2, 16, 16), (2, 2, 32, 32), (1, 3, 64, 64)]      # three planes leave a ragged last workgroup
VEC4 = [(2, 2, 8, 8), (1, 2, 12, 20)]
COLS = [(2, 2, 5, 7), (1, 2, 1, 5), (1, 2, 3, 1)]
JAC_ONE = [(2, 4, 4), (2, 8, 8), (2, 5, 9), (1, 48, 48), (1, 64, 64)]
JAC_TILED = [(1, 65, 65), (1, 70, 66), (2, 64, 130), (1, 129, 65)]   # 65: ring cell and folded row in different tiles
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
EX_KW = dict(dt=0.01, eps=1e-6, max_coeff=0.15, relax=0.1)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _gen(*key):
    return torch.Generator().manual_seed(70001 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _ptype(dtype):
    return dtype if dtype in (torch.float64, torch.float16) else torch.float32   # (fp16 route: every parameter fp16 too)


def _ex_tensors(g, shape, dtype):
    C = shape[1]
    u = torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype).cuda()
    gy = torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype).cuda()
    a = (0.05 * (1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64))).to(_ptype(dtype)).cuda()
    s = (1 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)).to(_ptype(dtype)).cuda()
    return u, gy, [a, s]


def _jac_tensors(g, shape, dtype):
    B, H, W = shape
    u = torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype).cuda()
    gy = torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype).cuda()
    a = (0.1 * (1 + 0.3 * torch.randn(H, generator=g, dtype=torch.float64))).to(_ptype(dtype)).cuda()
    b = (0.1 * (1 + 0.3 * torch.randn(W, generator=g, dtype=torch.float64))).to(_ptype(dtype)).cuda()
    return u, gy, [a, b]


def _gtraj(g, steps, u):
    return torch.randn(len(steps), *u.shape, generator=g, dtype=torch.float64).to(u.dtype).cuda()


def _gu(fam, u, gy, ps, n, frozen, steps=None, gtraj=None):
    """(output, gu) of one call whose parameters require grad or not.  ``n``: the step count of a plain call."""
    from cnn_with_pde_amd import functional as F_
    ud = u.clone().requires_grad_(True)
    pp = [p.clone().requires_grad_(not frozen) for p in ps]
    if fam == "explicit":
        y = F_.explicit5_step(ud, *pp, num_steps=n, **EX_KW) if steps is None else F_.explicit5_states(ud, *pp, steps=steps, **EX_KW)
    else:
        y = F_.jacobi_diffuse(ud, *pp, n) if steps is None else F_.jacobi_diffuse_states(ud, *pp, steps)
    (gu,) = torch.autograd.grad(y, ud, gy if steps is None else gtraj)
    assert all(p.grad is None for p in pp)
    return y.detach(), gu


def _both(fam, u, gy, ps, n, **kw):
    y0, full = _gu(fam, u, gy, ps, n, False, **kw)
    y1, only = _gu(fam, u, gy, ps, n, True, **kw)
    assert torch.equal(y0, y1)
    assert bool(torch.isfinite(only.double()).all())
    assert only.dtype == full.dtype and only.shape == full.shape
    assert torch.equal(only, full), f"{int((only != full).sum())} of {full.numel()} elements of gu differ"
    return only


def _plain_and_trajectories(fam, make, shape, dtype, counts):
    for n in counts:
        g = _gen(*shape, n, 1)
        u, gy, ps = make(g, shape, dtype)
        _both(fam, u, gy, ps, n)
    if max(counts) < 3:
        return
    # a cotangent on every emitted state; (3,) alone is the plain call of three steps
    g = _gen(*shape, 2)
    u, gy, ps = make(g, shape, dtype)
    gt = _gtraj(g, (1, 3), u)
    _both(fam, u, gy, ps, None, steps=(1, 3), gtraj=gt)
    alone = _both(fam, u, gy, ps, None, steps=(3,), gtraj=gt[1:])
    _, plain = _gu(fam, u, gt[1], ps, 3, True)
    assert torch.equal(alone, plain)


# ---------------------------------------------------------------------------------------------------- 1. bitwise
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", WAVE + VEC4 + COLS, ids=lambda s: "x".join(map(str, s)))
def test_explicit_frozen_gu_is_bitwise_the_full_backwards(shape, dt):
    _plain_and_trajectories("explicit", _ex_tensors, shape, DTYPES[dt], (1, 2, 3))


@pytest.mark.parametrize("shape", [(2, 2, 5, 7), (2, 2, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_explicit_float64_bitwise(shape):
    _plain_and_trajectories("explicit", _ex_tensors, shape, torch.float64, (1, 2, 3))


@pytest.mark.parametrize("shape,dt", [((2, 2, 16, 16), "f32"), ((2, 2, 8, 8), "bf16"), ((2, 2, 5, 7), "f32"),
                                      ((2, 2, 5, 7), "f64")], ids=lambda s: str(s))
def test_explicit_plain_call_of_130_steps(shape, dt):
    """More steps than the emission mask has bits: a plain call takes any count."""
    u, gy, ps = _ex_tensors(_gen(*shape, 130), shape, DTYPES[dt])
    _both("explicit", u, gy, ps, 130)


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("shape", JAC_ONE, ids=lambda s: "x".join(map(str, s)))
def test_jacobi_one_workgroup_bitwise(shape, dt):
    _plain_and_trajectories("jacobi", _jac_tensors, shape, DTYPES[dt], (0, 1, 3))


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("shape", JAC_TILED, ids=lambda s: "x".join(map(str, s)))
def test_jacobi_tiled_bitwise(shape, dt):
    from cnn_with_pde_amd import _lib as L
    assert L.load().pde_jacobi_plane_path(shape[1], shape[2]) == 2
    _plain_and_trajectories("jacobi", _jac_tensors, shape, DTYPES[dt], (0, 1, 3, 10, 11, 21))
    # a trajectory that straddles a launch boundary (10 steps per launch)
    g = _gen(*shape, 12)
    u, gy, ps = _jac_tensors(g, shape, DTYPES[dt])
    _both("jacobi", u, gy, ps, None, steps=(5, 12), gtraj=_gtraj(g, (5, 12), u))


@pytest.mark.parametrize("shape", JAC_ONE, ids=lambda s: "x".join(map(str, s)))
def test_jacobi_float64_bitwise(shape):
    _plain_and_trajectories("jacobi", _jac_tensors, shape, torch.float64, (0, 1, 3))


def test_jacobi_plain_call_of_130_steps():
    for shape in ((2, 5, 9), (1, 65, 65)):
        u, gy, ps = _jac_tensors(_gen(*shape, 130), shape, torch.float32)
        _both("jacobi", u, gy, ps, 130)


CHILD_CASES = [("explicit", (1, 3, 64, 64), "f32", 3), ("explicit", (1, 2, 12, 20), "bf16", 3), ("explicit", (2, 2, 5, 7), "f16", 2),
               ("explicit", (2, 2, 5, 7), "f64", 3), ("jacobi", (2, 5, 9), "f32", 3), ("jacobi", (1, 70, 66), "f16", 11),
               ("jacobi", (2, 8, 8), "f64", 3)]


def _child_case(case):
    fam, shape, dt, n = case
    make = _ex_tensors if fam == "explicit" else _jac_tensors
    return make(_gen(*shape, n, 5), shape, DTYPES[dt])


def test_the_switch_restores_the_full_backward(tmp_path):
    out = str(tmp_path / "gu.pt")
    env = dict(os.environ, PDE_BWD_INPUT="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = torch.load(out)
    assert len(got) == len(CHILD_CASES)
    for case, theirs in zip(CHILD_CASES, got):
        u, gy, ps = _child_case(case)
        _, mine = _gu(case[0], u, gy, ps, case[3], True)
        assert torch.equal(mine.cpu(), theirs), case


# ---------------------------------------------------------------------------------------------------- 2. against fp64
@pytest.mark.parametrize("fam,shape", [("explicit", s) for s in WAVE + VEC4 + COLS] + [("jacobi", s) for s in JAC_ONE],
                         ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_adjoint_identity_in_float64(fam, shape):
    """<F(v), g> = <v, F^T g> with F the library's float64 forward.  Both sides are sums of n products of doubles, each
    side's rounding error bounded by a small multiple of eps64 |F(v)| |g|; held at test_gpu_f64.TOL (1e-11, the bound of
    tests/test_gpu_backward_input.py) relative to that scale."""
    import cnn_with_pde_amd as P
    from test_gpu_f64 import TOL
    from cnn_with_pde_amd import functional as F_
    make = _ex_tensors if fam == "explicit" else _jac_tensors
    for n in (1, 3):
        v, g, ps = make(_gen(*shape, n, 8), shape, torch.float64)
        with torch.no_grad():
            Fv = F_.explicit5_step(v, *ps, num_steps=n, **EX_KW) if fam == "explicit" else F_.jacobi_diffuse(v, *ps, n)
        _, Ftg = _gu(fam, v, g, ps, n, True)
        lhs, rhs = float((Fv * g).sum()), float((v * Ftg).sum())
        scale = float(Fv.norm() * g.norm())
        print(f"{fam} {shape} n={n}: <F v, g> = {lhs:.15e}  <v, F^T g> = {rhs:.15e}  |diff| / scale = {abs(lhs - rhs) / scale:.2e}")
        assert abs(lhs - rhs) <= TOL * scale, (fam, shape, n, lhs, rhs)


@pytest.mark.parametrize("fam,shape", [("explicit", s) for s in WAVE + VEC4 + COLS] + [("jacobi", s) for s in JAC_ONE + JAC_TILED],
                         ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_fp32_gu_against_the_fp64_oracle(fam, shape):
    import golden_util as G
    from oracle import pde_oracle as O
    from test_gpu_parity import TOL
    n = 3 if fam == "explicit" or shape[1] <= 64 else 11
    u, gy, ps = (_ex_tensors if fam == "explicit" else _jac_tensors)(_gen(*shape, 9), shape, torch.float32)
    _, gu = _gu(fam, u, gy, ps, n, True)
    ud = u.double().cpu().requires_grad_(True)
    p64 = [p.double().cpu() for p in ps]
    if fam == "explicit":
        y = O.tiny_forward(ud, {"alpha_base": p64[0], "channel_scaling": p64[1]}, dt=EX_KW["dt"], num_steps=n, eps=EX_KW["eps"],
                           max_coeff=EX_KW["max_coeff"], relax=EX_KW["relax"])
    else:
        y = O.jacobi_forward(ud, p64[0], p64[1], n)
    (ref,) = torch.autograd.grad(y, ud, gy.double().cpu())
    err = G.rel_err(gu.cpu(), ref)
    print(f"{fam} {shape} n={n}: rel err of gu vs fp64 oracle {err:.2e}")
    assert err <= TOL, err


# ---------------------------------------------------------------------------------------------------- 3. the node
class _Counted:
    def __init__(self, fn):
        self.fn, self.calls, self.args = fn, 0, None

    def __call__(self, *a):
        self.calls += 1
        self.args = a
        return self.fn(*a)


NODE_CASES = [("pde_explicit5_", "explicit", (2, 2, 16, 16), "f32"), ("pde_explicit5_", "explicit", (1, 2, 12, 20), "bf16"),
              ("pde_explicit5_", "explicit", (2, 2, 5, 7), "f32"), ("pde_explicit5_f64_", "explicit", (2, 2, 16, 16), "f64"),
              ("pde_jacobi_io_", "jacobi", (2, 5, 9), "f32"), ("pde_jacobi_io_", "jacobi", (1, 70, 66), "f16"),
              ("pde_jacobi_f64_", "jacobi", (2, 8, 8), "f64")]


@pytest.mark.parametrize("sym,fam,shape,dt", NODE_CASES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
@pytest.mark.parametrize("steps", [None, (1, 3)], ids=["plain", "states"])
def test_what_the_python_node_keeps_and_calls(sym, fam, shape, dt, steps, monkeypatch):
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L
    from cnn_with_pde_amd import functional as F_
    lib = L.load()
    u, gy, ps = (_ex_tensors if fam == "explicit" else _jac_tensors)(_gen(*shape, 12), shape, DTYPES[dt])
    fwd = _Counted(getattr(lib, sym + "forward_states"))
    new, old = _Counted(getattr(lib, sym + "backward_input_states")), _Counted(getattr(lib, sym + "backward_states"))
    monkeypatch.setattr(lib, sym + "forward_states", fwd)
    monkeypatch.setattr(lib, sym + "backward_input_states", new)
    monkeypatch.setattr(lib, sym + "backward_states", old)
    wave = fam == "explicit" and dt != "f64" and shape[2:] in ((16, 16), (32, 32), (64, 64))
    states_arg = 13 if dt != "f64" else 12                    # `states` of pde_explicit5[_f64]_forward_states

    def call(ud, pp):
        if fam == "explicit":
            return F_.explicit5_step(ud, *pp, num_steps=3, **EX_KW) if steps is None else F_.explicit5_states(ud, *pp, steps=steps, **EX_KW)
        return F_.jacobi_diffuse(ud, *pp, 3) if steps is None else F_.jacobi_diffuse_states(ud, *pp, steps)

    for frozen in (True, False):
        fwd.calls = new.calls = old.calls = 0
        ud = u.clone().requires_grad_(True)
        pp = [p.clone().requires_grad_(not frozen) for p in ps]
        y = call(ud, pp)
        assert fwd.calls == 1
        if fam == "explicit":
            parked = fwd.args[states_arg].value
            assert (parked is None) == (frozen and wave)                 # a frozen register-plane forward writes no state
        saved = [t for t in y.grad_fn.saved_tensors if t is not None]
        big = [t for t in saved if tuple(t.shape[-len(shape):]) == tuple(shape)]
        if frozen:
            assert not big, [tuple(t.shape) for t in saved]               # neither u nor the states
            assert len(saved) == 2
        else:
            assert big
        y.backward(gy if steps is None else torch.ones_like(y))
        assert (new.calls, old.calls) == ((1, 0) if frozen else (0, 1))
        assert ud.grad is not None and all((p.grad is None) == frozen for p in pp)
    # under no_grad: the forward alone, with what it parked before (nothing on register planes)
    fwd.calls = new.calls = old.calls = 0
    with torch.no_grad():
        call(u, ps)
    assert (fwd.calls, new.calls, old.calls) == (1, 0, 0)
    if fam == "explicit":
        assert (fwd.args[states_arg].value is None) == wave


# ---------------------------------------------------------------------------------------------------- 4. repeat, capture
def _dirty():
    """Kernels that use LDS and leave arbitrary bit patterns (NaN payloads included) behind (tests/test_gpu_determinism.py)."""
    x = torch.randn(1 << 16, device="cuda")
    x[::7] = float("nan")
    x.sort()
    torch.cumsum(x, 0)
    (x.view(256, 256) @ x.view(256, 256)).sum()
    torch.softmax(x.view(64, -1), 1)


@pytest.mark.parametrize("fam,shape,dt,n", [("explicit", (1, 3, 64, 64), "f32", 3), ("explicit", (2, 2, 16, 16), "bf16", 3),
                                            ("explicit", (1, 2, 12, 20), "f16", 3), ("explicit", (2, 2, 5, 7), "f32", 3),
                                            ("explicit", (2, 2, 5, 7), "f64", 3), ("jacobi", (2, 5, 9), "f32", 3),
                                            ("jacobi", (1, 64, 64), "f16", 3), ("jacobi", (1, 70, 66), "f32", 12),
                                            ("jacobi", (2, 8, 8), "f64", 3)], ids=lambda s: str(s))
def test_repeatable_whatever_is_left_in_lds(fam, shape, dt, n):
    """The Jacobi kernels keep the adjoint in LDS and never read a cell they did not write; a run must not depend on what
    it finds there (nor on what the registers of the explicit kernels held)."""
    make = _ex_tensors if fam == "explicit" else _jac_tensors
    for steps in (None, (1, n)):
        g = _gen(*shape, 14)
        u, gy, ps = make(g, shape, DTYPES[dt])
        gtraj = None if steps is None else _gtraj(g, steps, u)
        first = None
        for _ in range(3):
            _dirty()
            _, gu = _gu(fam, u, gy, ps, n, True, steps=steps, gtraj=gtraj)
            assert bool(torch.isfinite(gu.double()).all())
            first = gu if first is None else first
            assert torch.equal(gu, first)


@pytest.mark.parametrize("which", ["PDELayer", "ImprovedDiffusionLayer"])
def test_frozen_layer_captured_in_a_graph(which):
    """Forward + backward of a frozen layer are launches only: captured as they are (``GraphedStep``: a
    ``torch.cuda.graph`` capture under the package's capture guard, which lets the autograd worker release the captured
    backward before the capture ends), the replay equals the eager call bitwise.  The queue count is the machine's."""
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(23)
    if which == "PDELayer":
        layer = quiet(P.PDELayer).cuda()
        shape = (5, 1, 48, 48)
    else:
        layer = quiet(P.ImprovedDiffusionLayer, 64, 3, num_steps=3).cuda()
        shape = (5, 3, 64, 64)
    for p in layer.parameters():
        p.requires_grad_(False)
    x = torch.randn(*shape, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(*shape, generator=g).cuda()

    def fn():
        y = layer(x)
        return (y,) + torch.autograd.grad(y, [x], gy)

    step = P.GraphedStep(fn)
    eager = [t.clone() for t in fn()]
    got = step()
    torch.cuda.synchronize()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    got = step()
    torch.cuda.synchronize()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    assert all(p.grad is None for p in layer.parameters())


if __name__ == "__main__":
    assert sys.argv[1] == "child" and os.environ.get("PDE_BWD_INPUT") == "0"
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    outs = []
    for case in CHILD_CASES:
        fam, shape, dt, n = case
        sym = ("pde_explicit5_" if fam == "explicit" else "pde_jacobi_io_") if dt != "f64" else \
            ("pde_explicit5_f64_" if fam == "explicit" else "pde_jacobi_f64_")
        new, old = _Counted(getattr(lib, sym + "backward_input_states")), _Counted(getattr(lib, sym + "backward_states"))
        setattr(lib, sym + "backward_input_states", new)
        setattr(lib, sym + "backward_states", old)
        u, gy, ps = _child_case(case)
        _, gu = _gu(fam, u, gy, ps, n, True)
        assert (new.calls, old.calls) == (0, 1), (case, new.calls, old.calls)
        setattr(lib, sym + "backward_input_states", new.fn)
        setattr(lib, sym + "backward_states", old.fn)
        outs.append(gu.cpu())
    torch.cuda.synchronize()
    torch.save(outs, sys.argv[2])
