"""The trajectory of the two explicit layers' time loops: ``jacobi_diffuse_states`` (PDELayer's loop: one-workgroup and
tiled Jacobi kernels) and ``explicit5_states`` (ImprovedDiffusionLayer's: wave-per-plane and generic explicit kernels), the
states after chosen time steps out of the launches of the plain call, differentiable in every state.

The reference is the fp64 oracle as it stands: a ``torch.stack`` of ``O.jacobi_forward(..., k)`` / ``O.tiny_forward(...,
num_steps=k)`` over the chosen k, differentiated by ``O.value_and_grads`` with a random cotangent of the stacked shape.
Metric ``golden_util.rel_err``; bounds imported: test_gpu_parity.TOL (1e-5) for fp32 — the fp32 oracle itself is within
3e-7 of the fp64 one on all four figures of every shape below — and test_gpu_f64.TOL for float64.  Inputs follow
``_jacobi_case`` and ``_ex_case`` of test_gpu_explicit_shapes.py.  Where the arithmetic is exact (small integers, dyadic
coefficients) the results must equal the fp32 oracle bit for bit, and every returned state must equal the plain call of
that many steps bit for bit."""
import ctypes as C
import functools

import pytest
import torch

import golden_util as G
import test_gpu_explicit_shapes as XS
from oracle import pde_oracle as O
from test_gpu_f16 import max_ulps
from test_gpu_f64 import TOL as TOL64
from test_gpu_jacobi_tiled import _K, _ord16
from test_gpu_parity import TOL             # 1e-5

pytestmark = pytest.mark.gpu

J_SMALL = [(5, 7, 9, tuple(range(1, 11)), None), (3, 64, 64, (1, 5, 10), None), (1, 4, 4, (1, 2), None),
           (3, 33, 31, (2, 7), 10)]                                   # (B, H, W, steps, nt of the case's seed)
J_TILED = [(2, 97, 130, "seams", None), (3, 65, 8, (1, 2, 3), None), (2, 129, 65, (3, 7), None)]
EX_WAVE = [(16, 16, (1, 2, 3)), (32, 32, (1, 3)), (64, 64, (2, 3))]
EX_GENERIC = [(20, 36, (1, 2, 3)), (33, 31, (1, 3)), (5, 1, (1, 2, 3))]
_ids = lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)     # noqa: E731


def _steps(steps):
    """"seams": an emission at a launch's last step, at the next launch's first step, and `out` after a remainder launch"""
    return (1, _K(), _K() + 1, 2 * _K() + 3) if steps == "seams" else tuple(steps)


# ---- inputs and references (computed once per case) ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _jac_inputs(B, H, W, steps, nt=None, dtype=torch.float32):
    u, _, A, Bc = XS._jacobi_case(B, H, W, steps[-1] if nt is None else nt, dtype)
    g = torch.Generator().manual_seed(7000 * H + W + len(steps))
    return u, torch.randn((len(steps), B, H, W), generator=g, dtype=dtype), A, Bc


def _jac_oracle(u, gy, A, Bc, steps, dtype):
    y, gu, gp = O.value_and_grads(lambda x, p: torch.stack([O.jacobi_forward(x, p["A"], p["B"], k) for k in steps]),
                                  u.to(dtype), {"A": A.to(dtype), "B": Bc.to(dtype)}, gy.to(dtype))
    return y, gu, gp["A"], gp["B"]


@functools.lru_cache(maxsize=None)
def _jac_ref(B, H, W, steps, nt=None):
    return _jac_oracle(*_jac_inputs(B, H, W, steps, nt), steps, torch.float64)


def _jac_gpu(u, gy, A, Bc, steps):
    import cnn_with_pde_amd as P
    ud, Ad, Bd = (t.cuda().requires_grad_(True) for t in (u, A, Bc))
    y = P.jacobi_diffuse_states(ud, Ad, Bd, steps)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    return y.detach(), ud.grad, Ad.grad, Bd.grad


@functools.lru_cache(maxsize=None)
def _ex_inputs(H, W, steps, dtype=torch.float32):
    u, _, a, s = XS._ex_case(H, W, dtype)
    g = torch.Generator().manual_seed(7000 * H + W + len(steps))
    gy = torch.randn((len(steps),) + tuple(u.shape), generator=g)
    if dtype in (torch.float16, torch.bfloat16):
        gy = gy.to(dtype).float()
    return u, gy, a, s


def _ex_oracle(u, gy, a, s, steps, dtype, relax=XS.EX_RELAX, dt=XS.EX_DT, eps=XS.EX_EPS, maxc=XS.EX_MAXC):
    y, gu, gp = O.value_and_grads(
        lambda x, p: torch.stack([O.tiny_forward(x, p, dt=dt, num_steps=k, eps=eps, max_coeff=maxc, relax=relax)
                                  for k in steps]),
        u.to(dtype), {"alpha_base": a.to(dtype), "channel_scaling": s.to(dtype)}, gy.to(dtype))
    return y, gu, gp["alpha_base"], gp["channel_scaling"]


@functools.lru_cache(maxsize=None)
def _ex_ref(H, W, steps):
    return _ex_oracle(*_ex_inputs(H, W, steps), steps, torch.float64)


def _ex_gpu(u, gy, a, s, steps, relax=XS.EX_RELAX, dt=XS.EX_DT, eps=XS.EX_EPS, maxc=XS.EX_MAXC):
    import cnn_with_pde_amd as P
    ud, ad, sd = (t.cuda().requires_grad_(True) for t in (u, a, s))
    y = P.explicit5_states(ud, ad, sd, dt, eps, maxc, relax, steps)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    return y.detach(), ud.grad, ad.grad, sd.grad


def _hold(tag, names, got, ref, tol):
    errs = {n: G.rel_err(x.cpu(), r) for n, x, r in zip(names, got, ref)}
    print(tag, errs)
    bad = {n: v for n, v in errs.items() if not v <= tol}
    assert not bad, (bad, errs)


J_NAMES = ("states", "gu", "gA", "gB")
EX_NAMES = ("states", "gu", "g_alpha_base", "g_channel_scaling")


# ---- 1, 2: the Jacobi kernels against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,steps,nt", J_SMALL, ids=_ids)
def test_jacobi_small_vs_oracle(B, H, W, steps, nt):
    from cnn_with_pde_amd import _lib as L
    assert L.load().pde_jacobi_plane_path(H, W) == 1
    got = _jac_gpu(*_jac_inputs(B, H, W, steps, nt), steps)
    assert got[0].shape == (len(steps), B, H, W) and all(t.dtype == torch.float32 for t in got)
    _hold((B, H, W, steps), J_NAMES, got, _jac_ref(B, H, W, steps, nt), TOL)


@pytest.mark.parametrize("B,H,W,steps,nt", J_TILED, ids=_ids)
def test_jacobi_tiled_vs_oracle(B, H, W, steps, nt):
    from cnn_with_pde_amd import _lib as L
    steps = _steps(steps)
    assert L.load().pde_jacobi_plane_path(H, W) == 2
    got = _jac_gpu(*_jac_inputs(B, H, W, steps, nt), steps)
    assert got[0].shape == (len(steps), B, H, W)
    _hold((B, H, W, steps), J_NAMES, got, _jac_ref(B, H, W, steps, nt), TOL)


# ---- 3: exact Jacobi ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,steps", [(3, 12, 9, (1, 2, 3)), (2, 64, 64, (1, 3)), (2, 65, 8, (1, 2, 3)),
                                         (2, 97, 130, (2, 3))], ids=_ids)
def test_jacobi_exact(B, H, W, steps):
    """test_gpu_jacobi_tiled.test_exact_seams with a cotangent on every returned state: a = b = 1/4 and small integers,
    every intermediate a short dyadic number, so states, gu, gA and gB must equal the oracle's bit for bit — an injection
    that misses a halo cell, lands on a ring cell or is added twice at a tile seam fails whatever the tolerance."""
    g = torch.Generator().manual_seed(H * 1000 + W)
    u = torch.randint(-2, 3, (B, H, W), generator=g).float()
    gy = torch.randint(-2, 3, (len(steps), B, H, W), generator=g).float()
    A, Bc = torch.full((H,), 0.25), torch.full((W,), 0.25)
    ref32 = _jac_oracle(u, gy, A, Bc, steps, torch.float32)
    ref64 = _jac_oracle(u, gy, A, Bc, steps, torch.float64)
    for r32, r64 in zip(ref32, ref64):                                  # the precondition
        assert torch.equal(r32.double(), r64)
    got = [t.cpu() for t in _jac_gpu(u, gy, A, Bc, steps)]
    for n, x, r in zip(J_NAMES, got, ref32):
        assert torch.equal(x, r), (n, "first index, got, want, how many:", XS._first_diff(x, r))


# ---- 4: explicit against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,steps", EX_WAVE + EX_GENERIC, ids=_ids)
def test_explicit_vs_oracle(H, W, steps):
    got = _ex_gpu(*_ex_inputs(H, W, steps), steps)
    u = _ex_inputs(H, W, steps)[0]
    assert got[0].shape == (len(steps),) + tuple(u.shape) and all(t.dtype == torch.float32 for t in got)
    _hold((H, W, steps), EX_NAMES, got, _ex_ref(H, W, steps), TOL)
    assert float(got[2][1]) == 0.0 and float(got[2][2]) == 0.0 and float(got[2][0]) != 0.0     # the clamp mask itself


# ---- 5: exact explicit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,steps", [(32, 32, (1, 2, 3)), (20, 36, (1, 2, 3)), (7, 9, (1, 2, 3)), (33, 31, (1, 3))], ids=_ids)
def test_explicit_exact(H, W, steps):
    """test_gpu_explicit_shapes.test_explicit_exact with a cotangent on every returned state."""
    kw = dict(relax=0.5, dt=1.0, eps=1e-6, maxc=1.0)
    g = torch.Generator().manual_seed(H * 1000 + W)
    u = torch.randint(-2, 3, (2, 3, H, W), generator=g).float()
    gy = torch.randint(-2, 3, (len(steps), 2, 3, H, W), generator=g).float()
    a, s = torch.full((3,), 0.125), torch.tensor([1.0, 2.0, 0.5])
    ref32 = _ex_oracle(u, gy, a, s, steps, torch.float32, **kw)
    ref64 = _ex_oracle(u, gy, a, s, steps, torch.float64, **kw)
    for r32, r64 in zip(ref32, ref64):                                  # the precondition
        assert torch.equal(r32.double(), r64)
    got = [t.cpu() for t in _ex_gpu(u, gy, a, s, steps, **kw)]
    for n, x, r in zip(EX_NAMES, got, ref32):
        assert torch.equal(x, r), (n, "first index, got, want, how many:", XS._first_diff(x, r))


# ---- 6: every state is the plain call of that many steps, bit for bit -----------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=str)
@pytest.mark.parametrize("B,H,W,steps,nt", J_SMALL + J_TILED, ids=_ids)
def test_jacobi_states_are_the_plain_calls(B, H, W, steps, nt, dtype):
    import cnn_with_pde_amd as P
    steps = _steps(steps)
    u, _, A, Bc = (t.to(dtype).cuda() for t in _jac_inputs(B, H, W, steps, nt))
    with torch.no_grad():
        traj = P.jacobi_diffuse_states(u, A, Bc, steps)
        plain = [P.jacobi_diffuse(u, A, Bc, k) for k in steps]
    grad = P.jacobi_diffuse_states(u.clone().requires_grad_(True), A.clone().requires_grad_(True),
                                   Bc.clone().requires_grad_(True), steps)
    torch.cuda.synchronize()
    assert traj.dtype == dtype and traj.shape == (len(steps), B, H, W) and not traj.requires_grad and grad.requires_grad
    for i, k in enumerate(steps):
        assert traj[i].is_contiguous()
        assert torch.equal(traj[i], plain[i]), (k, XS._first_diff(traj[i].float().cpu(), plain[i].float().cpu()))
    assert torch.equal(traj, grad.detach())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("H,W,steps", EX_WAVE + EX_GENERIC, ids=_ids)
def test_explicit_states_are_the_plain_calls(H, W, steps, dtype):
    import cnn_with_pde_amd as P
    u, _, a, s = (t.cuda() for t in _ex_inputs(H, W, steps, dtype))
    u = u.to(dtype)
    if dtype == torch.float16:                                         # the float16 route: every tensor of the call fp16
        a, s = a.half(), s.half()
    cfg = (XS.EX_DT, XS.EX_EPS, XS.EX_MAXC, XS.EX_RELAX)
    with torch.no_grad():
        traj = P.explicit5_states(u, a, s, *cfg, steps)
        plain = [P.explicit5_step(u, a, s, *cfg, k) for k in steps]
    grad = P.explicit5_states(u.clone().requires_grad_(True), a.clone().requires_grad_(True), s.clone().requires_grad_(True),
                              *cfg, steps)
    torch.cuda.synchronize()
    assert traj.dtype == dtype and traj.shape == (len(steps),) + tuple(u.shape)
    for i, k in enumerate(steps):
        assert traj[i].is_contiguous()
        assert torch.equal(traj[i], plain[i]), (k, XS._first_diff(traj[i].float().cpu(), plain[i].float().cpu()))
    assert torch.equal(traj, grad.detach())


# ---- 7: 16-bit tensors through the C ABI against the fp32 route -------------------------------------------------------------
def _mask(steps):
    bits = sum(1 << (k - 1) for k in steps[:-1])
    return (C.c_uint64 * 2)(bits & (2 ** 64 - 1), bits >> 64)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _fp(t):
    return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_float))


def _jac_cabi(io_dtype, u, gy, a, b, steps):
    """pde_jacobi_io_forward_states / _backward_states on tensors of any of the three I/O types"""
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    B, H, W = u.shape
    nt, K = steps[-1], len(steps)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    traj = torch.empty((K,) + tuple(u.shape), dtype=u.dtype, device="cuda")
    gu, ga, gb = torch.empty_like(u), torch.empty_like(a), torch.empty_like(b)
    nf = lib.pde_jacobi_forward_workspace_bytes(B, H, W, nt)
    fws = torch.empty(max(nf, 1), dtype=torch.uint8, device="cuda")
    assert lib.pde_jacobi_io_forward_states(B, H, W, nt, io_dtype, _p(u), _fp(a), _fp(b), _p(traj[K - 1]), _p(traj),
                                            _mask(steps), _p(fws), nf, st) == 0
    nb = lib.pde_jacobi_io_backward_workspace_bytes(B, H, W, nt, io_dtype)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    assert lib.pde_jacobi_io_backward_states(B, H, W, nt, io_dtype, _p(u), _p(gy[K - 1]), _p(gy), _mask(steps), _fp(a), _fp(b),
                                             _p(gu), _fp(ga), _fp(gb), _p(ws), nb, st) == 0
    torch.cuda.synchronize()
    return traj, gu, ga, gb


@pytest.mark.parametrize("narrow", [torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("B,H,W", [(4, 7, 9), (3, 65, 8)], ids=_ids)
def test_jacobi_narrow_io(B, H, W, narrow):
    """the gates of test_gpu_explicit_shapes._jacobi_narrow: states and gu the fp32 route's rounded once (1 ulp), the
    coefficient gradients the same fp32 sums over the same widened values"""
    from cnn_with_pde_amd import _lib as L
    steps = (1, 2, 3)
    io_dtype = L.PDE_IO_BF16 if narrow == torch.bfloat16 else L.PDE_IO_F16
    u, gy, a, b = _jac_inputs(B, H, W, steps)
    u, gy, a, b = u.to(narrow).cuda(), gy.to(narrow).cuda().contiguous(), a.cuda(), b.cuda()
    y, gu, ga, gb = _jac_cabi(io_dtype, u, gy, a, b, steps)
    y32, gu32, ga32, gb32 = _jac_cabi(L.PDE_IO_F32, u.float(), gy.float(), a, b, steps)
    assert y.dtype == narrow and gu.dtype == narrow and y32.dtype == torch.float32
    dy = int((_ord16(y) - _ord16(y32.to(narrow))).abs().max())
    dg = int((_ord16(gu) - _ord16(gu32.to(narrow))).abs().max())
    ea, eb = G.rel_err(ga.cpu(), ga32.cpu()), G.rel_err(gb.cpu(), gb32.cpu())
    print((B, H, W, narrow), dy, dg, ea, eb)
    assert dy <= 1 and dg <= 1
    assert ea <= 1e-6 and eb <= 1e-6


def _ex_cabi(io_dtype, u, gy, a, s, steps):
    """pde_explicit5_forward_states / _backward_states on tensors of any of the three I/O types"""
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    B, Cc, H, W = u.shape
    n, K = steps[-1], len(steps)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    traj = torch.empty((K,) + tuple(u.shape), dtype=u.dtype, device="cuda")
    gu, ga, gs = torch.empty_like(u), torch.empty_like(a), torch.empty_like(s)
    states = torch.empty((max(n - 1, 1),) + tuple(u.shape), dtype=torch.float32, device="cuda")
    cfg = (XS.EX_DT, XS.EX_EPS, XS.EX_MAXC, XS.EX_RELAX)
    assert lib.pde_explicit5_forward_states(B, Cc, H, W, io_dtype, _p(u), _fp(a), _fp(s), *cfg, n, _p(states), _p(traj[K - 1]),
                                            _p(traj), _mask(steps), st) == 0
    nb = lib.pde_explicit5_backward_workspace_bytes(B, Cc, H, W, io_dtype, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    assert lib.pde_explicit5_backward_states(B, Cc, H, W, io_dtype, _p(u), _p(states), _p(gy[K - 1]), _p(gy), _mask(steps),
                                             _fp(a), _fp(s), *cfg, n, _p(gu), _fp(ga), _fp(gs), _p(ws), nb, st) == 0
    torch.cuda.synchronize()
    return traj, gu, ga, gs


@pytest.mark.parametrize("H,W", [(16, 16), (7, 9)], ids=_ids)
def test_explicit_bf16_vs_f32_route(H, W):
    """test_gpu_explicit_shapes.test_explicit_bf16_vs_f32_route for the trajectory: states and gu that route's rounded
    once; what passes between the steps is fp32 in both routes and the cotangents are the same bf16 values, so the
    parameter gradients are that route's; and the C ABI's fp32 route is the module's."""
    from cnn_with_pde_amd import _lib as L
    steps = (1, 2, 3)
    u, gy, a, s = (t.cuda() for t in _ex_inputs(H, W, steps, torch.bfloat16))
    y, gu, ga, gs = _ex_cabi(L.PDE_IO_BF16, u.bfloat16(), gy.bfloat16(), a, s, steps)
    y32, gu32, ga32, gs32 = _ex_cabi(L.PDE_IO_F32, u, gy, a, s, steps)
    assert y.dtype == torch.bfloat16 and y32.dtype == torch.float32
    dy = int((_ord16(y) - _ord16(y32.bfloat16())).abs().max())
    dg = int((_ord16(gu) - _ord16(gu32.bfloat16())).abs().max())
    print((H, W), dy, dg)
    assert dy <= 1 and dg <= 1
    assert torch.equal(ga, ga32) and torch.equal(gs, gs32), (ga, ga32, gs, gs32)
    ym, gum, gam, gsm = _ex_gpu(u.cpu(), gy.cpu(), a.cpu(), s.cpu(), steps)
    assert torch.equal(ym, y32) and torch.equal(gum, gu32) and torch.equal(gam, ga32) and torch.equal(gsm, gs32)


# ---- 8: float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,steps", [(3, 7, 9, (1, 3, 5)), (2, 2, 5, (1, 2))], ids=_ids)
def test_jacobi_f64_vs_oracle(B, H, W, steps):
    u, gy, A, Bc = _jac_inputs(B, H, W, steps, None, torch.float64)
    got = _jac_gpu(u, gy, A, Bc, steps)
    assert all(t.dtype == torch.float64 for t in got)
    _hold((B, H, W, steps), J_NAMES, got, _jac_oracle(u, gy, A, Bc, steps, torch.float64), TOL64)


def test_explicit_f64_vs_oracle():
    H, W, steps = 7, 9, (2, 3)
    u, gy, a, s = (t.double() for t in _ex_inputs(H, W, steps))
    a = torch.tensor(XS.EX_ALPHA[:a.numel()], dtype=torch.float64)     # 0.3, 0.05, ... as doubles, not widened floats
    got = _ex_gpu(u, gy, a, s, steps)
    assert all(t.dtype == torch.float64 for t in got)
    _hold((H, W, steps), EX_NAMES, got, _ex_oracle(u, gy, a, s, steps, torch.float64), TOL64)
    assert float(got[2][1]) == 0.0 and float(got[2][2]) == 0.0 and float(got[2][0]) != 0.0


# ---- 9: module level: layer_trajectory(layer, u, steps), the layer-level entry of the two explicit classes ------------------------------------------------------------------------------------------------------
def _pde_layer():
    import cnn_with_pde_amd as P
    pl = P.PDELayer(Nx=24, Ny=20, Lx=2.0, Ly=2.0, T=0.004)
    with torch.no_grad():                                              # the coefficients of test_gpu_jacobi_tiled.test_module_level
        for n, v in dict(alpha_w1=0.04, alpha_w2=0.01, alpha_w3=0.02, beta_w1=0.05, beta_w2=-0.01, beta_w3=0.01).items():
            getattr(pl, n).fill_(v)
    return pl


def test_pde_layer_trajectory():
    import cnn_with_pde_amd as P
    pl = _pde_layer()
    assert pl.Nt == 4
    g = torch.Generator().manual_seed(78)
    params = {k: v.detach().clone() for k, v in pl.named_parameters()}
    u = torch.randn(4, 1, 20, 24, generator=g)                         # rows follow y (Ny), columns x (Nx)
    gy = torch.randn(4, 4, 1, 20, 24, generator=g)

    def ref(a, p):
        A, Bc = O.emotion_coefficients(p, Nx=24, Ny=20, Lx=2.0, Ly=2.0, dt=0.001, dtype=a.dtype)
        return torch.stack([O.jacobi_forward(a.squeeze(1), A, Bc, k).unsqueeze(1) for k in range(1, 5)])

    y_ref, gu_ref, gp_ref = O.value_and_grads(ref, u.double(), {k: v.double() for k, v in params.items()}, gy.double())
    dl = pl.cuda()
    ud = u.cuda().requires_grad_(True)
    y = P.layer_trajectory(dl, ud)
    assert y.shape == (4, 4, 1, 20, 24)
    y.backward(gy.cuda())
    errs = {"y": G.rel_err(y.detach().cpu(), y_ref), "gu": G.rel_err(ud.grad.cpu(), gu_ref)}
    for n, p in dl.named_parameters():
        errs["g_" + n] = G.rel_err(p.grad.cpu(), gp_ref[n])
    print(errs)
    assert len(errs) == 8 and all(v <= 2e-4 for v in errs.values()), errs
    with torch.no_grad():
        assert torch.equal(P.layer_trajectory(dl, ud)[-1], dl(ud))
        assert torch.equal(P.layer_trajectory(dl, ud, [2, 3])[1], P.layer_trajectory(dl, ud)[2])


def test_improved_layer_trajectory():
    import cnn_with_pde_amd as P
    layer = P.ImprovedDiffusionLayer(16, 3, num_steps=4)
    g = torch.Generator().manual_seed(79)
    u = torch.randn(3, 3, 16, 16, generator=g)
    gy = torch.randn(2, 3, 3, 16, 16, generator=g)
    params = {"alpha_base": layer.alpha_base.detach().clone(), "channel_scaling": layer.channel_scaling.detach().clone()}
    y_ref, gu_ref, gp_ref = O.value_and_grads(
        lambda x, p: torch.stack([O.tiny_forward(x, p, dt=layer.dt, num_steps=k, eps=layer.stability_eps,
                                                 max_coeff=layer.max_coeff, relax=0.1) for k in (2, 4)]),
        u.double(), {k: v.double() for k, v in params.items()}, gy.double())
    dl = layer.cuda()
    ud = u.cuda().requires_grad_(True)
    y = P.layer_trajectory(dl, ud, [2, 4])
    assert y.shape == (2, 3, 3, 16, 16)
    y.backward(gy.cuda())
    got = (y.detach(), ud.grad, dl.alpha_base.grad, dl.channel_scaling.grad)
    _hold("improved", EX_NAMES, got, (y_ref, gu_ref, gp_ref["alpha_base"], gp_ref["channel_scaling"]), TOL)
    assert dl.beta_base.grad is None
    with torch.no_grad():
        assert torch.equal(P.layer_trajectory(dl, ud)[-1], dl(ud))


def test_half_layers_return_fp16():
    import cnn_with_pde_amd as P
    pl = _pde_layer().half().cuda()
    u = torch.randn(2, 1, 20, 24, device="cuda").half().requires_grad_(True)
    y = P.layer_trajectory(pl, u, [1, 4])
    y.backward(torch.ones_like(y))
    assert y.dtype == torch.float16 and y.shape == (2, 2, 1, 20, 24) and u.grad.dtype == torch.float16
    assert all(p.grad is not None and p.grad.dtype == torch.float16 for p in pl.parameters())
    with torch.no_grad():
        assert torch.equal(P.layer_trajectory(pl, u)[-1], pl(u))
        assert max_ulps(y[0].detach(), P.layer_trajectory(pl, u, [1])[0]) == 0
    ti = P.ImprovedDiffusionLayer(16, 3, num_steps=4).half().cuda()
    v = torch.randn(3, 3, 16, 16, device="cuda").half().requires_grad_(True)
    z = P.layer_trajectory(ti, v, [2, 4])
    z.backward(torch.ones_like(z))
    torch.cuda.synchronize()
    assert z.dtype == torch.float16 and z.shape == (2, 3, 3, 16, 16) and v.grad.dtype == torch.float16
    assert ti.alpha_base.grad.dtype == torch.float16 and ti.channel_scaling.grad.dtype == torch.float16
    with torch.no_grad():
        assert torch.equal(P.layer_trajectory(ti, v)[-1], ti(v))


# ---- 10: refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L
    pl = _pde_layer().cuda()
    ti = P.ImprovedDiffusionLayer(16, 3, num_steps=4).cuda()
    up, ut = torch.zeros(2, 1, 20, 24, device="cuda"), torch.zeros(2, 3, 16, 16, device="cuda")
    for bad in ([], [0], [5], [3, 2], [2, 2], [1.5]):                  # empty, 0, beyond the end, not increasing, not whole
        with pytest.raises(ValueError):
            P.layer_trajectory(pl, up, bad)
        with pytest.raises(ValueError):
            P.layer_trajectory(ti, ut, bad)
    with pytest.raises(ValueError):
        P.layer_trajectory(pl, up.squeeze(1))                          # a 3-D input, as forward refuses it
    with pytest.raises(ValueError):
        P.layer_trajectory(pl, ut)                                     # (B,3,H,W)
    long = P.PDELayer(Nx=24, Ny=20, Lx=2.0, Ly=2.0, T=0.2).cuda()
    assert long.Nt > 128
    for steps in ([129], [1, 129], None):                              # beyond the 128 bits of the mask
        with pytest.raises(ValueError):
            P.layer_trajectory(long, up, steps)
    with pytest.raises(L.PdeError):
        P.jacobi_diffuse_states(up, pl.alpha(pl.y), pl.beta(pl.x), [1, 2])    # the functional call takes (B,H,W)
    # the library itself: 129 steps with a non-empty mask come back before any launch
    lib = L.load()
    u, a, b = torch.zeros(2, 20, 24, device="cuda"), torch.zeros(20, device="cuda"), torch.zeros(24, device="cuda")
    out = torch.full((2, 2, 20, 24), 7.0, device="cuda")
    rc = lib.pde_jacobi_io_forward_states(2, 20, 24, 129, L.PDE_IO_F32, _p(u), _fp(a), _fp(b), _p(out[1]), _p(out), _mask((1, 129)),
                                          None, 0, None)
    assert rc == -3                                                    # PDE_E_TOO_MANY_SWEEPS
    states = torch.empty(128, 2, 3, 16, 16, device="cuda")
    tout = torch.full((2, 2, 3, 16, 16), 7.0, device="cuda")
    rc = lib.pde_explicit5_forward_states(2, 3, 16, 16, L.PDE_IO_F32, _p(ut), _fp(a), _fp(a), 0.01, 1e-6, 0.15, 0.1, 129, _p(states),
                                          _p(tout[1]), _p(tout), _mask((1, 129)), None)
    assert rc == -3
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((tout == 7.0).all())      # nothing ran


# ---- 11: repeatability and capture ------------------------------------------------------------------------------------------
def test_repeatability():
    """No float atomics: two calls, with a large unrelated allocation between them, give the same bits."""
    case = _jac_inputs(5, 97, 130, (3, 10))
    first = _jac_gpu(*case, (3, 10))
    junk = torch.full((64 << 20,), 7.0, device="cuda")      # moves the next call's workspace somewhere else
    second = _jac_gpu(*case, (3, 10))
    del junk
    for x, y in zip(first, second):
        assert torch.equal(x, y)


def test_capture():
    """forward + autograd.grad as one captured graph: the trajectory entry points allocate, copy and synchronise nothing."""
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(8)
    B, H, W, steps = 4, 96, 96, (1, 10)
    u = torch.randn(B, H, W, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(2, B, H, W, generator=g).cuda()
    A = (0.04 + 0.02 * torch.randn(H, generator=g)).cuda().requires_grad_(True)
    Bc = (0.05 + 0.02 * torch.randn(W, generator=g)).cuda().requires_grad_(True)

    def fn():
        y = P.jacobi_diffuse_states(u, A, Bc, steps)
        return (y,) + torch.autograd.grad(y, [u, A, Bc], gy)

    step = P.GraphedStep(fn)
    for trial in range(2):
        eager = [t.clone() for t in fn()]
        got = step()
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert torch.equal(a, b)
        with torch.no_grad():                               # new values, same buffers
            u.copy_(torch.randn(B, H, W, generator=g))
            gy.copy_(torch.randn(2, B, H, W, generator=g))
            A.mul_(1.1)
