"""The CPU oracle on rectangular planes (H != W).  ``oracle.pde_oracle.adi_forward`` reads B, C, H, W from its input as the
reference's sweeps do (mnist_test.py:45,72,105; cifar10.py:67,76,126,152); the GPU tests of the rectangle entry points
(tests/test_gpu_rect.py) lean on it, so it is pinned here against something that shares no code with it: every line system
of every sweep assembled as a dense matrix in fp64 and handed to ``torch.linalg.solve``.

The reference's Thomas recurrences add eps to every pivot (den_0 = b_0 + eps, den_i = b_i - a_i c*_{i-1} + eps,
mnist_test.py:160-185): that is the exact LU factorisation of A + eps I, so the dense system is (A + eps I) x = d with
A = tridiag(-co, 1 + 2 co, -co), first and last diagonal entry 1 + co (Neumann ends), co = theta * delta / h^2.

Bound: 1e-12 max-norm relative.  Both sides are fp64; the systems are diagonally dominant M-matrices with condition
number at most 1 + 4 max(co) < 10 here, so each of the at most six solves loses a few ulps (2.2e-16 each): measured at
most 5e-16.

The reference's own classes run when their four coefficient parameters are replaced by rectangular tensors (its sweeps
are shape-generic, only the constructors fix size x size): tests/golden/rect/ holds two vectors made that way by
tools/make_golden.py (``rect``), pinned here at the tolerance tests/test_oracle_golden.py uses for K1 in fp32 — bitwise,
1e-6 for a scalar parameter's gradient."""
import os

import pytest
import torch
import torch.nn.functional as F

import golden_util as G
from oracle import pde_oracle as O

RECT_DIR = os.path.join(G.GOLDEN_DIR, "rect")


def _dense_sweep(u, theta, axis, delta, h, smooth3, eps):
    """One implicit sweep by dense solves.  u (B,C,H,W), theta (C,H,W) already clamped; axis 0: lines along W, 1: along H."""
    if axis == 1:
        u, theta = u.transpose(2, 3), theta.transpose(1, 2)
    B, Cc, L, n = u.shape
    th = theta
    if smooth3:                                       # replicate ends, (left + centre + right) / 3 along the line
        p = F.pad(th, (1, 1), mode="replicate")
        th = (p[..., :-2] + p[..., 1:-1] + p[..., 2:]) / 3
    co = th * delta / h ** 2                          # (C, L, n)
    A = torch.zeros(Cc, L, n, n, dtype=u.dtype)
    k = torch.arange(n)
    diag = 1 + 2 * co
    diag[..., 0] = 1 + co[..., 0]
    diag[..., -1] = 1 + co[..., -1]
    A[..., k, k] = diag + eps
    A[..., k[1:], k[:-1]] = -co[..., 1:]              # row i, column i-1: a_i = -co_i
    A[..., k[:-1], k[1:]] = -co[..., :-1]             # row i, column i+1: c_i = -co_i
    x = torch.linalg.solve(A.unsqueeze(0).expand(B, -1, -1, -1, -1), u.unsqueeze(-1)).squeeze(-1)
    return x.transpose(2, 3) if axis == 1 else x


def _dense_forward(u, params, spec):
    for axis, delta, t in O.sweep_schedule(spec):
        base, slope, h = ((params["alpha_base"], params["alpha_time_coeff"], spec.dx) if axis == 0 else
                          (params["beta_base"], params["beta_time_coeff"], spec.dy))
        theta = base + slope * t
        theta = theta.clamp(min=spec.eps) if spec.clamp_max is None else theta.clamp(min=spec.eps, max=spec.clamp_max)
        u = _dense_sweep(u, theta, axis, delta, h, spec.smooth3, spec.eps)
    return u


@pytest.mark.parametrize("hw", [(5, 9), (9, 5), (2, 13), (12, 3)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("split", ["strang", "lie"])
@pytest.mark.parametrize("smooth3", [False, True], ids=["plain", "smooth3"])
@pytest.mark.parametrize("clamp_max", [None, 2.5], ids=["min_only", "clamp_max"])
def test_adi_forward_on_rectangles_vs_dense_solves(hw, split, smooth3, clamp_max):
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    Cc, B = 2, 3
    spec = O.AdiSpec(hw[0], Cc, 0.4, 1.0, 1.3, 2, split, smooth3, clamp_max, "none", False)
    params = {"alpha_base": 2.0 + torch.randn(Cc, *hw, generator=g, dtype=torch.float64),      # crosses 2.5 and the floor
              "beta_base": 1.0 + 1.5 * torch.randn(Cc, *hw, generator=g, dtype=torch.float64),
              "alpha_time_coeff": 2.0 * torch.randn(Cc, *hw, generator=g, dtype=torch.float64),
              "beta_time_coeff": 2.0 * torch.randn(Cc, *hw, generator=g, dtype=torch.float64)}
    u = torch.randn(B, Cc, *hw, generator=g, dtype=torch.float64)
    got, want = O.adi_forward(u, params, spec), _dense_forward(u, params, spec)
    assert got.shape == u.shape
    err = float((got - want).abs().max() / want.abs().max())
    print(hw, split, smooth3, clamp_max, f"{err:.2e}")
    assert err <= 1e-12


def test_gradients_have_the_parameters_shape():
    hw, Cc = (5, 9), 2
    g = torch.Generator().manual_seed(1)
    spec = O.cifar10_spec(hw[0], Cc, dt=0.1, num_steps=2)
    params = {"alpha_base": 1.0 + torch.rand(Cc, *hw, generator=g, dtype=torch.float64),
              "beta_base": 1.0 + torch.rand(Cc, *hw, generator=g, dtype=torch.float64),
              "alpha_time_coeff": torch.randn(Cc, *hw, generator=g, dtype=torch.float64),
              "beta_time_coeff": torch.randn(Cc, *hw, generator=g, dtype=torch.float64),
              "channel_mixing": torch.eye(Cc, dtype=torch.float64)}
    u = torch.randn(3, Cc, *hw, generator=g, dtype=torch.float64)
    y, gu, gp = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec), u, params, torch.ones_like(u))
    assert y.shape == gu.shape == u.shape
    assert all(gp[k].shape == (Cc, *hw) for k in ("alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff"))


@pytest.mark.parametrize("name", ["mnist_20x36", "cifar10_c3_24x40"])
def test_oracle_matches_reference_vectors_on_rectangles(name):
    """As tests/test_oracle_golden.py::test_oracle_matches_reference_vectors: K1 in fp32 agrees BITWISE with the reference
    (same operations in the same order), a scalar parameter's gradient within 1e-6."""
    assert sorted(G.names(directory=RECT_DIR)) == ["cifar10_c3_24x40", "mnist_20x36"]
    g = G.Golden(name, directory=RECT_DIR)
    H, W = g.meta["plane"]
    assert H != W and tuple(g.u.shape[-2:]) == (H, W) and tuple(g.params["alpha_base"].shape[-2:]) == (H, W)
    assert g.family() == "adi" and g.dtype == torch.float32
    fn = g.oracle_fn()
    threads = torch.get_num_threads()
    torch.set_num_threads(G.GOLDEN_THREADS)        # as the vectors were made (golden_util)
    try:
        y, gu, grads = O.value_and_grads(fn, g.u, g.params, g.gy)
    finally:
        torch.set_num_threads(threads)
    tol = 0.0
    assert y.dtype == g.dtype and y.shape == g.y.shape
    assert G.rel_err(y, g.y) <= tol, ("y", G.rel_err(y, g.y))
    assert G.rel_err(gu, g.gu) <= tol, ("gu", G.rel_err(gu, g.gu))
    assert set(g.grads) >= {"alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff"}
    for n, ref in g.grads.items():
        assert not g.grad_is_none[n], n
        e = G.rel_err(grads[n], ref)
        assert e <= (max(tol, 1e-6) if ref.numel() == 1 else tol), (n, e)
