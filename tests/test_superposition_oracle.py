"""The superposition method of tests/superpose_util.py, on the CPU: for every layer kind that
tests/test_gpu_fullsize_oracle.py holds to the oracle by superposition, the fp64 oracle run directly on the composed batch
must equal the reconstruction from the basis (y, the input gradient and every parameter gradient, to 1e-12), and the
composed inputs must be exact in the dtype the layer sees.  A layer that is not linear in u fails here."""
import zlib

import pytest
import torch

import golden_util as G
import superpose_util as S
from oracle import pde_oracle as O

B = 6


def _params(kind, C, N, g):
    """float64 parameters of one layer kind, perturbed enough that every term of the operator matters."""
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    if kind == "tiny":
        return {"alpha_base": 0.2 * torch.rand(C, generator=g, dtype=torch.float64),
                "channel_scaling": 1 + 0.2 * rnd(C)}
    shape = (N, N) if kind == "fashion" else (C, N, N)
    base = {"plain": 1.0, "clamp": 1.0, "cifar10": 1.0, "fashion": 1.8, "svhn": 1.8}[kind]
    p = {"alpha_base": base * (1 + 0.15 * rnd(*shape)), "beta_base": base * (1 + 0.15 * rnd(*shape)),
         "alpha_time_coeff": 2.0 * rnd(*shape), "beta_time_coeff": 2.0 * rnd(*shape)}
    if kind == "clamp":           # coefficients that cross the clamp floor inside the time window (moving masks)
        for c in range(1, C, 2):
            p["alpha_base"][c, ::3, ::2] = 0.02
            p["alpha_time_coeff"][c, ::3, ::2] = -0.3
            p["beta_base"][c, 1::4, :] = 0.01
            p["beta_time_coeff"][c, 1::4, :] = -0.2
    if kind == "cifar10":
        p["channel_mixing"] = torch.eye(C, dtype=torch.float64) + 0.1 * rnd(C, C)
    if kind == "svhn":
        p["channel_coupling"] = torch.eye(C, dtype=torch.float64) + 0.1 * rnd(C, C)
        p["skip_weight"] = torch.tensor(0.3, dtype=torch.float64)
    return p


def _fn(kind, C, N):
    if kind == "tiny":
        return lambda u, p: O.tiny_forward(u, p, dt=0.01, num_steps=1)
    if kind in ("plain", "clamp"):
        spec = O.AdiSpec(N, C, 0.05, 1.0, 1.0, 3, "strang", False, 10.0, "none", False)
    elif kind == "cifar10":
        spec = O.cifar10_spec(N, C, dt=0.05, num_steps=3)
    elif kind == "fashion":
        spec = O.fashion_spec(N, dt=0.3, num_steps=2)
    else:
        spec = O.svhn_spec(N, C, dt=0.3, num_steps=2)
    return lambda u, p: O.adi_forward(u, p, spec)


CASES = [  # kind, C, N, dtype
    ("plain", 3, 8, torch.float32),         # the headline layer (no operator between the steps)
    ("clamp", 3, 8, torch.float32),         # moving clamp masks
    ("cifar10", 3, 12, torch.float32),      # channel mixing before every step (cfg2)
    ("fashion", 1, 12, torch.float32),      # smoothed coefficients, one channel (cfg3)
    ("svhn", 3, 8, torch.float32),          # coupling after every step, skip blend (cfg3 at 32 channels)
    ("svhn", 3, 8, torch.bfloat16),         # the same on bf16 tensors (cfg4)
    ("tiny", 3, 12, torch.float32),         # explicit 5-point step (cfg5)
]


@pytest.mark.parametrize("kind,C,N,dtype", CASES, ids=lambda c: str(c).replace("torch.", ""))
def test_direct_oracle_equals_reconstruction(kind, C, N, dtype):
    g = torch.Generator().manual_seed(zlib.crc32(repr((kind, C, N, str(dtype))).encode()))
    params, fn = _params(kind, C, N, g), _fn(kind, C, N)
    E, F = S.basis(dtype, C, N, seed=11)
    W, V = S.weights(dtype, B, seed=1), S.weights(dtype, B, seed=2)
    u, gy = S.compose(E, W, dtype), S.compose(F, V, dtype)
    assert u.dtype == dtype and gy.dtype == dtype
    # the composed inputs are exact in their dtype: the round trip through it loses nothing
    assert torch.equal(u.double(), S.exact_sum(E, W)) and torch.equal(gy.double(), S.exact_sum(F, V))
    assert torch.equal(u.double().to(dtype), u)

    basis = S.Basis(fn, params, E, F)
    y_ref, gu_ref, gp_ref = O.value_and_grads(fn, u.double(), params, gy.double())
    grads = {n: g for n, g in gp_ref.items() if g is not None}
    errs = S.errors(basis, W, V, y_ref, gu_ref, grads)
    assert set(errs) == {"y", "gu"} | {"g_" + n for n in grads}
    assert len(grads) >= 2
    bad = {k: v for k, v in errs.items() if not v <= 1e-12}
    assert not bad, (bad, errs)
    # (the metric is the suite's)
    assert S.sliced_rel_err(y_ref, W, basis.Y, rows=4) == pytest.approx(G.rel_err(y_ref, S.exact_sum(basis.Y, W)), abs=1e-15)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_weight_rows_differ_and_sums_stay_exact(dtype):
    """No two samples fewer than 64 indices apart share a row of W (a wave that touches the wrong plane shows), and the
    extreme sums the value grids allow are still exact in the dtype."""
    n = S.distinct_rows(dtype)
    assert n >= 64
    W = S.weights(dtype, 3 * n + 5, seed=3)
    assert not bool((W == 0).all(dim=1).any())
    for d in range(1, 64):
        assert not bool((W[d:] == W[:-d]).all(dim=1).any()), d
    s = S.SETUP[dtype]
    wmax = max(abs(w) for w in s["weights"])
    top = s["K"] * wmax * max(abs(s["lo"]), abs(s["hi"])) * s["scale"]
    for v in (top, top - s["scale"], -top + s["scale"]):
        assert float(torch.tensor(v, dtype=torch.float64).to(dtype).double()) == v
