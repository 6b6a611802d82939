"""The ground tests/test_gpu_rh_paths.py stands on, checked without a GPU: the closed-form fp64 reference of the symmetric
layer against fp64 autograd of oracle.pde_oracle.symmetric_layer; that every exact case is exact (its conditions hold, and
an fp32 evaluation in two different summation orders equals the fp64 reference bit for bit); that the case lists name
every path of the kernels' dispatch; and that the offset-column inputs are what they claim to be."""
import numpy as np
import pytest
import torch

import rh_cases as R
from oracle import pde_oracle as O


# --------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("act", ["identity", "relu", "tanh"])
@pytest.mark.parametrize("training,momentum", [(True, 0.1), (True, 1.0), (False, 0.1)])
@pytest.mark.parametrize("B,D", [(5, 64), (37, 128)])
def test_reference_vs_autograd_of_the_oracle(B, D, act, training, momentum):
    c = R.general_layer(B, D, act, training, momentum)
    ref = R.reference(c)
    X, K = c.X.clone().requires_grad_(True), c.K.clone().requires_grad_(True)
    gamma, beta, base = c.gamma.clone().requires_grad_(True), c.beta.clone().requires_grad_(True), c.base.clone().requires_grad_(True)
    # the oracle's BatchNorm has momentum 0.1 and eps 1e-5 built in: its running statistics are compared at 0.1 only
    sl = {"K.weight": K, "norm.weight": gamma, "norm.bias": beta, "norm.running_mean": c.running_mean.clone(),
          "norm.running_var": c.running_var.clone()}
    out = base + c.scale * (-O.symmetric_layer(X, sl, training, act))
    gX, gK, gg, gb, gbase = torch.autograd.grad(out, [X, K, gamma, beta, base], c.g)
    pairs = {"out": out.detach(), "gX": gX, "gK": gK, "g_gamma": gg, "g_beta": gb}
    if momentum == 0.1:
        pairs["running_mean"], pairs["running_var"] = sl["norm.running_mean"], sl["norm.running_var"]
    else:
        P = c.X @ c.K.t()
        pairs["running_mean"], pairs["running_var"] = P.mean(0), P.var(0, unbiased=True)      # momentum 1: the batch's own
    for name, want in pairs.items():
        err = float((ref[name] - want).abs().max())
        assert err <= 1e-13 * max(1.0, float(want.abs().max())), (name, err)
    assert torch.equal(gbase, c.g)                                          # the gradient of base is left to the caller
    # the saved tensors
    P = c.X @ c.K.t()
    assert float((ref["P"] - P).abs().max()) <= 1e-13 * float(P.abs().max())
    if training:
        assert float((ref["mean"] - P.mean(0)).abs().max()) <= 1e-13
        assert float((ref["invstd"] - 1 / torch.sqrt(P.var(0, unbiased=False) + 1e-5)).abs().max()) <= 1e-13 * float(ref["invstd"].max())
    else:
        assert torch.equal(ref["mean"], c.running_mean) and torch.equal(ref["running_var"], c.running_var)
    # dP is the gradient of the loss with respect to P
    Pq = ref["P"].clone().requires_grad_(True)
    bn = O.batch_norm_1d(Pq, c.gamma, c.beta, c.running_mean, c.running_var, training)[0]
    (dP,) = torch.autograd.grad(c.scale * (R.act_forward(bn, act) @ c.K), [Pq], c.g)
    assert float((ref["dP"] - dP).abs().max()) <= 1e-13 * max(1.0, float(dP.abs().max()))


def test_relu_derivative_at_the_tie_is_zero():
    h = torch.tensor([-1.0, 0.0, 0.5], dtype=torch.float64)
    assert R.act_derivative(torch.relu(h), "relu").tolist() == [0.0, 0.0, 1.0]
    c = R.exact_layer(33, 128, 1)                                           # variant 1: ReLU
    ref = R.reference(c)
    tie = (ref["xhat"] * c.gamma + c.beta) == 0
    assert c.act == "relu" and int(tie.sum()) > 0 and bool((ref["dN"][tie] == 0).all()) and bool((ref["dP"][tie] == 0).all())


# --------------------------------------------------------------------------------------------------- exact cases are exact
def _mm32(a, b, reverse):
    """a @ b in fp32 as partial products over 32-wide slices of the contraction, added first to last, or last to first with
    the order inside every slice reversed too"""
    a, b = a.float(), b.float()
    n = a.shape[1]
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    starts = list(range(0, n, 32))
    for k in (reversed(starts) if reverse else starts):
        sa, sb = a[:, k:k + 32], b[k:k + 32]
        acc = acc + (sa.flip(1) @ sb.flip(0) if reverse else sa @ sb)
    return acc


def _sum32(v, reverse):
    t = np.ascontiguousarray(v.float().numpy())
    if reverse:
        t = t[::-1]
    return torch.from_numpy(np.add.accumulate(t, axis=0, dtype=np.float32)[-1].copy())


def _eval_f32(c, reverse):
    """The exact case (eval mode) in fp32 with the kernels' formulas, every sum in the given order."""
    f = lambda v: None if v is None else v.float()
    X, K, gamma, beta, g, base, scale = f(c.X), f(c.K), f(c.gamma), f(c.beta), f(c.g), f(c.base), c.scale
    mean, invstd = f(c.running_mean), torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(f(c.running_var) + c.eps)
    P = _mm32(X, K.t(), reverse)
    xhat = (P - mean) * invstd
    H = R.act_forward(xhat * gamma + beta, c.act)
    Q = _mm32(H, K, reverse)
    out = scale * Q if base is None else scale * Q + base
    dN = scale * _mm32(g, K.t(), reverse) * R.act_derivative(H, c.act)
    dP = gamma * invstd * dN
    gK = _mm32(dP.t(), X, reverse) + _mm32(H.t(), scale * g, reverse) if not reverse else \
        _mm32(H.t(), scale * g, reverse) + _mm32(dP.t(), X, reverse)
    return {"P": P, "H": H, "mean": mean, "invstd": invstd, "out": out, "dP": dP, "gX": _mm32(dP, K, reverse), "gK": gK,
            "g_gamma": _sum32(dN * xhat, reverse), "g_beta": _sum32(dN, reverse)}


def _exact_shapes():
    seen, out = set(), []
    for c in R.exact_cases() + R.dk_cases() + [R.cap_case()]:
        if (c.B, c.D, c.variant) not in seen:
            seen.add((c.B, c.D, c.variant))
            out.append((c.B, c.D, c.variant))
    return out


@pytest.mark.parametrize("B,D,variant", _exact_shapes())
def test_exact_cases_are_exact(B, D, variant):
    """exact_case() asserts the conditions (term sums below 2^24 eighths, the bf16 piece condition of the gradient of K);
    here, in addition, two fp32 evaluations in different summation orders equal the fp64 reference bit for bit."""
    if D > 1024:                                              # the one large case: not cached, not kept
        c = R.exact_layer(B, D, variant)
        ref = R.reference(c)
        assert R.assert_exact(c, ref) < 2 ** 24
    else:
        c, ref = R.exact_case(B, D, variant)
    for reverse in (False, True):
        got = _eval_f32(c, reverse)
        for name, v in got.items():
            assert torch.equal(v.double(), ref[name]), (name, reverse)


def test_a_shape_that_breaks_the_conditions_fails_in_the_generator():
    c = R.exact_layer(17, 128, 0)
    c.X = c.X * 4096.0                                        # integers up to 12288: outside -3..3
    with pytest.raises(AssertionError):
        R.assert_exact(c, R.reference(c))
    c = R.exact_layer(17, 128, 0)
    c.K = c.K + c.K.t()                                       # symmetric
    with pytest.raises(AssertionError):
        R.assert_exact(c, R.reference(c))
    c = R.exact_layer(17, 128, 0)
    c.running_var = c.running_var * 3.0                       # invstd no power of two
    with pytest.raises(AssertionError):
        R.assert_exact(c, R.reference(c))


def test_exact_grid_alternates_and_relu_meets_ties():
    cases = R.exact_cases()
    layers = [R.exact_layer(c.B, c.D, c.variant) for c in cases]
    assert {(l.act, l.base is None, l.scale) for l in layers} == {(a, b, s) for a in ("identity", "relu") for b in (False, True)
                                                                 for s in R.EXACT_SCALES}
    for fam in (R.STRIP32, R.STRIP16, R.ROW_BLOCKS):
        mine = [l for c, l in zip(cases, layers) if c.family == fam]
        assert {l.act for l in mine} == {"identity", "relu"} and {l.base is None for l in mine} == {False, True}
        assert {l.scale for l in mine} == set(R.EXACT_SCALES)
    ties = 0
    for c in cases:
        l, ref = R.exact_case(c.B, c.D, c.variant)
        if l.act == "relu" and c.B * c.D >= 4096:
            n = int(((ref["xhat"] * l.gamma + l.beta) == 0).sum())
            assert n > 0, (c.B, c.D)
            ties += n
    assert ties > 1000


# --------------------------------------------------------------------------------------------------- the case lists
def test_case_lists_name_every_path():
    cases = R.exact_cases()
    ids = [R.case_id(c) for c in cases + R.dk_cases()]
    assert len(set(ids)) == len(ids)
    s32 = {(c.D, c.split, c.B) for c in cases if c.family == R.STRIP32 and not c.env}
    for D, S in ((128, 2), (256, 4), (512, 8), (384, 2)):
        assert {B for d, s, B in s32 if (d, s) == (D, S)} == {1, 31, 32, 33, 63, 64, 65, 96, 127, 128}
    assert {B for d, s, B in s32 if (d, s) == (768, 4)} == {33, 64, 65, 128}
    assert {(c.D, c.split) for c in cases if c.env and c.env[0][0] == "PDE_RH_SPLIT"} == {(1024, 16), (512, 2)}
    assert all(c.waves == (2 if c.B <= 64 else 4) for c in cases if c.family == R.STRIP32)
    s16 = [c for c in cases if c.family == R.STRIP16]
    assert {(c.D, c.B) for c in s16 if c.workspace and not c.env} == {(D, B) for D in (64, 192, 320) for B in (1, 15, 16, 17, 127, 128)}
    twins = {(B, D) for B, D, _ in R.NO_WORKSPACE_SHAPES}
    assert twins == {(33, 128), (128, 128), (33, 512), (128, 512)}
    assert {(c.B, c.D) for c in s16 if not c.workspace} == twins
    assert {(c.B, c.D) for c in s16 if c.env} == twins and all(c.env == (("PDE_RH_NO_STRIP32", "1"),) for c in s16 if c.env)
    rb = {(c.B, c.D, c.blocks) for c in cases if c.family == R.ROW_BLOCKS}
    assert rb == {(B, D, n) for B, n in ((129, 2), (256, 2), (257, 3), (385, 4)) for D in (64, 128, 320)}
    dk = R.dk_cases()
    assert {(c.D, c.B, c.dk) for c in dk} == {(D, B, k) for D in (64, 128, 192, 256, 320, 384) for B in (1, 15, 16, 17, 33)
                                              for k in (R.DK_SPLIT3, R.DK_MFMA_F32)}
    assert all((c.env == (("PDE_RH_NO_SPLIT", "1"),)) == (c.dk == R.DK_MFMA_F32) for c in dk)
    cap = R.cap_case()
    assert (cap.B, cap.D, cap.split, cap.waves) == (65, 4608, 4, 4)
    # no tensor beyond 385 x 768 or 1024 x 1024 apart from the cap case
    assert all((c.B <= 385 and c.D <= 768) or c.D == 1024 for c in cases + dk)
    assert all(c.B != 2 for c in R.GENERAL_CASES)        # no training batch of two rows (tests/test_gpu_rh.py)


@pytest.mark.parametrize("B,D", [(c.B, c.D) for c in R.OFFSET_CASES])
def test_offset_columns_have_means_100_times_their_deviation(B, D):
    c = R.general_layer(B, D, "tanh", True, 0.1, True)
    P = c.X @ c.K.t()
    ratio = P.mean(0).abs() / P.std(0, unbiased=False)
    assert float(ratio.min()) > 50 and float(ratio.max()) < 250, (float(ratio.min()), float(ratio.max()))
    for v in c.tensors().values():
        assert torch.equal(v.float().double(), v)             # the reference sees the fp32 inputs
    plain = R.general_layer(B, D, "tanh", True, 0.1, False)
    P = plain.X @ plain.K.t()
    assert float((P.mean(0).abs() / P.std(0, unbiased=False)).max()) < 1.5
