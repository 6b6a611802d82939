"""The ground tests/test_gpu_rh16_stages.py stands on, checked without a GPU (tests/rh16_cases.py): every exact case has the
right answers it claims (the narrow grid all of them, the wide grid at least P, H, a base-less out and dP, all finite); over
both grids every rounding point that can round in an exact case does, and meets exact ties; the contract agrees with plain
CPU autocast of SymmetricLayer(fused=False); the contract itself passes the stage-by-stage rule with CPU fp32 as the plain
route, inside the cap on two-ended elements; and both comparisons reject every mutant of the contract — a subtly wrong
kernel, without one being built or run.

Three rounding points of the contract cannot round in an exact case and are not counted: H = r(act(N)) with identity or
ReLU, S = r(scale Q) and gQ = r(scale r(g)) with a power-of-two scale — each is r() of a 16-bit value (assert_exact checks
that they did not).  The general cases (tanh, scale 0.7) exercise them."""
import pytest
import torch

import rh16_cases as S
import rh_cases as R

DT = pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: S.TAG[d])


# --------------------------------------------------------------------------------------------------- exact cases
@DT
@pytest.mark.parametrize("c", S.narrow_cases(), ids=S.case_id)
def test_narrow_cases_have_one_right_answer_everywhere(c, dtype):
    layer, ref, held = S.exact_case(c.family, c.B, c.D, c.variant, dtype)
    assert held == frozenset(S.OUTPUTS), sorted(set(S.OUTPUTS) - held)
    for name in S.OUTPUTS:
        assert bool(torch.isfinite(ref[name]).all()), name
    for name in ("X", "K", "g"):                              # small integers: 16-bit values already
        assert torch.equal(S.rne(dtype)(ref["pre"][name]), ref["pre"][name])
    S.compare_exact(layer, S.as_abi(layer, ref, dtype), ref, held, dtype)


@DT
def test_the_workload_shape_has_one_right_answer_everywhere(dtype):
    c = S.workload_case()
    assert (c.B, c.D, c.split, c.waves, c.slabs) == (64, 3072, 8, 2, 6)
    layer = S.exact_layer(c.family, c.B, c.D, c.variant, dtype)                        # the one large case: not cached
    ref = S.contract(layer, dtype)
    assert S.assert_exact(layer, ref, dtype) == frozenset(S.OUTPUTS)
    if dtype == torch.bfloat16:                            # integers beyond 256: P and dP round here
        assert not torch.equal(ref["pre"]["P"], ref["P"]) and not torch.equal(ref["pre"]["dP"], ref["dP"])


@DT
@pytest.mark.parametrize("c", S.wide_cases(), ids=S.case_id)
def test_wide_cases_keep_the_16_bit_tensors_exact_and_finite(c, dtype):
    layer, ref, held = S.exact_case(c.family, c.B, c.D, c.variant, dtype)
    assert {"P", "H", "dP", "mean", "invstd", "running_mean", "running_var"} <= held
    assert layer.base is not None or "out" in held
    for name in S.OUTPUTS:
        assert bool(torch.isfinite(ref[name]).all()), name
    r = S.rne(dtype)
    for name in ("X", "K", "g"):                              # the low bits are there, and r() takes them off
        v = ref["pre"][name]
        assert not torch.equal(r(v), v) and torch.equal(r(v), r(v).round())
    S.compare_exact(layer, S.as_abi(layer, ref, dtype), ref, held, dtype)


def test_the_grids_name_what_they_reach():
    narrow, wide = S.narrow_cases(), S.wide_cases()
    ids = [S.case_id(c) for c in narrow + wide]
    assert len(set(ids)) == len(ids) and len(narrow) == 4 * 15 + 5 * 5 and 10 <= len(wide) <= 12
    assert {(c.D, c.split, c.slabs, c.tiles) for c in narrow} == {
        (64, 1, 1, "ragged"), (128, 2, 1, "ragged"), (192, 1, 3, "whole"), (512, 8, 1, "ragged"), (256, 4, 1, "ragged"),
        (320, 1, 5, "ragged"), (384, 2, 3, "whole"), (768, 4, 3, "whole"), (1024, 8, 2, "ragged")}
    for D in S.NARROW_WIDTHS:
        assert {c.B for c in narrow if c.D == D} == {1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128}
    for D in S.NARROW_WIDTHS_2:
        assert {c.B for c in narrow if c.D == D} == {1, 17, 64, 65, 128}
    assert all(c.waves == (2 if c.B <= 64 else 4) for c in narrow + wide) and all(c.D <= 256 for c in wide)
    assert {c.split for c in wide} == {1, 2, 4} and {c.waves for c in wide} == {2, 4}
    for cases, dtype in ((narrow, torch.float16), (wide, torch.float16), (wide, torch.bfloat16)):
        layers = [S.exact_layer(c.family, c.B, c.D, c.variant, dtype) for c in cases]
        assert {l.act for l in layers} == {"identity", "relu"} and {l.base is None for l in layers} == {False, True}
        assert {l.scale for l in layers} == set(R.EXACT_SCALES)


@DT
def test_every_rounding_point_rounds_and_meets_exact_ties(dtype):
    """over both grids together, per type: X, K, g (the wide family's low bits), P, N, Q and dP"""
    r = S.rne(dtype)
    changed = {p: 0 for p in S.ROUNDING_POINTS}
    ties = dict(changed)
    for c in S.narrow_cases() + S.wide_cases():
        ref = S.exact_case(c.family, c.B, c.D, c.variant, dtype)[1]
        for p in S.ROUNDING_POINTS:
            v = ref["pre"][p]
            changed[p] += int((r(v) != v).sum())
            ties[p] += int(S.is_tie(v, dtype).sum())
    print(S.TAG[dtype], "elements changed", changed, "exact ties", ties)
    assert all(n > 0 for n in changed.values()) and all(n > 0 for n in ties.values()), (changed, ties)


def test_the_overflow_case_is_what_it_claims():
    layer, ref, held = S.overflow_case()                    # its own assertions: one element of P beyond 65504, ...
    assert not layer.training and layer.act == "identity" and (layer.B, layer.D) == (5, 64)
    assert bool(torch.isinf(ref["H"]).any()) and held == frozenset(S.OUTPUTS)
    got = S.as_abi(layer, ref, torch.float16)
    S.compare_exact(layer, got, ref, held, torch.float16)
    for name, value in (("P", 65504.0), ("H", float("nan")), ("gK", 0.0), ("out", 1.0)):         # a finite value where the contract has none
        wrong = dict(got)
        wrong[name] = got[name].clone()
        wrong[name][tuple(torch.nonzero(~torch.isfinite(got[name]))[0].tolist())] = value
        with pytest.raises(AssertionError):
            S.compare_exact(layer, wrong, ref, held, torch.float16)


def test_the_wrong_roundings_are_wrong_only_where_they_should_be():
    for dtype in S.DTYPES:
        step = 2.0 ** -S.MANTISSA[dtype]
        v = torch.tensor([1 + step / 2, 1 + 3 * step / 2, -(1 + step / 2), 1 + step / 4, -(1 + 3 * step / 4), 1.0, 0.0, 3.0],
                         dtype=torch.float64)
        assert S.is_tie(v, dtype).tolist() == [True, True, True, False, False, False, False, False]
        assert S.rne(dtype)(v).tolist() == [1.0, 1 + 2 * step, -1.0, 1.0, -(1 + step), 1.0, 0.0, 3.0]
        assert S.ties_away(dtype)(v).tolist() == [1 + step, 1 + 2 * step, -(1 + step), 1.0, -(1 + step), 1.0, 0.0, 3.0]
        assert S.truncating(dtype)(v).tolist() == [1.0, 1 + step, -1.0, 1.0, -1.0, 1.0, 0.0, 3.0]


# --------------------------------------------------------------------------------------------------- the contract vs autocast
@DT
@pytest.mark.parametrize("act,training", [("relu", True), ("tanh", False)])
def test_contract_agrees_with_plain_cpu_autocast(dtype, act, training):
    """SymmetricLayer(fused=False) under torch.autocast("cpu", dtype) — this build runs linear, batch_norm and matmul under CPU
    autocast in both types.  CPU autocast keeps batch_norm in fp32, so its rounding points are not the CUDA ones the contract
    has: the two agree to within the route's own rounding, seven rounding points (X, K, P, N, H, Q, S) of half a step
    (2^-(p+1) relative) each through a K of norm below 1.5 — 10.5 x 2^-(p+1) of the largest element."""
    import cnn_with_pde_amd as PK
    B, chan, side = 17, 3, 8
    D = chan * side * side
    c = S.general_layer(B, D, act, training, variant=1)
    l = PK.models.SymmetricLayer(chan, side, act)
    l.fused = False
    with torch.no_grad():
        l.K.weight.copy_(c.K); l.norm.weight.copy_(c.gamma); l.norm.bias.copy_(c.beta)
        l.norm.running_mean.copy_(c.running_mean); l.norm.running_var.copy_(c.running_var)
    l.train(training)
    with torch.autocast("cpu", dtype=dtype):
        out = l(c.X.float().view(B, chan, side, side)).detach()
    assert out.dtype == dtype
    ref = S.contract(c, dtype)                              # no base, scale = 0.7: F_sym is scale = -1
    want = -ref["out"] / c.scale
    err = float((out.double().view(B, D) - want).abs().max()) / float(want.abs().max())
    assert err <= 10.5 * 2.0 ** -(S.MANTISSA[dtype] + 1), err
    if training:
        assert float((l.norm.running_mean.double() - ref["running_mean"]).abs().max()) <= 2.0 ** -S.MANTISSA[dtype]


# --------------------------------------------------------------------------------------------------- the stage rule on the contract
@DT
@pytest.mark.parametrize("v", S.general_cases(), ids=S.general_id)
def test_the_contract_passes_the_stage_rule_inside_the_cap(v, dtype):
    """check_stages raises where more than TWO_ENDED_CAP of a stage's elements have two ends; the plain route is CPU fp32"""
    c, ref = S.general_contract(*v, dtype)
    fig = S.check_stages(c, dtype, S.as_abi(c, ref, dtype), "cpu", S.general_id(v))
    print(S.TAG[dtype], S.general_id(v), {k: f"{a:.2e}/{b:.2%}" for k, (a, b) in fig.items() if k in ("P", "N", "H", "Q", "dP")})
    for stage in S.CAPPED_STAGES:
        assert fig[stage][1] <= S.TWO_ENDED_CAP


# --------------------------------------------------------------------------------------------------- mutants
MUTANT_EXACT = (("narrow", 17, 192), ("narrow", 33, 128), ("wide", 5, 64), ("wide", 33, 128))
MUTANT_GENERAL = ((5, 64, "relu", True, 0, True), (128, 768, "tanh", True, 1, True))
MUTANT_NAMES = sorted(S.mutants(torch.float16))


def _variant(family, B, D):
    (c,) = [c for c in S.narrow_cases() + S.wide_cases() if (c.family, c.B, c.D) == (family, B, D)]
    return c.variant


def _rejections(dtype, rules):
    """the cases of MUTANT_EXACT / MUTANT_GENERAL on which the comparisons of the GPU test refuse this evaluation"""
    refused = []
    for family, B, D in MUTANT_EXACT:
        layer, ref, held = S.exact_case(family, B, D, _variant(family, B, D), dtype)
        got = S.as_abi(layer, S.contract(layer, dtype, rules=rules), dtype)
        try:
            S.compare_exact(layer, got, ref, held, dtype)
        except AssertionError:
            refused.append((family, B, D))
    for v in MUTANT_GENERAL:
        layer = S.general_layer(*v)
        got = S.as_abi(layer, S.contract(layer, dtype, rules=rules), dtype)
        try:
            S.check_stages(layer, dtype, got, "cpu")
        except AssertionError:
            refused.append(v)
    return refused


@DT
def test_the_comparisons_accept_the_contract(dtype):
    assert _rejections(dtype, S.Rules()) == []


@DT
@pytest.mark.parametrize("name", MUTANT_NAMES)
def test_the_comparisons_reject_the_mutant(name, dtype):
    refused = _rejections(dtype, S.mutants(dtype)[name])
    print(S.TAG[dtype], name, "refused on", refused)
    assert refused, f"no case notices: {name}"
    # "N not rounded" cannot show in an exact case: with identity or ReLU, r(act(N)) = r(act(r(N))); only tanh tells them apart
    if name in ("r truncates", "r rounds ties away from zero", "r(X) skipped", "K in place of K^T", "a row beyond B leaks into gK"):
        assert any(v[0] in ("narrow", "wide") for v in refused), "the exact cases do not notice"
    if name in ("r(P) skipped before the statistics", "biased and unbiased variance swapped", "K in place of K^T"):
        assert all(v in refused for v in MUTANT_GENERAL), "a general case does not notice"
    if name == "scale product rounded once":               # scale = 0.7: the general cases only, and both of them
        assert refused == list(MUTANT_GENERAL)
    if name == "N not rounded":
        assert MUTANT_GENERAL[1] in refused and MUTANT_GENERAL[1][2] == "tanh"
