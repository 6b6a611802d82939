"""CPU checks of tests/shared_input_cases.py: the tiled, count-weighted reference is the reference of the materialised
batch; the reference's own fp32 arithmetic stays well inside the limits the GPU tests apply; every case builds the
scenario its row of the table names; and every plausible kernel fault (a wrong-rule reference) lies at least ten
limits away from the right reference in an output the GPU tests compare."""
import dataclasses

import pytest
import torch

import shared_input_cases as S

CASE_IDS = [c.name for c in S.CASES]


def test_table_shapes_and_sides_of_the_threshold():
    """The rows of the table: arrangement against 1024, L, the steps, P <= 11, B >= P, at most four layers."""
    want = {"par-n32-c4-l4": (32, 4, 3, 3, (1, 3, 2, 4)), "par-n28-c1-l2-mask": (28, 1, 7, 7, (3, 2)),
            "par-n16-c2-l3-lie-max": (16, 2, 1023, 7, (2, 4, 1)), "par-l1-weight": (32, 3, 2, 2, (3,)),
            "seq-n16-c3-l3-1024": (16, 3, 1024, 8, (2, 3, 1)), "seq-n32-c4-l4-1025": (32, 4, 1025, 11, (1, 3, 2, 4)),
            "seq-n28-c2-l2-lie-2049": (28, 2, 2049, 6, (3, 2)), "seq-n16-c1-l4-1100": (16, 1, 1100, 11, (2, 1, 3, 2)),
            "bf16-par": (32, 3, 6, 6, (2, 3, 1)), "f16-par": (32, 3, 6, 6, (2, 3, 1)),
            "bf16-seq": (16, 3, 1025, 5, (2, 3)), "f16-seq": (16, 3, 1025, 5, (2, 3))}
    assert set(want) == set(S.BY_NAME)
    for c in S.CASES:
        assert (c.N, c.C, c.B, c.P, tuple(ly.steps for ly in c.layers)) == want[c.name], c.name
        assert 1 <= c.L <= 4 and c.P <= 11 and c.B >= c.P
        if c.arrangement == "par":
            assert c.L > 1 and c.B < S.THRESHOLD
        elif c.arrangement == "seq":
            assert c.L > 1 and c.B >= S.THRESHOLD
        else:
            assert c.L == 1 and float(S.make_inputs(c).w[0]) != 1.0
        assert c.kind == ("cifar2" if "lie" in c.name else "cifar10")
        assert float(c.counts().sum()) == c.B and float(c.counts().min()) >= 1
    assert S.BY_NAME["par-n16-c2-l3-lie-max"].B * 3 == 3069
    assert [ly.ckpt for ly in S.BY_NAME["par-n28-c1-l2-mask"].layers] == [0b01, 0]
    assert [ly.ckpt for ly in S.BY_NAME["seq-n16-c1-l4-1100"].layers] == [0b11, 0, 0b10, 0b01]
    two = S.BY_NAME["seq-n28-c2-l2-lie-2049"]
    assert not two.weights and two.loss == ("ys", "sums") and S.make_inputs(two).w is None
    for c in S.CASES:                                     # every other case carries every loss term
        if c is not two:
            assert c.weights and c.loss == ("out", "ys", "sums"), c.name


def test_inputs_are_exact_in_the_type_they_travel_in():
    for c in S.CASES:
        inp = S.make_inputs(c)
        io = S.IO_DTYPE[c.io]
        for t in [inp.u, inp.gy] + inp.gys:
            if t is not None:
                assert torch.equal(t.to(io).double(), t), c.name
        pt = torch.float16 if c.io == "f16" else torch.float32
        for p in inp.params:
            for v in p.values():
                assert torch.equal(v.to(pt).double(), v), c.name
        if inp.w is not None:
            assert torch.equal(inp.w.to(pt).double(), inp.w)
            assert c.arrangement == "one" or abs(float(inp.w.sum()) - 1) < 2e-3


@pytest.mark.parametrize("name", ["seq-n16-c3-l3-1024", "seq-n28-c2-l2-lie-2049"])
def test_tiled_reference_is_the_materialised_one(name):
    """B = 2P + 3 (not a multiple of P): the P-sample reference with count-weighted incoming gradients against the same
    reference on all B samples with unit counts."""
    base = S.BY_NAME[name]
    case = dataclasses.replace(base, B=2 * base.P + 3)
    inp = S.make_inputs(case)
    tiled = S.reference(case, inp).flat()
    idx = case.index()
    big = S.Inputs(inp.u[idx], None if inp.gy is None else inp.gy[idx], [None if t is None else t[idx] for t in inp.gys],
                   [None if t is None else t[idx] for t in inp.gs], inp.params, inp.w)
    full = S.reference(dataclasses.replace(case, P=case.B), big, counts=torch.ones(case.B, dtype=torch.float64)).flat()
    assert set(tiled) == set(full)
    for k, v in full.items():
        t = tiled[k]
        if t.dim() >= 2 and t.shape[0] == case.P and v.shape[0] == case.B:      # per-sample: that of sample b mod P
            t = t[idx]
        assert S.rel_err(t, v) <= 1e-12, (k, S.rel_err(t, v))


@pytest.mark.parametrize("name", [c.name for c in S.F32_CASES])
def test_fp32_oracle_within_a_quarter_of_the_limit(name):
    """The reference's own fp32 arithmetic is at most a quarter of what the GPU test allows the kernel, result by
    result (measured on these cases: at most 1.4e-6 on tensors)."""
    case = S.BY_NAME[name]
    o32, lim = S.oracle32(name), S.limits(case)
    print(name, {k: f"{v:.2e}" for k, v in o32.items()})
    bad = {k: (v, lim[k]) for k, v in o32.items() if not v <= 0.25 * lim[k]}
    assert not bad, bad


@pytest.mark.parametrize("name", [c.name for c in S.IO16_CASES])
def test_state_cast_oracle_in_fp32_within_a_quarter_of_the_16_bit_limits(name):
    """The rounding reference evaluated in fp32 against the same in fp64: where the two disagree in the last fp32 bits a
    rounding point flips a 16-bit ulp, so the distance is a 16-bit ulp of a few elements.  Measured, largest result of the
    case: bf16-par 3.4e-3 (y2), bf16-seq 7.1e-7 (gu), f16-par 2.3e-4 (y1), f16-seq 1.5e-4 (y1) — a quarter of the limits
    is 5e-3 (bf16) and 5e-4 (fp16).  g_weight, which the one-layer tests have no limit for: 1.7e-4, 7.9e-8, 7.5e-6 and
    3.6e-5 in the same order; four times that is below the one-layer limit, so g_weight is held to the one-layer limit."""
    case = S.BY_NAME[name]
    o32 = S.oracle32(name)
    print(name, {k: f"{v:.2e}" for k, v in o32.items()})
    bad = {k: v for k, v in o32.items() if not v <= 0.25 * case.tol}
    assert not bad, (bad, case.tol)
    assert max(case.tol, 4 * o32["g_weight"]) == case.tol == S.limits(case)["g_weight"]


def test_varying_channels_cross_a_bound_and_no_other_does():
    for c in S.CASES:
        inp = S.make_inputs(c)
        for i, ly in enumerate(c.layers):
            want = [ch == ly.varying for ch in range(c.C)]
            assert S.moving_channels(c, i, inp.params[i]) == want, (c.name, i)
    assert S.BY_NAME["par-n28-c1-l2-mask"].layers[0].varying == 0
    assert S.BY_NAME["seq-n32-c4-l4-1025"].layers[2].varying == 2


def test_automatic_plan_parks_for_the_fashion_size_layer_only():
    from cnn_with_pde_amd import functional as F_
    seen = 0
    for c in S.CASES:
        inp = S.make_inputs(c)
        sps = 3 if c.kind == "cifar10" else 2
        for i, ly in enumerate(c.layers):
            if ly.ckpt != "auto":
                assert isinstance(ly.ckpt, int) and ly.ckpt >> (sps - 1) == 0      # a step-local mask
                continue
            km = S.kappa_max(c, i, {k: v.float().double() for k, v in inp.params[i].items()})
            bits = 0
            for k in range(ly.steps):
                bits |= F_.plan_checkpoints(km[k * sps:(k + 1) * sps])
            assert (bits != 0) == ly.fashion, (c.name, i, km)
            seen += ly.fashion
        # diffuse_shared_input fuses only groups that are all "auto" or all masks
        assert len({ly.ckpt == "auto" for ly in c.layers}) == 1, c.name
    big = S.BY_NAME["seq-n32-c4-l4-1025"]
    assert seen == 1 and [ly.fashion for ly in big.layers] == [False, True, False, False]
    assert big.layers[1].dt == 0.3


def test_layer_forward_is_the_oracle_when_nothing_is_swapped():
    case = S.BY_NAME["seq-n16-c3-l3-1024"]
    inp = S.make_inputs(case)
    a = S.O.adi_forward(inp.u, inp.params[1], case.spec(1))
    b = S.layer_forward(inp.u, inp.params[1], case.spec(1), None, (inp.params[1], case.spec(1)))
    assert torch.equal(a, b)
    # ... and with the oracle's rounding points it is the oracle's state_cast forward
    cast = lambda t: t.bfloat16().to(t.dtype)                              # noqa: E731
    a = S.O.adi_forward(inp.u, inp.params[1], case.spec(1), cast)
    b = S.layer_forward(inp.u, inp.params[1], case.spec(1), cast, None, "oracle")
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", [c.name for c in S.IO16_CASES])
def test_kernel_rounding_points_against_the_oracles(name):
    """The reference rounds where the one-launch kernel rounds (the sweep output of every step, in value only); the
    oracle's state_cast placement (also behind every operator, adjoints too) stays within the 16-bit limit of it on
    every tensor — so the limits of the one-layer tests, made with that placement, carry over — but not on g_weight of
    f16-seq (measured 4.1e-3 against the limit 2e-3: a cancelling two-entry sum), which is why the kernel's own points are
    used.  Measured on tensors, largest: bf16-par 1.2e-2, bf16-seq 9.1e-3, f16-par 1.8e-3, f16-seq 1.2e-3."""
    case = S.BY_NAME[name]
    inp, ref = S.cached(name)
    other = S.reference(case, inp, points="oracle").flat()
    dist = {k: S.rel_err(other[k], v) for k, v in ref.flat().items()}
    print(name, {k: f"{v:.2e}" for k, v in dist.items()})
    bad = {k: v for k, v in dist.items() if not v <= case.tol and k != "g_weight"}
    assert not bad, bad
    assert max(dist.values()) > 0


@pytest.mark.parametrize("name", ["par-n32-c4-l4", "seq-n16-c3-l3-1024"])
@pytest.mark.parametrize("rule", S.RULES)
def test_wrong_rule_references_are_ten_limits_away(name, rule):
    """One fault per layer position: the wrong reference differs from the right one by at least ten times the limit of
    some result the GPU test compares — that test then fails by a factor of ten on the fault."""
    case = S.BY_NAME[name]
    inp, ref = S.cached(name)
    right, lim = ref.flat(), S.limits(case)
    for which in range(case.L):
        wrong = S.reference(case, inp, rule=rule, which=which).flat()
        ratio = {k: S.rel_err(wrong[k], right[k]) / lim[k] for k in right}
        worst = max(ratio, key=ratio.get)
        assert ratio[worst] >= 10.0, (rule, which, worst, ratio[worst])
        # ... and in the output the fault belongs to
        if rule in ("drop_gs", "drop_gys"):
            assert ratio["gu"] >= 10.0 and ratio[f"g{which}.alpha_base"] >= 10.0 and ratio[f"g{which}.channel_mixing"] >= 10.0
        elif rule == "gw_shift":
            assert ratio["g_weight"] >= 10.0
        else:
            assert ratio[f"y{which}"] >= 10.0 and ratio[f"s{which}"] >= 10.0 and ratio["out"] >= 10.0


def test_one_after_the_other_faults_show_without_weights_too():
    """seq-n28-c2-l2-lie-2049 has no `out`: gradients arrive at the y_i and the plane sums only."""
    case = S.BY_NAME["seq-n28-c2-l2-lie-2049"]
    inp, ref = S.cached(case.name)
    right, lim = ref.flat(), S.limits(case)
    assert "out" not in right and "g_weight" not in right
    for rule in ("drop_gs", "drop_gys"):
        for which in range(case.L):
            wrong = S.reference(case, inp, rule=rule, which=which).flat()
            assert S.rel_err(wrong["gu"], right["gu"]) >= 10 * lim["gu"], (rule, which)
    # layer 1 alone: layer 0 gets exactly nothing
    alone = S.reference(case, inp, only_layers=(1,))
    assert all(float(v.abs().max()) == 0.0 for v in alone.gp[0].values())
    assert S.rel_err(alone.gu, ref.gu) >= 10 * lim["gu"]
