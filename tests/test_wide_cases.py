"""CPU checks of tests/wide_cases.py itself: the stage references compose to the oracle's layer, the right emulation of
the three-piece operator product is fp32 arithmetic (1e-7 of fp64), and every wrong rule is at least four bars from fp64
on the mix stage — where tests/test_gpu_wide_stages.py holds the kernel to one bar — both on the scaled input and on the
state the kernel's mix stage starts from."""
import dataclasses

import pytest
import torch

import wide_cases as W
from oracle import pde_oracle as O

IDS = [c.name for c in W.CASES]
SHAPES = sorted({(c.C, c.N) for c in W.CASES})


def _first(C, N, mode=2, split="strang"):
    return next(c for c in W.CASES if (c.C, c.N, c.mode, c.split) == (C, N, mode, split))


def test_the_matrix_is_the_sixteen_instantiations():
    """C x N x step pattern x mode, K = 3, B = 3; one draw of inputs per (C, N)."""
    assert len(W.CASES) == 16 == len(set(IDS))
    assert {(c.C, c.N, c.split, c.mode) for c in W.CASES} == {(C, N, s, m) for C in (32, 64) for N in (28, 32)
                                                              for s in ("strang", "lie") for m in (1, 2)}
    assert all(c.K == 3 and c.B == 3 for c in W.CASES)
    assert (W.MANY.C, W.MANY.N, W.MANY.split, W.MANY.mode, W.MANY.K, W.MANY.B) == (32, 28, "lie", 2, 1, 2100)
    assert W.MANY.B - W.GRID == W.MANY_HEAD                        # samples 0..51 have a partner b + 2048


@pytest.mark.parametrize("name", IDS)
def test_stages_compose_to_the_oracles_layer(name):
    """Stage after stage in float64 is ``O.adi_forward`` of the case's spec (1e-13), and the schedule is the one the
    library is given (functional.adi_schedule accumulates t the same way)."""
    case = W.BY_NAME[name]
    u, p = W.cached(case)
    stored, y = W.trajectory(case, u, p)
    q = {k: v.double() for k, v in p.items() if k != "M"}
    q["channel_mixing" if case.mode == 1 else "channel_coupling"] = p["M"].double()
    y0 = O.adi_forward(u.double(), q, case.spec())
    assert W.rel_err(y, y0) <= 1e-13
    assert len(stored) == case.K and len(case.sweeps) == case.K * case.sps
    # the named stages: mode 1 keeps sweeps_k(M prev); mode 2 keeps sweeps_k(prev') with prev' = M prev behind step 0
    prev = u
    for k in range(case.K):
        if case.mode == 1:
            assert torch.equal(W.stage_pre(prev, k, case, p), stored[k])
        else:
            inp = prev.double() if k == 0 else W.mix(prev, p["M"])
            assert torch.equal(W.stage_post_sweeps(inp, k, case, p), stored[k])
        prev = stored[k]


@pytest.mark.parametrize("C,N", SHAPES)
def test_inputs_are_what_the_module_says(C, N):
    case = _first(C, N)
    u, p = W.cached(case)
    assert u.dtype == torch.float32 and all(v.dtype == torch.float32 for v in p.values())
    M = p["M"]
    assert not torch.allclose(M, M.t()) and 0.05 < float((M - torch.eye(C)).std()) < 0.15
    amp = u.abs().amax(dim=(0, 2, 3))
    assert 1e3 < float(amp[-1] / amp[0]) < 1e5                         # four decades across the channels
    # the inputs of a (C, N) do not depend on the step pattern or the mode
    for c in W.CASES:
        if (c.C, c.N) == (C, N):
            u2, p2 = W.cached(c)
            assert torch.equal(u, u2) and all(torch.equal(p[k], p2[k]) for k in p)
    for ax in ("alpha", "beta"):
        # no coefficient at a clamp bound inside the time window: the stages are smooth in the parameters
        for _, _, t in case.sweeps:
            raw = p[ax + "_base"] + p[ax + "_time_coeff"] * t
            assert float(raw.min()) > W.EPS and float(raw.max()) < 10.0


def test_split3_is_three_exact_pieces():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4096, generator=g) * torch.logspace(-6, 6, 4096)
    hi, mid, lo = W.split3(x)
    for piece in (hi, mid, lo):
        assert torch.equal(piece.float().bfloat16().double(), piece)       # each is a bf16 number
    rest = (x.double() - hi - mid - lo).abs()
    assert float((rest / x.double().abs()).max()) <= 2.0 ** -24            # 3 x 8 significant bits: all of fp32's 24


def _margins(case, M, s):
    ref = W.mix(s, M)
    return ref, {r: W.rel_err(W.emulate(M, s, r), ref) / W.BAR for r in W.rules_for(case)}


def accept(case, seed):
    """The conditions a draw must meet; (ok, {where: {rule: distance in bars}})."""
    u, p = W.make_inputs(case, seed, B=min(case.B, 3))
    where = {"input": u}
    for split in ("strang", "lie"):
        c2 = dataclasses.replace(case, split=split, mode=2, seed=seed)
        where["state-" + split] = W.trajectory(c2, u, p)[0][-1].float()    # what the kernel's mix stage starts from
    out, ok = {}, True
    for k, s in where.items():
        ref, m = _margins(case, p["M"], s)
        out[k] = m
        ok &= W.rel_err(W.emulate(p["M"], s), ref) <= W.EMU_TOL
        ok &= all(v >= (W.MARGIN_GROSS if r in W.GROSS else W.MARGIN) for r, v in m.items())
    return ok, out


@pytest.mark.parametrize("C,N", SHAPES)
def test_right_rule_is_fp32_arithmetic_and_wrong_rules_are_four_bars_away(C, N):
    """On the mix stage, against fp64: the right emulation within 1e-7 (measured 0.8-2.3e-8; torch's fp32 matmul
    4.5 ... 7.3e-8), every wrong rule at least 4 bars of 5e-7 away (measured: one low product dropped 4.2 ... 17,
    two pieces 8.3 ... 18), bf16 / transposed / swap_halves / pad_live at least 100 (measured 4e3 and more)."""
    case = _first(C, N)
    ok, m = accept(case, case.seed)
    for k, v in m.items():
        print(case.name, k, {r: f"{x:.1f}" for r, x in v.items()})
    assert ok, m
    assert ("pad_live" in m["input"]) == (N == 28)
    u, p = W.cached(case)
    right = W.emulate(p["M"], u)
    assert W.rel_err_channel(right, W.mix(u, p["M"])) <= W.EMU_TOL       # the small channels too


def test_many_samples_case_meets_the_same_margins():
    """(On three samples of its draw: the margins are a property of M and of the channel scaling, not of the batch.)"""
    ok, m = accept(W.MANY, W.MANY.seed)
    print({k: {r: f"{x:.1f}" for r, x in v.items()} for k, v in m.items()})
    assert ok, m


def test_rejected_draws_are_recorded_truthfully():
    """RESEED lists the draws the margins rejected: each listed draw is indeed rejected (one of four so far: (32, 32),
    where the product A2 B0 dropped was 3.2 bars away)."""
    assert set(W.RESEED) <= set(SHAPES) and sum(W.RESEED.values()) <= 2
    for (C, N), n in W.RESEED.items():
        case = _first(C, N)
        for k in range(n):
            assert not accept(case, case.seed - 100 * (n - k))[0], (C, N, k)


@pytest.mark.parametrize("name", IDS)
def test_oracle32_distance_leaves_the_step_bar_meaningful(name):
    """The step stages are held to 4 x oracle32's distance.  That distance must itself be fp32 rounding, 1e-7 ... 1e-6
    (measured 2.0e-7 ... 4.0e-7), so the bar stays between fp32 accuracy and the 1e-5 of the whole-layer tests, and a
    bf16-grade operator (4e-3) or a dropped low product in front of the sweeps (2e-6 and more, undiminished: the sweeps
    do not expand the max norm) cannot pass it."""
    case = W.BY_NAME[name]
    u, p = W.cached(case)
    stored, _ = W.trajectory(case, u, p)
    prev = u
    for k in range(case.K):
        ref = W.step_stage(prev, k, case, p)
        d32 = W.rel_err(W.step_stage(prev, k, case, p, torch.float32), ref)
        assert 1e-7 <= d32 <= 1e-6, (k, d32)
        if case.mode == 1 or k > 0:
            # the operator's error arrives undiminished at the stage's output
            worst = W.rel_err(W.sweeps_k(W.emulate(p["M"], prev, "drop20"), k, case, p), ref)
            assert worst >= 0.5 * W.rel_err(W.emulate(p["M"], prev, "drop20"), W.mix(prev, p["M"])), (k, worst)
        prev = stored[k].float()
