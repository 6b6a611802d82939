"""CPU checks of tests/adi_edge_cases.py itself: the reference is the oracle's autograd, the designated coefficients are
bit-identical in fp32 and fp64, the blocked elements have gradient exactly 0, the plain fp32 oracle's own noise leaves
room under the tolerance, and every wrong-rule reference is at least ten tolerances away where the GPU tests look."""
import pytest
import torch

import adi_edge_cases as E
import golden_util as G
from oracle import pde_oracle as O

IDS = [c.name for c in E.CASES]


def _oracle_spec(case):
    return O.AdiSpec(case.N, case.C, E.DT, case.dx, case.dy, case.steps, case.sched, case.smooth3, case.clamp_max,
                     case.mix, False, E.EPS)


@pytest.mark.parametrize("name", ["A-n8-c3-strang", "A-n12-c2-smooth-all", "A-n20-c3-lie-auto", "A-n32-c3-lie-dx2",
                                  "C-c5-pre", "C-c8-post-smooth", "D-c4-n16-post",
                                  "G-c32-n28-strang-pre-smooth", "G-c64-n32-lie-post", "G-c32-n32-strang-post-smooth"])
def test_reference_is_the_oracles_autograd(name):
    """Strang and Lie schedules, with and without a channel operator: 1e-13 of ``O.adi_forward`` under autograd."""
    case = E.BY_NAME[name]
    (u, p, gy), (y, gu, gp) = E.cached(case)
    q = {k: v for k, v in p.items() if k != "M"}
    if case.mix != "none":
        q["channel_mixing" if case.mix == "pre" else "channel_coupling"] = p["M"]
    spec = _oracle_spec(case)
    y0, gu0, gp0 = O.value_and_grads(lambda a, r: O.adi_forward(a, r, spec), u, q, gy)
    assert G.rel_err(y, y0) <= 1e-13 and G.rel_err(gu, gu0) <= 1e-13
    for k in E.NAMES:
        assert G.rel_err(gp[k], gp0[k]) <= 1e-13, k
    if case.mix != "none":
        assert G.rel_err(gp["M"], gp0["channel_mixing" if case.mix == "pre" else "channel_coupling"]) <= 1e-13


@pytest.mark.parametrize("name", IDS)
def test_every_coefficient_is_exact_in_fp32(name):
    """base + slope*t of EVERY element at every sweep — the designated ones included — is the same number in fp32 and
    fp64 (so a tie is a tie in both, contracted to an FMA or not), and so is the pass-through mask."""
    case = E.BY_NAME[name]
    u, p, gy = E.make_inputs(case)
    for axis, delta, t in case.sweeps:
        ax = "alpha" if axis == 0 else "beta"
        b, s = p[ax + "_base"], p[ax + "_time_coeff"]
        assert torch.equal(b.float().double(), b) and torch.equal(s.float().double(), s)
        prod32 = s.float() * torch.tensor(t, dtype=torch.float32)
        assert torch.equal(prod32.double(), s * t)                       # the product is exact: an FMA changes nothing
        raw32 = b.float() + prod32
        assert torch.equal(raw32.double(), b + s * t)
        assert float(torch.tensor(t, dtype=torch.float32)) == t and float(torch.tensor(delta, dtype=torch.float32)) == delta
    for q in E.placements(case):
        assert p[q.axis + "_base"][q.c, q.i, q.j] == q.base and p[q.axis + "_time_coeff"][q.c, q.i, q.j] == q.slope
    if case.io == "f16":                                                  # parameters travel as fp16 there
        for k in E.NAMES:
            assert torch.equal(p[k].half().double(), p[k]), k


@pytest.mark.parametrize("name", IDS)
def test_scenarios_do_what_the_table_says(name):
    case = E.BY_NAME[name]
    (u, p, gy), (y, gu, gp) = E.cached(case)
    placed = E.placements(case)
    seen = {(q.c, q.axis, q.i, q.j) for q in placed}
    assert len(seen) == len(placed)                                        # no two scenarios on one element
    has = {0: any(a == 0 for a, _, _ in case.sweeps), 1: any(a == 1 for a, _, _ in case.sweeps)}
    for q in placed:
        times = [t for a, _, t in case.sweeps if a == (0 if q.axis == "alpha" else 1)]
        passes = [bool(E.pass_mask(torch.tensor(q.base + q.slope * t, dtype=torch.float64), case)) for t in times]
        gb, gs = gp[q.axis + "_base"][q.c, q.i, q.j], gp[q.axis + "_time_coeff"][q.c, q.i, q.j]
        if q.scen in E.ZERO:
            assert not any(passes)
            assert float(gb) == 0.0 and float(gs) == 0.0, q
        elif q.scen in ("S1", "S3"):
            assert all(passes)
            if times:
                assert float(gb) != 0.0, q
        elif q.scen in ("S5", "S8"):
            assert passes[:-1] == [True] * (len(times) - 1) and not passes[-1]
            if q.scen == "S8":
                last = max(i for i, (a, _, _) in enumerate(case.sweeps) if a == 0)
                assert last >= 64
        elif q.scen == "S7":
            k = passes.index(False)
            assert 0 < k and not any(passes[k:]) and q.base + q.slope * times[k - 1] == case.clamp_max
    if not has[1]:
        assert not gp["beta_base"].any() and not gp["beta_time_coeff"].any()
    # exactly the designed channel is flagged
    moving = {q.c for q in placed if q.scen in E.MOVING}
    assert E.expected_flags(case, p) == [c in moving for c in range(case.C)]
    if case.C > 1 and moving:
        assert moving == {case.cstar} and case.cnon != case.cstar


def _separation(case, right, wrong):
    """{rule: smallest separation over the elements that rule is judged at}, in units of the tensor's maximum."""
    gp, out = right[2], {}
    has_y = any(a == 1 for a, _, _ in case.sweeps)

    def at(rule, q):
        return max(abs(float(wrong[rule][2][k][q.c, q.i, q.j] - gp[k][q.c, q.i, q.j])) / float(gp[k].abs().max())
                   for k in (q.axis + "_base", q.axis + "_time_coeff"))

    judged = {"strict": ("S1", "S3"), "first": E.MOVING, "t0": ("S6",)}
    for rule, scens in judged.items():
        vals = [at(rule, q) for q in E.placements(case) if q.scen in scens and (q.axis == "alpha" or has_y)]
        if vals:
            out[rule] = min(vals)
    if case.smooth3:
        vals = []
        for ax, (c, m) in E.line_ends(case).items():
            if ax == "beta" and not has_y:
                continue
            k = ax + "_base"
            vals.append(float((wrong["end1"][2][k][c] - gp[k][c])[m].abs().max()) / float(gp[k].abs().max()))
        out["end1"] = min(vals)
    return out


def accept(case, seed):
    """The two conditions a draw must meet; returns (ok, worst fp32-oracle error, {rule: separation})."""
    u, p, gy = E.make_inputs(case, seed)
    right = E.reference(case, u, p, gy)
    noise = 0.0
    if case.io == "f32":
        y32, gu32, gp32 = E.reference(case, u, p, gy, dtype=torch.float32)
        noise = max([G.rel_err(y32, right[0]), G.rel_err(gu32, right[1])] +
                    [G.rel_err(gp32[k], right[2][k]) for k in gp32 if float(right[2][k].abs().max()) > 0])
    wrong = {r: E.reference(case, u, p, gy, rule=r) for r in E.RULES if r != "end1" or case.smooth3}
    sep = _separation(case, right, wrong)
    ok = noise <= case.tol / 2 and all(v >= 10 * case.tol for v in sep.values())
    return ok, noise, sep


@pytest.mark.parametrize("name", [c.name for c in E.CASES if c.io in ("f32", "f64")])
def test_noise_and_separation(name):
    """The stored draw of every case: the plain fp32 oracle within half the tolerance of fp64 per tensor, every wrong rule
    at least ten tolerances away at the elements it is about.  (Measured over the cases: fp32 oracle 1.8e-7 .. 1.6e-6,
    smallest separation 5.8e-4; the 66-sweep case 8.2e-3 against the 2e-4 it needs.)"""
    case = E.BY_NAME[name]
    ok, noise, sep = accept(case, case.seed)
    print(name, f"noise {noise:.2e}", {k: f"{v:.2e}" for k, v in sep.items()})
    assert ok, (noise, sep, case.tol)
    # the rules this case can host are judged somewhere
    scens = {q.scen for q in E.placements(case)}
    assert ("strict" in sep) and (("first" in sep) == bool(scens & set(E.MOVING))) and (("t0" in sep) == ("S6" in scens))


def test_rejected_draws_are_few_and_recorded_truthfully():
    """RESEED lists the draws the conditions rejected: each listed draw is indeed rejected, and they are at most one in
    ten of all draws (more would mean the generator, not the draw, is wrong)."""
    assert set(E.RESEED) <= set(E.BY_NAME)
    rejected = sum(E.RESEED.values())
    assert rejected * 10 <= len(E.CASES) + rejected
    for name, n in E.RESEED.items():
        case = E.BY_NAME[name]
        for k in range(n):
            assert not accept(case, case.seed - 100 * (n - k))[0], (name, k)


def test_f64_bound_from_two_summation_orders():
    """The 1e-12 held against float64 tensors (at most 9 sweeps): every operation of a sweep is a double rounding, 2**-53
    each; a line solve of 16 unknowns chains ~5 of them per unknown in each direction and a gradient adds 9 sweeps and B
    planes — a few hundred roundings, ~1e-13 relative in the worst case.  The reference's own fp64 evaluated in two
    summation orders (batch reversed, so every parameter gradient is accumulated the other way round) shows its share:
    it must stay under a tenth of the bound."""
    case = E.BY_NAME["E-n16-f64"]
    assert len(case.sweeps) <= 9 and case.tol == 1e-12
    (u, p, gy), (y, gu, gp) = E.cached(case)
    y2, gu2, gp2 = E.reference(case, u.flip(0), p, gy.flip(0))
    errs = [G.rel_err(y2.flip(0), y), G.rel_err(gu2.flip(0), gu)] + [G.rel_err(gp2[k], gp[k]) for k in E.NAMES]
    print("fp64 reference, two orders:", [f"{e:.1e}" for e in errs])
    assert max(errs) <= 1e-13


@pytest.mark.parametrize("case,where", E.kappa_cases(), ids=[c.name for c, _ in E.kappa_cases()])
def test_kappa_cases_have_a_unique_exact_peak(case, where):
    u, p, gy = E.make_inputs(case)
    q = E.place_kappa_peak(case, p, where)
    want = E.kappa_reference(case, q)
    for (axis, delta, t), v in zip(case.sweeps, want):
        h = case.dx if axis == 0 else case.dy
        ax = "alpha" if axis == 0 else "beta"
        th = O.coefficient_at(q[ax + "_base"], q[ax + "_time_coeff"], t, case.spec())
        assert int((th == th.max()).sum()) == 1                            # the peak is one element ...
        peak = min(16.0 if where == "clamped" else 4.0, case.clamp_max or 1e9)
        assert float(th.max()) == peak
        if not case.smooth3:
            assert v == peak * delta / h ** 2                              # ... and decides the maximum
            assert float(torch.tensor(v, dtype=torch.float32)) == v        # exact in fp32
        else:
            assert v < peak * delta / h ** 2 and v > (peak / 3) * delta / h ** 2
    if where == "clamped":
        assert case.clamp_max is not None
