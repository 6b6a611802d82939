"""tests/io16_cases.py on the CPU: the case table is what it says it is, and the gates of tests/test_gpu_io16.py bite.

"Kernel outputs" are fabricated from the oracle: the fp32 oracle's states rounded to nearest even (a correct kernel), the
same rounded toward zero, one element moved by one ulp, two neighbours of a row swapped, a plane's rows shifted by one
packed 8-byte store.  The ulp gate alone lets the first three through; the bracket stops all but the correct one."""
import dataclasses

import pytest
import torch

import io16_cases as K
from oracle import pde_oracle as O

ALL = [(c["name"], d) for c in K.TABLE for d in K.DTYPES]
HANDFUL = ["fused12-strang-37x1-mnist", "fused12-lie-5x3-mnist", "fused32-moving-masks", "anysize30", "rect5x9"]


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_every_listed_path_is_present():
    fused = [c for c in K.TABLE if c["family"] == "fused"]
    for N in (8, 12, 16, 20, 24, 28, 32):
        mine = [c for c in fused if c["H"] == N and not c["moving"] and not c["ckpt"]]
        assert all(c["H"] == c["W"] and c["steps"] == 2 for c in mine)
        assert {c["split"] for c in mine} == {"strang", "lie"}
        assert {(c["B"], c["C"]) for c in mine} == {(5, 3), (37, 1)}
        assert {(c["smooth3"], c["clamp_max"]) for c in mine} == {(True, None), (False, 10.0)}
        for split in ("strang", "lie"):                    # each split at both batch shapes and both configurations
            assert len({(c["B"], c["smooth3"]) for c in mine if c["split"] == split}) == 2
    assert sorted(c["H"] for c in fused if c["moving"]) == [20, 32] and all(c["C"] == 4 for c in fused if c["moving"])
    assert sorted(c["H"] for c in fused if c["ckpt"]) == [28, 32]
    assert [c["H"] for c in K.TABLE if c["family"] == "anysize"] == [5, 30, 44, 50, 82, 84, 100, 104, 128]
    assert all((c["B"], c["C"], c["steps"], c["split"]) == (2, 2, 2, "strang") for c in K.TABLE if c["family"] == "anysize")
    assert [(c["H"], c["W"]) for c in K.TABLE if c["family"] == "rect"] == [(5, 9), (28, 32), (2, 128), (128, 82)]
    for c in K.TABLE:
        S = c["num_sweeps"]
        assert S == len(K.sweeps_of(c)) == len(O.sweep_schedule(K.spec_of(c)))
        assert c["emit"][0] == 0 and 0 < c["emit"][1] < S - 1           # sweep 0, a middle sweep; the last one is y
        assert c["slope"] != 0.0
        assert 0 <= c["ckpt"] < 1 << (S - 1)
        fam = "fused" if c["H"] == c["W"] and c["H"] % 4 == 0 and 8 <= c["H"] <= 32 else ("anysize" if c["H"] == c["W"] else "rect")
        assert c["family"] == fam, c["name"]


def test_the_schedule_is_the_oracles_and_exact_in_fp32():
    for split, steps in (("strang", 2), ("lie", 2)):
        c = K._case("x", "fused", 1, 1, 8, 8, split, steps)
        for s, (axis, delta, t) in zip(K.sweeps_of(c), O.sweep_schedule(K.spec_of(c))):
            assert (s.axis, s.delta, s.t) == (axis, delta, t)
            assert s.h2 == (K.DX ** 2 if axis == 0 else K.DY ** 2)
            for v in (s.delta, s.h2, s.t):
                assert float(torch.tensor(v, dtype=torch.float32)) == v


@pytest.mark.parametrize("name,dname", ALL)
def test_inputs_are_exact_seeded_and_stable(name, dname):
    c, dt = K.BY_NAME[name], K.DTYPES[dname]
    a, b = K.inputs(name, dname), K.inputs.__wrapped__(name, dname)
    assert set(a) == {"u", "gy", "gstates", *K.PARAMS}
    for k in a:
        assert a[k].dtype == torch.float32 and a[k].is_contiguous() and torch.equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all())
    shape = (c["B"], c["C"], c["H"], c["W"])
    assert tuple(a["u"].shape) == tuple(a["gy"].shape) == shape and tuple(a["gstates"].shape) == (len(c["emit"]),) + shape
    for k in ("u", "gy", "gstates"):
        assert torch.equal(K.exact(a[k], dt), a[k]), k                   # every value exact in its type
        assert float(a[k].abs().max()) > 1.0
    for k in K.PARAMS:
        assert tuple(a[k].shape) == shape[1:]
        assert not torch.equal(K.exact(a[k], dt), a[k]), k               # the parameters stay fp32
    assert not torch.equal(a["u"], a["gy"])
    assert float(a["as"].abs().max()) > 0 and float(a["bs"].abs().max()) > 0


def test_seeds_differ():
    seeds = [c["seed"] for c in K.TABLE]
    assert len(set(seeds)) == len(seeds)


@pytest.mark.parametrize("name", ["fused20-moving-masks", "fused32-moving-masks"])
def test_clamp_masks_move_on_channels_1_and_3_only(name):
    c, inp = K.BY_NAME[name], K.inputs(name, "bf16")
    spec = K.spec_of(c)
    masks = {0: [], 1: []}
    for axis, _, t in O.sweep_schedule(spec):
        raw = inp["ab" if axis == 0 else "bb"] + inp["as" if axis == 0 else "bs"] * t
        masks[axis].append((raw > spec.eps) & (raw < spec.clamp_max))
    for axis in (0, 1):
        moved = torch.stack([m != masks[axis][0] for m in masks[axis]]).any(0)           # (C, H, W)
        assert [bool(moved[ch].any()) for ch in range(4)] == [False, True, False, True], axis


@pytest.mark.parametrize("name", HANDFUL + ["fused28-checkpoint", "rect128x82"])
def test_last_slice_is_the_oracles_forward_bit_for_bit(name):
    c, inp = K.BY_NAME[name], K.inputs(name, "f16")
    names = {"ab": "alpha_base", "bb": "beta_base", "as": "alpha_time_coeff", "bs": "beta_time_coeff"}
    for dt in (torch.float32, torch.float64):
        p = {k: inp[k].to(dt) for k in K.PARAMS}
        with torch.no_grad():
            st = K.oracle_states(c, inp["u"].to(dt), p)
            y = O.adi_forward(inp["u"].to(dt), {names[k]: v for k, v in p.items()}, K.spec_of(c))
            mid = O.adi_forward(inp["u"].to(dt), {names[k]: v for k, v in p.items()},
                                dataclasses.replace(K.spec_of(c), num_steps=1))
        assert st.shape[0] == 3 and torch.equal(st[-1], y)
        assert not torch.equal(st[1], mid)            # the middle sweep opens step 2: no state a step boundary would give
        assert not torch.equal(st[0], st[1]) and not torch.equal(st[1], st[2])


# ---- the gates ----------------------------------------------------------------------------------------------------------
def _states32(name, dname):
    """The fp32 oracle's states on the exact values: the stand-in for a correct kernel's fp32 registers."""
    c, inp = K.BY_NAME[name], K.inputs(name, dname)
    with torch.no_grad():
        return K.oracle_states(c, inp["u"], {k: inp[k] for k in K.PARAMS})


@pytest.mark.parametrize("name,dname", ALL)
def test_truncation_passes_the_ulp_gate_and_fails_the_bracket(name, dname):
    c, dt = K.BY_NAME[name], K.DTYPES[dname]
    ref = K.reference(name, dname, False)["states"]
    x32 = _states32(name, dname)
    for i in range(ref.shape[0]):
        tau = K.tau_rel(c) * float(ref[i].abs().max())
        assert float((x32[i].double() - ref[i]).abs().max()) <= tau          # the fp32 route's bound holds for the stand-in
        rne, cut = x32[i].to(dt), K.rtz(x32[i], dt)
        ok, worst = K.bracket_ok(rne, ref[i], tau)
        assert ok, worst
        assert K.ulps(rne, x32[i].to(dt)) == 0
        frac = K.n_diff(rne, cut) / rne.numel()
        assert frac >= 0.25, (name, i, frac)                                 # a condition on the inputs: the seeds meet it
        assert K.ulps(cut, rne) == 1                                         # the old gate: passes
        ok, worst = K.bracket_ok(cut, ref[i], tau)
        assert not ok and worst["outside"] >= 0.2 * rne.numel(), worst      # the new one: fails, and not by one element


def _bump(t16, idx):
    """``t16`` with the element at flat index ``idx`` moved one ulp away from zero."""
    bits = t16.clone().contiguous().view(torch.int16)
    bits.view(-1)[idx] += 1
    return bits.view(t16.dtype)


@pytest.mark.parametrize("dname", list(K.DTYPES))
@pytest.mark.parametrize("name", HANDFUL)
def test_fabricated_faults(name, dname):
    c, dt = K.BY_NAME[name], K.DTYPES[dname]
    ref = K.reference(name, dname, False)["states"][-1]
    tau = K.tau_rel(c) * float(ref.abs().max())
    good = _states32(name, dname)[-1].to(dt)
    assert K.bracket_ok(good, ref, tau)[0]
    lo, hi = K.bracket(ref, tau, dt)
    tight = (lo == hi).flatten()
    # tau is below an ulp wherever |value| > max|ref| / 400 (bf16) or / 50 (fp16; / 25 at the moving masks' 2e-5): from
    # half (fp16, moving masks) to 94 % (bf16) of the brackets are one value wide
    assert float(tight.double().mean()) > 0.4
    # one element moved by one ulp
    i = int(tight.nonzero()[0])
    moved = _bump(good, i)
    assert K.n_diff(moved, good) == 1 and K.ulps(moved, good) == 1
    ok, worst = K.bracket_ok(moved, ref, tau)
    assert not ok and worst["outside"] == 1 and worst["index"] == tuple(int(v) for v in torch.unravel_index(torch.tensor(i), good.shape))
    # two adjacent elements of a row swapped: the first pair of different values whose brackets are both tight
    flat = good.flatten()
    W = c["W"]
    pair = next(j for j in range(flat.numel() - 1) if j % W != W - 1 and bool(tight[j]) and bool(tight[j + 1])
                and float(flat[j]) != float(flat[j + 1]))
    swapped = flat.clone()
    swapped[pair], swapped[pair + 1] = flat[pair + 1], flat[pair]
    ok, worst = K.bracket_ok(swapped.view(good.shape), ref, tau)
    assert not ok and worst["outside"] == 2
    # every row of a plane lands one packed store (four 16-bit values) late
    shifted = good.clone()
    shifted[0, 0] = torch.roll(good[0, 0].flatten(), 4).view(c["H"], W)
    ok, worst = K.bracket_ok(shifted, ref, tau)
    assert not ok and worst["index"][:2] == (0, 0)
    # NaN and infinity are outside every bracket
    bad = good.clone()
    bad.view(-1)[3] = float("nan")
    assert not K.bracket_ok(bad, ref, tau)[0]


def test_helpers_on_small_vectors():
    for dt, drop in ((torch.bfloat16, 16), (torch.float16, 13)):
        x = torch.tensor([1.0, 1.0 + 2.0 ** -(23 - drop) * 0.75, -3.0 - 2.0 ** -(22 - drop) * 0.75, 0.5, -0.0])
        assert torch.equal(K.exact(x, dt), x.to(dt).float())
        cut = K.rtz(x, dt)
        assert cut.tolist() == [1.0, 1.0, -3.0, 0.5, -0.0]                    # toward zero on both signs
        assert K.n_diff(cut, x.to(dt)) == 2 and K.ulps(cut, x.to(dt)) == 1
        ok, worst = K.bracket_ok(cut, x.double(), 1e-9)
        assert not ok and worst["index"] == (2,) and worst["outside"] == 2       # the one farthest outside: the larger ulp
        assert K.bracket_ok(x.to(dt), x.double(), 1e-9) == (True, None)
    assert K.expected_kernels(K.BY_NAME["anysize30"], True, {}) == (2, 2)
    assert K.expected_kernels(K.BY_NAME["fused32-strang-37x1-mnist"], True, {}) == (3, 1)
    assert K.expected_kernels(K.BY_NAME["fused32-strang-37x1-mnist"], False, {}) == (0, 0)
    assert K.expected_kernels(K.BY_NAME["fused32-checkpoint"], True, {}) == (3, 0)
    assert K.expected_kernels(K.BY_NAME["fused32-lie-37x1-cifar"], True, {}) == (0, 0)
    assert K.expected_kernels(K.BY_NAME["fused28-checkpoint"], True, {}) == (0, 0)
