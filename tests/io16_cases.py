"""Ground for the tests of the implicit sweeps on 16-bit tensors (tests/test_io16_cases.py on the CPU,
tests/test_gpu_io16.py on the GPU): the gates, the case table and the fp64 reference.

The contract under test (include/pdecnn.h, pde_adi_forward_states): a whole-schedule call reads its
bf16 / fp16 tensors once, computes in fp32 and rounds to nearest even once on every tensor it writes — ``y``, every
emitted state, ``gu``; the parameter gradients are fp32 sums.  So the 16-bit call is the fp32 call on the widened values,
rounded once, and three gates hold it to that:

1. ``ulps(got, fp32.to(dtype)) <= 1`` — the gate the fp16 and the explicit routes have; it cannot see the rounding mode
   (a store that truncates stays inside one ulp);
2. ``torch.equal`` where the two routes run the same template (any-size squares, rectangles);
3. ``bracket_ok(got, ref64, tau)`` — rounding is monotone, so the rounding of a value within ``tau`` of the fp64 reference
   lies between RNE(ref - tau) and RNE(ref + tau).  With ``tau`` far below an ulp the bracket is one value wide for most
   elements, which is what sees the rounding mode, a value moved by one ulp, and elements stored in the wrong place.

Nothing here needs a GPU."""
import functools

import torch

import epilogue_util as E
from oracle import pde_oracle as O

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
PARAMS = ("ab", "bb", "as", "bs")                                   # alpha_base, beta_base, alpha_slope, beta_slope

#: the schedule of every case: values a float holds exactly, so that the fp32 descriptor and the fp64 reference walk the
#: same schedule (delta, h2 = dx**2 / dy**2 and every current_time are binary fractions)
DT, DX, DY = 0.0625, 1.0, 1.25


# ---- helpers ------------------------------------------------------------------------------------------------------------
def exact(t, dtype):
    """The values of ``t`` rounded to ``dtype`` (to nearest even) and widened back to the type of ``t``."""
    return t.to(dtype).to(t.dtype)


def ulps(a, b):
    """Largest distance between two bf16 or two fp16 tensors in units in the last place: test_gpu_f16.max_ulps for fp16 (it
    is written for fp16 alone), epilogue_util.ulps16 for bf16."""
    assert a.dtype == b.dtype and a.shape == b.shape
    if a.dtype == torch.float16:
        import test_gpu_f16 as T16
        return T16.max_ulps(a, b)
    return E.ulps16(a, b)


def n_diff(a, b):
    """How many elements of two tensors of one shape and type differ."""
    assert a.shape == b.shape and a.dtype == b.dtype
    return int((a.detach().cpu() != b.detach().cpu()).sum())


def rtz(t32, dtype):
    """Finite fp32 values rounded TOWARD ZERO to bf16 / fp16 (what a store that drops the low bits writes): the nearest
    value, stepped one place toward zero where rounding went away from it (both types are sign-magnitude, so that is the
    bit pattern minus one; fp16 subnormals included)."""
    assert t32.dtype == torch.float32 and dtype in (torch.bfloat16, torch.float16)
    near = t32.contiguous().to(dtype)
    away = near.float().abs() > t32.abs()
    bits = near.view(torch.int16)
    return torch.where(away, bits - 1, bits).view(dtype)


def bracket(ref64, tau, dtype):
    """(lo, hi) in fp64: the roundings to ``dtype`` of ref - tau and ref + tau."""
    ref = ref64.detach().double().cpu()
    return (ref - tau).to(dtype).double(), (ref + tau).to(dtype).double()


def bracket_ok(got, ref64, tau):
    """The monotone-rounding test of test_gpu_epilogues._within_after_rounding, element by element:
    RNE(ref - tau) <= got <= RNE(ref + tau) in ``got``'s type.  Returns ``(True, None)`` or ``(False, worst)`` where
    ``worst`` describes the element farthest outside its bracket: index, got, lo, hi and the reference value."""
    assert got.dtype in (torch.bfloat16, torch.float16)
    ref = ref64.detach().double().cpu().reshape(got.shape)
    lo, hi = bracket(ref, tau, got.dtype)
    g = got.detach().cpu().double()
    out = torch.clamp(lo - g, min=0) + torch.clamp(g - hi, min=0)
    out = torch.where(torch.isfinite(g), out, torch.full_like(out, float("inf")))
    if not bool((out > 0).any()):
        return True, None
    i = int(out.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
    return False, {"index": idx, "got": float(g.flatten()[i]), "lo": float(lo.flatten()[i]), "hi": float(hi.flatten()[i]),
                   "ref": float(ref.flatten()[i]), "outside": int((out > 0).sum())}


# ---- the case table -----------------------------------------------------------------------------------------------------
def _case(name, family, B, C, H, W, split="strang", steps=2, smooth3=False, clamp_max=10.0, slope=0.4, ckpt=0,
          moving=False, seed=0):
    S = steps * (3 if split == "strang" else 2)
    return dict(name=name, family=family, B=B, C=C, H=H, W=W, split=split, steps=steps, smooth3=smooth3,
                clamp_max=clamp_max, slope=slope, ckpt=ckpt, moving=moving, seed=seed, eps=1e-6, num_sweeps=S,
                emit=(0, S // 2))             # the state after sweep 0 and after one middle sweep; the last one is y


FUSED_N = (8, 12, 16, 20, 24, 28, 32)
ANYSIZE_N = (5, 30, 44, 50, 82, 84, 100, 104, 128)      # both sides of the LDS limits test_gpu_anysize.test_longest_lines names
RECTS = ((5, 9), (28, 32), (2, 128), (128, 82))
MNIST = dict(smooth3=True, clamp_max=None)              # smoothed, floor only (mnist_test.py)
CIFAR = dict(smooth3=False, clamp_max=10.0)             # clamped to [eps, 10], no smoothing (cifar10.py)


def _table():
    t = []
    for N in FUSED_N:
        # (5, 3): less than one workgroup pass; (37, 1): several passes with a ragged last one.  Both splits at both batch
        # shapes would double the table for nothing: each N has both splits, both shapes and both configurations
        t.append(_case(f"fused{N}-strang-37x1-mnist", "fused", 37, 1, N, N, "strang", **MNIST, seed=1000 + N))
        t.append(_case(f"fused{N}-strang-5x3-cifar", "fused", 5, 3, N, N, "strang", **CIFAR, seed=2000 + N))
        t.append(_case(f"fused{N}-lie-5x3-mnist", "fused", 5, 3, N, N, "lie", **MNIST, seed=3000 + N))
        t.append(_case(f"fused{N}-lie-37x1-cifar", "fused", 37, 1, N, N, "lie", **CIFAR, seed=4000 + N))
    for N in (20, 32):                        # the masked body with a 16-bit IO: clamp masks that move on channels 1 and 3
        t.append(_case(f"fused{N}-moving-masks", "fused", 5, 4, N, N, "strang", **CIFAR, slope=0.2, moving=True, seed=5000 + N))
    for N in (28, 32):                        # parked fp32 states; the backward reads u in the 16-bit type
        t.append(_case(f"fused{N}-checkpoint", "fused", 5, 3, N, N, "strang", **CIFAR, ckpt=0b00100, seed=6000 + N))
    for N in ANYSIZE_N:
        t.append(_case(f"anysize{N}", "anysize", 2, 2, N, N, "strang", **CIFAR, seed=7000 + N))
    for H, W in RECTS:
        t.append(_case(f"rect{H}x{W}", "rect", 2, 2, H, W, "strang", **CIFAR, seed=8000 + 131 * H + W))
    return t


TABLE = _table()
BY_NAME = {c["name"]: c for c in TABLE}
assert len(BY_NAME) == len(TABLE)


def sweeps_of(case):
    """The schedule as the library takes it (functional.Sweep, flat)."""
    from cnn_with_pde_amd import functional as F_
    return tuple(s for st in F_.adi_schedule(DT, DX, DY, case["steps"], case["split"]) for s in st)


def spec_of(case):
    return O.AdiSpec(case["H"], case["C"], DT, DX, DY, case["steps"], case["split"], case["smooth3"], case["clamp_max"],
                     "none", False, case["eps"])


def tau_rel(case):
    """The fp32 route's bound against the oracle, relative to max|ref|: test_gpu_parity.TOL; 2e-5 where the clamp masks
    move in time (test_gpu_anysize.test_clamp_masks_that_move_in_time)."""
    return 2e-5 if case["moving"] else 1e-5


@functools.lru_cache(maxsize=None)
def inputs(name, dname):
    """Seeded inputs of one case for one 16-bit type: fp32 tensors; ``u``, ``gy`` and ``gstates`` (one cotangent per
    emitted state, in the order of ``emit``) hold values exact in that type, the four parameter planes stay fp32.  The
    cached tensors are shared: never written."""
    c, dt = BY_NAME[name], DTYPES[dname]
    g = torch.Generator().manual_seed(c["seed"])
    B, Cc, H, W = c["B"], c["C"], c["H"], c["W"]
    base = 2.0 if c["smooth3"] else 1.0
    p = {"ab": base * (1 + 0.15 * torch.randn(Cc, H, W, generator=g)), "bb": base * (1 + 0.15 * torch.randn(Cc, H, W, generator=g)),
         "as": c["slope"] * torch.randn(Cc, H, W, generator=g), "bs": c["slope"] * torch.randn(Cc, H, W, generator=g)}
    if c["moving"]:
        # test_gpu_asm_bwd.test_channels_with_moving_clamp_masks_share_the_call: base + slope * t crosses the floor inside
        # the time window at some points of channels 1 and 3 (alpha at t = 1/15, beta at t = 1/20; the sweeps sit at
        # multiples of 1/32 up to 1/8)
        for ch in (1, 3):
            p["ab"][ch, ::3, ::2] = 0.02
            p["as"][ch, ::3, ::2] = -0.3
            p["bb"][ch, 1::4, :] = 0.01
            p["bs"][ch, 1::4, :] = -0.2
    out = {k: v.contiguous() for k, v in p.items()}
    out["u"] = exact(torch.randn(B, Cc, H, W, generator=g), dt)
    out["gy"] = exact(torch.randn(B, Cc, H, W, generator=g), dt)
    out["gstates"] = exact(torch.randn(len(c["emit"]), B, Cc, H, W, generator=g), dt)
    return out


def oracle_states(case, u, params):
    """The oracle's time loop (pde_oracle.adi_forward without a channel operator) with the states after the sweeps in
    ``emit`` kept: (len(emit) + 1, B, C, H, W), the last slice the output.  Differentiable, any float type.  The
    trajectory tests take the state after a time STEP from ``adi_forward`` built with fewer steps; sweep 0 is no step
    boundary, so the same loop is walked here sweep by sweep with the oracle's own functions (the last slice is
    ``adi_forward`` bit for bit: tests/test_io16_cases.py)."""
    spec = spec_of(case)
    keep = []
    for s, (axis, delta, t) in enumerate(O.sweep_schedule(spec)):
        if axis == 0:
            u = O._implicit_sweep(u, O.coefficient_at(params["ab"], params["as"], t, spec), 0, delta, spec.dx, spec)
        else:
            u = O._implicit_sweep(u, O.coefficient_at(params["bb"], params["bs"], t, spec), 1, delta, spec.dy, spec)
        if s in case["emit"]:
            keep.append(u)
    return torch.stack(keep + [u])


@functools.lru_cache(maxsize=None)
def reference(name, dname, grads=True):
    """fp64 reference of one case on the exact values: ``states`` (the emitted states, then y) and, with ``grads``, ``gu``
    for the cotangents of ``inputs`` (gstates on the emitted states, gy on y)."""
    c, inp = BY_NAME[name], inputs(name, dname)
    params = {k: inp[k].double() for k in PARAMS}
    if not grads:
        with torch.no_grad():
            return {"states": oracle_states(c, inp["u"].double(), params)}
    cot = torch.cat([inp["gstates"], inp["gy"][None]]).double()
    states, gu, _ = O.value_and_grads(lambda a, p: oracle_states(c, a, p), inp["u"].double(), params, cot)
    return {"states": states, "gu": gu}


def expected_kernels(case, io_f32, env):
    """(pde_adi_forward_kernel, pde_adi_backward_kernel) of the plain call of a square case, from the rules in
    include/pdecnn.h: 2 / 2 off the fused line lengths; at N = 32 on fp32 tensors and Strang steps the hand-over forward
    (3: more sweeps than stay resident) and, without checkpoints, the assembly backward (1); the HIP kernels (0) for
    everything else, 16-bit tensors included.  ``env``: the two switches that turn 3 and 1 into 0."""
    if case["family"] != "fused":
        return 2, 2
    fast = io_f32 and case["H"] == 32 and case["split"] == "strang" and case["num_sweeps"] >= 6
    if not fast:
        return 0, 0
    fwd = 1 if env.get("PDE_ASM_FWD", "")[:1] == "1" else (0 if env.get("PDE_FWD_SCHED", "")[:1] == "0" else 3)
    bwd = 0 if case["ckpt"] or env.get("PDE_ASM_BWD", "")[:1] == "0" else 1
    return fwd, bwd
