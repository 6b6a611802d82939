"""Case generators and fp64 references for the coefficient stage of the implicit (ADI) layers: theta = clamp(base +
slope*t, eps[, max]) (mnist_test.py:33-42, cifar10.py:53-63), the optional 3-tap smoothing (mnist_test.py:135-149), the
clamp's pass-through mask in the backward, the per-channel "mask moves in time" flag and the per-sweep coefficient maxima.
tests/test_adi_edge_cases.py checks what is built here on the CPU; tests/test_gpu_adi_edges.py holds every kernel path to it
(families A .. G; G is the one-launch wide forward at C = 32 / 64 with its lane-major copy of the coefficient records).

Exact inputs.  Everything that decides a mask is dyadic — eps = 2**-20, clamp_max = 8, dt = 2**-4, bases multiples of 2**-6,
slopes multiples of 2**-3, sweep times multiples of dt/2 — so base + slope*t has at most 24 significant bits: a tie with a
clamp bound is a tie in fp32, in fp64 and under FMA contraction alike.

Scenarios (the element's own parameters; every other element of the case is a seeded draw that never reaches a bound):

    S1 alpha  base = eps, slope 0                 passes (>= eps), gradient non-zero
    S2 alpha  base = 0, slope 0                   blocked on every sweep: gradients exactly 0
    S3 beta   base = clamp_max, slope 0           passes (<= max)
    S4 beta   base = clamp_max + over, slope 0    blocked: exactly 0 (over = 2**-20; 2**-7 where parameters are fp16)
    S5 alpha  slope 1, above clamp_max at the LAST x sweep only: one element at one sweep sets the channel's flag
    S6 beta   slope -1, base 2**-6: passes at t = 0, below eps from the first y sweep (t >= dt/2) on: exactly 0, and the
              mask does NOT move between the y sweeps (the channel stays unflagged: its mask is taken at t_first[y])
    S7 either slope 1, theta == clamp_max exactly at a middle sweep of its axis and above it afterwards: a tie, then blocked
    S8 alpha  S5 on the 22-step Strang schedule (66 sweeps): the single flip is at sweep 65

Designated positions: the four corners, the junction of the two half lines (m-1, m) and (m, m-1), and (N-1, m); which
scenario sits where rotates with the case's ``rot``.  With C > 1 the moving scenarios (S5, S7, S8) sit in channel ``cstar``
(with S1, S2: ties inside the masked body) — the ONLY flagged channel — and the static ones in channel ``cnon`` = cstar+1,
whose line ends are also compared (the ownership check: every channel is computed by exactly one backward body).

Wrong-rule references: the same computation with one plausible mistake in the BACKWARD's mask or smoothing ("strict":
> / < at the bounds; "first": every sweep's mask taken from its axis' first sweep; "t0": every mask evaluated at t = 0;
"end1": the transposed 3-tap average with end weight 1 instead of 2).  The CPU tests require each of them to differ from
the right reference by at least ten tolerances where the GPU tests look, so each mistake fails there by a factor of ten.
"""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from oracle import pde_oracle as O

EPS = 2.0 ** -20
CMAX = 8.0
DT = 2.0 ** -4
HALF = DT / 2
NAMES = ["alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff"]
TOL = 1e-5            # the project's standing bound for this family (max-norm relative, golden_util.rel_err)
TOL_LONG = 2e-5       # schedules of 66 sweeps (tests/test_gpu_parity.py::test_schedules_longer_than_one_launch)
TOL_F64 = 1e-12       # float64 tensors, at most 9 sweeps: see test_adi_edge_cases.py::test_f64_bound_from_two_summation_orders
RULES = ("strict", "first", "t0", "end1")
MOVING = ("S5", "S7", "S8")
ZERO = ("S2", "S4", "S6")


# --------------------------------------------------------------------------------------------------------------------- #
# schedules: tuples of (axis, delta, t) like oracle.pde_oracle.sweep_schedule                                            #
# --------------------------------------------------------------------------------------------------------------------- #
def schedule(kind: str, steps: int = 0) -> Tuple[Tuple[int, float, float], ...]:
    if kind in ("strang", "lie"):
        return tuple(O.sweep_schedule(O.AdiSpec(dt=DT, num_steps=steps, split=kind)))
    if kind == "xyxxy":       # neither Strang nor Lie: the kernels look the axis of every sweep up
        return ((0, HALF, 0.0), (1, DT, HALF), (0, HALF, HALF), (0, HALF, 2 * HALF), (1, DT, 3 * HALF))
    if kind == "xonly":
        return ((0, HALF, 0.0), (0, HALF, HALF), (0, HALF, 2 * HALF))
    raise ValueError(kind)


@dataclass(frozen=True)
class Case:
    name: str
    family: str                       # "A" .. "G"
    N: int
    C: int
    B: int
    sched: str = "strang"
    steps: int = 2
    clamp_max: Optional[float] = CMAX
    smooth3: bool = False
    ckpt: object = 0                  # 0, "all", "auto" or an int mask
    dx: float = 1.0
    dy: float = 1.0
    cstar: int = 0
    rot: int = 0
    moving: bool = True               # place S5 / S7 / S8 (needs clamp_max)
    seed: int = 0
    W: Optional[int] = None           # rectangle: N rows, W columns
    io: str = "f32"                   # "f32" | "bf16" | "f16" | "f64"
    mix: str = "none"                 # "pre" | "post": a channel operator M between the steps
    emit: Tuple[int, ...] = ()        # adi_diffuse_states: emitted sweeps before the last
    gy_last_zero: bool = False        # family F: only the emitted state carries a cotangent

    @property
    def sweeps(self):
        return schedule(self.sched, self.steps)

    @property
    def shape(self):
        return (self.N, self.W if self.W else self.N)

    @property
    def tol(self):
        if self.io == "f64":
            return TOL_F64
        return TOL_LONG if len(self.sweeps) >= 64 else TOL

    @property
    def over(self):
        return 2.0 ** -7 if self.io == "f16" else 2.0 ** -20

    @property
    def cnon(self):
        return (self.cstar + 1) % self.C

    def spec(self) -> O.AdiSpec:
        return O.AdiSpec(self.N, self.C, DT, self.dx, self.dy, self.steps, "strang", self.smooth3, self.clamp_max, "none",
                         False, EPS)

    def ckpt_bits(self):
        S = len(self.sweeps)
        return (1 << (S - 1)) - 1 if self.ckpt == "all" else self.ckpt


def positions(H: int, W: int) -> List[Tuple[int, int]]:
    mh, mw = H // 2, W // 2
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (mh - 1, mw), (mh, mw - 1), (H - 1, mw)]


@dataclass(frozen=True)
class Placed:
    scen: str
    axis: str          # "alpha" | "beta"
    c: int
    i: int
    j: int
    base: float
    slope: float


def _times(case: Case, axis: int) -> List[float]:
    return [t for a, _, t in case.sweeps if a == axis]


def placements(case: Case) -> List[Placed]:
    """Which scenario sits at which element of which channel."""
    tx, ty = _times(case, 0), _times(case, 1)
    cm = case.clamp_max
    static = [("S1", "alpha", EPS, 0.0), ("S2", "alpha", 0.0, 0.0)]
    if cm is not None:
        static += [("S3", "beta", cm, 0.0), ("S4", "beta", cm + case.over, 0.0)]
    if ty and min(ty) >= HALF:
        static.append(("S6", "beta", 2.0 ** -6, -1.0))
    moving = []
    if cm is not None and case.moving:
        # (a case whose last state carries no cotangent cannot see the last sweep: no S5 there)
        if len(tx) >= 2 and tx.count(max(tx)) == 1 and tx[-1] == max(tx) and not case.gy_last_zero:
            moving.append(("S8" if len(case.sweeps) >= 64 else "S5", "alpha", cm - max(tx) + 2.0 ** -6, 1.0))
        ax7 = "beta" if (case.rot % 2 and len(set(ty)) >= 3) else "alpha"
        uniq = sorted(set(ty if ax7 == "beta" else tx))
        if len(uniq) >= 3 and len(case.sweeps) < 64:      # (S8's flip must be the channel's ONLY one: no S7 beside it)
            moving.append(("S7", ax7, cm - uniq[len(uniq) // 2], 1.0))
    pos = positions(*case.shape)
    out = []

    def put(c, scens, shift):
        for k, (name, axis, base, slope) in enumerate(scens):
            i, j = pos[(k + shift) % len(pos)]
            out.append(Placed(name, axis, c, i, j, base, slope))

    if case.C == 1:
        put(0, static + moving, case.rot)
    else:
        put(case.cstar, moving + static[:2], case.rot)
        put(case.cnon, static, case.rot + 3)
    return out


def line_ends(case: Case) -> Dict[str, Tuple[int, torch.Tensor]]:
    """Per axis: (channel, boolean (H, W) mask) of the line ends of the non-flagged channel ``cnon`` (every channel when
    nothing moves).  alpha's lines run along W, beta's along H."""
    H, W = case.shape
    a = torch.zeros(H, W, dtype=torch.bool)
    a[:, 0] = a[:, W - 1] = True
    b = torch.zeros(H, W, dtype=torch.bool)
    b[0, :] = b[H - 1, :] = True
    return {"alpha": (case.cnon, a), "beta": (case.cnon, b)}


def make_inputs(case: Case, seed: Optional[int] = None):
    """(u, params, gy) in float64 holding values exact in the case's tensor type.  ``gy`` is (K', B, C, H, W) for the
    emitting family."""
    g = torch.Generator().manual_seed(1000003 * (case.seed if seed is None else seed) + 17)
    H, W = case.shape
    C, B = case.C, case.B
    tmax = max(t for _, _, t in case.sweeps)
    p = {}
    for ax in ("alpha", "beta"):
        base = torch.randint(32, 129, (C, H, W), generator=g).double() / 64
        slope = torch.randint(-8, 9, (C, H, W), generator=g).double() / 8
        # no drawn element may reach the floor inside the time window (long schedules): theta(tmax) >= 1/8
        lim = -torch.floor((base - 0.125) / max(tmax, HALF) * 8) / 8
        slope = torch.maximum(slope, lim)
        p[ax + "_base"], p[ax + "_time_coeff"] = base, slope
    for q in placements(case):
        p[q.axis + "_base"][q.c, q.i, q.j] = q.base
        p[q.axis + "_time_coeff"][q.c, q.i, q.j] = q.slope
    if case.mix != "none":
        p["M"] = torch.eye(C, dtype=torch.float64) + torch.randint(-4, 5, (C, C), generator=g).double() / 32
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}[case.io]
    u = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).to(dt).double()
    K = len(case.emit) + 1
    gy = torch.randn(K, B, C, H, W, generator=g, dtype=torch.float64).to(dt).double()
    if case.gy_last_zero:
        gy[-1] = 0
    if not case.emit:
        gy = gy[0]
    return u, p, gy


# --------------------------------------------------------------------------------------------------------------------- #
# the reference: oracle.pde_oracle's pieces over an arbitrary sweep list                                                 #
# --------------------------------------------------------------------------------------------------------------------- #
def pass_mask(raw: torch.Tensor, case: Case, strict: bool = False) -> torch.Tensor:
    if strict:
        m = raw > EPS
        return m & (raw < case.clamp_max) if case.clamp_max is not None else m
    m = raw >= EPS
    return m & (raw <= case.clamp_max) if case.clamp_max is not None else m


def _smooth_end1(theta: torch.Tensor, axis: int) -> torch.Tensor:
    """The replicate-padded 3-tap average in value; in gradient its transpose with end weight 1 (the zero-padded one)."""
    th = theta if axis == 0 else theta.transpose(1, 2)
    z = torch.zeros_like(th[..., :1])
    zp = torch.cat([z, th, z], dim=-1)
    zero_padded = (zp[..., :-2] + zp[..., 1:-1] + zp[..., 2:]) / 3
    rp = torch.cat([th[..., :1], th, th[..., -1:]], dim=-1)
    replicate = (rp[..., :-2] + rp[..., 1:-1] + rp[..., 2:]) / 3
    out = zero_padded + (replicate - zero_padded).detach()
    return out if axis == 0 else out.transpose(1, 2)


def forward(u: torch.Tensor, p: Dict[str, torch.Tensor], case: Case, rule: str = "right", state_cast=None):
    """The case's forward, differentiable.  ``rule`` "right": torch's clamp (gradient passes at ties) through
    ``O.coefficient_at``; a wrong rule keeps every VALUE and changes what the backward sees.  Returns y, or the stacked
    (K', B, C, H, W) trajectory when the case emits states."""
    spec = case.spec()
    plain = dataclasses.replace(spec, smooth3=False)
    cast = state_cast if state_cast is not None else (lambda t: t)
    sweeps = case.sweeps
    sps = {"strang": 3, "lie": 2}.get(case.sched, len(sweeps))
    tfirst = {}
    for a, _, t in sweeps:
        tfirst.setdefault(a, t)
    B, C, H, W = u.shape
    outs = []
    for s, (axis, delta, t) in enumerate(sweeps):
        if case.mix == "pre" and s % sps == 0:
            u = cast(torch.matmul(p["M"], u.reshape(B, C, H * W)).view(B, C, H, W))
        ax = "alpha" if axis == 0 else "beta"
        base, slope, h = p[ax + "_base"], p[ax + "_time_coeff"], (case.dx if axis == 0 else case.dy)
        if rule in ("right", "end1"):
            theta = O.coefficient_at(base, slope, t, spec)
        else:
            raw = base + slope * t
            tm = {"strict": t, "first": tfirst[axis], "t0": 0.0}[rule]
            m = pass_mask((base + slope * tm).detach(), case, strict=(rule == "strict")).to(raw.dtype)
            theta = O.coefficient_at(base, slope, t, spec).detach() + m * (raw - raw.detach())
        if rule == "end1" and case.smooth3:
            u = O._implicit_sweep(u, _smooth_end1(theta, axis), axis, delta, h, plain)
        else:
            u = O._implicit_sweep(u, theta, axis, delta, h, spec)
        if case.mix != "none" and s % sps == sps - 1:
            u = cast(u)
        if case.mix == "post" and s % sps == sps - 1:
            u = cast(torch.matmul(p["M"], u.reshape(B, C, H * W)).view(B, C, H, W))
        if s in case.emit:
            outs.append(cast(u))
    y = cast(u)
    return torch.stack(outs + [y]) if case.emit else y


def reference(case: Case, u, p, gy, rule: str = "right", dtype=torch.float64, state_cast=None):
    """(y, gu, {name: grad}) of the case under ``rule`` in ``dtype``; a parameter nothing reads gets zeros."""
    pp = {k: v.to(dtype) for k, v in p.items()}
    y, gu, gp = O.value_and_grads(lambda a, q: forward(a, q, case, rule, state_cast), u.to(dtype), pp, gy.to(dtype))
    gp = {k: (torch.zeros_like(pp[k]) if g is None else g) for k, g in gp.items()}
    return y, gu, gp


@functools.lru_cache(maxsize=None)
def cached(case: Case):
    """Inputs and right-rule fp64 reference of a case, computed once per process and shared (never modified)."""
    u, p, gy = make_inputs(case)
    cast = {"bf16": lambda t: t.bfloat16().to(t.dtype), "f16": lambda t: t.half().to(t.dtype)}.get(case.io)
    return (u, p, gy), reference(case, u, p, gy, state_cast=cast)


def expected_flags(case: Case, p) -> List[bool]:
    """Per channel: does any element's pass-through mask at any sweep differ from the mask at its axis' first sweep."""
    tfirst = {}
    for a, _, t in case.sweeps:
        tfirst.setdefault(a, t)
    flag = torch.zeros(case.C, dtype=torch.bool)
    for axis, _, t in case.sweeps:
        ax = "alpha" if axis == 0 else "beta"
        b, s = p[ax + "_base"], p[ax + "_time_coeff"]
        flag |= (pass_mask(b + s * t, case) != pass_mask(b + s * tfirst[axis], case)).flatten(1).any(1)
    return flag.tolist()


def kappa_reference(case: Case, p, dtype=torch.float64) -> List[float]:
    """max over the tensor of the (smoothed) clamped coefficient times delta / h**2, per sweep."""
    spec = case.spec()
    out = []
    for axis, delta, t in case.sweeps:
        ax = "alpha" if axis == 0 else "beta"
        th = O.coefficient_at(p[ax + "_base"].to(dtype), p[ax + "_time_coeff"].to(dtype), t, spec)
        if case.smooth3:
            th = th if axis == 0 else th.transpose(1, 2)
            th = O._smooth3(th.reshape(-1, th.shape[-1]))
        h = case.dx if axis == 0 else case.dy
        out.append(float((th * delta / h ** 2).max()))
    return out


def place_kappa_peak(case: Case, p, where: str):
    """Make the per-sweep maximum unique and put it at ``where``: "corner" (N-1, N-1), "junction" (m-1, m) of the upper
    half, "lastc" (last channel, (0, m)), "clamped" (16 > clamp_max at (m, m-1): the maximum is clamp_max*delta/h2)."""
    H, W = case.shape
    c, i, j, v = {"corner": (0, H - 1, W - 1, 4.0), "junction": (0, H // 2 - 1, W // 2, 4.0),
                  "lastc": (case.C - 1, 0, W // 2, 4.0), "clamped": (case.C - 1, H // 2, W // 2 - 1, 16.0)}[where]
    q = {k: t.clone() for k, t in p.items()}
    for ax in ("alpha", "beta"):
        q[ax + "_base"].clamp_(max=2.0)
        q[ax + "_base"][c, i, j] = v
        q[ax + "_time_coeff"][c, i, j] = 0.0
    return q


# --------------------------------------------------------------------------------------------------------------------- #
# the cases                                                                                                              #
# --------------------------------------------------------------------------------------------------------------------- #
def _cases() -> List[Case]:
    A = [
        Case("A-n8-c3-strang", "A", 8, 3, 5, "strang", 2, ckpt=0, cstar=2, rot=0),
        Case("A-n12-c2-smooth-all", "A", 12, 2, 1, "strang", 3, smooth3=True, ckpt="all", cstar=0, rot=1),
        Case("A-n20-c3-lie-auto", "A", 20, 3, 2, "lie", 3, ckpt="auto", cstar=1, rot=2),
        Case("A-n28-c1-xyxxy-smooth", "A", 28, 1, 3, "xyxxy", 0, smooth3=True, ckpt=0, rot=3),
        Case("A-n32-c3-lie-dx2", "A", 32, 3, 2, "lie", 3, ckpt="auto", dx=2.0, dy=0.5, cstar=2, rot=5),
        Case("A-n8-c1-xonly", "A", 8, 1, 1, "xonly", 0, ckpt=0, rot=4),
        Case("A-n16-c3-nomax-smooth", "A", 16, 3, 2, "strang", 2, clamp_max=None, smooth3=True, ckpt="all", rot=6),
        Case("A-n8-c8-xcd", "A", 8, 8, 2, "strang", 2, smooth3=True, ckpt=0, cstar=5, rot=2),
        Case("A-n8-c65-flag64", "A", 8, 65, 1, "strang", 2, smooth3=True, ckpt=0, cstar=64, rot=1),
        Case("A-n8-c65-flag0", "A", 8, 65, 1, "strang", 2, smooth3=True, ckpt=0, cstar=0, rot=4),
        Case("A-n8-b1", "A", 8, 1, 1, "strang", 2, ckpt=0, rot=0),
        Case("A-n8-b5-static-smooth", "A", 8, 1, 5, "strang", 2, smooth3=True, ckpt=0, rot=1, moving=False),
        Case("A-n8-b17", "A", 8, 1, 17, "strang", 2, ckpt=0, rot=2),
        Case("A-n8-b130-static-smooth", "A", 8, 1, 130, "strang", 2, smooth3=True, ckpt=0, rot=3, moving=False),
        Case("A-n8-b257", "A", 8, 1, 257, "strang", 2, ckpt=0, rot=4),
        Case("A-n8-long66", "A", 8, 1, 1, "strang", 22, ckpt="auto", rot=0),
        Case("A-n16-c3-bf16", "A", 16, 3, 2, "strang", 2, ckpt=0, cstar=1, rot=3, io="bf16"),
        Case("A-n16-c3-f16", "A", 16, 3, 2, "strang", 2, ckpt=0, cstar=1, rot=3, io="f16"),
    ]
    Bf = [
        Case("B-n32-c3-2steps", "B", 32, 3, 2, "strang", 2, ckpt=0, cstar=1, rot=0),
        Case("B-n32-c2-3steps-smooth", "B", 32, 2, 3, "strang", 3, smooth3=True, ckpt=0, cstar=1, rot=4),
    ]
    Bf += [dataclasses.replace(c, name=c.name + "-ckpt", ckpt=0b100) for c in Bf]
    Cf = [
        Case("C-c5-pre", "C", 16, 5, 2, "strang", 3, ckpt=0, cstar=4, rot=1, mix="pre"),
        Case("C-c8-post-smooth", "C", 16, 8, 2, "strang", 3, smooth3=True, ckpt=0, cstar=3, rot=2, mix="post"),
    ]
    D = [
        Case("D-c1-n16-pre", "D", 16, 1, 3, "strang", 2, ckpt=0, rot=0, mix="pre"),
        Case("D-c3-n28-post-smooth", "D", 28, 3, 2, "strang", 2, smooth3=True, ckpt=0, cstar=2, rot=1, mix="post"),
        Case("D-c4-n16-post", "D", 16, 4, 2, "lie", 3, ckpt=0, cstar=3, rot=2, mix="post"),
        Case("D-c3-n16-pre-smooth", "D", 16, 3, 5, "strang", 3, smooth3=True, ckpt="auto", cstar=0, rot=3, mix="pre"),
        Case("D-c4-n28-pre", "D", 28, 4, 1, "strang", 2, ckpt=0, cstar=1, rot=4, mix="pre"),
        Case("D-c1-n28-post-static", "D", 28, 1, 2, "strang", 2, smooth3=True, ckpt=0, rot=5, mix="post", moving=False),
    ]
    E = [
        Case("E-n9-c3", "E", 9, 3, 5, "strang", 2, ckpt=0, cstar=2, rot=1),
        Case("E-n36-c2-smooth", "E", 36, 2, 2, "strang", 2, smooth3=True, ckpt="auto", cstar=0, rot=2),
        Case("E-rect-12x20", "E", 12, 3, 2, "lie", 3, smooth3=True, ckpt=0, cstar=1, rot=3, W=20, dx=2.0, dy=0.5),
        Case("E-n16-f64", "E", 16, 3, 3, "strang", 3, smooth3=True, ckpt=0, cstar=1, rot=4, io="f64"),
        Case("E-n9-c1-b17-static", "E", 9, 1, 17, "xyxxy", 0, smooth3=True, ckpt=0, rot=5, moving=False),
    ]
    Ff = [
        Case("F-n16-two-states", "F", 16, 3, 2, "strang", 2, ckpt=0, cstar=1, rot=0, emit=(2,)),
        Case("F-n16-emitted-only", "F", 16, 2, 3, "strang", 3, smooth3=True, ckpt="auto", cstar=0, rot=5, emit=(7,),
             gy_last_zero=True),
    ]
    # the one-launch wide forward (C = 32 / 64, pde_adi_wide.h): its own lane-major copy of the coefficient records, and —
    # with a step-local checkpoint mask — the backward that first recomputes the operator outputs the forward did not keep
    Gf = [
        Case("G-c32-n28-strang-pre-smooth", "G", 28, 32, 2, "strang", 3, smooth3=True, ckpt=0, cstar=30, rot=1, mix="pre"),
        Case("G-c64-n32-lie-post", "G", 32, 64, 2, "lie", 3, ckpt=0, cstar=63, rot=2, mix="post"),
        Case("G-c32-n32-strang-post-smooth", "G", 32, 32, 2, "strang", 3, smooth3=True, ckpt=0, cstar=7, rot=4, mix="post"),
    ]
    Gf += [dataclasses.replace(c, name=c.name + "-ckpt", ckpt=m) for c, m in zip(Gf, (0b10, 0b01, 0b01))]
    return A + Bf + Cf + D + E + Ff + Gf


#: seeds the CPU conditions accepted (test_adi_edge_cases.py::test_noise_and_separation): the case's index, plus 100 for
#: every draw that was rejected before
RESEED: Dict[str, int] = {}

def _seeded(cs: List[Case]) -> List[Case]:
    idx: Dict[str, int] = {}
    out = []
    for c in cs:
        base = c.name[:-5] if c.name.endswith("-ckpt") else c.name      # "-ckpt": the same inputs, another checkpoint mask
        i = idx.setdefault(base, len(idx))
        out.append(dataclasses.replace(c, seed=i + 100 * RESEED.get(base, 0)))
    return out


CASES: List[Case] = _seeded(_cases())
BY_NAME = {c.name: c for c in CASES}

KAPPA_SHAPES = [(8, 1), (20, 3), (32, 65), (8, 65), (32, 1), (20, 65)]
KAPPA_PLACES = ["corner", "junction", "lastc", "clamped"]


def kappa_cases() -> List[Tuple[Case, str]]:
    out = []
    for k, (N, C) in enumerate(KAPPA_SHAPES):
        for w, where in enumerate(KAPPA_PLACES):
            smooth = (k + w) % 2 == 1
            c = Case(f"K-n{N}-c{C}-{where}" + ("-smooth" if smooth else ""), "K", N, C, 1, "strang", 2, smooth3=smooth,
                     clamp_max=CMAX if (where == "clamped" or w % 2) else None, moving=False, seed=500 + 4 * k + w,
                     dx=2.0 if k % 2 else 1.0, dy=0.5 if k % 2 else 1.0)
            out.append((c, where))
    return out
