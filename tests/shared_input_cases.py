"""Cases and fp64 references for the shared-input layer group (pde_adi_multi_forward / pde_adi_multi_backward: up to four
mixing-first layers on ONE input in one launch per pass; cifar10.py:272-280, cifar_2version.py:287-296).
tests/test_shared_input_cases.py checks what is built here on the CPU; tests/test_gpu_shared_input.py holds both launch
arrangements of the kernel to it.

The two arrangements (csrc/pde_adi.hip multi_parallel): B < 1024 runs the layers SIDE BY SIDE, one layer per workgroup,
grid B*L, every layer's term of `out` / `gu` in a slab of its own and a second launch that adds the slabs in layer order;
B >= 1024 runs them ONE AFTER THE OTHER inside each of 1024 workgroups, which walk their samples b, b + 1024, ... through
layer after layer and build `out` / `gu` by re-reading their own earlier store.

The loss of a case is  <out, gy> + sum_i <y_i, gys_i> + sum_i <s_i, gs_i>  with out = sum_i w_i y_i and
s_i[b, c] = sum_hw y_i[b, c]; each of the three terms may be absent, and without weights there is no `out`.

Periodic batches.  u, gy, gys_i and gs_i are drawn for P <= 11 samples and tiled, x[b] = x[b mod P], so the fp64 reference
runs on P samples whatever B is: every per-sample result (y_i, s_i, out, gu) of sample b is that of sample b mod P, and
every batch-summed gradient (the four coefficient gradients, gM, g_weight) — linear in the incoming gradients — is the
P-sample one with sample r's incoming gradients multiplied by count_r = |{b < B : b mod P = r}|.  B need not be a
multiple of P.  ``reference`` does this in ONE backward (incoming gradients times count_r; gu divided by count_r after).

16-bit cases.  Inputs are rounded to the tensor type first (parameters, M and the weights too for fp16, where they
travel as fp16); the reference is the fp64 oracle rounding its state where THIS kernel rounds: the sweep output of
every step (what the forward stores for the backward and goes on from), and nothing else — the one-launch kernel applies
the channel operator in registers and never stores its result, and its adjoints stay in fp32, so the rounding is applied in
value only (``kernel_cast``).  oracle.pde_oracle.adi_forward's ``state_cast`` also rounds behind each operator (the
per-step kernels store there) and rounds the adjoint at the same points; ``reference(points="oracle")`` is that
placement.  On tensors the two agree within the 16-bit limits (a few 16-bit ulps, as tests/test_gpu_f16.py measures);
on the two-entry g_weight of f16-seq, a sum of 3840 distinct signed terms that cancels to 1/3 of its rms size, the extra
roundings alone move the reference by 4e-3, twice the fp16 limit: hence the kernel's own points.

Wrong-rule references (``reference(rule=..., which=layer)``): the same computation with one plausible kernel fault —
    "drop_gs"      a layer's plane-sum gradient never joins the adjoint
    "drop_gys"     a layer's dL/dy_i never joins the adjoint
    "gw_shift"     g_weight of layer i taken from layer i + 1 (cyclically)
    "swap_last"    the coefficient records of the LAST step of two layers exchanged (a record prefetched for the wrong
                   layer at the layer boundary)
The CPU tests require each of them to lie at least ten limits away from the right reference in a checked output.
"""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from oracle import pde_oracle as O

NAMES = ["alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff"]
TOL = 1e-5               # golden_util.rel_err: the bound the one-layer kernels are held to (tests/test_gpu_small.py)
TOL_BF16 = 2e-2          # tests/test_gpu_small.py::test_small_kernels_bf16_and_many_samples
TOL_F16 = 2e-3           # tests/test_gpu_f16.py TOL_CAST / TOL_PGRAD (against the state_cast oracle)
THRESHOLD = 1024         # multi_parallel(): B < 1024 side by side
RULES = ("drop_gs", "drop_gys", "gw_shift", "swap_last")
IO_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
IO_TOL = {"f32": TOL, "bf16": TOL_BF16, "f16": TOL_F16}


def small_window(oracle32: float) -> float:
    """The window of tests/test_gpu_fuzz.py::check_case for results of a few entries (gM at C <= 2, g_weight)."""
    return max(2e-5, 4.0 * min(oracle32, 1e-4))


@dataclass(frozen=True)
class Layer:
    dt: float
    steps: int
    dx: float = 1.0
    scale: float = 1.0                # bases times scale * (1 + 0.2 randn)
    slope: float = 0.3                # slopes slope * randn
    varying: Optional[int] = None     # the channel whose coefficients cross the clamp bounds inside the time window
    ckpt: object = "auto"             # "auto" or a step-local bit mask
    fashion: bool = False             # bases times 1.8 at dt = 0.3: the automatic plan parks states


@dataclass(frozen=True)
class Case:
    name: str
    arrangement: str                  # "par" (side by side) | "seq" (one after the other) | "one" (a single layer)
    kind: str                         # "cifar10" (Strang) | "cifar2" (Lie)
    N: int
    C: int
    B: int
    P: int
    layers: Tuple[Layer, ...]
    io: str = "f32"
    weights: bool = True
    loss: Tuple[str, ...] = ("out", "ys", "sums")
    seed: int = 0

    @property
    def L(self):
        return len(self.layers)

    @property
    def tol(self):
        return IO_TOL[self.io]

    def spec(self, i: int) -> O.AdiSpec:
        ly = self.layers[i]
        mk = O.cifar10_spec if self.kind == "cifar10" else O.cifar2_spec
        return mk(self.N, self.C, dt=ly.dt, dx=ly.dx, dy=ly.dx, num_steps=ly.steps)

    def counts(self) -> torch.Tensor:
        return torch.bincount(torch.arange(self.B) % self.P, minlength=self.P).double()

    def index(self) -> torch.Tensor:
        return torch.arange(self.B) % self.P


def _L(dt, steps, dx=1.0, **kw):
    return Layer(dt, steps, dx, **kw)


_FASHION = dict(scale=1.8, slope=0.2, fashion=True)

CASES: List[Case] = [
    Case("par-n32-c4-l4", "par", "cifar10", 32, 4, 3, 3,
         (_L(0.02, 1), _L(0.04, 3, 2.0), _L(0.05, 2, 1.5), _L(0.03, 4, 1.0, scale=0.7))),
    Case("par-n28-c1-l2-mask", "par", "cifar10", 28, 1, 7, 7,
         (_L(0.25, 3, 2.0, slope=0.1, varying=0, ckpt=0b01), _L(0.04, 2, 1.0, ckpt=0))),
    Case("par-n16-c2-l3-lie-max", "par", "cifar2", 16, 2, 1023, 7,
         (_L(0.02, 2), _L(0.04, 4, 2.0), _L(0.05, 1, 1.5))),
    Case("par-l1-weight", "one", "cifar10", 32, 3, 2, 2, (_L(0.03, 3, 1.5),)),
    Case("seq-n16-c3-l3-1024", "seq", "cifar10", 16, 3, 1024, 8,
         (_L(0.02, 2), _L(0.05, 3, 2.0), _L(0.03, 1, 1.5))),
    Case("seq-n32-c4-l4-1025", "seq", "cifar10", 32, 4, 1025, 11,
         (_L(0.02, 1), _L(0.3, 3, 1.0, **_FASHION), _L(0.25, 2, 4.0, slope=0.1, varying=2), _L(0.03, 4, 1.5, scale=0.7))),
    Case("seq-n28-c2-l2-lie-2049", "seq", "cifar2", 28, 2, 2049, 6,
         (_L(0.02, 3), _L(0.05, 2, 1.5)), weights=False, loss=("ys", "sums")),
    Case("seq-n16-c1-l4-1100", "seq", "cifar10", 16, 1, 1100, 11,
         (_L(0.02, 2, ckpt=0b11), _L(0.05, 1, 2.0, ckpt=0), _L(0.03, 3, 1.5, ckpt=0b10), _L(0.04, 2, 1.0, ckpt=0b01))),
    Case("bf16-par", "par", "cifar10", 32, 3, 6, 6, (_L(0.02, 2), _L(0.05, 3, 2.0), _L(0.03, 1, 1.5)), io="bf16"),
    Case("f16-par", "par", "cifar10", 32, 3, 6, 6, (_L(0.02, 2), _L(0.05, 3, 2.0), _L(0.03, 1, 1.5)), io="f16"),
    Case("bf16-seq", "seq", "cifar10", 16, 3, 1025, 5, (_L(0.02, 2), _L(0.05, 3, 2.0)), io="bf16"),
    Case("f16-seq", "seq", "cifar10", 16, 3, 1025, 5, (_L(0.02, 2), _L(0.05, 3, 2.0)), io="f16"),
]
#: draws the CPU conditions rejected before the one in use (test_shared_input_cases.py: the fp32 oracle's own noise must
#: stay within a quarter of every limit, and no channel but the "varying" one may reach a clamp bound); the seed is the
#: case's index plus 100 per rejected draw.  seq-n32-c4-l4-1025, draw 0: gM of the one-step layer 0 at 3.2e-6 > 2.5e-6;
#: f16-par, draw 0: one fp16 ulp flipped at an element of y_0 close to the largest, 5.7e-4 > 5e-4
RESEED: Dict[str, int] = {"seq-n32-c4-l4-1025": 1, "f16-par": 1}
CASES = [dataclasses.replace(c, seed=i + 100 * RESEED.get(c.name, 0)) for i, c in enumerate(CASES)]
BY_NAME: Dict[str, Case] = {c.name: c for c in CASES}
F32_CASES = [c for c in CASES if c.io == "f32"]
IO16_CASES = [c for c in CASES if c.io != "f32"]


# --------------------------------------------------------------------------------------------------------------------- #
# inputs                                                                                                                 #
# --------------------------------------------------------------------------------------------------------------------- #
@dataclass
class Inputs:
    """Everything in float64, holding values that are exact in the type they travel in.  u, gy, gys[i]: (P,C,N,N);
    gs[i]: (P,C); params[i]: the layer's named parameters; w: (L,) or None."""
    u: torch.Tensor
    gy: Optional[torch.Tensor]
    gys: List[Optional[torch.Tensor]]
    gs: List[Optional[torch.Tensor]]
    params: List[Dict[str, torch.Tensor]]
    w: Optional[torch.Tensor]


def make_inputs(case: Case) -> Inputs:
    g = torch.Generator().manual_seed(7919 * case.seed + 41)
    N, C, P = case.N, case.C, case.P
    io = IO_DTYPE[case.io]
    pt = torch.float16 if case.io == "f16" else torch.float32      # parameters, M and weights travel as fp16 only there
    st = torch.float16 if case.io == "f16" else torch.float32      # plane sums (and their gradients) likewise
    params = []
    for ly in case.layers:
        sc = 1.8 if ly.fashion else ly.scale
        p = {"alpha_base": sc * (1 + 0.2 * torch.randn(C, N, N, generator=g)),
             "beta_base": sc * (1 + 0.2 * torch.randn(C, N, N, generator=g)),
             "alpha_time_coeff": ly.slope * torch.randn(C, N, N, generator=g),
             "beta_time_coeff": ly.slope * torch.randn(C, N, N, generator=g),
             "channel_mixing": torch.eye(C) + 0.1 * torch.randn(C, C, generator=g)}
        if ly.varying is not None:                               # tests/test_gpu_small.py::..._time_varying_clamp_mask
            v = ly.varying
            p["alpha_base"][v].fill_(9.9)                        # crosses the upper bound (10) inside the window ...
            p["alpha_time_coeff"][v].copy_(0.4 + 0.1 * torch.randn(N, N, generator=g))
            p["beta_base"][v, :8].fill_(0.02)                    # ... and the lower one (1e-6) in a few rows
            p["beta_time_coeff"][v, :8].fill_(-0.05)
        params.append({k: t.to(pt).double() for k, t in p.items()})
    w = torch.softmax(torch.randn(case.L, generator=g), 0).to(pt).double() if case.weights else None
    if case.arrangement == "one" and w is not None:              # a single layer: its weight is NOT 1
        w = torch.tensor([0.7], dtype=pt).double()

    def draw(*shape, dt=io):
        return torch.randn(*shape, generator=g).to(dt).double()
    u = draw(P, C, N, N)
    gy = draw(P, C, N, N) if "out" in case.loss else None
    gys = [draw(P, C, N, N) if "ys" in case.loss else None for _ in case.layers]
    gs = [draw(P, C, dt=st) if "sums" in case.loss else None for _ in case.layers]
    if gy is not None and w is None:
        raise ValueError("a gradient at `out` needs weights")
    return Inputs(u, gy, gys, gs, params, w)


def state_cast(case: Case):
    if case.io == "f32":
        return None
    io = IO_DTYPE[case.io]
    return lambda t: t.to(io).to(t.dtype)


class _RoundValue(torch.autograd.Function):
    """t rounded to ``dtype`` in value; the adjoint passes unrounded (the kernel keeps its adjoints in fp32)."""

    @staticmethod
    def forward(ctx, t, dtype):
        return t.to(dtype).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


def kernel_cast(case: Case):
    if case.io == "f32":
        return None
    io = IO_DTYPE[case.io]
    return lambda t: _RoundValue.apply(t, io)


# --------------------------------------------------------------------------------------------------------------------- #
# the reference                                                                                                          #
# --------------------------------------------------------------------------------------------------------------------- #
def layer_forward(u, p, spec: O.AdiSpec, cast=None, last_from=None, points="kernel"):
    """A mixing-first layer from the oracle's own pieces (O.sweep_schedule, O.coefficient_at, O._implicit_sweep), written
    out step by step so that
      - the rounding points of 16-bit tensors can be the one-launch kernel's: ``points`` "kernel" rounds the sweep output
        of every step and nothing else (csrc/pde_adi_small.h: the operator is applied in registers, its result is never
        stored), "oracle" rounds after the operator too, as O.adi_forward's state_cast does for the kernels that store it;
      - the LAST step can take another layer's coefficient records: ``last_from`` = (params, spec) whose last step's
        (theta, delta, h, t) replace this layer's.
    Without a cast and without a swap this is O.adi_forward itself."""
    if last_from is None and cast is None:
        return O.adi_forward(u, p, spec)
    cast = cast if cast is not None else (lambda t: t)
    B, C, H, W = u.shape
    sps = 3 if spec.split == "strang" else 2
    sched = O.sweep_schedule(spec)
    q, qspec = last_from if last_from is not None else (p, spec)
    qsched = O.sweep_schedule(qspec)
    for k in range(spec.num_steps):
        u = torch.matmul(p["channel_mixing"], u.reshape(B, C, H * W)).view(B, C, H, W)
        if points == "oracle":
            u = cast(u)
        last = k == spec.num_steps - 1
        src, sspec, sw = (q, qspec, qsched[-sps:]) if last else (p, spec, sched[k * sps:(k + 1) * sps])
        for axis, delta, t in sw:
            ax = "alpha" if axis == 0 else "beta"
            theta = O.coefficient_at(src[ax + "_base"], src[ax + "_time_coeff"], t, sspec)
            u = O._implicit_sweep(u, theta, axis, delta, sspec.dx if axis == 0 else sspec.dy, sspec)
        u = cast(u)
    return u


@dataclass
class Reference:
    """Per-sample results for the P drawn samples, batch-summed gradients for the whole batch of B."""
    ys: List[torch.Tensor]
    sums: List[torch.Tensor]
    out: Optional[torch.Tensor]
    gu: torch.Tensor
    gp: List[Dict[str, torch.Tensor]]          # per layer: the four coefficient gradients and "channel_mixing"
    gw: Optional[torch.Tensor]

    def flat(self) -> Dict[str, torch.Tensor]:
        d = {"gu": self.gu}
        for i, (y, s) in enumerate(zip(self.ys, self.sums)):
            d[f"y{i}"], d[f"s{i}"] = y, s
        if self.out is not None:
            d["out"] = self.out
        for i, gp in enumerate(self.gp):
            for k, v in gp.items():
                d[f"g{i}.{k}"] = v
        if self.gw is not None:
            d["g_weight"] = self.gw
        return d


def reference(case: Case, inp: Inputs, dtype=torch.float64, rule: str = "right", which: int = 0,
              counts: Optional[torch.Tensor] = None, only_layers: Optional[Tuple[int, ...]] = None,
              points: str = "kernel") -> Reference:
    """The group's results on ``inp`` (P samples standing for case.B tiled ones; ``counts`` overrides the multiplicities,
    e.g. ones for a fully materialised batch).  ``only_layers``: gys / gs reach these layers only.  ``rule`` / ``which``:
    see the module docstring (``which`` = the layer the fault sits in; "swap_last" exchanges which and which + 1).
    ``points`` (16-bit cases): where the state is rounded, see ``layer_forward``."""
    cast = kernel_cast(case) if points == "kernel" else state_cast(case)
    Lc = case.L
    cnt = (case.counts() if counts is None else counts).to(dtype)
    u = inp.u.detach().clone().to(dtype).requires_grad_(True)
    ps = [{k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p.items()} for p in inp.params]
    w = inp.w.detach().clone().to(dtype).requires_grad_(True) if inp.w is not None else None
    specs = [case.spec(i) for i in range(Lc)]
    ys = []
    for i in range(Lc):
        other = None
        if rule == "swap_last" and i in (which, (which + 1) % Lc):
            j = (which + 1) % Lc if i == which else which
            other = (ps[j], specs[j])
        ys.append(layer_forward(u, ps[i], specs[i], cast, other, points))
    sums = [y.sum(dim=(2, 3)) for y in ys]
    out = sum(w[i] * ys[i] for i in range(Lc)) if w is not None else None
    c4, c2 = cnt.view(-1, 1, 1, 1), cnt.view(-1, 1)
    loss = u.sum() * 0
    if out is not None and inp.gy is not None:
        loss = loss + (out * (c4 * inp.gy.to(dtype))).sum()
    for i in range(Lc):
        if only_layers is not None and i not in only_layers:
            continue
        if inp.gys[i] is not None and not (rule == "drop_gys" and i == which):
            loss = loss + (ys[i] * (c4 * inp.gys[i].to(dtype))).sum()
        if inp.gs[i] is not None and not (rule == "drop_gs" and i == which):
            loss = loss + (sums[i] * (c2 * inp.gs[i].to(dtype))).sum()
    loss.backward()

    def grad(t):
        return torch.zeros_like(t) if t.grad is None else t.grad
    gw = grad(w) if w is not None else None
    if rule == "gw_shift" and gw is not None:
        gw = torch.roll(gw, -1)
    return Reference([y.detach() for y in ys], [s.detach() for s in sums], None if out is None else out.detach(),
                     grad(u) / c4, [{k: grad(v) for k, v in p.items()} for p in ps], gw)


@functools.lru_cache(maxsize=None)
def cached(name: str) -> Tuple[Inputs, Reference]:
    """Inputs and right-rule fp64 reference (with state_cast for the 16-bit cases) of a case, computed once per process
    and shared: never modified."""
    case = BY_NAME[name]
    inp = make_inputs(case)
    return inp, reference(case, inp)


def few_entries(case: Case) -> List[str]:
    """Results of at most four entries: sums of B*C*N*N signed terms that largely cancel (tests/test_gpu_fuzz.py)."""
    keys = ["g_weight"] if case.weights else []
    if case.C <= 2:
        keys += [f"g{i}.channel_mixing" for i in range(case.L)]
    return keys


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """golden_util.rel_err (max|a-b| / max|b|), restated so that this module imports without the golden fixtures."""
    a, b = a.double(), b.double()
    den = float(b.abs().max())
    e = float((a - b).abs().max())
    return e if den == 0.0 else e / den


@functools.lru_cache(maxsize=None)
def oracle32(name: str) -> Dict[str, float]:
    """Distance of the plain oracle evaluated in fp32 (for a 16-bit case: with state_cast) from the cached fp64
    reference, per result: the reference's own arithmetic noise, which opens the window of the few-entry results."""
    case = BY_NAME[name]
    inp, ref = cached(name)
    r32 = reference(case, inp, dtype=torch.float32).flat()
    return {k: rel_err(r32[k], v) for k, v in ref.flat().items()}


def limits(case: Case) -> Dict[str, float]:
    """The limit of every checked result of a case (rel_err against ``cached``)."""
    keys = cached(case.name)[1].flat().keys()
    lim = {k: case.tol for k in keys}
    if case.io == "f32":
        o32 = oracle32(case.name)
        for k in few_entries(case):
            lim[k] = small_window(o32[k])
    return lim


# --------------------------------------------------------------------------------------------------------------------- #
# scenario checks                                                                                                        #
# --------------------------------------------------------------------------------------------------------------------- #
def moving_channels(case: Case, i: int, p: Dict[str, torch.Tensor]) -> List[bool]:
    """Per channel: does any element's clamp pass-through mask differ between two sweeps of its axis."""
    spec = case.spec(i)
    flag = torch.zeros(case.C, dtype=torch.bool)
    first = {}
    for axis, _, t in O.sweep_schedule(spec):
        ax = "alpha" if axis == 0 else "beta"
        raw = p[ax + "_base"] + p[ax + "_time_coeff"] * t
        m = (raw >= spec.eps) & (raw <= spec.clamp_max)
        if axis in first:
            flag |= (m != first[axis]).flatten(1).any(1)
        else:
            first[axis] = m
    return flag.tolist()


def kappa_max(case: Case, i: int, p: Dict[str, torch.Tensor]) -> List[float]:
    """Per sweep: max over the tensor of the clamped coefficient times delta / h**2 (what the plan is made from)."""
    spec = case.spec(i)
    out = []
    for axis, delta, t in O.sweep_schedule(spec):
        ax = "alpha" if axis == 0 else "beta"
        th = O.coefficient_at(p[ax + "_base"], p[ax + "_time_coeff"], t, spec)
        h = spec.dx if axis == 0 else spec.dy
        out.append(float((th * delta / h ** 2).max()))
    return out
