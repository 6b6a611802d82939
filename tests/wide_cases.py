"""Case generators and fp64 references for the STAGES of the one-launch wide forward (csrc/pde_adi_wide.h,
adi_wide_fwd_kernel: fp32 tensors, C = 32 / 64, N = 28 / 32, Strang or Lie steps, the channel operator before ("pre",
mode 1) or after ("post", mode 2) every step).  tests/test_wide_cases.py checks what is built here on the CPU;
tests/test_gpu_wide_stages.py holds the kernel to it through the C ABI.

Stages.  The kernel stores the sweep output of every step and the layer output, nothing else.  From a STORED fp32 state
``prev`` one stage leads to the next stored state, so every stored state is compared with a float64 reference that starts
from the device's own previous one and an error cannot hide behind the ones made before it:

    stage_pre(prev, k)          sweeps_k(M prev)       mode 1: slot 2k+1 from slot 2k-1 (or u)
    stage_post_sweeps(prev, k)  sweeps_k(prev)         mode 2: slot 2k from M slot 2k-2 (or from u)
    mix(prev)                   M prev                 mode 2: y from slot 2(K-1)

built from oracle.pde_oracle (``_implicit_sweep``, ``coefficient_at``, ``sweep_schedule``) in float64; the same functions
with ``dtype=torch.float32`` are the "oracle32" whose own distance from float64 sets the bar of the step stages.

The operator product.  The kernel splits every fp32 operand in registers into three bf16 pieces (``wide_split3``) and
adds six of the nine piece products on the bf16 matrix cores (``PDE_WIDE_MFMA6``).  ``emulate`` does the same on the CPU —
pieces by successive ``.bfloat16()`` roundings, piece products accumulated in float64 — under the right rule and with one
mistake each (``RULES``):

    drop11, drop02, drop20   one of the three low-order products missing
    two_piece                operands cut to hi + mid
    bf16                     operands cut to hi
    transposed               M^T
    swap_halves              inside every contraction group of 16 channels the channel groups 4ks+{0,1} and 4ks+{2,3}
                             (channels 16ks+0..7 and 16ks+8..15) exchanged on the state's side: lanes 0-31 and 32-63 of
                             the matrix-core operand read each other's k
    pad_live  (N = 28)       a lane owns 14 elements of a half row and the exchange image has 16 slots per lane; slots 14
                             and 15 hold no element and are written as 0 and never read back.  Here they are live: they
                             carry the neighbouring line's elements 0 and 1 and come back through the clamped register
                             index (k < MM ? k : 0), so element 0 of every half row ends as the product at the neighbour
                             line's element 1

Inputs: M = I + 0.1 randn (not symmetric); the state's channels scaled by logspace(-2, 2, C), so a small channel must not
drown in the rounding of a large one; the PDE parameters as ``_randomise`` of tests/test_gpu_wide.py draws them (bases
times 1 + 0.2 randn, slopes 0.3 randn).  Mode 1 runs the cifar10 flavour of the coefficient stage (clamp to [eps, 10], no
smoothing), mode 2 the SVHN flavour (smoothed, no upper clamp); both with both step patterns.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from oracle import pde_oracle as O

#: whole-tensor max-norm bar of a three-piece product against fp64, and the per-channel one: the project's standing bars,
#: tests/test_gpu_parity.py::test_channel_mix_three_piece_products
BAR = 5e-7
BAR_CHANNEL = 2e-6
#: the right emulation against fp64 (measured 1-3e-8: six exact products, the dropped three are below 2**-24 of the sum)
EMU_TOL = 1e-7
#: step stages: this many times oracle32's own distance from the same fp64 reference (tests/test_gpu_fuzz.py's window)
ORACLE32_FACTOR = 4.0
#: CPU margins of the wrong rules on the mix stage, in bars
MARGIN = 4.0
MARGIN_GROSS = 100.0
RULES = ("drop11", "drop02", "drop20", "two_piece", "bf16", "transposed", "swap_halves", "pad_live")
GROSS = ("pad_live", "transposed", "swap_halves", "bf16")
EPS = O.EPS
DT = 0.05


@dataclass(frozen=True)
class Case:
    C: int
    N: int
    split: str            # "strang" | "lie"
    mode: int             # 1: operator before every step, 2: after
    K: int = 3
    B: int = 3
    seed: int = 0

    @property
    def name(self):
        return f"c{self.C}-n{self.N}-{self.split}-m{self.mode}"

    @property
    def sps(self):
        return 3 if self.split == "strang" else 2

    @property
    def smooth3(self):
        return self.mode == 2

    @property
    def clamp_max(self):
        return 10.0 if self.mode == 1 else None

    def spec(self) -> O.AdiSpec:
        return O.AdiSpec(self.N, self.C, DT, 1.0, 1.0, self.K, self.split, self.smooth3, self.clamp_max,
                         "pre" if self.mode == 1 else "post", False, EPS)

    @property
    def sweeps(self) -> List[Tuple[int, float, float]]:
        return O.sweep_schedule(self.spec())


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """golden_util.rel_err: max|a - b| / max|b|."""
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / float(b.abs().max())


def rel_err_channel(a: torch.Tensor, b: torch.Tensor) -> float:
    """The worst channel of (B, C, ...) tensors, each against its own maximum."""
    a, b = a.double().flatten(2), b.double().flatten(2)
    return float(((a - b).abs().amax(dim=(0, 2)) / b.abs().amax(dim=(0, 2))).max())


def make_inputs(case: Case, seed: Optional[int] = None, B: Optional[int] = None):
    """(u, params) in fp32; params: the four coefficient tensors (C, N, N) and "M" (C, C)."""
    g = torch.Generator().manual_seed(7919 * (case.seed if seed is None else seed) + 31 * case.C + case.N + 5)
    C, N = case.C, case.N
    p = {}
    for ax in ("alpha", "beta"):
        p[ax + "_base"] = torch.ones(C, N, N) * (1 + 0.2 * torch.randn(C, N, N, generator=g))
        p[ax + "_time_coeff"] = 0.3 * torch.randn(C, N, N, generator=g)
    p["M"] = torch.eye(C) + 0.1 * torch.randn(C, C, generator=g)
    u = torch.randn(B or case.B, C, N, N, generator=g) * torch.logspace(-2, 2, C).view(1, C, 1, 1)
    return u, p


# --------------------------------------------------------------------------------------------------------------------- #
# stage references                                                                                                       #
# --------------------------------------------------------------------------------------------------------------------- #
def mix(prev: torch.Tensor, M: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    B, C = prev.shape[:2]
    return torch.matmul(M.to(dtype), prev.to(dtype).reshape(B, C, -1)).view(prev.shape)


def sweeps_k(x: torch.Tensor, k: int, case: Case, p: Dict[str, torch.Tensor], dtype=torch.float64) -> torch.Tensor:
    """The sweeps of time step k applied to ``x``, all arithmetic in ``dtype``."""
    spec = case.spec()
    x = x.to(dtype)
    for axis, delta, t in case.sweeps[k * case.sps:(k + 1) * case.sps]:
        ax = "alpha" if axis == 0 else "beta"
        theta = O.coefficient_at(p[ax + "_base"].to(dtype), p[ax + "_time_coeff"].to(dtype), t, spec)
        x = O._implicit_sweep(x, theta, axis, delta, spec.dx if axis == 0 else spec.dy, spec)
    return x


def stage_pre(prev, k, case, p, dtype=torch.float64):
    return sweeps_k(mix(prev, p["M"], dtype), k, case, p, dtype)


def stage_post_sweeps(prev, k, case, p, dtype=torch.float64):
    return sweeps_k(prev, k, case, p, dtype)


def step_stage(stored_prev, k: int, case: Case, p, dtype=torch.float64):
    """The stored state of step k from the stored state before it (``u`` for k = 0): one operator and one step's sweeps.
    Mode 2 keeps slot 2k, the sweeps of step k applied to M slot 2k-2; its step 0 has no operator before it."""
    if case.mode == 1 or k > 0:
        return stage_pre(stored_prev, k, case, p, dtype)
    return stage_post_sweeps(stored_prev, k, case, p, dtype)


def trajectory(case: Case, u, p, dtype=torch.float64):
    """([stored state of step 0..K-1], y) of the whole layer in ``dtype`` — what the kernel stores, in its order."""
    stored, cur = [], u.to(dtype)
    for k in range(case.K):
        cur = step_stage(cur, k, case, p, dtype)
        stored.append(cur)
    return stored, (cur if case.mode == 1 else mix(cur, p["M"], dtype))


# --------------------------------------------------------------------------------------------------------------------- #
# the three-piece product                                                                                                #
# --------------------------------------------------------------------------------------------------------------------- #
def split3(x: torch.Tensor) -> List[torch.Tensor]:
    """``wide_split3``: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); the differences are exact in fp32."""
    x = x.float()
    hi = x.bfloat16().float()
    r1 = x - hi
    mid = r1.bfloat16().float()
    lo = (r1 - mid).bfloat16().float()
    return [hi.double(), mid.double(), lo.double()]


SIX = ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0))           # PDE_WIDE_MFMA6's (A piece, B piece), in its order


def _products(M, s, pairs):
    B, C = s.shape[:2]
    A, S = split3(M), split3(s.reshape(B, C, -1))
    out = torch.zeros(B, C, S[0].shape[-1], dtype=torch.float64)
    for i, j in pairs:
        out += torch.matmul(A[i], S[j])
    return out.view(s.shape)


def emulate(M: torch.Tensor, s: torch.Tensor, rule: str = "right") -> torch.Tensor:
    """M s as the kernel's three-piece product forms it (float64 accumulation), under ``rule``."""
    drop = {"drop11": (1, 1), "drop02": (0, 2), "drop20": (2, 0)}
    if rule == "right":
        return _products(M, s, SIX)
    if rule in drop:
        return _products(M, s, [q for q in SIX if q != drop[rule]])
    if rule == "two_piece":
        return _products(M, s, [(0, 0), (0, 1), (1, 0), (1, 1)])
    if rule == "bf16":
        return _products(M, s, [(0, 0)])
    if rule == "transposed":
        return _products(M.t().contiguous(), s, SIX)
    if rule == "swap_halves":
        C = s.shape[1]
        perm = torch.arange(C).view(C // 16, 2, 8).flip(1).reshape(C)
        return _products(M, s[:, perm], SIX)
    if rule == "pad_live":
        out = _products(M, s, SIX)
        N = s.shape[-1]
        if N // 2 >= 16:
            raise ValueError("pad_live needs a half row shorter than the 16 slots of a lane (N = 28)")
        nb = out.roll(-1, dims=2)                                 # line l + 1 (cyclic)
        bad = out.clone()
        bad[..., 0] = nb[..., 1]                                  # half 0: element k is column k
        bad[..., N - 1] = nb[..., N - 2]                          # half 1: element k is column N-1-k
        return bad
    raise ValueError(rule)


def rules_for(case: Case) -> Tuple[str, ...]:
    return tuple(r for r in RULES if r != "pad_live" or case.N // 2 < 16)


# --------------------------------------------------------------------------------------------------------------------- #
# the cases                                                                                                              #
# --------------------------------------------------------------------------------------------------------------------- #
#: draws the CPU margins rejected, per (C, N): the seed moves on by 100 for each (test_wide_cases.py checks the record)
RESEED: Dict[Tuple[int, int], int] = {(32, 32): 1}


def _cases() -> List[Case]:
    out = []
    for i, (C, N) in enumerate(((32, 28), (32, 32), (64, 28), (64, 32))):
        for split in ("strang", "lie"):
            for mode in (1, 2):
                out.append(Case(C, N, split, mode, seed=i + 100 * RESEED.get((C, N), 0)))
    return out


CASES: List[Case] = _cases()
BY_NAME = {c.name: c for c in CASES}
#: one workgroup, several samples: 2100 samples on 2048 workgroups, samples b and b + 2048 share one
GRID = 2048
MANY = Case(32, 28, "lie", 2, K=1, B=2100, seed=50)
MANY_HEAD = 52                                                    # samples 0..51 and 2048..2099


@functools.lru_cache(maxsize=None)
def cached(case: Case):
    """Inputs of a case, drawn once per process and shared (never modified)."""
    return make_inputs(case)
