"""The round trips the forward's hand-over schedule issues ahead of their use (PDE_FWD_AHEAD, adi_fwd_kernel with HO = true):
the hand-over counters are looked at a solve ahead (bit 2, the one candidate that paid and was kept).  Only WHEN a round
trip is asked for changes — so `y`, `gu` and every parameter gradient must be BITWISE equal with the switch unset (the
default set), at 0 (the schedule as it was), with every single kept bit, and on the barrier schedule (PDE_FWD_SCHED=0).

Cases (N = 32, fp32, Strang, dt = 0.001, time-dependent coefficients, checkpoints = 0), the smallest at which each path
can go wrong:
  0  70 x 5, 2 steps, one workgroup per channel (PDE_G_FWD=1): it walks three chunks of 32, 32 and 6 planes — polls
     ahead across chunk boundaries and up to the job's last record, a ragged chunk;
  1  the same at 3 steps with the time of every sweep 3k (k >= 1) perturbed: the twins are not identical, pair_x = 0,
     three staged records per step;
  2  300 x 64, 3 steps: 8 groups per channel, chunks 8 and 9 go to groups 0 and 1, chunk 9 has 12 planes; XCD map on;
  3  512 x 8, 2 steps, PDE_G_FWD=8: two full chunks per workgroup;
  4  case 0 on integers with dt = 0 in every sweep: all coefficients are 0, every sweep multiplies by the fp32 value of
     1 / (1 + eps) and nothing else, so y is u times that factor S times over, to the last bit — a plane that lands in the
     wrong register component or the wrong place shows as a wrong integer.
Each switch value runs in its own interpreter (the library reads its switches once per process), once for all tests here."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

from oracle import pde_oracle as O

pytestmark = pytest.mark.gpu
N, DT, EPS = 32, 0.001, 1e-6
NAMES = ["alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff"]
#         B,  C, steps, PDE_G_FWD, twins perturbed, integers with dt = 0
CASES = [(70, 5, 2, "1", False, False),
         (70, 5, 3, "1", True, False),
         (300, 64, 3, None, False, False),
         (512, 8, 2, "8", False, False),
         (70, 5, 2, "1", False, True)]
KEPT_BITS = (2,)
VARIANTS = {"default": {}, "none": {"PDE_FWD_AHEAD": "0"}, "barrier": {"PDE_FWD_SCHED": "0"}}
VARIANTS.update({f"bit{b}": {"PDE_FWD_AHEAD": str(b)} for b in KEPT_BITS})


def _sweeps(ci):
    import cnn_with_pde_amd as P
    B, C, steps, gfwd, twins, exact = CASES[ci]
    sw = [s for st in P.adi_schedule(DT, 1.0, 1.0, steps) for s in st]
    if twins:
        sw = [dataclasses.replace(s, t=s.t + 0.25 * DT) if (i % 3 == 0 and i >= 3) else s for i, s in enumerate(sw)]
    if exact:
        sw = [dataclasses.replace(s, delta=0.0) for s in sw]
    return sw


def _inputs(ci):
    B, C, steps, gfwd, twins, exact = CASES[ci]
    g = torch.Generator().manual_seed(4100 + ci)
    spec = O.cifar10_spec(N, C, dt=DT, num_steps=steps)
    params = O.adi_init_params(spec, "cifar10", gen=g)
    for k in ("alpha_base", "beta_base"):
        params[k] = params[k] * (1 + 0.15 * torch.randn(params[k].shape, generator=g))
    for k in ("alpha_time_coeff", "beta_time_coeff"):
        params[k] = 1.0 * torch.randn(params[k].shape, generator=g)
    if exact:
        u = torch.randint(-2000, 2001, (B, C, N, N), generator=g).float()
    else:
        u = torch.randn(B, C, N, N, generator=g)
    gy = torch.randn(B, C, N, N, generator=g)
    return params, u, gy


CHILD = r"""
import os, sys, torch
sys.path[:0] = [%(root)r, %(tests)r]
import ctypes as C
import cnn_with_pde_amd as P
import cnn_with_pde_amd.functional as F
import cnn_with_pde_amd._lib as L
import test_gpu_fwd_ahead as T
lib = L.load()
out = {"kernel": []}
for ci, (B, Cc, steps, gfwd, twins, exact) in enumerate(T.CASES):
    os.environ.pop("PDE_G_FWD", None)
    if gfwd is not None:
        os.environ["PDE_G_FWD"] = gfwd
    params, u, gy = T._inputs(ci)
    sweeps = T._sweeps(ci)
    ud = u.cuda().requires_grad_(True)
    ps = [params[k].cuda().requires_grad_(True) for k in T.NAMES]
    y = P.adi_diffuse(ud, *ps, sweeps, smooth3=False, clamp_max=10.0, eps=T.EPS, checkpoints=0)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    out[ci] = (y.detach().cpu(), ud.grad.cpu(), {k: p.grad.cpu() for k, p in zip(T.NAMES, ps)})
    d = F._build_desc(B, Cc, T.N, L.PDE_IO_F32, sweeps, False, 10.0, T.EPS)
    out["kernel"].append(lib.pde_adi_forward_kernel(C.byref(d)))
torch.save(out, %(path)r)
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("fwd_ahead")
    drop = ("PDE_FWD_AHEAD", "PDE_FWD_SCHED", "PDE_FWD_STAGGER", "PDE_ASM_FWD", "PDE_G_FWD", "PDE_XCD")
    env0 = {k: v for k, v in os.environ.items() if k not in drop}
    res = {}
    for tag, env in VARIANTS.items():
        path = str(tmp / f"{tag}.pt")
        code = CHILD % {"root": os.path.dirname(here), "tests": here, "path": path}
        r = subprocess.run([sys.executable, "-c", code], env=dict(env0, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (tag, r.stderr[-1500:])
        res[tag] = torch.load(path, weights_only=True)
    return res


def test_the_hand_over_kernel_is_what_runs(runs):
    # 3 = the hand-over schedule, 0 = the barrier schedule (pde_adi_forward_kernel)
    for tag in VARIANTS:
        assert runs[tag]["kernel"] == [0 if tag == "barrier" else 3] * len(CASES), tag


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_bitwise_equal_under_every_switch_value(runs, ci):
    y0, gu0, gp0 = runs["default"][ci]
    assert torch.isfinite(y0).all() and torch.isfinite(gu0).all()
    for tag in VARIANTS:
        if tag == "default":
            continue
        y1, gu1, gp1 = runs[tag][ci]
        assert torch.equal(y0, y1), (tag, CASES[ci])
        assert torch.equal(gu0, gu1), (tag, CASES[ci])           # the backward reads y
        assert gp0.keys() == gp1.keys() and len(gp0) == 4
        for name in gp0:
            assert torch.equal(gp0[name], gp1[name]), (tag, CASES[ci], name)


def test_exact_on_integers_when_every_coefficient_is_zero(runs):
    ci = len(CASES) - 1
    B, C, steps, gfwd, twins, exact = CASES[ci]
    assert exact
    params, u, gy = _inputs(ci)
    # one sweep with dt = 0: the pivot is 1 + eps, e = 0, the junction divides by 1 - 0 * 0 — x = d * (1 / (1 + eps)), each
    # operation rounded to fp32 once
    factor = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) + torch.tensor(EPS, dtype=torch.float32))
    ref = u.clone()
    for _ in range(3 * steps):
        ref = ref * factor
    for tag in VARIANTS:
        y = runs[tag][ci][0]
        wrong = int((y != ref).sum())
        print(f"{tag}: {wrong} of {y.numel()} values differ from u (1 + eps)^-S; largest difference {float((y - ref).abs().max()):.3e}")
        assert wrong == 0, tag
