"""The look-ahead schedule of the assembly backward (MODE D, `8d`, gen_adi_bwd_asm.py) against the schedule it derives from
(MODE C, `8c`): the same floating-point instructions on the same registers in the same order, only the step top's two
round trips (time increments, hand-over counters) issued one step ahead — so `gu` and the four parameter gradients of the
library's default and of `PDE_ASM_VARIANT=8c` must be BITWISE equal.  Shapes: the five of test_gpu_asm_bwd.CASES and three
chosen for the hand-over (below).  Each variant runs in its own interpreter (the loader reads PDE_ASM_VARIANT once per
process); the default one also runs one case twice: a hand-over race shows as a run-to-run difference."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
BASE = "8c"
N = 32
HANDOVER = [  # B, C, steps, dt, relative spread, slope scale, step-closing and next step-opening x sweeps differ in time
    (17, 1, 3, 0.02, 0.15, 1.0, False),    # odd step count: the set parity flips across the chunk boundary; second chunk of one plane
    (49, 2, 2, 0.03, 0.15, 0.7, False),    # the shortest eligible schedule: the plane prefetch in the step right after a chunk's first
    (33, 8, 4, 0.01, 0.10, 1.0, True),     # no twin records: every step loads its rows at its top (load_rows_now)
]
REPEAT = 0                                 # index into test_gpu_asm_bwd.CASES: (37, 5, 3)


def handover_inputs(hi):
    """(params, u, gy, sweeps, shape) of HANDOVER[hi], seeded"""
    import cnn_with_pde_amd as P
    import test_gpu_asm_bwd as T
    from oracle import pde_oracle as O
    B, C, steps, dt, rel, slope, untwin = HANDOVER[hi]
    g = torch.Generator().manual_seed(900 + hi)
    params = O.adi_init_params(O.cifar10_spec(N, C, dt=dt, num_steps=steps), "cifar10", gen=g)
    for k in ("alpha_base", "beta_base"):
        params[k] = params[k] * (1 + rel * torch.randn(params[k].shape, generator=g))
    for k in ("alpha_time_coeff", "beta_time_coeff"):
        params[k] = slope * torch.randn(params[k].shape, generator=g)
    u = torch.randn(B, C, N, N, generator=g)
    gy = torch.randn(B, C, N, N, generator=g)
    sched = P.adi_schedule(dt, 1.0, 1.0, steps)
    if untwin:
        # every step but the first opens a quarter of a time step later than the step before it closed
        sched = [[dataclasses.replace(s, t=s.t + 0.25 * dt) if (si and j == 0) else s for j, s in enumerate(st)]
                 for si, st in enumerate(sched)]
        assert all(a[2].t != b[0].t for a, b in zip(sched, sched[1:]))
    return {k: params[k] for k in T.NAMES}, u, gy, [s for st in sched for s in st], (B, C, steps)


def run_sweeps(params, u, gy, sweeps):
    import cnn_with_pde_amd as P
    import test_gpu_asm_bwd as T
    ud = u.cuda().requires_grad_(True)
    ps = [params[k].cuda().requires_grad_(True) for k in T.NAMES]
    P.adi_diffuse(ud, *ps, sweeps, smooth3=False, clamp_max=10.0, checkpoints=0).backward(gy.cuda())
    torch.cuda.synchronize()
    return ud.grad.cpu(), {k: p.grad.cpu() for k, p in zip(T.NAMES, ps)}


def kernel_of(B, C, sweeps):
    """what pde_adi_backward says it runs for this schedule: 1 = the assembly kernel"""
    import ctypes as C_
    import cnn_with_pde_amd.functional as F
    import cnn_with_pde_amd._lib as L
    return L.load().pde_adi_backward_kernel(C_.byref(F._build_desc(B, C, N, L.PDE_IO_F32, sweeps, False, 10.0, 1e-6)), 0)


CHILD = r"""
import sys, torch
sys.path[:0] = [%(root)r, %(tests)r]
import cnn_with_pde_amd as P
import test_gpu_asm_bwd as T
import test_gpu_asm_bwd_sched_d as D
out, kern = {}, []
for ci in range(len(T.CASES)):
    spec, params, u, gy, steps, dt = T._inputs(ci)
    sweeps = [s for st in P.adi_schedule(dt, 1.0, 1.0, steps) for s in st]
    out["case%%d" %% ci] = D.run_sweeps(params, u, gy, sweeps)
    kern.append(D.kernel_of(u.shape[0], u.shape[1], sweeps))
    if %(twice)d and ci == D.REPEAT:
        out["again"] = D.run_sweeps(params, u, gy, sweeps)
for hi in range(len(D.HANDOVER)):
    params, u, gy, sweeps, (B, C, steps) = D.handover_inputs(hi)
    out["handover%%d" %% hi] = D.run_sweeps(params, u, gy, sweeps)
    kern.append(D.kernel_of(B, C, sweeps))
out["kernel"] = kern
torch.save(out, %(path)r)
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("sched_d")
    res = {}
    env0 = {k: v for k, v in os.environ.items() if k not in ("PDE_ASM_VARIANT", "PDE_ASM_BWD")}
    for tag, env in (("base", dict(env0, PDE_ASM_VARIANT=BASE)), ("default", env0)):
        path = str(tmp / f"{tag}.pt")
        code = CHILD % {"root": os.path.dirname(here), "tests": here, "path": path, "twice": int(tag == "default")}
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (tag, r.stderr[-1500:])
        res[tag] = torch.load(path, weights_only=True)
    return res


def _same(a, b, key):
    (gu0, gp0), (gu1, gp1) = a, b
    assert torch.equal(gu0, gu1), key
    assert gp0.keys() == gp1.keys() and len(gp0) == 4
    for name in gp0:
        assert torch.equal(gp0[name], gp1[name]), (key, name)


def test_every_child_ran_the_assembly_kernel(runs):
    for tag in ("base", "default"):
        assert runs[tag]["kernel"] == [1] * 8, (tag, runs[tag]["kernel"])


@pytest.mark.parametrize("key", [f"case{i}" for i in range(5)] + [f"handover{i}" for i in range(len(HANDOVER))])
def test_default_is_bitwise_equal_to_8c(runs, key):
    _same(runs["base"][key], runs["default"][key], key)


def test_default_repeats_bitwise(runs):
    _same(runs["default"][f"case{REPEAT}"], runs["default"]["again"], "again")
