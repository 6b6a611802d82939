"""The stagger of the forward's hand-over schedule (PDE_FWD_STAGGER, adi_fwd_kernel with HO = true): the second workgroup
of every CU holds its first plane loads back and the two take turns in priority, so that they run out of phase and end
together.  Only WHEN a workgroup runs changes — so `y`, `gu` and every parameter gradient must be BITWISE equal with the
stagger on (PDE_FWD_STAGGER=1), off (PDE_FWD_STAGGER=0) and on the barrier schedule (PDE_FWD_SCHED=0), `y` must agree
with the fp64 oracle, and a call with the stagger on must capture into a graph and replay to the same bits.

Shapes (N = 32, fp32, Strang, dt = 0.001, time-dependent coefficients, 2 and 3 steps: more than three sweeps select the
hand-over kernel): a ragged second chunk with most workgroups idle (33 x 1), groups with one and two chunks and a partial
last chunk (96 x 2, 70 x 3), fewer planes than one wave set (7 x 3), and 2048 x 8 = 64 chunks per channel, 8 x 64 = 512
workgroups: two on every CU, the only launches here that the library staggers.  Each variant runs in its own interpreter
(the switches are read once per process), once for all tests of this file."""
import os
import subprocess
import sys

import pytest
import torch

import golden_util as G
from oracle import pde_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5                      # tests/test_gpu_asm_bwd.py, same layer
N, DT = 32, 0.001
NAMES = ["alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff"]
SHAPES = [(33, 1), (96, 2), (70, 3), (7, 3), (2048, 8)]
CASES = [(B, C, steps) for (B, C) in SHAPES for steps in (2, 3)]
VARIANTS = {"stagger": {"PDE_FWD_STAGGER": "1"}, "plain": {"PDE_FWD_STAGGER": "0"}, "barrier": {"PDE_FWD_SCHED": "0"}}


def _inputs(ci):
    B, C, steps = CASES[ci]
    g = torch.Generator().manual_seed(900 + ci)
    spec = O.cifar10_spec(N, C, dt=DT, num_steps=steps)
    params = O.adi_init_params(spec, "cifar10", gen=g)
    params["channel_mixing"] = torch.eye(C)
    for k in ("alpha_base", "beta_base"):
        params[k] = params[k] * (1 + 0.15 * torch.randn(params[k].shape, generator=g))
    for k in ("alpha_time_coeff", "beta_time_coeff"):
        params[k] = 1.0 * torch.randn(params[k].shape, generator=g)
    u = torch.randn(B, C, N, N, generator=g)
    gy = torch.randn(B, C, N, N, generator=g)
    return spec, params, u, gy


CHILD = r"""
import sys, torch
sys.path[:0] = [%(root)r, %(tests)r]
import ctypes as C
import cnn_with_pde_amd as P
import cnn_with_pde_amd._lib as L
import test_gpu_asm_bwd as A
import test_gpu_fwd_stagger as T
lib = L.load()
out = {"kernel": []}
for ci, (B, Cc, steps) in enumerate(T.CASES):
    spec, params, u, gy = T._inputs(ci)
    out[ci] = A._run_gpu(params, u, gy, steps, T.DT)
    out["kernel"].append(lib.pde_adi_forward_kernel(C.byref(A._desc(B, Cc, T.N, steps, T.DT))))
# the staggered launch inside a graph: captured once, replayed twice, against the eager call
ci = len(T.CASES) - 1
B, Cc, steps = T.CASES[ci]
spec, params, u, gy = T._inputs(ci)
sweeps = [s for st in P.adi_schedule(T.DT, 1.0, 1.0, steps) for s in st]
ud = u.cuda()
ps = [params[k].cuda() for k in T.NAMES]
with torch.no_grad():
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            P.adi_diffuse(ud, *ps, sweeps, smooth3=False, clamp_max=10.0, checkpoints=0)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yg = P.adi_diffuse(ud, *ps, sweeps, smooth3=False, clamp_max=10.0, checkpoints=0)
    replays = []
    for _ in range(2):
        yg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replays.append(yg.cpu().clone())
out["graph"] = replays
torch.save(out, %(path)r)
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("fwd_stagger")
    env0 = {k: v for k, v in os.environ.items() if k not in ("PDE_FWD_STAGGER", "PDE_FWD_SCHED", "PDE_ASM_FWD")}
    res = {}
    for tag, env in VARIANTS.items():
        path = str(tmp / f"{tag}.pt")
        code = CHILD % {"root": os.path.dirname(here), "tests": here, "path": path}
        r = subprocess.run([sys.executable, "-c", code], env=dict(env0, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (tag, r.stderr[-1500:])
        res[tag] = torch.load(path, weights_only=True)
    return res


def test_the_hand_over_kernel_is_what_runs(runs):
    # 3 = the hand-over schedule, 0 = the barrier schedule (pde_adi_forward_kernel)
    assert runs["stagger"]["kernel"] == [3] * len(CASES)
    assert runs["plain"]["kernel"] == [3] * len(CASES)
    assert runs["barrier"]["kernel"] == [0] * len(CASES)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_bitwise_equal_across_the_three_schedules(runs, ci):
    y0, gu0, gp0 = runs["stagger"][ci]
    for tag in ("plain", "barrier"):
        y1, gu1, gp1 = runs[tag][ci]
        assert torch.equal(y0, y1), (tag, CASES[ci])
        assert torch.equal(gu0, gu1), (tag, CASES[ci])           # the backward reads y
        assert gp0.keys() == gp1.keys() and len(gp0) == 4
        for name in gp0:
            assert torch.equal(gp0[name], gp1[name]), (tag, CASES[ci], name)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_y_against_the_fp64_oracle(runs, ci):
    spec, params, u, gy = _inputs(ci)
    with torch.no_grad():
        y_ref = O.adi_forward(u.double(), {k: v.double() for k, v in params.items()}, spec)
    err = G.rel_err(runs["stagger"][ci][0], y_ref)
    print(f"case {CASES[ci]}: rel err of y against the fp64 oracle {err:.3e}")
    assert err <= TOL, (CASES[ci], err)


def test_a_staggered_call_replays_from_a_graph_to_the_same_bits(runs):
    for tag in VARIANTS:                                       # (the capture itself fails on an allocation or a synchronisation)
        y = runs[tag][len(CASES) - 1][0]
        for r in runs[tag]["graph"]:
            assert torch.equal(r, y), tag
