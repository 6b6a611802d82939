"""The hand-over schedule of the HIP forward (adi_fwd_kernel with HO = true: counters in LDS instead of a barrier per sweep,
a four-slot record ring) against the barrier schedule it replaces (PDE_FWD_SCHED=0): the same operations in the same
order per element, only their schedule changed — so `y`, `gu` and every parameter gradient must be BITWISE equal, on the
shapes of test_gpu_asm_bwd.CASES (ragged batches, time-dependent coefficients), on the headline shape of bench.py
(512 x 64 x 32 x 32, ten Strang steps) and on a batch whose workgroups end on a partial chunk.  Each schedule runs in its
own interpreter (the library reads PDE_FWD_SCHED once per process)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

CHILD = r"""
import sys, torch
sys.path[:0] = [%(root)r, %(tests)r]
import cnn_with_pde_amd as P
import cnn_with_pde_amd._lib as L
import ctypes as C
import test_gpu_asm_bwd as T
out = {}
for ci in range(len(T.CASES)):
    spec, params, u, gy, steps, dt = T._inputs(ci)
    out[ci] = T._run_gpu(params, u, gy, steps, dt)

def run(B, Cc, N, steps, dt, seed):
    g = torch.Generator().manual_seed(seed)
    ps = [(2.0 * (1 + 0.1 * torch.randn(Cc, N, N, generator=g))), (1.8 * (1 + 0.1 * torch.randn(Cc, N, N, generator=g))),
          0.1 * torch.randn(Cc, N, N, generator=g), 0.1 * torch.randn(Cc, N, N, generator=g)]
    ps = [p.cuda().requires_grad_(True) for p in ps]
    u = torch.randn(B, Cc, N, N, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(B, Cc, N, N, generator=g).cuda()
    sweeps = [s for st in P.adi_schedule(dt, 1.0, 1.0, steps) for s in st]
    y = P.adi_diffuse(u, *ps, sweeps, smooth3=False, clamp_max=10.0, checkpoints=0)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach().cpu(), u.grad.cpu(), {k: p.grad.cpu() for k, p in zip(T.NAMES, ps)}

# the headline shape (bench.py: EnhancedDiffusionLayer(32, 64), 10 steps, dt = 0.001)
out["bench"] = run(512, 64, 32, 10, 0.001, 11)
# 500 planes per channel = 15 full chunks of 32 and one of 20, two chunks per workgroup: one workgroup ends on a partial one
out["partial"] = run(500, 64, 32, 4, 0.004, 12)
lib = L.load()
out["kernel"] = [lib.pde_adi_forward_kernel(C.byref(T._desc(B, Cc, 32, steps, 0.001)))
                 for B, Cc, steps in ((512, 64, 10), (500, 64, 4), (37, 5, 1))]
torch.save(out, %(path)r)
"""


def test_hand_over_schedule_is_bitwise_equal_to_the_barrier_schedule(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    res = {}
    env0 = {k: v for k, v in os.environ.items() if k not in ("PDE_FWD_SCHED", "PDE_ASM_FWD")}
    for tag, env in (("previous", dict(env0, PDE_FWD_SCHED="0")), ("default", env0)):
        path = str(tmp_path / f"{tag}.pt")
        code = CHILD % {"root": os.path.dirname(here), "tests": here, "path": path}
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (tag, r.stderr[-1500:])
        res[tag] = torch.load(path, weights_only=True)
    # which forward ran: 0 = barrier schedule, 3 = hand-over schedule (a single-step schedule, 3 sweeps, keeps its records
    # resident and stays on the barrier-free resident path of the old schedule)
    assert res["previous"]["kernel"] == [0, 0, 0]
    assert res["default"]["kernel"] == [3, 3, 0]
    keys = [k for k in res["previous"] if k != "kernel"]
    assert len(keys) == 7
    for key in keys:
        (y0, gu0, gp0), (y1, gu1, gp1) = res["previous"][key], res["default"][key]
        assert torch.equal(y0, y1), key
        assert torch.equal(gu0, gu1), key
        assert gp0.keys() == gp1.keys()
        for name in gp0:
            assert torch.equal(gp0[name], gp1[name]), (key, name)
