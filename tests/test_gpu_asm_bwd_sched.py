"""The scalar-trimmed schedule of the assembly backward (MODE C, `8c`, gen_adi_bwd_asm.py) against the round-4 schedule it
replaces (MODE B, `8b`): the same operations in the same order per element, only the scalar work, the counter hand-over
and the wait states moved — so `gu` and every parameter gradient must be BITWISE equal, on the shapes of
test_gpu_asm_bwd.CASES (ragged batches, time-dependent coefficients, chunk-to-chunk summation by parts) and on the
headline shape of bench.py (512 x 64 x 32 x 32, ten Strang steps).  Each variant runs in its own interpreter (the
loader reads PDE_ASM_VARIANT once per process)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
PREVIOUS = "8b"

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
    y, gu, gp = T._run_gpu(params, u, gy, steps, dt)
    out[ci] = (gu, gp)
# the headline shape (bench.py: EnhancedDiffusionLayer(32, 64), 10 steps, dt = 0.001)
B, Cc, N, steps, dt = 512, 64, 32, 10, 0.001
g = torch.Generator().manual_seed(11)
ps = [(2.0 * (1 + 0.1 * torch.randn(Cc, N, N, generator=g))), (1.8 * (1 + 0.1 * torch.randn(Cc, N, N, generator=g))),
      0.1 * torch.randn(Cc, N, N, generator=g), 0.1 * torch.randn(Cc, N, N, generator=g)]
ps = [p.cuda().requires_grad_(True) for p in ps]
u = torch.randn(B, Cc, N, N, generator=g).cuda().requires_grad_(True)
gy = torch.randn(B, Cc, N, N, generator=g).cuda()
sweeps = [s for st in P.adi_schedule(dt, 1.0, 1.0, steps) for s in st]
P.adi_diffuse(u, *ps, sweeps, smooth3=False, clamp_max=10.0, checkpoints=0).backward(gy)
torch.cuda.synchronize()
out["bench"] = (u.grad.cpu(), {k: p.grad.cpu() for k, p in zip(T.NAMES, ps)})
lib = L.load()
out["waves"] = lib.pde_adi_backward_kernel(C.byref(T._desc(B, Cc, N, steps, dt)), 0)
torch.save(out, %(path)r)
"""


def test_new_schedule_is_bitwise_equal_to_the_previous(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    res = {}
    env0 = {k: v for k, v in os.environ.items() if k not in ("PDE_ASM_VARIANT", "PDE_ASM_BWD")}
    for tag, env in (("previous", dict(env0, PDE_ASM_VARIANT=PREVIOUS)), ("default", env0)):
        path = str(tmp_path / f"{tag}.pt")
        code = CHILD % {"root": os.path.dirname(here), "tests": here, "path": path}
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (tag, r.stderr[-1500:])
        res[tag] = torch.load(path, weights_only=True)
    assert res["previous"]["waves"] == 1 and res["default"]["waves"] == 1     # both runs took the assembly kernel
    keys = [k for k in res["previous"] if k != "waves"]
    assert len(keys) == 6
    for key in keys:
        (gu0, gp0), (gu1, gp1) = res["previous"][key], res["default"][key]
        assert torch.equal(gu0, gu1), key
        assert gp0.keys() == gp1.keys()
        for name in gp0:
            assert torch.equal(gp0[name], gp1[name]), (key, name)
