#!/usr/bin/env python3
"""Diagnostic: forward + backward time of one implicit layer call (10 Strang steps = 30 sweeps, no channel operator) at
line lengths with and without fused kernels (pde_adi_line_length_path 1 / 2), or on ONE plane shape:

    perf_anysize.py [B] [C]                        the square sweep over N = 32 ... 128 (event-free wall time per call)
    perf_anysize.py B C H W [old|rect] [steps]     one plane: H != W runs the rectangle entry points (pde_adi_rect_*);
                                                   H == W the square ones ("old", default) or, with "rect", the rectangle
                                                   entry points on the square — same kernels, same work

The wall time printed includes the host's launch path.  For kernel time run the one-plane form under
``rocprofv3 --kernel-trace --stats -- python tools/perf_anysize.py ...`` and add the gen_*_kernel rows: ``steps`` calls are
timed after 3 warm-up calls, so per call it is the rows' TotalDurationNs / (steps + 3)  (DESIGN §4)."""
import contextlib
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import cnn_with_pde_amd as P  # noqa: E402
from cnn_with_pde_amd import functional as F_  # noqa: E402


def run(B, C, H, W, entry="old", n=10):
    with contextlib.redirect_stdout(io.StringIO()):
        ly = P.EnhancedDiffusionLayer(H if H == W else (H, W), C, dt=0.01, num_steps=10, channel_mixing_enabled=False).cuda()
    u = torch.randn(B, C, H, W, device="cuda", requires_grad=True)
    gy = torch.randn_like(u)
    args = (ly.alpha_base, ly.beta_base, ly.alpha_time_coeff, ly.beta_time_coeff)
    sweeps = ly._schedule().flat

    def step():
        for p in ly.parameters():
            p.grad = None
        u.grad = None
        if entry == "rect" and H == W:          # the layer sends squares to the square entry points: call the function itself
            y = F_._AdiFn.apply(u, *args, sweeps, False, ly._clamp_max, ly.stability_eps, "auto", None, None, True, False)
        else:
            y = ly(u)
        y.backward(gy)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    which = "rect entry" if (H != W or entry == "rect") else "square entry"
    print(f"{H:4d} x {W:4d} {which} ({B}x{C} planes, 30 sweeps): {ms:8.3f} ms fwd+bwd wall, "
          f"{B * C * H * W * 30 / ms / 1e6:8.1f} M element-sweeps/ms", flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    B = int(a[0]) if len(a) > 0 else 64
    C = int(a[1]) if len(a) > 1 else 16
    if len(a) >= 4:
        run(B, C, int(a[2]), int(a[3]), a[4] if len(a) > 4 else "old", int(a[5]) if len(a) > 5 else 10)
    else:
        for N in (32, 36, 48, 64, 96, 128):
            run(B, C, N, N)
