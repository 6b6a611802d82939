#!/usr/bin/env python3
"""Forward + backward time of the diffusion trajectory ("the trajectory"), with HIP events on a warm device:

    traj   layer.trajectory(u) — all K states out of one sweep launch per pass, a cotangent on every state
    plain  layer(u)            — the plain layer call on the same schedule, a cotangent on the output
    chain  K chained functional.adi_diffuse calls on the one-step slices of the same schedule, a cotangent on every
           state: the only way to get these states before ``trajectory`` existed (uses nothing newer than adi_diffuse,
           so it also runs against an older checkout: --root)

    perf_trajectory.py [--modes traj,plain,chain] [--shape B C N] [--steps K] [--dtype fp32|bf16] [--rounds R] [--iters I]
                       [--root CHECKOUT] [--json FILE]

Every round times each mode once (I calls between two events, after a warm-up of the same calls), the modes alternating,
so drift of the device hits them alike; printed per mode: median, minimum and maximum over the rounds (the run-to-run
spread) in ms per forward + backward, and the bytes the algorithm has to move (fp32: forward 4 + 4K B/element, backward
4K + 4 + 4; the chain 8 and 12 per step) with the time they take at the 6.3 TB/s copy rate DESIGN quotes."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="traj,plain,chain")
    ap.add_argument("--shape", type=int, nargs=3, default=[512, 64, 32], metavar=("B", "C", "N"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import functional as F_

    if not torch.cuda.is_available():
        sys.exit("perf_trajectory.py measures on the GPU; there is none here")
    B, C, N = a.shape
    K = a.steps
    dt = torch.float32 if a.dtype == "fp32" else torch.bfloat16
    with contextlib.redirect_stdout(io.StringIO()):
        ly = P.EnhancedDiffusionLayer(N, C, dt=0.001, num_steps=K, channel_mixing_enabled=False).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    u = torch.randn(B, C, N, N, device="cuda", generator=g).to(dt).requires_grad_(True)
    gy = torch.randn(K, B, C, N, N, device="cuda", generator=g).to(dt)
    args = (ly.alpha_base, ly.beta_base, ly.alpha_time_coeff, ly.beta_time_coeff)
    kw = dict(smooth3=False, clamp_max=ly._clamp_max, eps=ly.stability_eps)
    sched = ly._schedule()
    gys = list(gy.unbind(0))

    def clear():
        u.grad = None
        for p in ly.parameters():
            p.grad = None

    def traj():
        clear()
        ly.trajectory(u).backward(gy)

    def plain():
        clear()
        ly(u).backward(gy[-1])

    def chain():
        clear()
        x, states = u, []
        for st in sched:
            x = F_.adi_diffuse(x, *args, st, **kw)
            states.append(x)
        torch.autograd.backward(states, gys)

    fns = {"traj": traj, "plain": plain, "chain": chain}
    modes = [m for m in a.modes.split(",") if m]
    for m in modes:
        for _ in range(3):
            fns[m]()
    torch.cuda.synchronize()
    times = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fns[m]()
            e1.record()
            e1.synchronize()
            times[m].append(e0.elapsed_time(e1) / a.iters)
    el = B * C * N * N
    eb = 4 if a.dtype == "fp32" else 2
    nbytes = {"traj": el * eb * ((1 + K) + (K + 2)), "plain": el * eb * (2 + 3), "chain": el * eb * K * (2 + 3)}
    out = {"shape": [B, C, N, N], "steps": K, "dtype": a.dtype, "iters": a.iters, "rounds": a.rounds,
           "library": P.library_version(), "modes": {}}
    for m in modes:
        t = times[m]
        out["modes"][m] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "all_ms": t,
                           "algorithmic_bytes": nbytes[m], "ms_at_6.3TBps": nbytes[m] / 6.3e12 * 1e3}
        print(f"{m:6s} {B}x{C}x{N}x{N} {a.dtype} {K} steps: median {statistics.median(t):8.3f} ms  "
              f"[{min(t):8.3f} .. {max(t):8.3f}] fwd+bwd; {nbytes[m] / 1e9:6.2f} GB = {nbytes[m] / 6.3e12 * 1e3:6.3f} ms at 6.3 TB/s",
              flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
