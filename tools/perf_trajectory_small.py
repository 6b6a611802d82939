#!/usr/bin/env python3
"""Forward + backward time of ``layer.trajectory(u)`` for the layers with a channel operator at C <= 4 ("the
trajectory"), with HIP events on a warm device, in ONE process:

    small     small_channel_kernels = True:  functional.adi_diffuse_small_states, one launch per pass
    per_step  small_channel_kernels = False: functional.adi_diffuse_mixed_per_step, one operator call and one sweep call
              per step and pass — the only route before the one-launch kernels emitted states, and unchanged since

for SvhnDiffusionLayer(32, 3, num_steps=10) and EnhancedDiffusionLayer(32, 3, num_steps=10) at batch sizes 64 and 512,
a cotangent on every state.

    perf_trajectory_small.py [--layers svhn,enhanced] [--batches 64 512] [--steps K] [--rounds R] [--iters I] [--json FILE]

Every round times each route once (I calls between two events, after a warm-up of the same calls), the routes
alternating, so drift of the device hits them alike; printed per case: median, minimum and maximum over the rounds in ms
per forward + backward, and the ratio of the medians (per_step / small).  Before timing, the two routes are compared on
the same input (states and input gradient; the largest relative difference is printed)."""
import argparse
import contextlib
import copy
import io
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="svhn,enhanced")
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import cnn_with_pde_amd as P

    if not torch.cuda.is_available():
        sys.exit("perf_trajectory_small.py measures on the GPU; there is none here")
    N, C, K = 32, 3, a.steps
    out = {"steps": K, "iters": a.iters, "rounds": a.rounds, "library": P.library_version(), "cases": []}
    for kind in [k for k in a.layers.split(",") if k]:
        with contextlib.redirect_stdout(io.StringIO()):
            cls = {"svhn": P.SvhnDiffusionLayer, "enhanced": P.EnhancedDiffusionLayer}[kind]
            small = cls(N, C, num_steps=K).cuda()
        per_step = copy.deepcopy(small)
        per_step.small_channel_kernels = False
        for B in a.batches:
            g = torch.Generator(device="cuda").manual_seed(1)
            u = torch.randn(B, C, N, N, device="cuda", generator=g).requires_grad_(True)
            gy = torch.randn(K, B, C, N, N, device="cuda", generator=g)

            def call(ly):
                u.grad = None
                for p in ly.parameters():
                    p.grad = None
                y = ly.trajectory(u)
                y.backward(gy)
                return y.detach(), u.grad

            ys, gs = call(small)
            yp, gp = call(per_step)
            diff = max(float((ys - yp).abs().max() / yp.abs().max()), float((gs - gp).abs().max() / gp.abs().max()))
            routes = {"small": small, "per_step": per_step}
            for ly in routes.values():
                for _ in range(3):
                    call(ly)
            torch.cuda.synchronize()
            times = {m: [] for m in routes}
            for _ in range(a.rounds):
                for m, ly in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        call(ly)
                    e1.record()
                    e1.synchronize()
                    times[m].append(e0.elapsed_time(e1) / a.iters)
            med = {m: statistics.median(t) for m, t in times.items()}
            ratio = med["per_step"] / med["small"]
            out["cases"].append({"layer": kind, "shape": [B, C, N, N], "max_rel_diff": diff, "ratio": ratio,
                                 "routes": {m: {"median_ms": med[m], "min_ms": min(t), "max_ms": max(t), "all_ms": t}
                                            for m, t in times.items()}})
            for m, t in times.items():
                print(f"{kind:8s} {B}x{C}x{N}x{N} {K} steps {m:8s}: median {med[m]:8.3f} ms  [{min(t):8.3f} .. {max(t):8.3f}] "
                      f"fwd+bwd", flush=True)
            print(f"{kind:8s} {B}x{C}x{N}x{N} per_step / small = {ratio:.2f}x   (routes differ by {diff:.1e})", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
