#!/usr/bin/env python3
"""Time of a gradient-penalty step through a PDE layer against the plain training step ("second order"), with
HIP events on a warm device:

    plain    forward, backward                                              (what every training step runs)
    penalty  forward, backward with create_graph=True, backward of |grad_u|^2 + the loss
             (an input-gradient penalty: the second-order pass runs the layer's forward and full backward once more,
             at the penalty's cotangent — functional.linear_adjoint)

    perf_double_backward.py [--shapes headline,svhn] [--rounds R] [--iters I] [--json FILE] [--once]

From the code one expects the penalty step to cost about two plain steps: one more forward and one more full backward.
Every round times each of the two once (I calls between two events, after a warm-up of the same calls), alternating in
one process, so drift of the device hits them alike; printed: median [min .. max] over the rounds in ms per step, and the
ratio of the medians.  The method of tools/perf_backward_input.py.  --once runs each three times and stops."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys


def build(P, name):
    """(layer, input shape) of the two shapes DESIGN quotes."""
    with contextlib.redirect_stdout(io.StringIO()):
        if name == "headline":          # 512 x 64 x 32 x 32, 10 Strang steps, fp32, no channel operator
            return P.EnhancedDiffusionLayer(32, 64, dt=0.001, num_steps=10, channel_mixing_enabled=False), (512, 64, 32, 32)
        if name == "svhn":              # the one-launch C <= 4 kernels with the skip blend
            return P.SvhnDiffusionLayer(32, 3, num_steps=10), (512, 3, 32, 32)
    raise SystemExit(f"unknown shape {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,svhn")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--weight", type=float, default=0.1, help="the penalty's weight")
    ap.add_argument("--json", default=None)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import cnn_with_pde_amd as P

    if not torch.cuda.is_available():
        sys.exit("perf_double_backward.py measures on the GPU; there is none here")
    routes = ["plain", "penalty"]
    out = {"library": P.library_version(), "iters": a.iters, "rounds": a.rounds, "shapes": {}}
    for name in [s for s in a.shapes.split(",") if s]:
        g = torch.Generator(device="cuda").manual_seed(1)
        layer, shape = build(P, name)
        layer = layer.cuda()
        if not getattr(layer, "channel_mixing_enabled", True):
            layer.channel_mixing.requires_grad_(False)            # (identity, unused: the layer runs no channel operator)
        u = torch.randn(*shape, device="cuda", generator=g).requires_grad_(True)
        c = torch.randn(*shape, device="cuda", generator=g)

        def call(r):
            u.grad = None
            for p in layer.parameters():
                p.grad = None
            loss = (layer(u) * c).sum()
            if r == "plain":
                loss.backward()
                return
            (gu,) = torch.autograd.grad(loss, u, create_graph=True)
            (loss + a.weight * gu.pow(2).sum()).backward()

        for r in routes:
            for _ in range(3):
                call(r)
        torch.cuda.synchronize()
        if a.once:
            continue
        times = {r: [] for r in routes}
        for _ in range(a.rounds):
            for r in routes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    call(r)
                e1.record()
                e1.synchronize()
                times[r].append(e0.elapsed_time(e1) / a.iters)
        out["shapes"][name] = {"shape": list(shape), "routes": {}}
        for r in routes:
            t = times[r]
            out["shapes"][name]["routes"][r] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "all_ms": t}
            print(f"{name:9s} {'x'.join(map(str, shape)):>16s} {r:7s}: median {statistics.median(t):8.3f} ms  "
                  f"[{min(t):8.3f} .. {max(t):8.3f}] per step", flush=True)
        ratio = statistics.median(times["penalty"]) / statistics.median(times["plain"])
        out["shapes"][name]["penalty_over_plain"] = ratio
        print(f"{name:9s} penalty / plain (medians): {ratio:.3f}", flush=True)
    if a.json and not a.once:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
