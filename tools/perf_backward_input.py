#!/usr/bin/env python3
"""Forward + backward time of an implicit layer whose coefficients are frozen ("the backward for the input
alone"), with HIP events on a warm device:

    frozen  the layer with requires_grad_(False) on every parameter: the backward is gu = F^T gy alone
            (pde_adi_backward_input: 8 B/element, the forward's launch shape)
    full    the same layer with parameters that require grad: the full training backward (12 B/element, state rebuild
            or parked states, four gradient sums, adi_pgrad_kernel) — what a frozen layer ran before the input-only
            backward existed, and what PDE_BWD_INPUT=0 still runs for it

    perf_backward_input.py [--shapes headline,fashion,small,anysize] [--routes frozen,full] [--rounds R] [--iters I]
                           [--root CHECKOUT] [--json FILE] [--once]

Every round times each route once (I calls between two events, after a warm-up of the same calls), the routes
alternating in one process, so drift of the device hits them alike; printed per route: median [min .. max] over the rounds
in ms per forward + backward.  --root runs the same script against another checkout (an older one knows no frozen path:
both routes then run the full backward there, which is the confirmation that `full` is what a frozen layer cost).
--once runs every route three times and stops: the run to put under `rocprofv3 --kernel-trace --stats`."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys


def build(P, torch, name):
    """(layer, input shape) of one of the shapes DESIGN §4 quotes."""
    with contextlib.redirect_stdout(io.StringIO()):
        if name == "headline":          # 512 x 64 x 32 x 32, 10 Strang steps, fp32, no channel operator
            return P.EnhancedDiffusionLayer(32, 64, dt=0.001, num_steps=10, channel_mixing_enabled=False), (512, 64, 32, 32)
        if name == "fashion":           # fashion-sized coefficients: the full backward parks states (checkpoints)
            return P.FashionDiffusionLayer(28, dt=0.3, num_steps=4), (512 * 32, 1, 28, 28)
        if name == "small":             # launch-bound
            return P.MnistDiffusionLayer(28), (64, 1, 28, 28)
        if name == "anysize":           # 64 x 16 planes of 64 x 64 on the any-size kernels
            return P.EnhancedDiffusionLayer(64, 16, dt=0.001, num_steps=10, channel_mixing_enabled=False), (64, 16, 64, 64)
    raise SystemExit(f"unknown shape {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,fashion,small,anysize")
    ap.add_argument("--routes", default="frozen,full")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--json", default=None)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch
    import cnn_with_pde_amd as P

    if not torch.cuda.is_available():
        sys.exit("perf_backward_input.py measures on the GPU; there is none here")
    routes = [r for r in a.routes.split(",") if r]
    out = {"library": P.library_version(), "root": a.root, "iters": a.iters, "rounds": a.rounds, "shapes": {}}
    for name in [s for s in a.shapes.split(",") if s]:
        g = torch.Generator(device="cuda").manual_seed(1)
        layers = {}
        for r in routes:
            ly, shape = build(P, torch, name)
            ly = ly.cuda()
            if "channel_mixing" in dict(ly.named_parameters()):
                ly.channel_mixing.requires_grad_(False)           # (identity, unused: the layer runs no channel operator)
            if r == "frozen":
                for p in ly.parameters():
                    p.requires_grad_(False)
            layers[r] = ly
        u = torch.randn(*shape, device="cuda", generator=g).requires_grad_(True)
        gy = torch.randn(*shape, device="cuda", generator=g)

        def call(r):
            u.grad = None
            for p in layers[r].parameters():
                p.grad = None
            layers[r](u).backward(gy)

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
            print(f"{name:9s} {'x'.join(map(str, shape)):>16s} {r:6s}: median {statistics.median(t):8.3f} ms  "
                  f"[{min(t):8.3f} .. {max(t):8.3f}] fwd+bwd", flush=True)
        if len(routes) == 2:
            lo, hi = times[routes[0]], times[routes[1]]
            print(f"{name:9s} {routes[0]} / {routes[1]} (medians): {statistics.median(lo) / statistics.median(hi):.3f}; "
                  f"[min .. max] of {routes[0]} lies wholly below that of {routes[1]}: {max(lo) < min(hi)}", flush=True)
    if a.json and not a.once:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
