#!/usr/bin/env python3
"""Forward + backward time of the explicit 5-point and the Jacobi layers with frozen parameters ("the backward
for the input alone, explicit and Jacobi layers"), with HIP events on a warm device:

    frozen   every parameter with requires_grad_(False), the input requires grad: the forward that parks nothing (register
             planes) and pde_explicit5_backward_input_states / pde_jacobi_io_backward_input_states
    full     the SAME layer with trainable parameters: the forward that parks its states and the full backward — which is
             what a frozen layer ran before (a build without the input-only route shows the two columns alike)
    forward  the layer under no_grad

    perf_backward_input_explicit.py [--shapes pde48,pde224,improved3,cfg5,generic48] [--rounds R] [--iters I] [--memory]
                                    [--json FILE]

Shapes: pde48 = PDELayer() on (B,1,48,48) at B = 64 and 512; pde224 = PDELayer(224, 224) at B = 64 (Nt = 10, the
coefficients of the 48 x 48 layer); improved3 = ImprovedDiffusionLayer(64, 3, num_steps=10) at B = 256; cfg5 =
ImprovedDiffusionLayer(64, 64, num_steps=10) at B = 64 (BASELINE cfg5); generic48 = ImprovedDiffusionLayer(48, 16,
num_steps=10) at B = 64, a plane size without register kernels.  All routes run in ONE process and alternate round by
round: R rounds of I calls between two events per route, after a warm-up of the same calls.  Printed per shape: median
[min .. max] of every route, frozen / full, and whether the frozen median exceeds the full one.  --memory adds the peak
memory of one forward + backward beside the inputs (torch.cuda.max_memory_allocated) on pde224 and cfg5, both routes."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: shape -> (layer class, constructor arguments, input shape without the batch, batches)
SHAPES = {"pde48": ("PDELayer", dict(Nx=48, Ny=48), (1, 48, 48), (64, 512)),
          "pde224": ("PDELayer", dict(Nx=224, Ny=224), (1, 224, 224), (64,)),
          "improved3": ("ImprovedDiffusionLayer", dict(size=64, channels=3, num_steps=10), (3, 64, 64), (256,)),
          "cfg5": ("ImprovedDiffusionLayer", dict(size=64, channels=64, num_steps=10), (64, 64, 64), (64,)),
          "generic48": ("ImprovedDiffusionLayer", dict(size=48, channels=16, num_steps=10), (16, 48, 48), (64,))}
MEMORY = ("pde224", "cfg5")


def build(P, torch, name, B, route):
    """A callable that runs one call of the route."""
    cls, kw, plane, _ = SHAPES[name]
    g = torch.Generator(device="cuda").manual_seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        m = getattr(P, cls)(**kw).cuda()
    if cls == "PDELayer" and kw["Nx"] != 48:
        with torch.no_grad():                                  # the step coefficients of the 48 x 48 layer: a stable time loop
            for p in m.parameters():
                p.mul_((48.0 / kw["Nx"]) ** 2)
    for p in m.parameters():
        p.requires_grad_(route == "full")
    x = torch.randn(B, *plane, device="cuda", generator=g).requires_grad_(route != "forward")
    gy = torch.randn(B, *plane, device="cuda", generator=g)
    if route == "forward":
        def call():
            with torch.no_grad():
                return m(x)
    elif route == "full":
        ps = [p for p in m.parameters() if p.requires_grad and p is not getattr(m, "beta_base", None)]

        def call():
            return torch.autograd.grad(m(x), [x] + ps, gy)
    else:
        def call():
            return torch.autograd.grad(m(x), x, gy)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="pde48,pde224,improved3,cfg5,generic48")
    ap.add_argument("--routes", default="frozen,full,forward")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--memory", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L

    if not torch.cuda.is_available():
        sys.exit("perf_backward_input_explicit.py measures on the GPU; there is none here")
    routes = [r for r in a.routes.split(",") if r]
    res = {"bwd_input": L.bwd_input_enabled() and hasattr(L, "SIGNATURES_EXPLICIT_INPUT"), "version": P.library_version(),
           "rows": {}}
    print(f"library {res['version']}; input-only route of the explicit layers: {res['bwd_input']}", flush=True)
    for name in [s for s in a.shapes.split(",") if s]:
        for B in SHAPES[name][3]:
            calls = {r: build(P, torch, name, B, r) for r in routes}
            for c in calls.values():
                for _ in range(3):
                    c()
            torch.cuda.synchronize()
            t = {r: [] for r in routes}
            for _ in range(a.rounds):
                for r in routes:                               # the routes alternate round by round
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        calls[r]()
                    e1.record()
                    e1.synchronize()
                    t[r].append(e0.elapsed_time(e1) / a.iters)
            row = {r: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for r, v in t.items()}
            if a.memory and name in MEMORY:
                del calls
                for r in routes:
                    if r == "forward":
                        continue
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    c = build(P, torch, name, B, r)
                    c()                                        # (the workspace of the first call, the parameter views)
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    c()
                    torch.cuda.synchronize()
                    row[r]["peak_bytes"] = torch.cuda.max_memory_allocated() - base
                    del c
            res["rows"][f"{name}-b{B}"] = row
            line = "  ".join(f"{r} {v['median_ms']:.4f} [{v['min_ms']:.4f} .. {v['max_ms']:.4f}]" for r, v in row.items())
            if "frozen" in row and "full" in row:
                line += f"  frozen / full {row['frozen']['median_ms'] / row['full']['median_ms']:.3f}" \
                        f"  frozen median above full median: {row['frozen']['median_ms'] > row['full']['median_ms']}"
            print(f"{name + '-b' + str(B):16s} {line}", flush=True)
            if "peak_bytes" in row.get("frozen", {}):
                print(f"{'':16s} peak memory of one forward + backward beside the inputs: frozen "
                      f"{row['frozen']['peak_bytes'] / 2 ** 20:.1f} MiB, full {row['full']['peak_bytes'] / 2 ** 20:.1f} MiB", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
