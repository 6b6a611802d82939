#!/usr/bin/env python3
"""Forward + backward time of the layers with a channel operator above C = 4 with frozen parameters ("the
backward for the input alone, channel-operator layers"), with HIP events on a warm device:

    frozen  every parameter with requires_grad_(False), the input requires grad: pde_adi_mixed_forward_input +
            pde_adi_mixed_backward_input (and the skip split alone behind an SVHN layer)
    full    the SAME call in a process started with PDE_BWD_INPUT=0: the forward that keeps 2K - 1 states and the full
            training backward — state rebuild, gradient sums, g u^T on the matrix cores, the parameter-gradient epilogue,
            the wait for the coefficient maxima — which is what such a call ran before

    perf_backward_input_mixed.py [--shapes enhanced64,svhn32,enhanced64_bf16,c5] [--batches 64,512] [--rounds R]
                                 [--iters I] [--processes P] [--memory] [--json FILE]

Shapes: enhanced64 = EnhancedDiffusionLayer(32, 64, num_steps=10) at B = 64 and 512; svhn32 = SvhnDiffusionLayer(32, 32,
num_steps=10) at B = 512; enhanced64_bf16 the first on bf16 tensors at B = 512; c5 = EnhancedDiffusionLayer(28, 5,
num_steps=10) at B = 64.  Each route runs in child processes of its own (the switch is read once per process), P of them
one after the other, routes alternating.  A child times every shape R times (I calls between two events after a warm-up
of the same calls) and reports the median with [min .. max].  Printed per shape: the P medians of either route, and whether
every frozen median lies below every full median by more than the process-to-process spread (max - min of the medians of
a route, the larger of the two routes).  --memory adds the peak memory of one call of the first shape on either route."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: shape -> (layer class, size, channels, tensors, batches it is timed at; None: --batches)
SHAPES = {"enhanced64": ("EnhancedDiffusionLayer", 32, 64, "f32", None), "svhn32": ("SvhnDiffusionLayer", 32, 32, "f32", (512,)),
          "enhanced64_bf16": ("EnhancedDiffusionLayer", 32, 64, "bf16", (512,)), "c5": ("EnhancedDiffusionLayer", 28, 5, "f32", (64,))}


def build(P, torch, name, B):
    """A callable that runs one forward + backward of the frozen layer."""
    cls, N, Cc, io_t, _ = SHAPES[name]
    g = torch.Generator(device="cuda").manual_seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        m = getattr(P, cls)(N, Cc, num_steps=10).cuda()
    for p in m.parameters():
        p.requires_grad_(False)
    dt = torch.bfloat16 if io_t == "bf16" else torch.float32
    x = torch.randn(B, Cc, N, N, device="cuda", generator=g).to(dt).requires_grad_(True)
    gy = torch.randn(B, Cc, N, N, device="cuda", generator=g).to(dt)

    def call():
        return torch.autograd.grad(m(x), x, gy)
    return call


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L

    if not torch.cuda.is_available():
        sys.exit("perf_backward_input_mixed.py measures on the GPU; there is none here")
    out = {"bwd_input": L.bwd_input_enabled(), "rows": {}}
    for name in a.shapes:
        for B in SHAPES[name][4] or a.batches:
            call = build(P, torch, name, B)
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            t = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    call()
                e1.record()
                e1.synchronize()
                t.append(e0.elapsed_time(e1) / a.iters)
            row = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
            if a.memory and not out["rows"]:
                del call
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                call = build(P, torch, name, B)
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                call()
                torch.cuda.synchronize()
                row["peak_bytes"] = torch.cuda.max_memory_allocated() - base
            out["rows"][f"{name}-b{B}"] = row
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="enhanced64,svhn32,enhanced64_bf16,c5")
    ap.add_argument("--batches", default="64,512")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--memory", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    a.shapes = [s for s in a.shapes.split(",") if s]
    a.batches = [int(b) for b in a.batches.split(",") if b]
    if a.child:
        return child(a)
    res = {"frozen": [], "full": []}
    for i in range(a.processes):
        for route in ("frozen", "full"):
            env = dict(os.environ)
            env.pop("PDE_BWD_INPUT", None)
            if route == "full":
                env["PDE_BWD_INPUT"] = "0"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shapes", ",".join(a.shapes), "--batches",
                   ",".join(map(str, a.batches)), "--rounds", str(a.rounds), "--iters", str(a.iters)]
            r = subprocess.run(cmd + (["--memory"] if a.memory else []), env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"child {route} {i} failed ({r.returncode}): {r.stderr[-2000:]}")
            got = json.loads(r.stdout.strip().splitlines()[-1])
            assert got["bwd_input"] == (route == "frozen")
            res[route].append(got["rows"])
    ok_all = True
    for row in res["frozen"][0]:
        fz = [p[row] for p in res["frozen"]]
        fu = [p[row] for p in res["full"]]
        mf, mu = [p["median_ms"] for p in fz], [p["median_ms"] for p in fu]
        spread = max(max(mf) - min(mf), max(mu) - min(mu))
        ok = max(mf) + spread < min(mu)
        ok_all = ok_all and ok

        def fmt(ps):
            return "  ".join(f"{p['median_ms']:.3f} [{p['min_ms']:.3f}..{p['max_ms']:.3f}]" for p in ps)
        print(f"{row:22s} frozen {fmt(fz)}\n{'':22s} full   {fmt(fu)}\n{'':22s} frozen / full (medians of medians) "
              f"{statistics.median(mf) / statistics.median(mu):.3f}; spread between processes {spread:.3f} ms; "
              f"frozen below full by more than the spread: {ok}", flush=True)
        if "peak_bytes" in fz[0]:
            print(f"{'':22s} peak memory of one call beside the inputs: frozen {fz[0]['peak_bytes'] / 2 ** 20:.1f} MiB, "
                  f"full {fu[0]['peak_bytes'] / 2 ** 20:.1f} MiB", flush=True)
    print("every shape:", ok_all)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
