#!/usr/bin/env python3
"""Time of the tangent-linear pass (functional.adi_diffuse_tangent, pde_adi*_tangent) against the forward of the same shape
("forward mode"), with HIP events on a warm device:

    forward_anysize   the any-size forward (gen_fwd_kernel) of the shape: what the tangent kernel's primal half repeats
    tangent           y and ydot with du and all four parameter tangents (factor, factor-tangent, tangent kernel)
    tangent_du        y and ydot with du alone (no source term, no factor-tangent launch)
    forward_fused     at fused line lengths (N <= 32): the plain forward, which runs the two-lane register kernels

At the fused line lengths ``tangent`` and ``tangent_du`` take the default route, which is pde_adi_tangent_fused there; run with
PDE_TANGENT_FUSED=0 for the any-size tangent kernels this tool was written for (perf_tangent_fused.py times both routes).

    perf_tangent.py [--shapes any36,headline] [--rounds R] [--iters I] [--procs P] [--json FILE] [--once]

Shapes: any36 = 64 x 16 x 36 x 36, headline = 512 x 64 x 32 x 32, ten Strang steps each, fp32.  At N = 32 the any-size
forward is reached through the rectangle entry points, which take squares too and have no fused kernels.  From the code one
expects tangent / forward_anysize between 2 and 3: two solves and the source term per line, and twice the LDS per
workgroup.  Every round times each route once (I calls between two events, after a warm-up of the same calls),
alternating in one process, so drift of the device hits them alike; the whole is repeated in P fresh processes and the
medians over all rounds of all processes are printed with [min .. max], then the ratios of the medians.  Last, the host
time of a plain ``adi_diffuse`` call outside any dual level (wall clock per call over a queue of small launches): the check
for a dual level sits on that path.  --once runs each route three times and stops."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

SHAPES = {"any36": (64, 16, 36, 36), "headline": (512, 64, 32, 32)}
STEPS, DT = 10, 0.01


def measure(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import cnn_with_pde_amd as P
    import cnn_with_pde_amd.functional as F_

    if not torch.cuda.is_available():
        sys.exit("perf_tangent.py measures on the GPU; there is none here")
    out = {"library": P.library_version(), "iters": a.iters, "rounds": a.rounds, "shapes": {}}
    sweeps = tuple(s for st in F_.adi_schedule(DT, 1.0, 1.0, STEPS) for s in st)
    for name in [s for s in a.shapes.split(",") if s]:
        B, C, H, W = SHAPES[name]
        g = torch.Generator(device="cuda").manual_seed(1)
        u, du = (torch.randn(B, C, H, W, device="cuda", generator=g) for _ in range(2))
        p = [1 + 0.2 * torch.randn(C, H, W, device="cuda", generator=g) for _ in range(2)] + \
            [torch.randn(C, H, W, device="cuda", generator=g) for _ in range(2)]
        dp = [torch.randn(C, H, W, device="cuda", generator=g) for _ in range(4)]
        kw = dict(smooth3=False, clamp_max=10.0, eps=1e-6)
        fused = H == W and H % 4 == 0 and 8 <= H <= 32

        def call(r):
            if r == "forward_anysize":
                if fused:                                         # the rectangle family: any-size kernels at every plane
                    return F_._AdiFn.apply(u, *p, sweeps, False, 10.0, 1e-6, 0, None, None, True, False)
                return F_.adi_diffuse(u, *p, sweeps, **kw)
            if r == "forward_fused":
                return F_.adi_diffuse(u, *p, sweeps, **kw)
            if r == "tangent":
                return F_.adi_diffuse_tangent(u, *p, sweeps, du=du, d_alpha_base=dp[0], d_beta_base=dp[1],
                                              d_alpha_time_coeff=dp[2], d_beta_time_coeff=dp[3], **kw)
            return F_.adi_diffuse_tangent(u, *p, sweeps, du=du, **kw)

        routes = ["forward_anysize", "tangent", "tangent_du"] + (["forward_fused"] if fused else [])
        with torch.no_grad():
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
        out["shapes"][name] = {"shape": [B, C, H, W], "routes": times}
    if not a.once:
        # host time of a plain call: a queue of small launches, wall clock per call (the device keeps up: 2 launches each)
        u = torch.randn(3, 3, 16, 16, device="cuda")
        p = [torch.ones(3, 16, 16, device="cuda") for _ in range(2)] + [torch.zeros(3, 16, 16, device="cuda") for _ in range(2)]
        sw = tuple(s for st in F_.adi_schedule(DT, 1.0, 1.0, 2) for s in st)
        host = []
        with torch.no_grad():
            for _ in range(200):
                F_.adi_diffuse(u, *p, sw)
            for _ in range(a.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(500):
                    F_.adi_diffuse(u, *p, sw)
                host.append((time.perf_counter() - t0) / 500 * 1e6)
                torch.cuda.synchronize()
        out["host_us_per_plain_call"] = host
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="any36,headline")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child or a.once:
        res = measure(a)
        if a.child:
            with open(a.child, "w") as f:
                json.dump(res, f)
        return
    runs = []
    for i in range(a.procs):                                      # fresh processes, one after the other
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "r.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--shapes", a.shapes, "--rounds", str(a.rounds),
                            "--iters", str(a.iters), "--child", path], check=True, timeout=900)
            runs.append(json.load(open(path)))
    out = {"library": runs[0]["library"], "procs": a.procs, "rounds": a.rounds, "iters": a.iters, "shapes": {}}
    for name in runs[0]["shapes"]:
        shape = runs[0]["shapes"][name]["shape"]
        routes = {r: [t for run in runs for t in run["shapes"][name]["routes"][r]] for r in runs[0]["shapes"][name]["routes"]}
        med = {r: statistics.median(t) for r, t in routes.items()}
        out["shapes"][name] = {"shape": shape, "routes": {r: {"median_ms": med[r], "min_ms": min(t), "max_ms": max(t),
                                                             "per_process_median_ms": [statistics.median(
                                                                 run["shapes"][name]["routes"][r]) for run in runs]}
                                                         for r, t in routes.items()}}
        for r, t in routes.items():
            print(f"{name:9s} {'x'.join(map(str, shape)):>16s} {r:16s}: median {med[r]:8.3f} ms  [{min(t):8.3f} .. {max(t):8.3f}]",
                  flush=True)
        ratios = {"tangent_over_forward_anysize": med["tangent"] / med["forward_anysize"],
                  "tangent_du_over_forward_anysize": med["tangent_du"] / med["forward_anysize"]}
        if "forward_fused" in med:
            ratios["tangent_over_forward_fused"] = med["tangent"] / med["forward_fused"]
            ratios["forward_anysize_over_forward_fused"] = med["forward_anysize"] / med["forward_fused"]
        out["shapes"][name]["ratios"] = ratios
        for k, v in ratios.items():
            print(f"{name:9s} {k}: {v:.3f}", flush=True)
    host = [t for run in runs for t in run["host_us_per_plain_call"]]
    out["host_us_per_plain_call"] = {"median": statistics.median(host), "min": min(host), "max": max(host)}
    print(f"host time of a plain adi_diffuse call: median {statistics.median(host):.2f} us  [{min(host):.2f} .. {max(host):.2f}]")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
