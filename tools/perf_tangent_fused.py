#!/usr/bin/env python3
"""Time of the tangent-linear pass on the fused two-sided solver (pde_adi_tangent_fused, N = 8 .. 32) against the fused
forward and against the any-size tangent it replaces as the default route ("forward mode on the fused solver"),
with HIP events on a warm device:

    forward_fused     the plain forward (functional.adi_diffuse): the fused register kernels
    tangent_fused     y and ydot with du and all four parameter tangents (factor, factor-tangent, adi_tangent_kernel)
    tangent_fused_du  y and ydot with du alone (no source term, no dco ring, no factor-tangent launch)
    tangent_anysize   the same call as tangent_fused with the route switched off: pde_adi_tangent on the any-size kernels,
                      what PDE_TANGENT_FUSED=0 gives (the switch is read once per process; here the cached value is flipped
                      between calls so that both routes alternate inside one process)

    perf_tangent_fused.py [--shapes headline,small28,...] [--rounds R] [--iters I] [--procs P] [--json FILE] [--once]

Shapes: headline = 512 x 64 x 32 x 32, small28 = 64 x 1 x 28 x 28, ten Strang steps each, fp32; nN = 64 x 16 x N x N for every
fused N, ten Strang steps (where the default route is decided per N); stepN = 64 x 16 x N x N, ONE Strang step (the per-step
launches of the layers with a channel operator: records resident, launch count matters).  perf_tangent.py's method: every
round times each route once (I calls between two events, after a warm-up of the same calls), alternating in one process;
the whole is repeated in P fresh processes; medians over all rounds of all processes with [min .. max] and the medians of
each process (their distance is the process-to-process spread), then the two ratios tangent_fused / forward_fused and
tangent_anysize / tangent_fused.  Last, the host time of a plain ``adi_diffuse`` call outside any dual level (3 x 3 x 16 x 16,
500 queued calls), which this route must not touch.  --once runs each route three times and stops."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

FUSED = (8, 12, 16, 20, 24, 28, 32)
SHAPES = {"headline": (512, 64, 32, 32, 10), "small28": (64, 1, 28, 28, 10)}
SHAPES.update({f"n{n}": (64, 16, n, n, 10) for n in FUSED})
SHAPES.update({f"step{n}": (64, 16, n, n, 1) for n in FUSED})
DT = 0.01
ROUTES = ["forward_fused", "tangent_fused", "tangent_fused_du", "tangent_anysize"]


def measure(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import cnn_with_pde_amd as P
    import cnn_with_pde_amd._lib as L
    import cnn_with_pde_amd.functional as F_

    if not torch.cuda.is_available():
        sys.exit("perf_tangent_fused.py measures on the GPU; there is none here")
    assert L.tangent_fused_enabled(), "run without PDE_TANGENT_FUSED=0: the tool switches the route itself"
    out = {"library": P.library_version(), "iters": a.iters, "rounds": a.rounds, "shapes": {}}
    for name in [s for s in a.shapes.split(",") if s]:
        B, C, H, W, steps = SHAPES[name]
        sweeps = tuple(s for st in F_.adi_schedule(DT, 1.0, 1.0, steps) for s in st)
        g = torch.Generator(device="cuda").manual_seed(1)
        u, du = (torch.randn(B, C, H, W, device="cuda", generator=g) for _ in range(2))
        p = [1 + 0.2 * torch.randn(C, H, W, device="cuda", generator=g) for _ in range(2)] + \
            [torch.randn(C, H, W, device="cuda", generator=g) for _ in range(2)]
        dp = [torch.randn(C, H, W, device="cuda", generator=g) for _ in range(4)]
        kw = dict(smooth3=False, clamp_max=10.0, eps=1e-6)

        def call(r):
            if r == "forward_fused":
                return F_.adi_diffuse(u, *p, sweeps, **kw)
            L._tangent_fused = r != "tangent_anysize"
            try:
                if r == "tangent_fused_du":
                    return F_.adi_diffuse_tangent(u, *p, sweeps, du=du, **kw)
                return F_.adi_diffuse_tangent(u, *p, sweeps, du=du, d_alpha_base=dp[0], d_beta_base=dp[1],
                                              d_alpha_time_coeff=dp[2], d_beta_time_coeff=dp[3], **kw)
            finally:
                L._tangent_fused = True

        with torch.no_grad():
            for r in ROUTES:
                for _ in range(3):
                    call(r)
            torch.cuda.synchronize()
            if a.once:
                continue
            times = {r: [] for r in ROUTES}
            for _ in range(a.rounds):
                for r in ROUTES:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        call(r)
                    e1.record()
                    e1.synchronize()
                    times[r].append(e0.elapsed_time(e1) / a.iters)
        out["shapes"][name] = {"shape": [B, C, H, W], "steps": steps, "routes": times}
    if not a.once:
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
    ap.add_argument("--shapes", default="headline,small28")
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
        shape, steps = runs[0]["shapes"][name]["shape"], runs[0]["shapes"][name]["steps"]
        routes = {r: [t for run in runs for t in run["shapes"][name]["routes"][r]] for r in ROUTES}
        med = {r: statistics.median(t) for r, t in routes.items()}
        per = {r: [statistics.median(run["shapes"][name]["routes"][r]) for run in runs] for r in ROUTES}
        out["shapes"][name] = {"shape": shape, "steps": steps,
                               "routes": {r: {"median_ms": med[r], "min_ms": min(t), "max_ms": max(t),
                                              "per_process_median_ms": per[r]} for r, t in routes.items()}}
        for r, t in routes.items():
            print(f"{name:9s} {'x'.join(map(str, shape)):>16s} K={steps:<2d} {r:16s}: median {med[r]:8.4f} ms  "
                  f"[{min(t):8.4f} .. {max(t):8.4f}]  per process {' '.join('%.4f' % v for v in per[r])}", flush=True)
        ratios = {"tangent_fused_over_forward_fused": med["tangent_fused"] / med["forward_fused"],
                  "tangent_fused_du_over_forward_fused": med["tangent_fused_du"] / med["forward_fused"],
                  "tangent_anysize_over_tangent_fused": med["tangent_anysize"] / med["tangent_fused"]}
        out["shapes"][name]["ratios"] = ratios
        for k, v in ratios.items():
            print(f"{name:9s} {k}: {v:.3f}", flush=True)
    host = [t for run in runs for t in run["host_us_per_plain_call"]]
    out["host_us_per_plain_call"] = {"median": statistics.median(host), "min": min(host), "max": max(host),
                                     "per_process_median": [statistics.median(run["host_us_per_plain_call"]) for run in runs]}
    print(f"host time of a plain adi_diffuse call: median {statistics.median(host):.2f} us  [{min(host):.2f} .. {max(host):.2f}]")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
