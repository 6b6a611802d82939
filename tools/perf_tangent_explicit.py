#!/usr/bin/env python3
"""Time of the tangent-linear pass of the explicit 5-point and the Jacobi layers (functional.explicit5_tangent,
functional.jacobi_diffuse_tangent: pde_explicit5_tangent, pde_jacobi_io_tangent) against the plain forward of the same
shape ("forward mode, the explicit layers"), with HIP events on a warm device:

    forward    layer(u) under no_grad: explicit5_step / jacobi_diffuse
    tangent    y and ydot with du and both parameter tangents, one call

    perf_tangent_explicit.py [--shapes pde48,pde224,tiny64c64,tiny64c3] [--rounds R] [--iters I] [--procs P] [--json FILE]
                             [--root CHECKOUT] [--once]

Shapes: pde48 = PDELayer() 48 x 48 at B = 512 (one workgroup per sample), pde224 = PDELayer(224, 224) at B = 64 (tiled),
tiny64c64 = ImprovedDiffusionLayer(64, 64, num_steps=10) at B = 64, tiny64c3 = ImprovedDiffusionLayer(64, 3, num_steps=10)
at B = 256 (one wave per plane).  The tangent call moves two tensors in and two out where the forward moves one and one,
so about 2 is what the bytes predict where the forward is bandwidth-bound.  Every round times each route once (I calls
between two events, after a warm-up of the same calls), alternating in one process; the whole is repeated in P fresh
processes and the medians over all rounds of all processes are printed with [min .. max], then the ratio of the medians.
Last, the host time of a plain ``explicit5_step`` and of a plain ``jacobi_diffuse`` call outside any dual level (wall clock
per call over a queue of small launches): the check for a dual level sits on that path.  ``--root`` imports the package
from another checkout (one built before the tangent pass existed times the forward and the host path only).  --once runs
each route three times and stops."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

SHAPES = {"pde48": ("pde", (48, 48), 512), "pde224": ("pde", (224, 224), 64), "tiny64c64": ("tiny", (64, 64), 64),
          "tiny64c3": ("tiny", (64, 3), 256)}


def measure(a):
    sys.path.insert(0, a.root or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import contextlib
    import io
    import torch
    import cnn_with_pde_amd as P
    import cnn_with_pde_amd.functional as F_

    if not torch.cuda.is_available():
        sys.exit("perf_tangent_explicit.py measures on the GPU; there is none here")
    has_tangent = hasattr(F_, "explicit5_tangent")
    out = {"library": P.library_version(), "iters": a.iters, "rounds": a.rounds, "shapes": {}}
    for name in [s for s in a.shapes.split(",") if s]:
        kind, args, B = SHAPES[name]
        g = torch.Generator(device="cuda").manual_seed(1)
        with contextlib.redirect_stdout(io.StringIO()):
            ly = (P.PDELayer(*args) if kind == "pde" else P.ImprovedDiffusionLayer(args[0], args[1], num_steps=10)).cuda()
        if kind == "pde":
            H, W = args[1], args[0]
            u, du = (torch.randn(B, H, W, device="cuda", generator=g) for _ in range(2))
            with torch.no_grad():
                p = [ly.alpha(ly.y).contiguous(), ly.beta(ly.x).contiguous()]
            dp = [0.1 * torch.randn_like(t) for t in p]
            fwd = lambda: F_.jacobi_diffuse(u, *p, ly.Nt)
            tan = lambda: F_.jacobi_diffuse_tangent(u, *p, ly.Nt, du=du, d_a_row=dp[0], d_b_col=dp[1])
            shape = [B, H, W]
        else:
            S, C = args
            u, du = (torch.randn(B, C, S, S, device="cuda", generator=g) for _ in range(2))
            p = [ly.alpha_base.detach(), ly.channel_scaling.detach()]
            dp = [torch.randn_like(t) for t in p]
            kw = dict(dt=ly.dt, eps=ly.stability_eps, max_coeff=ly.max_coeff, relax=ly._relax, num_steps=ly.num_steps)
            fwd = lambda: F_.explicit5_step(u, *p, **kw)
            tan = lambda: F_.explicit5_tangent(u, *p, du=du, d_alpha_base=dp[0], d_channel_scaling=dp[1], **kw)
            shape = [B, C, S, S]
        routes = {"forward": fwd}
        if has_tangent:
            routes["tangent"] = tan
        with torch.no_grad():
            for r in routes.values():
                for _ in range(3):
                    r()
            torch.cuda.synchronize()
            if a.once:
                continue
            times = {r: [] for r in routes}
            for _ in range(a.rounds):
                for r, call in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        call()
                    e1.record()
                    e1.synchronize()
                    times[r].append(e0.elapsed_time(e1) / a.iters)
        out["shapes"][name] = {"shape": shape, "routes": times}
    if not a.once:
        # host time of a plain call: a queue of small launches, wall clock per call (the device keeps up: one launch each)
        ue = torch.randn(3, 3, 16, 16, device="cuda")
        pe = [torch.full((3,), 0.05, device="cuda"), torch.ones(3, device="cuda")]
        uj = torch.randn(3, 16, 16, device="cuda")
        pj = [torch.full((16,), 0.1, device="cuda"), torch.full((16,), 0.1, device="cuda")]
        calls = {"explicit5_step": lambda: F_.explicit5_step(ue, *pe, num_steps=2), "jacobi_diffuse": lambda: F_.jacobi_diffuse(uj, *pj, 3)}
        host = {k: [] for k in calls}
        with torch.no_grad():
            for call in calls.values():
                for _ in range(200):
                    call()
            for _ in range(a.rounds):
                for k, call in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(500):
                        call()
                    host[k].append((time.perf_counter() - t0) / 500 * 1e6)
                    torch.cuda.synchronize()
        out["host_us_per_plain_call"] = host
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="pde48,pde224,tiny64c64,tiny64c3")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--root", default=None)
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
                            "--iters", str(a.iters), "--child", path] + (["--root", a.root] if a.root else []),
                           check=True, timeout=900)
            runs.append(json.load(open(path)))
    out = {"library": runs[0]["library"], "root": a.root, "procs": a.procs, "rounds": a.rounds, "iters": a.iters, "shapes": {}}
    for name in runs[0]["shapes"]:
        shape = runs[0]["shapes"][name]["shape"]
        routes = {r: [t for run in runs for t in run["shapes"][name]["routes"][r]] for r in runs[0]["shapes"][name]["routes"]}
        med = {r: statistics.median(t) for r, t in routes.items()}
        out["shapes"][name] = {"shape": shape, "routes": {r: {"median_ms": med[r], "min_ms": min(t), "max_ms": max(t),
                                                             "per_process_median_ms": [statistics.median(
                                                                 run["shapes"][name]["routes"][r]) for run in runs]}
                                                         for r, t in routes.items()}}
        for r, t in routes.items():
            print(f"{name:10s} {'x'.join(map(str, shape)):>16s} {r:8s}: median {med[r]:8.4f} ms  [{min(t):8.4f} .. {max(t):8.4f}]",
                  flush=True)
        if "tangent" in med:
            out["shapes"][name]["tangent_over_forward"] = med["tangent"] / med["forward"]
            print(f"{name:10s} tangent / forward: {med['tangent'] / med['forward']:.3f}", flush=True)
    out["host_us_per_plain_call"] = {}
    for k in runs[0]["host_us_per_plain_call"]:
        host = [t for run in runs for t in run["host_us_per_plain_call"][k]]
        per = [statistics.median(run["host_us_per_plain_call"][k]) for run in runs]
        out["host_us_per_plain_call"][k] = {"median": statistics.median(host), "min": min(host), "max": max(host),
                                            "per_process_median": per}
        print(f"host time of a plain {k} call: median {statistics.median(host):.2f} us  [{min(host):.2f} .. {max(host):.2f}]"
              f"  per process {', '.join('%.2f' % t for t in per)}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
