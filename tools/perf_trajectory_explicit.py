#!/usr/bin/env python3
"""Forward + backward time of ``layer_trajectory(layer, u)`` for the two explicit layers ("the trajectory of the
explicit layers"), with HIP events on a warm device, in ONE process, against the only equivalent route there was before
the kernels emitted states:

    PDELayer                 trajectory: functional.jacobi_diffuse_states, the launches of ONE call of Nt steps
                             plain_calls: K plain calls with Nt = 1 .. K (the plane is padded once and the ring keeps the
                             input's values, so chained one-step calls compute another function): K (K + 1) / 2 time steps
    ImprovedDiffusionLayer   trajectory: functional.explicit5_states, one launch per pass at 64x64
                             chained: K one-step calls, each feeding the next

at PDELayer 48x48 with Nt = 10 (batches 64 and 512) and 224x224 (batch 64), ImprovedDiffusionLayer(64, 3, num_steps=10)
at batch 256, fp32, a cotangent on every state; and the plain ``forward`` + backward of both layers (the figure that must
not move from one commit to the next).

    perf_trajectory_explicit.py [--cases pde48,pde224,tiny64] [--rounds R] [--iters I] [--json FILE]

Every round times each route once (I calls between two events, after a warm-up of the same calls), the routes
alternating, so drift of the device hits them alike; printed per case: median, minimum and maximum over the rounds in ms
per forward + backward, and the ratio of the medians (old route / trajectory).  Before timing, the routes are compared on
the same input (states and input gradient; the largest relative difference is printed)."""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="pde48,pde224,tiny64")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import cnn_with_pde_amd as P

    if not torch.cuda.is_available():
        sys.exit("perf_trajectory_explicit.py measures on the GPU; there is none here")
    K = 10
    shapes = {"pde48": [(64, 48), (512, 48)], "pde224": [(64, 224)], "tiny64": [(256, 64)]}
    out = {"steps": K, "iters": a.iters, "rounds": a.rounds, "library": P.library_version(), "cases": []}
    for case in [c for c in a.cases.split(",") if c]:
        for B, N in shapes[case]:
            g = torch.Generator(device="cuda").manual_seed(1)
            if case == "tiny64":
                layer = P.ImprovedDiffusionLayer(N, 3, num_steps=K).cuda()
                one = P.ImprovedDiffusionLayer(N, 3, num_steps=1).cuda()
                shape = (B, 3, N, N)
            else:
                layer = P.PDELayer(Nx=N, Ny=N, Lx=2.0, Ly=2.0, T=K * 0.001).cuda()
                assert layer.Nt == K
                with torch.no_grad():                       # stable coefficients at every size here
                    for n, v in dict(alpha_w1=0.04, alpha_w2=0.01, alpha_w3=0.02, beta_w1=0.05, beta_w2=-0.01,
                                     beta_w3=0.01).items():
                        getattr(layer, n).fill_(v * (48.0 / N) ** 2)
                shape = (B, 1, N, N)
            u = torch.randn(shape, device="cuda", generator=g).requires_grad_(True)
            gy = torch.randn((K,) + shape, device="cuda", generator=g)

            def trajectory():
                u.grad = None
                y = P.layer_trajectory(layer, u)
                y.backward(gy)
                return y.detach(), u.grad

            def old_route():
                u.grad = None
                if case == "tiny64":                        # chained one-step calls
                    ys, x = [], u
                    for _ in range(K):
                        x = one(x)
                        ys.append(x)
                else:                                       # K plain calls, Nt = 1 .. K
                    ys = [P.jacobi_diffuse(u.squeeze(1), layer.alpha(layer.y), layer.beta(layer.x), k).unsqueeze(1)
                          for k in range(1, K + 1)]
                torch.autograd.backward(ys, list(gy))
                return torch.stack([y.detach() for y in ys]), u.grad

            def forward():
                u.grad = None
                y = layer(u)
                y.backward(gy[-1])
                return y.detach(), u.grad

            yt, gt = trajectory()
            yo, go = old_route()
            diff = max(float((yt - yo).abs().max() / yo.abs().max()), float((gt - go).abs().max() / go.abs().max()))
            routes = {"trajectory": trajectory, "old_route": old_route, "forward": forward}
            for fn in routes.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {m: [] for m in routes}
            for _ in range(a.rounds):
                for m, fn in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[m].append(e0.elapsed_time(e1) / a.iters)
            med = {m: statistics.median(t) for m, t in times.items()}
            ratio = med["old_route"] / med["trajectory"]
            tag = f"{case:7s} {'x'.join(str(s) for s in shape)} {K} steps"
            out["cases"].append({"case": case, "shape": list(shape), "max_rel_diff": diff, "ratio": ratio,
                                 "routes": {m: {"median_ms": med[m], "min_ms": min(t), "max_ms": max(t), "all_ms": t}
                                            for m, t in times.items()}})
            for m, t in times.items():
                print(f"{tag} {m:10s}: median {med[m]:8.3f} ms  [{min(t):8.3f} .. {max(t):8.3f}] fwd+bwd", flush=True)
            print(f"{tag} old_route / trajectory = {ratio:.2f}x   (routes differ by {diff:.1e})", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
