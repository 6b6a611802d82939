#!/usr/bin/env python3
"""Forward + backward time of the one-launch C <= 4 layers with frozen parameters ("the backward for the input
alone, one-launch layers"), with HIP events on a warm device:

    frozen  every parameter with requires_grad_(False), the input requires grad: pde_adi_small_forward_input +
            pde_adi_small_backward_input (a group: pde_adi_multi_forward + pde_adi_multi_backward_input)
    full    the SAME call in a process started with PDE_BWD_INPUT=0: the full training backward — parked sweep outputs,
            state rebuild, the checkpoint pre-pass where the plan parks states, gradient sums, the parameter-gradient
            epilogue — which is what such a call ran before

    perf_backward_input_small.py [--shapes svhn,enhanced,group,svhn_model,cifar_model] [--batches 64,512] [--rounds R]
                                 [--iters I] [--processes P] [--json FILE]

Each route runs in child processes of its own (the switch is read once per process), P of them one after the other,
routes alternating.  A child times every shape R times (I calls between two events after a warm-up of the same calls)
and reports the median with [min .. max].  Printed per shape: the P medians of either route, and whether every frozen
median lies below every full median by more than the process-to-process spread (max - min of the medians of a route,
the larger of the two routes).  The two model rows time one input-gradient step (forward, loss, gradient with respect to
the image) of a frozen classifier in eval mode."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(P, torch, name, B):
    """(callable that runs one forward + backward, label) for one shape."""
    g = torch.Generator(device="cuda").manual_seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        if name in ("svhn", "enhanced"):
            cls = P.SvhnDiffusionLayer if name == "svhn" else P.EnhancedDiffusionLayer
            m = cls(32, 3, num_steps=10).cuda()
            shape = (B, 3, 32, 32)
        elif name == "group":
            m = P.CIFAR10PDENoConv().cuda().eval().feature_extractor
            shape = (B, 3, 32, 32)
        elif name == "svhn_model":
            m = P.SvhnPDEClassifier().cuda().eval()
            shape = (B, 3, 32, 32)
        elif name == "cifar_model":
            m = P.CIFAR10PDENoConv().cuda().eval()
            shape = (B, 3, 32, 32)
        else:
            raise SystemExit(f"unknown shape {name}")
    for p in m.parameters():
        p.requires_grad_(False)
    x = torch.randn(*shape, device="cuda", generator=g).requires_grad_(True)
    if name.endswith("_model"):
        target = torch.randint(0, 10, (B,), device="cuda", generator=g)

        def call():
            loss = torch.nn.functional.cross_entropy(m(x), target)
            return torch.autograd.grad(loss, x)
    else:
        def run():                                   # (the extractor returns a tuple; `combined` is its first entry)
            y = m(x)
            return y[0] if isinstance(y, (tuple, list)) else y
        gy = torch.randn(*run().shape, device="cuda", generator=g)

        def call():
            return torch.autograd.grad(run(), x, gy)
    return call


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L

    if not torch.cuda.is_available():
        sys.exit("perf_backward_input_small.py measures on the GPU; there is none here")
    out = {"bwd_input": L.bwd_input_enabled(), "rows": {}}
    for name in a.shapes:
        for B in a.batches:
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
            out["rows"][f"{name}-b{B}"] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="svhn,enhanced,group,svhn_model,cifar_model")
    ap.add_argument("--batches", default="64,512")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--processes", type=int, default=3)
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
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shapes", ",".join(a.shapes), "--batches",
                                ",".join(map(str, a.batches)), "--rounds", str(a.rounds), "--iters", str(a.iters)],
                               env=env, capture_output=True, text=True, timeout=600)
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
        print(f"{row:18s} frozen {fmt(fz)}\n{'':18s} full   {fmt(fu)}\n{'':18s} frozen / full (medians of medians) "
              f"{statistics.median(mf) / statistics.median(mu):.3f}; spread between processes {spread:.3f} ms; "
              f"frozen below full by more than the spread: {ok}", flush=True)
    print("every shape:", ok_all)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
