#!/usr/bin/env python3
"""Host time of the implicit-layer autograd nodes, forward + backward per call, through the native nodes
(csrc/host_ext.cpp) and through the ctypes nodes (functional.py; the switch PDE_HOST_EXT=0 sets):

    host_time_nodes.py [--root CHECKOUT] [--calls 200]

One JSON line: {row: microseconds per call}, wall time around ``--calls`` calls on a warm device.  These calls are
launch-bound, so the number is the glue's.  To compare two commits, run this in separate processes, the two checkouts
(``--root``: a built tree of the other commit) alternating, and compare the medians over the processes."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--calls", type=int, default=200)
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch  # noqa: E402

import cnn_with_pde_amd as P  # noqa: E402
from cnn_with_pde_amd import _lib as L  # noqa: E402
from cnn_with_pde_amd import functional as F_  # noqa: E402


def _layer_step(layer, shape):
    x = torch.randn(*shape, device="cuda", requires_grad=True)
    gy = torch.randn_like(x)

    def step():
        layer(x).backward(gy)
    return step


def rows():
    with contextlib.redirect_stdout(io.StringIO()):
        mnist = P.MnistDiffusionLayer().cuda()
        cifar = P.EnhancedDiffusionLayer(32, 3, num_steps=8).cuda()
        trio = [P.EnhancedDiffusionLayer(32, 3, dt=0.001, num_steps=5, dx=1.0, dy=1.0).cuda(),
                P.EnhancedDiffusionLayer(32, 3, dt=0.002, num_steps=8, dx=2.0, dy=2.0).cuda(),
                P.EnhancedDiffusionLayer(32, 3, dt=0.005, num_steps=4, dx=1.5, dy=1.5).cuda()]
        wide = P.EnhancedDiffusionLayer(32, 32, num_steps=3).cuda()
    yield "mnist (64,1,28,28)", _layer_step(mnist, (64, 1, 28, 28))
    yield "cifar10 C=3 8 steps (128,3,32,32)", _layer_step(cifar, (128, 3, 32, 32))
    x = torch.randn(128, 3, 32, 32, device="cuda", requires_grad=True)
    gy = torch.randn_like(x)
    w = torch.softmax(torch.zeros(3, device="cuda"), 0).requires_grad_(True)

    def group():
        out, _ = P.diffuse_shared_input(trio, x, w)
        out.backward(gy)
    yield "three layers on one input (128,3,32,32)", group
    xw = torch.randn(4, 32, 32, 32, device="cuda", requires_grad=True)
    gw = torch.randn_like(xw)
    co = (wide.alpha_base, wide.beta_base, wide.alpha_time_coeff, wide.beta_time_coeff)

    def mixed():
        F_.adi_diffuse_mixed(xw, *co, wide.channel_mixing, wide._schedule(), "pre", clamp_max=10.0).backward(gw)
    yield "adi_diffuse_mixed C=32 (4,32,32,32)", mixed


def measure(step, calls):
    for _ in range(20):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


ext = L.host_ext()
assert ext is not None
res = {}
for name, step in rows():
    for path in ("native", "ctypes"):
        L._host = ext if path == "native" else False
        try:
            res[f"{name} | {path}"] = round(measure(step, args.calls), 2)
        finally:
            L._host = ext
print(json.dumps(res))
