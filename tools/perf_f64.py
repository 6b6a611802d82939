#!/usr/bin/env python3
"""Forward + backward time of one PDE layer in float64 beside the same layer in float32: the mnist layer at
(64,1,28,28) and the cifar10 layer (channel mixing before every step) at (64,64,32,32), reference defaults otherwise.
Wall time of a loop of calls on a warm device, median of 5 repeats of 10.  usage: perf_f64.py"""
import contextlib
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import cnn_with_pde_amd as P  # noqa: E402


def timed(layer, shape, dtype):
    u = torch.randn(shape, device="cuda", dtype=dtype, requires_grad=True)
    gy = torch.randn_like(u)

    def step():
        for p in layer.parameters():
            p.grad = None
        u.grad = None
        layer(u).backward(gy)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        reps.append((time.perf_counter() - t0) / 10 * 1e3)
    return statistics.median(reps)


cases = [("mnist", lambda: P.MnistDiffusionLayer(28), (64, 1, 28, 28)),
         ("cifar10", lambda: P.EnhancedDiffusionLayer(32, 64), (64, 64, 32, 32))]
for name, make, shape in cases:
    row = {"layer": name, "shape": list(shape)}
    for dtype in (torch.float32, torch.float64):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            layer = make().to(device="cuda", dtype=dtype)
        row[str(dtype).split(".")[1] + "_ms"] = round(timed(layer, shape, dtype), 3)
    row["ratio"] = round(row["float64_ms"] / row["float32_ms"], 2)
    print(json.dumps(row), flush=True)
