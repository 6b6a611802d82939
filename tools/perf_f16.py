#!/usr/bin/env python3
"""Forward and backward time of one PDE layer on fp16 tensors (``layer.half()``, the float16 route) beside bf16 tensors (an
fp32 layer fed bf16: the bf16 I/O route) and fp32, at three shapes:
  headline  cifar10.EnhancedDiffusionLayer(32, 64, num_steps=10), channel mixing off, (512, 64, 32, 32)  (bench.py's workload)
  svhn      SVHN.DiffusionLayer(32, 128, num_steps=20), coupling after every step, (512, 128, 32, 32)
  mnist     mnist_test.DiffusionLayer(28), (64, 1, 28, 28)
Wall time of a loop of calls on a warm device, median of 5 repeats of 10; backward = (forward + backward) - forward.
usage: perf_f16.py"""
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


def median_ms(fn, reps=5, inner=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / inner * 1e3)
    return statistics.median(out)


def timed(layer, shape, dtype):
    u = torch.randn(shape, device="cuda", dtype=dtype, requires_grad=True)
    gy = torch.randn_like(u)

    def fwd():
        layer(u)

    def both():
        for p in layer.parameters():
            p.grad = None
        u.grad = None
        layer(u).backward(gy)
    f = median_ms(fwd)
    fb = median_ms(both)
    return f, fb - f


def svhn():
    L = P.SvhnDiffusionLayer(32, 128, num_steps=20)
    with torch.no_grad():
        L.channel_coupling.copy_(torch.eye(128) + 0.01 * torch.randn(128, 128))
    return L


cases = [("headline", lambda: P.EnhancedDiffusionLayer(32, 64, num_steps=10, channel_mixing_enabled=False),
          (512, 64, 32, 32)),
         ("svhn", svhn, (512, 128, 32, 32)),
         ("mnist", lambda: P.MnistDiffusionLayer(28), (64, 1, 28, 28))]
for name, make, shape in cases:
    row = {"layer": name, "shape": list(shape)}
    for tag, io_dtype, param_dtype in (("fp32", torch.float32, torch.float32), ("bf16", torch.bfloat16, torch.float32),
                                       ("fp16", torch.float16, torch.float16)):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            layer = make().to(device="cuda", dtype=param_dtype)
        f, b = timed(layer, shape, io_dtype)
        row[tag + "_fwd_ms"], row[tag + "_bwd_ms"] = round(f, 3), round(b, 3)
    for k in ("fwd", "bwd"):
        row["fp16/bf16_" + k] = round(row["fp16_" + k + "_ms"] / row["bf16_" + k + "_ms"], 3)
    print(json.dumps(row), flush=True)
