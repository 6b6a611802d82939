#!/usr/bin/env python3
"""Diagnostic: launch times (HIP events inside the library) of the headline forward + backward under a list of
PDE_FWD_STAGGER values (0 = off, 1 = default, <n> = n naps of 512 cycles for the second workgroup of a CU, t<n>/<p> =
turns in priority passing after p percent of the time steps, with n naps), one child process per
value and round, the values alternating round by round.  Also a two-step schedule (6 sweeps) of the same tensors.
usage: perf_fwd_stagger.py [rounds] [value ...]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child():
    import torch
    import cnn_with_pde_amd.functional as F
    B, C, N = 512, 64, 32
    g = torch.Generator().manual_seed(3)
    ab = (2.0 * (1 + 0.1 * torch.randn(C, N, N, generator=g))).cuda().requires_grad_(True)
    bb = (1.8 * (1 + 0.1 * torch.randn(C, N, N, generator=g))).cuda().requires_grad_(True)
    asl = (0.1 * torch.randn(C, N, N, generator=g)).cuda().requires_grad_(True)
    bsl = (0.1 * torch.randn(C, N, N, generator=g)).cuda().requires_grad_(True)
    u = torch.randn(B, C, N, N, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(B, C, N, N, generator=g).cuda()
    F.timing_enable(True)
    out = []
    for steps in (10, 2):
        sweeps = [s for st in F.adi_schedule(0.001, 1.0, 1.0, steps, "strang") for s in st]

        def run(n):
            for _ in range(n):
                for t in (ab, bb, asl, bsl, u):
                    t.grad = None
                F.adi_diffuse(u, ab, bb, asl, bsl, sweeps, checkpoints=0).backward(gy)
            torch.cuda.synchronize()
        run(5)
        f0, nf0, b0, nb0 = F.timing_read()
        run(20)
        f1, nf1, b1, nb1 = F.timing_read()
        out.append(f"{steps:2d} steps: fwd {(f1 - f0) / (nf1 - nf0) * 1e3:6.1f} us  bwd {(b1 - b0) / (nb1 - nb0) * 1e3:6.1f} us")
    print("   ".join(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
        sys.exit(0)
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    values = sys.argv[2:] or ["0", "1", "24", "t/30", "t24/30", "t24/50"]
    for r in range(rounds):
        for v in values:
            env = dict(os.environ, PDE_FWD_STAGGER=v)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                print(f"stagger {v}: FAILED ({p.returncode}) {p.stderr[-300:]}", flush=True)
                sys.exit(1)                  # nothing more is started on the device after a failure
            print(f"round {r} stagger {v:>3s}: {p.stdout.strip().splitlines()[-1]}", flush=True)
