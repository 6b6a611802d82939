"""Event-timed on a warm device: the Ruthotto-Haber symmetric layer under fp16 (or, with --bf16, bf16) autocast, three ways
at B = 64 and 128, D = 3072 (3 x 32 x 32) — the fused 16-bit-operand path (pde_rh.hip, fp16 / bf16 MFMAs), plain-torch
autocast (fused = False) and the fused fp32 path without autocast:
  layer  one SymmetricLayer forward + backward;
  rh     the RH part of a HybridPDEExtractor step: ParabolicBlock (4 steps) + HamiltonianBlock (3 steps), forward + backward.
Usage: python tools/perf_rh_amp.py [iters] [--bf16] [--json out.json]"""
import contextlib
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import cnn_with_pde_amd as P  # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 50
AMP, TAG = (torch.bfloat16, "bf16") if "--bf16" in sys.argv else (torch.float16, "f16")
WAYS = [("fused_" + TAG, True, True), ("torch_amp", False, True), ("fused_f32", True, False)]


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def make(what):
    torch.manual_seed(0)
    if what == "layer":
        mods = [quiet(P.SymmetricLayer, 3, 32).cuda().train()]
    else:
        mods = [quiet(P.models.ParabolicBlock, 3, 32, num_steps=4, dt=0.5).cuda().train(),
                quiet(P.models.HamiltonianBlock, 3, 32, num_steps=3, dt=0.8).cuda().train()]
    return mods


def set_fused(mods, fused):
    for m in mods:
        for s in m.modules():
            if isinstance(s, P.SymmetricLayer):
                s.fused = fused


def step_fn(mods, x, gy, amp):
    params = [p for m in mods for p in m.parameters()]

    def step():
        for p in params:
            p.grad = None
        with torch.autocast("cuda", dtype=AMP, enabled=amp):
            outs = [m(x) for m in mods]
        torch.autograd.backward(outs, [gy.to(o.dtype) for o in outs])
    return step


def time_ms(step, iters):
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best = []
    for _ in range(5):                                    # five windows of `iters` steps: the median window
        ev[0].record()
        for _ in range(iters):
            step()
        ev[1].record()
        torch.cuda.synchronize()
        best.append(ev[0].elapsed_time(ev[1]) / iters)
    best.sort()
    return best[len(best) // 2], best[0], best[-1]


def main():
    assert torch.cuda.is_available(), "perf_rh_amp.py needs a GPU"
    rows = []
    # device preconditioning: a few seconds of the heaviest leg so that the first timed leg does not start on an idle chip
    mods = make("rh")
    x = torch.randn(128, 3, 32, 32, device="cuda", requires_grad=True)
    pre = step_fn(mods, x, torch.randn_like(x), True)
    for _ in range(200):
        pre()
    torch.cuda.synchronize()
    for B in (64, 128):
        for what in ("layer", "rh"):
            mods = make(what)
            g = torch.Generator().manual_seed(B)
            x = torch.randn(B, 3, 32, 32, generator=g).cuda().requires_grad_(True)
            gy = torch.randn(B, 3, 32, 32, generator=g).cuda()
            res = {}
            for rep in range(2):                          # the three ways alternated, twice: the second pass is reported
                for name, fused, amp in WAYS:
                    set_fused(mods, fused)
                    res[name] = time_ms(step_fn(mods, x, gy, amp), ITERS)
            row = {"B": B, "what": what, **{k: round(v[0], 4) for k, v in res.items()},
                   "spread": {k: [round(v[1], 4), round(v[2], 4)] for k, v in res.items()}}
            row[TAG + "_vs_torch_amp"] = round(res["torch_amp"][0] / res["fused_" + TAG][0], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
