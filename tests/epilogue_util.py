"""Ground for the tests of the epilogue kernels (pde_blend.hip, blend64_* in pde_f64.hip, pde_gate.hip, pde_tail.hip):
fp64 references written from the formulas in the kernels' header comments, and the generators of the inputs the tests
use.  tests/test_epilogue_cases.py checks this module on the CPU; tests/test_gpu_epilogues.py runs the kernels against it.

Exact cases are made of small integers and of weights that are powers of two (or their negatives), so that every value a
correct kernel can form — in any order of summation — is representable in fp32 and every tensor it writes is representable
in the case's I/O type: such a case is compared with ``torch.equal``.  Where a wrapper hands a gradient back in fp16 (the
float16 route needs its parameters in fp16, and autograd returns a gradient in its parameter's type) the exact fp32 value
is rounded once, and so is the expected one."""
import functools
import math

import torch
import torch.nn as nn

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}


# --------------------------------------------------------------------------------------------------- 16-bit distances
def ord16(t):
    """Bit patterns of a bf16 or fp16 tensor as integers in value order (+0 and -0 coincide); both are sign-magnitude."""
    assert t.dtype in (torch.float16, torch.bfloat16)
    i = t.detach().cpu().contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulps16(a, b):
    """Largest distance, in units in the last place of their common 16-bit type, between two tensors."""
    assert a.dtype == b.dtype
    return int((ord16(a) - ord16(b)).abs().max())


# --------------------------------------------------------------------------------------------------- skip blend
def blend_ref(u0, u, w, g):
    """out = s u0 + (1-s) u, s = sigmoid(w);  g_u0 = s g, g_u = (1-s) g, g_w = s (1-s) sum g (u0 - u).  Everything fp64;
    ``w`` is the weight as stored (a Python float or a 0-d tensor of any type)."""
    u0, u, g = u0.double(), u.double(), g.double()
    w = float(w)
    s = 1.0 / (1.0 + math.exp(-w))
    t = 1.0 / (1.0 + math.exp(w))                       # 1 - s without the cancellation
    return {"out": s * u0 + t * u, "g_u0": s * g, "g_u": t * g, "g_w": s * t * float((g * (u0 - u)).sum())}


#: sizes of the exact cases: below one vector of 8, around one workgroup's 2048 elements, the grid cap of 2048 workgroups
#: (one trip), some workgroups on a second trip with a ragged last vector, every workgroup on two trips and one on a third
BLEND_SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 4194304, 4194304 + 2048 + 5, 2 * 4194304 + 3)
#: blend64: 256 elements per workgroup, 512 workgroups in the backward
BLEND64_SIZES = (1, 255, 256, 257, 131072, 131073, 3 * 131072 + 77)
BLEND_SMALL_RANGE_FROM = 1 << 20


@functools.lru_cache(maxsize=None)
def blend_exact_case(n):
    """Integer inputs (int64, on the CPU) of the exact blend case of size ``n`` at skip_weight = 0, s = 1/2, and what it
    must give: out = (u0 + u)/2, g_u0 = g_u = g/2 (fp64, multiples of 1/2 up to 32) and the integer sum g (u0 - u).
    u0, u, g in [-32, 32]; from 2^20 elements on g and u0 - u stay in [-3, 3]."""
    gen = torch.Generator().manual_seed(7000 + n % 9973)
    if n >= BLEND_SMALL_RANGE_FROM:
        u0 = torch.randint(-29, 30, (n,), generator=gen)
        u = u0 - torch.randint(-3, 4, (n,), generator=gen)
        g = torch.randint(-3, 4, (n,), generator=gen)
    else:
        u0 = torch.randint(-32, 33, (n,), generator=gen)
        u = torch.randint(-32, 33, (n,), generator=gen)
        g = torch.randint(-32, 33, (n,), generator=gen)
    total = int((g * (u0 - u)).sum())
    return {"u0": u0, "u": u, "g": g, "out": 0.5 * (u0 + u).double(), "g_u0": 0.5 * g.double(), "g_u": 0.5 * g.double(),
            "sum": total, "g_w": 0.25 * total}


@functools.lru_cache(maxsize=None)
def blend_general_case(n, noise=None):
    """fp32 inputs of a general blend case: standard normal, or with ``noise`` u = u0 + noise * normal (the cancelling sum
    the double-precision reduction was written for)."""
    gen = torch.Generator().manual_seed(11 + n)
    u0 = torch.randn(n, generator=gen)
    u = torch.randn(n, generator=gen) if noise is None else u0 + noise * torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    return u0, u, g


# --------------------------------------------------------------------------------------------------- gate and combination
def gate_ref(ys, gates, w, g):
    """combined = sum_i w_i gate_i[b,c] y_i;  gy_i = w_i gate_i g,  dot_i[b,c] = sum_p g y_i,  dL/dgate_i = w_i dot_i,
    dL/dw_i = sum_bc gate_i dot_i.  Everything fp64; ys (B,C,H,W), gates (B,C), w (L)."""
    ys, gates = [y.double() for y in ys], [t.double().reshape(t.shape[0], t.shape[1]) for t in gates]
    w, g = w.double(), g.double()
    out = torch.zeros_like(ys[0])
    res = {"gy": [], "ggate": [], "gw": []}
    for i, (y, gt) in enumerate(zip(ys, gates)):
        f = (w[i] * gt)[:, :, None, None]
        out = out + f * y
        dot = (g * y).sum(dim=(2, 3))
        res["gy"].append(f * g)
        res["ggate"].append(w[i] * dot)
        res["gw"].append((gt * dot).sum())
    res["out"], res["gw"] = out, torch.stack(res["gw"])
    return res


GATE_WEIGHTS = (0.5, 1.0, 2.0, -1.0)
#: plane shapes: one lane, four lanes, 252 (the last lane idle), 256 (one full trip), 260 (one lane on a second trip),
#: 784 (the fourth trip has 4 lanes), 1024, 4096
GATE_PLANES = ((2, 2), (4, 4), (7, 36), (16, 16), (10, 26), (28, 28), (32, 32), (64, 64))
GATE_BC = ((1, 1), (1, 3), (2, 2), (5, 1), (1, 67))         # B*C = 1, 3, 4 (one workgroup), 5, 67


def gate_exact_cases():
    """A covering set of (L, (H, W), (B, C), gate4d): every L, plane shape and plane count at least once, L = 4 with
    HW = 4, 260 and 4096, both layouts of the gates.  Each is run in every I/O type."""
    return [(1, (2, 2), (1, 1), False), (4, (2, 2), (1, 3), True), (2, (4, 4), (2, 2), False), (3, (7, 36), (5, 1), True),
            (2, (16, 16), (1, 67), False), (4, (10, 26), (5, 1), False), (1, (28, 28), (2, 2), True),
            (3, (32, 32), (1, 3), False), (4, (64, 64), (1, 1), True), (3, (64, 64), (1, 67), False),
            (4, (10, 26), (1, 67), True), (1, (16, 16), (5, 1), False), (2, (28, 28), (1, 1), True)]


def gate_case_id(v):
    """pytest id of one value of a gate case: L, HxW, BxC, the gates' layout"""
    if isinstance(v, bool):
        return "gate4d" if v else "gate2d"
    return f"L{v}" if isinstance(v, int) else f"{v[0]}x{v[1]}"


@functools.lru_cache(maxsize=None)
def gate_exact_case(L, hw, bc):
    """Integer inputs (int64) of an exact gate case: y_i and g in [-3, 3], gates in [-2, 2], weights the first L of
    GATE_WEIGHTS; and the fp64 results."""
    (H, W), (B, C) = hw, bc
    gen = torch.Generator().manual_seed(100000 * L + 1000 * H + 10 * W + 7 * B + C)
    ys = [torch.randint(-3, 4, (B, C, H, W), generator=gen) for _ in range(L)]
    gates = [torch.randint(-2, 3, (B, C), generator=gen) for _ in range(L)]
    g = torch.randint(-3, 4, (B, C, H, W), generator=gen)
    w = torch.tensor(GATE_WEIGHTS[:L], dtype=torch.float64)
    return {"ys": ys, "gates": gates, "g": g, "w": w, "ref": gate_ref(ys, gates, w, g)}


@functools.lru_cache(maxsize=None)
def gate_general_case(L=4, shape=(5, 3, 28, 28)):
    gen = torch.Generator().manual_seed(3)
    ys = [torch.randn(*shape, generator=gen) for _ in range(L)]
    gates = [torch.rand(shape[0], shape[1], generator=gen) for _ in range(L)]
    w = torch.softmax(torch.randn(L, generator=gen), 0)
    g = torch.randn(*shape, generator=gen)
    return ys, gates, w, g


# --------------------------------------------------------------------------------------------------- BatchNorm + pooling
TAIL_WEIGHTS = (1.25, -0.75, 0.0, 2.0, 0.5)                 # per channel, in this order: C >= 3 has the negative and the zero
TAIL_BIASES = (0.25, -0.5, 0.75, 0.0, -1.0)
TAIL_SHAPES = ((2, 1, 4), (65, 2, 8), (3, 5, 12), (130, 3, 20), (7, 3, 64), (1, 3, 32))
#: name -> (shape, what differs from the plain case)
TAIL_VARIANTS = {"shift100": (3, 3, 8), "no_affine": (3, 3, 8), "no_running_stats": (3, 3, 8), "constant_plane": (3, 3, 8)}


class TailCase:
    """Inputs of one BatchNorm2d + pooling case: x = k/64 (|k| <= 256, so pooling windows hold exact ties and no two
    different values are closer than 2^-6), gout multiples of 1/4 without zeros (a wrong arg-max moves a whole entry),
    the module's weight, bias and running statistics."""

    def __init__(self, B, C, N, variant=None):
        gen = torch.Generator().manual_seed(1000 * B + 10 * N + C)
        self.B, self.C, self.N, self.variant = B, C, N, variant
        self.x = torch.randint(-256, 257, (B, C, N, N), generator=gen).double() / 64
        if variant == "shift100":
            self.x = self.x + 100.0
        if variant == "constant_plane":
            self.x[B // 2, 0] = 1.5
        k = torch.randint(1, 9, (B, 2 * C, 4, 4), generator=gen) * (2 * torch.randint(0, 2, (B, 2 * C, 4, 4), generator=gen) - 1)
        self.gout = k.double() / 4
        self.affine = variant != "no_affine"
        self.track = variant != "no_running_stats"
        self.weight = torch.tensor([TAIL_WEIGHTS[c % 5] for c in range(C)], dtype=torch.float64)
        if C == 1:
            self.weight[0] = -0.75                          # the single-channel shape takes the arg-min side
        self.bias = torch.tensor([TAIL_BIASES[c % 5] for c in range(C)], dtype=torch.float64)
        centre = 100.0 if variant == "shift100" else 0.0
        self.running_mean = centre + torch.randint(-8, 9, (C,), generator=gen).double() / 16
        self.running_var = 4 + torch.randint(0, 9, (C,), generator=gen).double() / 4

    def module(self, dtype, device, training):
        bn = nn.BatchNorm2d(self.C, affine=self.affine, track_running_stats=self.track).to(dtype=dtype, device=device)
        with torch.no_grad():
            if self.affine:
                bn.weight.copy_(self.weight)
                bn.bias.copy_(self.bias)
            if self.track:
                bn.running_mean.copy_(self.running_mean)
                bn.running_var.copy_(self.running_var)
        return bn.train(training)


@functools.lru_cache(maxsize=None)
def tail_case(B, C, N, variant=None):
    return TailCase(B, C, N, variant)


def tail_collect(bn, x, out, gout):
    """Backward through ``out`` and everything the comparison needs, as fp64 CPU tensors (None where the module has none)."""
    out.backward(gout)
    cpu = lambda t: None if t is None else t.detach().double().cpu()
    return {"out": cpu(out), "dx": cpu(x.grad),
            "dweight": cpu(bn.weight.grad) if bn.weight is not None else None,
            "dbias": cpu(bn.bias.grad) if bn.bias is not None else None,
            "running_mean": cpu(bn.running_mean), "running_var": cpu(bn.running_var),
            "num_batches_tracked": None if bn.num_batches_tracked is None else int(bn.num_batches_tracked)}


def tail_torch(case, training, dtype=torch.float64, device="cpu"):
    """torch's own BatchNorm2d and adaptive pools on the case: in fp64 on the CPU this is the reference (its max pool takes
    the first maximum in row-major order on exact ties, the rule of the kernel — test_epilogue_cases.py), in fp32 on the
    GPU the plain implementation whose error the fused kernels are allowed twice of."""
    bn = case.module(dtype, device, training)
    x = case.x.clone().to(dtype=dtype, device=device).requires_grad_(True)      # never the cached tensor itself
    f = bn(x)
    out = torch.cat([nn.functional.adaptive_avg_pool2d(f, 4), nn.functional.adaptive_max_pool2d(f, 4)], dim=1)
    return tail_collect(bn, x, out, case.gout.to(dtype=dtype, device=device))


@functools.lru_cache(maxsize=None)
def tail_reference(B, C, N, variant, training):
    return tail_torch(tail_case(B, C, N, variant), training)

