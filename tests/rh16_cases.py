"""Ground for the tests of the 16-bit Ruthotto-Haber symmetric layer (csrc/pde_rh.hip: rh_part16, rh_fwd16_epi, rh_out16_epi,
rh_bwd16_epi, rh_outer16 and rh_k_to_f16 kernels; include/pdecnn.h pde_sym_layer_f16_* / pde_sym_layer_bf16_* / pde_sym_k_to_*):
the header's contract written out in fp64, the generators of the inputs, the lists of cases, and the two comparisons
(``compare_exact``, ``check_stages``) that tests/test_gpu_rh16_stages.py applies to the kernels and tests/test_rh16_cases.py
applies, on the CPU, to the contract itself and to mutants of it.  Everything is parametrised by the 16-bit type.

The contract, r(v) = v.to(dtype).double() (round to nearest even; fp16 overflows to +-inf), every product and sum exact:

    X16 = r(X);  K16 = r(K);  P = r(X16 K16^T);  mean, invstd, running statistics from the 16-bit values of P
    N = r(gamma (P - mean) invstd + beta);  H = r(act(N));  Q = r(H K16);  S = r(fl32(scale Q));  out = S  (16-bit)  or  base + S  (fp32)
    gQ = r(fl32(scale r(g)));  dH = gQ K16^T;  dN = dH act'(H);  g_beta = sum_b dN;  g_gamma = sum_b dN xhat,  xhat = (P - mean) invstd
    dP = r(BatchNorm backward of dN);  gX = dP K16;  gK = dP^T X16 + H^T gQ

The two products by ``scale`` (the fp32 value the ABI receives) are fp32 operations, rounded to fp32 (fl32) before r(), as
in autocast's element-wise kernels: the fp32 rounding lands on a 16-bit tie for one value in ten at scale = 0.7, so this is
not r() of the exact product.  r() itself is a correct rounding of the fp64 value (``rne``), not torch's cast.

(a) Exact cases (eval mode, eps = 0, identity / ReLU, power-of-two scales and deviations).  ``assert_exact`` decides, per
output tensor, whether every fp32 operation of the kernels that leads to it is exact — then each r() has an exactly known
argument and the tensor has one right answer.  The rule: every operand of a sum is a multiple of a power of two u (taken
from the data: the lowest set bit over the tensor), and the sum of the absolute terms of every element is below 2^24 u, so
every partial sum in every order is an fp32 value; the element-wise steps ((P - mean), the fused multiply-add of N, base + S)
must give fp32 values; and the same must hold for everything upstream.  Non-finite elements (the fp16 overflow case) are
left out of the sums' condition and compared by position.  Two families: the narrow one is rh_cases.exact_layer as it is
(Q, and for bf16 N, round and meet ties; X, K, g never round); the wide one has integers of larger magnitude with low bits
of a quarter or a half of the element's 16-bit spacing added to X, g and K, so that X, K, g, P, N, Q and dP all round and
meet exact ties, at the price of gK (and g_gamma) leaving the bitwise set at larger widths.

(b) General cases, stage by stage (``check_stages``).  Each stage is evaluated in fp64 from the tensors that the code under
test itself produced upstream, so one stage's legitimate choice at a near-tie does not propagate.  A 16-bit output with fp64
pre-rounding value v must lie in [r(v - m), r(v + m)] — rounding and the three activations are monotone — where the margin m
is 4 x the largest deviation from v, over the tensor, of the same stage computed by plain fp32 torch (matmul on the widened
16-bit operands, element-wise ops, torch.tanh) on the same device from the same operands: the project's factor 2 for
another summation order, doubled because this is an element-wise maximum and not a norm.  m never comes from the code under
test.  Where the two ends coincide the element has one right answer; elsewhere it is held to the two neighbouring 16-bit
values, and at most TWO_ENDED_CAP of the elements of P, N, H and Q may have two ends.  dP is held to its interval but not
to the cap: in training mode it is a difference of nearly equal terms (with two batch rows it vanishes but for eps), so a
margin that is one absolute number per tensor spans several neighbours of its many small elements — 91 to 100 % of them at
B = 2 for the contract itself, whatever the kernel does; its share is reported, and every element is still within m plus
half a step of the fp64 value, m a few 1e-6 of the largest element.  ``out`` with a base is base + S with S a
16-bit value: the interval of S is pushed through the (correctly rounded) fp32 addition, which holds every element to
fl32(base + one of the two neighbours) — a rel_err bound of a few 1e-6 would refuse the legitimate neighbour, and one of
twice the plain route's error would admit any element being a step off as soon as the plain route is a step off somewhere.
The other fp32 outputs (mean, invstd, running statistics, gX, gK, g_gamma, g_beta) see identical 16-bit operands, so only
fp32 accumulation is left: golden_util.rel_err against the fp64 stage is at most max(FLOOR, 2 x the plain route's).

H with identity / ReLU and the two multiplications by a power-of-two scale (scale Q, scale r(g)) never round in the exact
cases: r() of a 16-bit value is the value.  Those three points are exercised by the general cases only (scale = 0.7, tanh)."""
import collections
import functools

import torch

import golden_util as G
import rh_cases as R

DTYPES = (torch.float16, torch.bfloat16)
TAG = {torch.float16: "f16", torch.bfloat16: "bf16"}
MANTISSA = {torch.float16: 10, torch.bfloat16: 7}           # stored fraction bits
OUTPUTS = R.OUTPUTS
ROUNDING_POINTS = ("X", "K", "g", "P", "N", "Q", "dP")      # the points that round in the exact cases (module docstring)
FLOOR = 3e-6                                                # tests/test_gpu_rh_paths.py: the measured floor of fp32 accumulation
TWO_ENDED_CAP = 0.25
CAPPED_STAGES = ("P", "N", "H", "Q")                        # dP: see the module docstring
MARGIN_FACTOR = 4.0


def sixteen_bit(name, c):
    """whether the ABI writes this output as a 16-bit tensor"""
    return name in ("P", "H", "dP") or (name == "out" and c.base is None)


# --------------------------------------------------------------------------------------------------- rounding
def _step16(q, up):
    """the next 16-bit value above (up) or below q, q a 16-bit tensor (zero's neighbours are the smallest subnormals)"""
    bits = q.view(torch.int16).to(torch.int32) & 0xFFFF
    key = torch.where(bits >= 0x8000, -(bits & 0x7FFF), bits) + (1 if up else -1)
    bits = torch.where(key < 0, (-key) | 0x8000, key)
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16)
    return bits.view(q.dtype)


def _bracket(v, dtype):
    """(lo, hi) as 16-bit tensors: the neighbouring values that bracket the finite fp64 values v (the same where v is one)"""
    q16 = v.to(dtype)                                       # within a step of v, whatever the cast's own rounding
    q = q16.double()
    return torch.where(q > v, _step16(q16, False), q16), torch.where(q < v, _step16(q16, True), q16)


def _wide(x16, dtype):
    """fp64 of a 16-bit tensor with +-inf taken as the next power of two, the value a rounding to nearest measures against"""
    x = x16.double()
    top = 2.0 ** (16 if dtype == torch.float16 else 128)
    return torch.where(torch.isinf(x), torch.sign(x) * top, x)


def neighbours(v, dtype):
    """(lo, hi) of ``_bracket`` as fp64"""
    lo, hi = _bracket(v, dtype)
    return lo.double(), hi.double()


def rne(dtype):
    """r(): fp64 to the nearest 16-bit value, ties to even, beyond the largest finite value plus half a step to +-inf, as
    fp64.  Not ``v.to(dtype)``: torch casts fp64 by way of fp32, and that first rounding can land on a 16-bit tie (the
    product of an fp32 scale and a 16-bit value does so for one value in ten at scale = 0.7)."""
    def r(v):
        lo, hi = _bracket(v, dtype)
        dlo, dhi = v - _wide(lo, dtype), _wide(hi, dtype) - v
        even = (lo.view(torch.int16) & 1) == 0
        q = torch.where((dlo < dhi) | ((dlo == dhi) & even), lo, hi).double()
        return torch.where(torch.isfinite(v), q, v)
    return r


def via_fp32(v):
    """an fp32 operation's own rounding"""
    return v.float().double()


def is_tie(v, dtype):
    """exactly half way between two neighbouring 16-bit values (v - lo and hi - v are exact in fp64 for fp32-sized data)"""
    lo, hi = neighbours(v, dtype)
    return torch.isfinite(lo) & torch.isfinite(hi) & (lo != hi) & ((v - lo) == (hi - v))


def truncating(dtype):
    """a wrong r(): toward zero"""
    def r(v):
        lo, hi = neighbours(v, dtype)
        return torch.where(torch.isfinite(v), torch.where(v >= 0, lo, hi), v)
    return r


def ties_away(dtype):
    """a wrong r(): to nearest, ties away from zero"""
    def r(v):
        lo, hi = neighbours(v, dtype)
        return torch.where(is_tie(v, dtype), torch.where(v >= 0, hi, lo), v.to(dtype).double())
    return r


class Rules:
    """How ``contract`` evaluates: the header's text by default; every other setting is a mutant (a subtly wrong kernel).
    r: the rounding function; skip: rounding points left out ("X", "N"); stats_unrounded: statistics and N taken from P before
    its rounding; k_not_t: K16 in place of K16^T in the first product; swap_var: the unbiased variance normalises and the
    biased one updates the running statistic; leak_row: one batch row beyond B (a copy of the last) counted into gK;
    fused_scale: the products by scale not rounded to fp32 (what the fp16 kernels did until the stage tests were written)."""

    def __init__(self, r=None, skip=(), stats_unrounded=False, k_not_t=False, swap_var=False, leak_row=False, fused_scale=False):
        self.r, self.skip, self.stats_unrounded = r, frozenset(skip), stats_unrounded
        self.k_not_t, self.swap_var, self.leak_row, self.fused_scale = k_not_t, swap_var, leak_row, fused_scale


def mutants(dtype):
    return {"r truncates": Rules(r=truncating(dtype)), "r rounds ties away from zero": Rules(r=ties_away(dtype)),
            "r(P) skipped before the statistics": Rules(stats_unrounded=True), "N not rounded": Rules(skip=("N",)),
            "r(X) skipped": Rules(skip=("X",)), "K in place of K^T": Rules(k_not_t=True),
            "biased and unbiased variance swapped": Rules(swap_var=True), "a row beyond B leaks into gK": Rules(leak_row=True),
            "scale product rounded once": Rules(fused_scale=True)}


# --------------------------------------------------------------------------------------------------- the contract
def _mm(a, b):
    """a @ b in fp64; the zero of an accumulator that starts at +0 is +0; inf 0 = NaN whatever the BLAS does with it"""
    if bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()):
        return (a @ b) + 0.0
    return (a[:, :, None] * b[None, :, :]).sum(dim=1) + 0.0


def scale32(c):
    """the scale as the ABI receives it: the fp32 value nearest to the layer's"""
    return float(torch.tensor(c.scale, dtype=torch.float32))


def contract(c, dtype, device="cpu", rules=None):
    """Every tensor of OUTPUTS in fp64 as the header's contract defines it, the intermediates (X16, K16, N, Q, S, gQ, dH,
    dN, xhat) and, under "pre", the value of every rounding point before its rounding."""
    rules = rules or Rules()
    r0 = rules.r or rne(dtype)
    r = lambda name, v: v if name in rules.skip else r0(v)
    fl32 = (lambda v: v) if rules.fused_scale else via_fp32
    t = lambda v: None if v is None else v.to(device=device, dtype=torch.float64)
    X, K, gamma, beta, g, base = t(c.X), t(c.K), t(c.gamma), t(c.beta), t(c.g), t(c.base)
    rm, rv = t(c.running_mean), t(c.running_var)
    B = c.B
    pre = {"X": X, "K": K, "g": g}
    X16, K16 = r("X", X), r("K", K)
    pre["P"] = _mm(X16, K16 if rules.k_not_t else K16.t())
    P = r("P", pre["P"])
    Ps = pre["P"] if rules.stats_unrounded else P
    new_rm, new_rv = rm, rv
    if c.training:
        mean = Ps.mean(dim=0)
        var = ((Ps - mean) ** 2).mean(dim=0)
        unbiased = var * (B / (B - 1)) if B > 1 else var
        if rules.swap_var:
            var, unbiased = unbiased, var
        invstd = 1.0 / torch.sqrt(var + c.eps)
        if rm is not None:
            new_rm = (1.0 - c.momentum) * rm + c.momentum * mean
            new_rv = (1.0 - c.momentum) * rv + c.momentum * unbiased
    else:
        mean, invstd = rm, 1.0 / torch.sqrt(rv + c.eps)
    pre["N"] = gamma * ((Ps - mean) * invstd) + beta
    N = r("N", pre["N"])
    pre["H"] = R.act_forward(N, c.act)
    H = r("H", pre["H"])
    pre["Q"] = _mm(H, K16)
    Q = r("Q", pre["Q"])
    pre["S"] = fl32(scale32(c) * Q)                         # an fp32 product: rounded to fp32 before r()
    S = r("S", pre["S"])
    out = S if base is None else base + S
    pre["gQ"] = fl32(scale32(c) * r("g", g))
    gQ = r("gQ", pre["gQ"])
    dH = _mm(gQ, K16.t())
    dN = dH * R.act_derivative(H, c.act)
    xhat = (P - mean) * invstd
    g_beta = dN.sum(dim=0)
    g_gamma = (dN * xhat).sum(dim=0)
    if c.training:
        pre["dP"] = (gamma * invstd) * (dN - (g_beta + xhat * g_gamma) / B)
    else:
        pre["dP"] = (gamma * invstd) * dN
    dP = r("dP", pre["dP"])
    gX = _mm(dP, K16)
    gK = _mm(dP.t(), X16) + _mm(H.t(), gQ)
    if rules.leak_row:
        gK = gK + torch.outer(dP[-1], X16[-1]) + torch.outer(H[-1], gQ[-1])
    return {"P": P, "H": H, "mean": mean, "invstd": invstd, "out": out, "running_mean": new_rm, "running_var": new_rv,
            "dP": dP, "gX": gX, "gK": gK, "g_gamma": g_gamma, "g_beta": g_beta, "X16": X16, "K16": K16, "N": N, "Q": Q, "S": S,
            "gQ": gQ, "dH": dH, "dN": dN, "xhat": xhat, "pre": pre}


def as_abi(c, ref, dtype):
    """the tensors of OUTPUTS in the types the ABI writes them in (None where nothing is tracked)"""
    return {k: None if ref[k] is None else ref[k].to(dtype if sixteen_bit(k, c) else torch.float32) for k in OUTPUTS}


# --------------------------------------------------------------------------------------------------- exact cases
def _unit(*tensors):
    """the largest power of two that divides every finite non-zero element (1 where there is none)"""
    u = 1.0
    first = True
    for t in tensors:
        v = t[torch.isfinite(t) & (t != 0)]
        if v.numel() == 0:
            continue
        m, e = torch.frexp(v)
        k = (m.abs() * 2.0 ** 53).to(torch.int64)
        low = (k & -k).double()
        w = float(torch.exp2((e.double() - 53.0) + torch.log2(low).round()).min())
        u = w if first else min(u, w)
        first = False
    return u


def _fp32_values(v):
    f = torch.isfinite(v)
    return bool((v.float().double()[f] == v[f]).all())


def _sums_exact(value, abs_sum, unit):
    """every finite element's sum of absolute terms is below 2^24 units: every partial sum, in any order, is an fp32 value"""
    f = torch.isfinite(value)
    return bool((abs_sum[f] < unit * 2.0 ** 24).all())


def assert_exact(c, ref, dtype):
    """The conditions of an exact case (module docstring, (a)); raises where the inputs are not of that kind or where P, H, a
    base-less out or dP would not have one right answer.  Returns the set of outputs that have one, to be compared bitwise."""
    dev = ref["P"].device
    t = lambda v: None if v is None else v.to(device=dev, dtype=torch.float64)
    rv, gamma, base = t(c.running_var), t(c.gamma), t(c.base)
    isin = lambda v, vals: bool(torch.isin(v, torch.tensor(vals, dtype=torch.float64, device=dev)).all())
    assert not c.training and c.eps == 0.0 and c.act in ("identity", "relu") and c.scale in R.EXACT_SCALES
    assert isin(rv, (0.25, 1.0, 4.0)) and isin(gamma, (1.0, 2.0, -1.0)) and isin(ref["invstd"], (2.0, 1.0, 0.5))
    for v in (t(c.running_mean), t(c.beta)) + (() if base is None else (base,)):
        assert bool((v == v.round()).all())
    for v in (t(c.X), t(c.K), t(c.g)):
        assert _fp32_values(v)
    K16 = ref["K16"]
    assert not torch.equal(K16, K16.t()) and bool((K16 != 0).any(dim=0).all()) and bool((K16 != 0).any(dim=1).all())
    X16, gQ, P, H, dP, dN, xhat, pre = ref["X16"], ref["gQ"], ref["P"], ref["H"], ref["dP"], ref["dN"], ref["xhat"], ref["pre"]
    assert torch.equal(pre["S"], ref["S"]) and torch.equal(pre["gQ"], gQ) and torch.equal(pre["H"], H), \
        "a power-of-two multiple or the identity / ReLU of a 16-bit value rounds"
    aK = K16.abs()
    ok = {}
    ok["P"] = _sums_exact(P, X16.abs() @ aK.t(), _unit(X16) * _unit(K16))
    ok["mean"] = ok["invstd"] = ok["running_mean"] = ok["running_var"] = True
    centred = P - ref["mean"]
    ok["H"] = ok["P"] and _fp32_values(centred) and _fp32_values(pre["N"])
    ok["out"] = ok["H"] and _sums_exact(ref["out"], H.abs() @ aK, _unit(H) * _unit(K16)) and _fp32_values(ref["out"])
    dh_ok = _sums_exact(ref["dH"], gQ.abs() @ aK.t(), _unit(gQ) * _unit(K16))
    ok["dP"] = ok["H"] and dh_ok and _fp32_values(pre["dP"])
    ok["g_beta"] = ok["H"] and dh_ok and _sums_exact(ref["g_beta"], dN.abs().sum(dim=0), _unit(dN)) and _fp32_values(ref["g_beta"])
    ok["g_gamma"] = (ok["H"] and dh_ok and _fp32_values(xhat) and _fp32_values(ref["g_gamma"])
                     and _sums_exact(ref["g_gamma"], (dN * xhat).abs().sum(dim=0), _unit(dN) * _unit(xhat)))
    ok["gX"] = ok["dP"] and _sums_exact(ref["gX"], dP.abs() @ aK, _unit(dP) * _unit(K16)) and _fp32_values(ref["gX"])
    ok["gK"] = (ok["dP"] and _fp32_values(ref["gK"])
                and _sums_exact(ref["gK"], dP.abs().t() @ X16.abs() + H.abs().t() @ gQ.abs(),
                                min(_unit(dP) * _unit(X16), _unit(H) * _unit(gQ))))
    for name in ("P", "H", "out", "dP"):
        assert ok[name] or (name == "out" and base is not None), f"{name} has no single right answer in this case"
    return frozenset(k for k, v in ok.items() if v)


def _low_bits(n, dtype, gen):
    """n (integers, or K's -1 / 0 / 1) plus a quarter or a half of the element's 16-bit spacing, either sign — bits r() must
    remove to give n back; kept only where it does (a half step only where n is the even neighbour), zeros left alone"""
    _, e = torch.frexp(n)
    ulp = torch.exp2((e - 1 - MANTISSA[dtype]).double())
    frac = torch.tensor((0.25, -0.25, 0.5, -0.5), dtype=torch.float64)[torch.randint(0, 4, n.shape, generator=gen)]
    v = torch.where(n != 0, n + frac * ulp, n)
    v = torch.where(v.to(dtype).double() == n, v, n)
    assert torch.equal(v.float().double(), v) and torch.equal(v.to(dtype).double(), n)
    return v


#: the largest |integer| of X and g: fp16 must keep Q = H K16 below 65504, so its magnitude falls with the width (P, beyond
#: 2048, rounds at D = 64 only; N and Q round everywhere); bf16 alternates
WIDE_MAGNITUDE = {torch.float16: {64: (255,), 128: (127,), 192: (63,), 256: (63,)},
                  torch.bfloat16: {D: (31, 63) for D in (64, 128, 192, 256)}}


def wide_layer(B, D, variant, dtype):
    """The wide exact case: exact_layer's parameters with X and g integers of the type's larger magnitude, and low bits on X,
    g and K."""
    c = R.exact_layer(B, D, variant)
    mags = WIDE_MAGNITUDE[dtype][D]
    mag = mags[variant % len(mags)]
    gen = torch.Generator().manual_seed(70000 + 977 * B + D + 13 * variant + (1 if dtype == torch.bfloat16 else 0))
    ints = lambda: torch.randint(-mag, mag + 1, (B, D), generator=gen).double()
    c.X, c.g = _low_bits(ints(), dtype, gen), _low_bits(ints(), dtype, gen)
    c.K = _low_bits(c.K, dtype, gen)
    return c


OVERFLOW_SHAPE = (5, 64)
OVERFLOW_ROW, OVERFLOW_COL = 2, 7


def overflow_layer():
    """fp16 only, eval mode, identity: row 7 of K is all +-1 and row 2 of X is 1024 times its signs, so P[2][7] = 65536 is
    the one element of P beyond 65504."""
    B, D = OVERFLOW_SHAPE
    c = R.exact_layer(B, D, 0)                              # variant 0: identity, a base, scale -1
    assert c.act == "identity"
    k = c.K[OVERFLOW_COL]
    c.K[OVERFLOW_COL] = torch.where(k == 0, torch.ones_like(k), k)
    c.X[OVERFLOW_ROW] = 1024.0 * c.K[OVERFLOW_COL]
    return c


@functools.lru_cache(maxsize=None)
def overflow_case():
    c = overflow_layer()
    ref = contract(c, torch.float16)
    over = ref["pre"]["P"].abs() > 65504
    assert int(over.sum()) == 1 and bool(over[OVERFLOW_ROW, OVERFLOW_COL]) and bool(torch.isinf(ref["P"][OVERFLOW_ROW, OVERFLOW_COL]))
    assert int(torch.isinf(ref["P"]).sum()) == 1 and not bool(torch.isnan(ref["P"]).any()) and not bool(torch.isnan(ref["H"]).any())
    for name in ("out", "g_gamma", "gK"):
        assert not bool(torch.isfinite(ref[name]).all()), name
    held = assert_exact(c, ref, torch.float16)
    assert held == frozenset(OUTPUTS), sorted(set(OUTPUTS) - held)
    return c, ref, held


def exact_layer(family, B, D, variant, dtype):
    return R.exact_layer(B, D, variant) if family == "narrow" else wide_layer(B, D, variant, dtype)


@functools.lru_cache(maxsize=None)
def exact_case(family, B, D, variant, dtype):
    """(inputs, contract, the bitwise set) of an exact case on the CPU; shared and never modified"""
    c = exact_layer(family, B, D, variant, dtype)
    ref = contract(c, dtype)
    return c, ref, assert_exact(c, ref, dtype)


#: one exact case, named after what it reaches: the split S of rh_split16, the waves of the strip kernels, the 64-wide slabs
#: per slice, whether rh_outer16's 64 x 192 tiles are whole, and the row edge
Case = collections.namedtuple("Case", "family B D split waves slabs tiles variant")


def split16(D):
    S = 8
    while S > 1 and D % (S * 64) != 0:
        S //= 2
    return S


def _case(family, B, D, variant):
    S = split16(D)
    return Case(family, B, D, S, 2 if B <= 64 else 4, D // (64 * S), "whole" if D % 192 == 0 else "ragged", variant)


def case_id(c):
    return f"{c.family}-B{c.B}-D{c.D}-S{c.split}-w{c.waves}-slabs{c.slabs}-{c.tiles}"


#: row quads of the epilogues, 16-row groups of rh_outer16, 32-row waves, the 2 -> 4 wave switch
NARROW_BATCHES = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)
NARROW_WIDTHS = (64, 128, 192, 512)                         # S 1; S 2; S 1, three slabs, a whole tile; S 8
NARROW_BATCHES_2 = (1, 17, 64, 65, 128)
NARROW_WIDTHS_2 = (256, 320, 384, 768, 1024)                # S 4; S 1 ragged second tile; S 2 two whole tiles; S 4 x 3; S 8 x 2
WORKLOAD_SHAPE = (64, 3072)                                 # the reference's own shape; its fp64 products are taken on the GPU
#: (B, D): every width up to 256, every wave count, ragged quads, groups and waves; chosen by tests/test_rh16_cases.py's
#: check that P, H, a base-less out and dP keep one right answer and that every 16-bit tensor stays finite
WIDE_SHAPES = ((5, 64), (17, 64), (64, 64), (65, 64), (128, 64), (16, 128), (33, 128), (127, 128), (15, 192), (65, 192),
               (31, 256), (128, 256))


def narrow_cases():
    cs = [(B, D) for D in NARROW_WIDTHS for B in NARROW_BATCHES] + [(B, D) for D in NARROW_WIDTHS_2 for B in NARROW_BATCHES_2]
    return [_case("narrow", B, D, i) for i, (B, D) in enumerate(cs)]


def workload_case():
    return _case("narrow", *WORKLOAD_SHAPE, 1)              # variant 1: ReLU, a base, scale 1/2


def wide_cases():
    return [_case("wide", B, D, i) for i, (B, D) in enumerate(WIDE_SHAPES)]


def patterns(t):
    """the bit patterns of a 16-bit tensor, the two zeros as one: the sign of a zero is not part of the contract (a ReLU
    backward that selects, as torch's does, gives +0 where the multiplication by a zero derivative gives -0, and a compiler
    may turn the one into the other); torch.equal on the fp32 tensors does not tell the zeros apart either"""
    v = t.view(torch.int16)
    return torch.where(v == -32768, torch.zeros_like(v), v)


def compare_exact(c, got, ref, held, dtype, what=""):
    """The tensors of ``held``: 16-bit ones equal as bit patterns (``patterns``), fp32 ones torch.equal; where the contract is
    not finite (the overflow case) the same positions are not finite, with +-inf matched by the patterns of P and H.
    ``got``: the tensors in the ABI's types."""
    want = as_abi(c, ref, dtype)
    bad = []
    for name in OUTPUTS:
        if name not in held or want[name] is None:
            continue
        g, w = got[name].cpu(), want[name].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape)
        if name in ("P", "H"):                             # patterns throughout: an inf is an inf of the same sign
            same = patterns(g) == patterns(w)
        else:
            fin = torch.isfinite(w)
            bits = (patterns(g) == patterns(w)) if sixteen_bit(name, c) else (g == w)
            same = torch.where(fin, bits, ~torch.isfinite(g))
        if not bool(same.all()):
            where = torch.nonzero(~same)[0].tolist()
            idx = tuple(where)
            bad.append(f"{name}: {int((~same).sum())} of {same.numel()} elements differ, first at {where}: "
                       f"{float(g[idx])} for {float(w[idx])}")
    assert not bad, f"{what}: " + "; ".join(bad)


# --------------------------------------------------------------------------------------------------- general cases
GENERAL_SHAPES = ((2, 64), (5, 64), (17, 192), (33, 128), (64, 256), (65, 512), (128, 768), (100, 1024))
GENERAL_MODES = R.GENERAL_MODES
UNTRACKED_CASE = (33, 128, "tanh")                          # training mode with running_mean = running_var = NULL


def general_layer(B, D, act, training, variant=0, track=True):
    """rh_cases.general_layer's seeded values; odd variants have no base; ``track`` False: no running statistics"""
    src = R.general_layer(B, D, act, training)
    c = R.Layer(src.X, src.K, src.gamma, src.beta, src.running_mean if track else None, src.running_var if track else None,
                src.base if variant % 2 == 0 else None, src.scale, src.g, act, training, src.momentum, src.eps)
    assert training or track
    return c


def general_cases():
    """(B, D, act, training, variant, track)"""
    cs = []
    for i, (B, D) in enumerate(GENERAL_SHAPES):
        for j, (act, training) in enumerate(GENERAL_MODES):
            cs.append((B, D, act, training, i + j, True))
    B, D, act = UNTRACKED_CASE
    cs.append((B, D, act, True, 1, False))
    return cs


def general_id(v):
    B, D, act, training, variant, track = v
    return f"B{B}-D{D}-{act}-{'train' if training else 'eval'}-{'base' if variant % 2 == 0 else 'nobase'}" + ("" if track else "-untracked")


def check_stages(c, dtype, got, device="cpu", what=""):
    """Rule (b) of the module docstring on the tensors ``got`` (in the ABI's types, on ``device``) that some evaluation of the
    layer ``c`` produced; the plain fp32 route runs on ``device``.  Raises on a tensor outside its rule or on more than
    TWO_ENDED_CAP two-ended elements; returns the figures: {stage: (margin, share of two-ended elements)} for the 16-bit
    stages P, N, H, Q, dP and {name: (error, the plain route's error)} for the fp32 outputs."""
    d = lambda v: None if v is None else v.to(device=device, dtype=torch.float64)
    r = rne(dtype)
    f32 = lambda v: v.float()
    gamma, beta, base, rm, rv = d(c.gamma), d(c.beta), d(c.base), d(c.running_mean), d(c.running_var)
    X16, K16 = r(d(c.X)), r(d(c.K))
    gQ = r(via_fp32(scale32(c) * r(d(c.g))))
    B = c.B
    k = {n: None if got[n] is None else got[n].to(device).double() for n in OUTPUTS}
    bad, fig = [], {}
    for n in OUTPUTS:
        if k[n] is not None and not bool(torch.isfinite(k[n]).all()):
            bad.append(f"{n} is not finite")

    def margin(stage, v, plain):
        m = MARGIN_FACTOR * float((plain.double() - v).abs().max())
        return m

    def ends(stage, lo, hi, m):
        share = float((lo != hi).double().mean())
        fig[stage] = (m, share)
        if stage in CAPPED_STAGES and share > TWO_ENDED_CAP:
            bad.append(f"{stage}: {share:.1%} of the elements have two ends (margin {m:.3e})")

    def inside(name, value, lo, hi):
        out = ~((value >= lo) & (value <= hi))
        if bool(out.any()):
            i = tuple(torch.nonzero(out)[0].tolist())
            bad.append(f"{name}: {int(out.sum())} of {out.numel()} elements outside their interval, first at {list(i)}: "
                       f"{float(value[i])!r} not in [{float(lo[i])!r}, {float(hi[i])!r}]")

    def hold(name, value, v, plain):
        e, p = G.rel_err(value, v), G.rel_err(plain.double(), v)
        fig[name] = (e, p)
        if not e <= max(FLOOR, 2 * p):
            bad.append(f"{name}: error {e:.3e} against fp64, the plain fp32 route {p:.3e}, floor {FLOOR:.0e}")

    # P from r(X), K16
    v = X16 @ K16.t()
    m = margin("P", v, f32(X16) @ f32(K16).t())
    lo, hi = r(v - m), r(v + m)
    ends("P", lo, hi, m)
    inside("P", k["P"], lo, hi)
    # statistics from the P under test
    P, Pf = k["P"], f32(k["P"])
    if c.training:
        mean_v = P.mean(dim=0)
        var_v = ((P - mean_v) ** 2).mean(dim=0)
        mean_p, var_p = Pf.mean(dim=0), Pf.var(dim=0, unbiased=False)
        hold("mean", k["mean"], mean_v, mean_p)
        hold("invstd", k["invstd"], 1.0 / torch.sqrt(var_v + c.eps), 1.0 / torch.sqrt(var_p + c.eps))
        if rm is not None:
            ub = B / (B - 1) if B > 1 else 1.0
            hold("running_mean", k["running_mean"], (1.0 - c.momentum) * rm + c.momentum * mean_v,
                 (1.0 - c.momentum) * f32(rm) + c.momentum * mean_p)
            hold("running_var", k["running_var"], (1.0 - c.momentum) * rv + c.momentum * (var_v * ub),
                 (1.0 - c.momentum) * f32(rv) + c.momentum * (var_p * ub))
        else:
            assert got["running_mean"] is None and got["running_var"] is None
    else:
        if not (torch.equal(k["mean"], rm) and torch.equal(k["running_mean"], rm) and torch.equal(k["running_var"], rv)):
            bad.append("eval mode: mean is not running_mean, or the running statistics moved")
        hold("invstd", k["invstd"], 1.0 / torch.sqrt(rv + c.eps), 1.0 / torch.sqrt(f32(rv) + c.eps))
    # H from the P, mean and invstd under test: the interval of N pushed through r, the activation and r again
    mean, invstd = k["mean"], k["invstd"]
    v = gamma * ((P - mean) * invstd) + beta
    m = margin("N", v, f32(gamma) * ((Pf - f32(mean)) * f32(invstd)) + f32(beta))
    nlo, nhi = r(v - m), r(v + m)
    ends("N", nlo, nhi, m)
    ma = 0.0
    if c.act == "tanh":
        n16 = r(v)
        ma = margin("H", torch.tanh(n16), torch.tanh(f32(n16)))
    lo, hi = r(R.act_forward(nlo, c.act) - ma), r(R.act_forward(nhi, c.act) + ma)
    ends("H", lo, hi, max(m, ma))
    inside("H", k["H"], lo, hi)
    # out from the H under test
    H, Hf = k["H"], f32(k["H"])
    v = H @ K16
    m = margin("Q", v, Hf @ f32(K16))
    qlo, qhi = r(v - m), r(v + m)
    ends("Q", qlo, qhi, m)
    sa, sb = r(via_fp32(scale32(c) * qlo)), r(via_fp32(scale32(c) * qhi))
    lo, hi = torch.minimum(sa, sb), torch.maximum(sa, sb)
    if base is not None:
        lo, hi = (base + lo).float().double(), (base + hi).float().double()
    inside("out", k["out"], lo, hi)
    # dP, g_gamma, g_beta from the P, H, mean and invstd under test and the exact gQ
    dH_v, dH_p = gQ @ K16.t(), f32(gQ) @ f32(K16).t()
    dN_v, dN_p = dH_v * R.act_derivative(H, c.act), dH_p * R.act_derivative(Hf, c.act)
    xh_v, xh_p = (P - mean) * invstd, (Pf - f32(mean)) * f32(invstd)
    gb_v, gb_p = dN_v.sum(dim=0), dN_p.sum(dim=0)
    gg_v, gg_p = (dN_v * xh_v).sum(dim=0), (dN_p * xh_p).sum(dim=0)
    hold("g_beta", k["g_beta"], gb_v, gb_p)
    hold("g_gamma", k["g_gamma"], gg_v, gg_p)
    if c.training:
        v = (gamma * invstd) * (dN_v - (gb_v + xh_v * gg_v) / B)
        p = (f32(gamma) * f32(invstd)) * (dN_p - (gb_p + xh_p * gg_p) / B)
    else:
        v, p = (gamma * invstd) * dN_v, (f32(gamma) * f32(invstd)) * dN_p
    m = margin("dP", v, p)
    lo, hi = r(v - m), r(v + m)
    ends("dP", lo, hi, m)
    inside("dP", k["dP"], lo, hi)
    # gX, gK from the dP and H under test
    dP, dPf = k["dP"], f32(k["dP"])
    hold("gX", k["gX"], dP @ K16, dPf @ f32(K16))
    hold("gK", k["gK"], dP.t() @ X16 + H.t() @ gQ, dPf.t() @ f32(X16) + Hf.t() @ f32(gQ))
    assert not bad, f"{what}: " + "; ".join(bad)
    return fig


@functools.lru_cache(maxsize=None)
def general_contract(B, D, act, training, variant, track, dtype):
    c = general_layer(B, D, act, training, variant, track)
    return c, contract(c, dtype)
