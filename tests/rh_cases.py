"""Ground for the tests of the fp32 Ruthotto-Haber symmetric layer (csrc/pde_rh.hip; include/pdecnn.h
pde_sym_layer_forward / _backward): a closed-form fp64 reference of the layer and its backward written as the C ABI sees
them, the generators of the inputs, and the lists of cases, each named after the kernel path it is meant to take.
tests/test_rh_cases.py checks this module on the CPU; tests/test_gpu_rh_paths.py runs the kernels against it.

    P = X K^T;  mean, invstd (batch statistics in training mode, the running ones otherwise);  xhat = (P - mean) invstd
    H = act(gamma xhat + beta);  out = base + scale (H K)
    dH = (scale g) K^T;  dN = dH act'(H)  (ReLU: 1 where H > 0, 0 at the tie);  g_beta = sum_b dN;  g_gamma = sum_b dN xhat
    dP = gamma invstd (dN - (g_beta + xhat g_gamma) / B)  (training)   or   gamma invstd dN  (eval)
    gX = dP K;  gK = dP^T X + H^T (scale g)

Exact cases run in eval mode with eps = 0: running_var in {0.25, 1, 4} (invstd exactly 2, 1, 0.5), running_mean, beta
and base integers, gamma in {1, 2, -1}, scale in {-1, 0.5, -0.25}, X and g integers in -3..3, K with entries in
{-1, 0, 1}, not symmetric and without a zero row or column.  Every stage is then a multiple of 1/8 (P of 1, H of 1/2,
out, dP, gX, gK of |scale| / 2 >= 1/8), and ``assert_exact`` checks on each case, before anything is compared, that the
sum of the absolute values of the terms of every output element is below 2^24 eighths — any summation order is then exact
in fp32 — and the piece condition of the three-piece gradient of K (rh_outer_split_kernel keeps the piece products (0,0),
(0,1), (1,0), (1,1), (0,2), (2,0)): X and scale g are one bf16 piece each, dP and H two, so the kept products are the
whole product.  Each output then has one right answer in fp32 and is compared with ``torch.equal``."""
import collections
import functools

import torch

STRIP32, STRIP16, ROW_BLOCKS = 0, 1, 2                      # PDE_RH_PATH_* of include/pdecnn.h
DK_SPLIT3, DK_MFMA_F32 = 0, 1                               # PDE_RH_DK_*
ACT_CODE = {"identity": 0, "relu": 1, "tanh": 2}
SWITCHES = ("PDE_RH_NO_STRIP32", "PDE_RH_SPLIT", "PDE_RH_NO_SPLIT")
UNIT = 0.125                                                # the finest granularity of an exact case

#: what the kernels write, in the order of the C ABI; the running statistics are the buffers after the forward
OUTPUTS = ("P", "H", "mean", "invstd", "out", "running_mean", "running_var", "dP", "gX", "gK", "g_gamma", "g_beta")


class Layer:
    """Inputs of one call pair (forward, backward) as fp64 tensors that hold fp32 values."""

    def __init__(self, X, K, gamma, beta, running_mean, running_var, base, scale, g, act, training, momentum, eps):
        self.X, self.K, self.gamma, self.beta = X, K, gamma, beta
        self.running_mean, self.running_var, self.base, self.g = running_mean, running_var, base, g
        self.scale, self.act, self.training, self.momentum, self.eps = float(scale), act, bool(training), float(momentum), float(eps)
        self.B, self.D = X.shape

    def tensors(self):
        return {"X": self.X, "K": self.K, "gamma": self.gamma, "beta": self.beta, "running_mean": self.running_mean,
                "running_var": self.running_var, "base": self.base, "g": self.g}


def act_forward(n, act):
    return torch.relu(n) if act == "relu" else (torch.tanh(n) if act == "tanh" else n)


def act_derivative(h, act):
    """in terms of the activation's output; ReLU's derivative at 0 is 0"""
    if act == "relu":
        return (h > 0).to(h.dtype)
    return 1.0 - h * h if act == "tanh" else torch.ones_like(h)


def reference(c, device="cpu"):
    """Every tensor of OUTPUTS in fp64 (plus the intermediates xhat, dN, dQ = scale g), computed on ``device``."""
    t = lambda v: None if v is None else v.to(device=device, dtype=torch.float64)
    X, K, gamma, beta, g, base = t(c.X), t(c.K), t(c.gamma), t(c.beta), t(c.g), t(c.base)
    rm, rv = t(c.running_mean), t(c.running_var)
    B = c.B
    P = X @ K.t()
    if c.training:
        mean = P.mean(dim=0)
        var = ((P - mean) ** 2).mean(dim=0)
        invstd = 1.0 / torch.sqrt(var + c.eps)
        new_rm, new_rv = rm, rv
        if rm is not None:
            unbiased = var * (B / (B - 1)) if B > 1 else var
            new_rm = (1.0 - c.momentum) * rm + c.momentum * mean
            new_rv = (1.0 - c.momentum) * rv + c.momentum * unbiased
    else:
        mean, invstd = rm, 1.0 / torch.sqrt(rv + c.eps)
        new_rm, new_rv = rm, rv
    xhat = (P - mean) * invstd
    H = act_forward(xhat * gamma + beta, c.act)
    Q = H @ K
    out = c.scale * Q if base is None else base + c.scale * Q
    dQ = c.scale * g
    dN = (dQ @ K.t()) * act_derivative(H, c.act)
    g_beta = dN.sum(dim=0)
    g_gamma = (dN * xhat).sum(dim=0)
    if c.training:
        dP = gamma * invstd * (dN - (g_beta + xhat * g_gamma) / B)
    else:
        dP = gamma * invstd * dN
    gX = dP @ K
    gK = dP.t() @ X + H.t() @ dQ
    return {"P": P, "H": H, "mean": mean, "invstd": invstd, "out": out, "running_mean": new_rm, "running_var": new_rv,
            "dP": dP, "gX": gX, "gK": gK, "g_gamma": g_gamma, "g_beta": g_beta, "xhat": xhat, "dN": dN, "dQ": dQ}


# --------------------------------------------------------------------------------------------------- exact cases
def int_matrix(D, gen):
    """entries in {-1, 0, 1}, no zero row or column, not symmetric: K in place of K^T gives another result"""
    K = torch.randint(-1, 2, (D, D), generator=gen).double()
    idx = torch.arange(D)
    K[idx, (idx + 1) % D] = 1.0
    K[0, 1], K[1, 0] = 1.0, -1.0
    return K


def _choice(values, n, gen):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), (n,), generator=gen)]


EXACT_SCALES = (-1.0, 0.5, -0.25)


def exact_layer(B, D, variant):
    """The exact case of shape (B, D); ``variant`` (the case's place in its grid) picks the activation (identity, ReLU),
    whether there is a ``base``, and the scale, so that a grid alternates over all of them."""
    gen = torch.Generator().manual_seed(90000 + 977 * B + D + 13 * variant)
    ints = lambda *shape: torch.randint(-3, 4, shape, generator=gen).double()
    X, g = ints(B, D), ints(B, D)
    K = int_matrix(D, gen)
    gamma = _choice((1.0, 2.0, -1.0), D, gen)
    beta = torch.randint(-2, 3, (D,), generator=gen).double()
    rm = torch.randint(-2, 3, (D,), generator=gen).double()
    rv = _choice((0.25, 1.0, 4.0), D, gen)
    base = ints(B, D) if (variant // 2) % 2 == 0 else None
    return Layer(X, K, gamma, beta, rm, rv, base, EXACT_SCALES[variant % 3], g, ("identity", "relu")[variant % 2],
                 training=False, momentum=0.1, eps=0.0)


def bf16_pieces(v, n):
    """the first n pieces of the fp32 values v = hi + mid + lo, each rounded to nearest even as the kernel does"""
    rest, pieces = v.float(), []
    for _ in range(n):
        p = rest.to(torch.bfloat16).float()
        pieces.append(p.double())
        rest = rest - p
    return pieces


def assert_exact(c, ref):
    """The conditions under which the case has one right answer in fp32 (module docstring); raises where one fails.
    Works on whatever device ``ref`` is on.  Returns the largest absolute-term sum, in eighths."""
    dev = ref["P"].device
    t = lambda v: None if v is None else v.to(device=dev, dtype=torch.float64)
    X, K, g, base = t(c.X), t(c.K), t(c.g), t(c.base)
    assert not c.training and c.eps == 0.0 and c.act in ("identity", "relu") and c.scale in EXACT_SCALES
    assert float(X.abs().max()) <= 3 and float(g.abs().max()) <= 3 and bool((X == X.round()).all()) and bool((g == g.round()).all())
    assert bool(((K == 0) | (K.abs() == 1)).all()) and not torch.equal(K, K.t())
    assert bool((K != 0).any(dim=0).all()) and bool((K != 0).any(dim=1).all())
    assert bool(torch.isin(t(c.running_var), torch.tensor((0.25, 1.0, 4.0), dtype=torch.float64, device=dev)).all())
    assert bool(torch.isin(t(c.gamma), torch.tensor((1.0, 2.0, -1.0), dtype=torch.float64, device=dev)).all())
    for v in (t(c.running_mean), t(c.beta)) + (() if base is None else (base,)):
        assert bool((v == v.round()).all())
    assert bool(torch.isin(ref["invstd"], torch.tensor((2.0, 1.0, 0.5), dtype=torch.float64, device=dev)).all())
    for name in OUTPUTS:
        v = ref[name]
        assert bool(((v / UNIT) == (v / UNIT).round()).all()), f"{name} is not a multiple of 1/8"
        assert torch.equal(v.float().double(), v), f"{name} is not an fp32 value"
    # sums of absolute terms, per output element
    aK = K.abs()
    dp_hi, dp_lo = bf16_pieces(ref["dP"], 2)
    h_hi, h_lo = bf16_pieces(ref["H"], 2)
    assert torch.equal(dp_hi + dp_lo, ref["dP"]), "dP does not fit two bf16 pieces"
    assert torch.equal(h_hi + h_lo, ref["H"]), "H does not fit two bf16 pieces"
    assert float(ref["dP"].abs().max()) / UNIT < 2 ** 16 and float(ref["H"].abs().max()) / UNIT < 2 ** 16
    assert torch.equal(bf16_pieces(X, 1)[0], X) and torch.equal(bf16_pieces(ref["dQ"], 1)[0], ref["dQ"]), \
        "X or scale g does not fit one bf16 piece"
    sums = {"P": X.abs() @ aK.t(),
            "out": abs(c.scale) * (ref["H"].abs() @ aK) + (0 if base is None else base.abs()),
            "dH": ref["dQ"].abs() @ aK.t(),
            "g_beta": ref["dN"].abs().sum(dim=0), "g_gamma": (ref["dN"] * ref["xhat"]).abs().sum(dim=0),
            "gX": ref["dP"].abs() @ aK,
            # the gradient of K as its piece products: the same bound covers the fp32-MFMA kernel (|hi| + |lo| >= |hi + lo|)
            "gK": (dp_hi.abs() + dp_lo.abs()).t() @ X.abs() + (h_hi.abs() + h_lo.abs()).t() @ ref["dQ"].abs()}
    worst = max(float(v.max()) for v in sums.values()) / UNIT
    assert worst < 2 ** 24, {k: float(v.max()) / UNIT for k, v in sums.items()}
    return worst


@functools.lru_cache(maxsize=None)
def exact_case(B, D, variant):
    """(inputs, fp64 reference) of an exact case on the CPU, its conditions checked; shared and never modified"""
    c = exact_layer(B, D, variant)
    ref = reference(c)
    assert_exact(c, ref)
    return c, ref


#: one case of a GPU grid: the path it is named after and what pde_sym_layer_path must report for it
#:   env: the PDE_RH_* switches the case sets (a tuple of (name, value)); workspace: whether one is passed;
#:   dk: the kernel of the gradient of K the case selects (None: whichever the process's PDE_RH_NO_SPLIT gives)
Case = collections.namedtuple("Case", "family B D split waves blocks workspace env dk variant")
FAMILY_NAME = {STRIP32: "strip32", STRIP16: "strip16", ROW_BLOCKS: "rowblocks"}


def case_id(c):
    s = f"{FAMILY_NAME[c.family]}-B{c.B}-D{c.D}"
    if c.family == STRIP32:
        s += f"-S{c.split}-w{c.waves}"
    if c.family == ROW_BLOCKS:
        s += f"-blocks{c.blocks}"
    if not c.workspace:
        s += "-nows"
    for k, v in c.env:
        s += "-" + k[len("PDE_RH_"):].lower() + (v if k == "PDE_RH_SPLIT" else "")
    if c.dk is not None:
        s += "-dk" + ("split3" if c.dk == DK_SPLIT3 else "f32")
    return s


def _waves(B):
    return 2 if B <= 64 else 4


def strip32_case(B, D, S, env=()):
    return dict(family=STRIP32, B=B, D=D, split=S, waves=_waves(B), blocks=1, workspace=True, env=env, dk=None)


def strip16_case(B, D, workspace=True, env=()):
    return dict(family=STRIP16, B=B, D=D, split=0, waves=8, blocks=1, workspace=workspace, env=env, dk=None)


def row_blocks_case(B, D):
    return dict(family=ROW_BLOCKS, B=B, D=D, split=0, waves=8, blocks=(B + 127) // 128, workspace=True, env=(), dk=None)


def _numbered(cases):
    return [Case(variant=i, **c) for i, c in enumerate(cases)]


STRIP32_BATCHES = (1, 31, 32, 33, 63, 64, 65, 96, 127, 128)
STRIP16_BATCHES = (1, 15, 16, 17, 127, 128)
NO_WORKSPACE_SHAPES = ((33, 128, 2), (128, 128, 2), (33, 512, 8), (128, 512, 8))          # (B, D, the split of the STRIP32 twin)
CAP_CASE = (65, 4608, 4)                                    # (4608 / 32) * 8 = 1152 workgroups > 1024 with four waves


def exact_cases():
    """The exact grid of tests/test_gpu_rh_paths.py, (a): every family, split, wave count and block count."""
    cs = []
    # 32-column strips: S = 2, 4, 8 are three trip shapes of strip32_sum (four tiles per trip); D = 384 is S = 2 with three
    # slab pairs per slice; both wave counts with full, ragged and nearly empty waves
    for D, S in ((128, 2), (256, 4), (512, 8), (384, 2)):
        cs += [strip32_case(B, D, S) for B in STRIP32_BATCHES]
    cs += [strip32_case(B, 768, 4) for B in (33, 64, 65, 128)]
    cs += [strip32_case(B, 1024, 16, env=(("PDE_RH_SPLIT", "16"),)) for B in (33, 65)]
    cs += [strip32_case(B, 512, 2, env=(("PDE_RH_SPLIT", "2"),)) for B in (33, 128)]
    # one workgroup per 16-column strip: the widths that do not split, no workspace, the switch
    for D in (64, 192, 320):
        cs += [strip16_case(B, D) for B in STRIP16_BATCHES]
    cs += [strip16_case(B, D, workspace=False) for B, D, _ in NO_WORKSPACE_SHAPES]
    cs += [strip16_case(B, D, env=(("PDE_RH_NO_STRIP32", "1"),)) for B, D, _ in NO_WORKSPACE_SHAPES]
    # row blocks: one row in the last block, whole multiples of 128, three and four blocks
    for B in (129, 256, 257, 385):
        cs += [row_blocks_case(B, D) for D in (64, 128, 320)]
    return _numbered(cs)


def cap_case():
    B, D, S = CAP_CASE
    return Case(variant=0, **strip32_case(B, D, S))


def dk_cases():
    """Both kernels of the gradient of K at ragged 192-wide tiles (D = 192 is the only whole one; D = 64 a third of one)
    and ragged 16-row contraction groups (B = 1 and 15 leave the slab mostly zero rows)."""
    cs = []
    for D in (64, 128, 192, 256, 320, 384):
        for B in (1, 15, 16, 17, 33):
            S = {64: 0, 128: 2, 192: 0, 256: 4, 320: 0, 384: 2}[D]
            for dk in (DK_SPLIT3, DK_MFMA_F32):
                base = strip32_case(B, D, S) if S else strip16_case(B, D)
                base["dk"] = dk
                base["env"] = (("PDE_RH_NO_SPLIT", "1"),) if dk == DK_MFMA_F32 else ()
                cs.append(base)
    # the two kernels of one shape share a variant: one reference serves both
    return [Case(variant=i // 2, **c) for i, c in enumerate(cs)]


# --------------------------------------------------------------------------------------------------- general cases
#: one shape per family and wave count, with the plan each is meant to have
GENERAL_CASES = _numbered([strip16_case(5, 64), strip32_case(33, 128, 2), strip32_case(64, 256, 4), strip32_case(65, 512, 8),
                           strip32_case(128, 768, 4), strip16_case(100, 192), strip16_case(128, 512, workspace=False),
                           row_blocks_case(129, 128), row_blocks_case(257, 320)])
GENERAL_MODES = (("relu", True), ("tanh", True), ("tanh", False))
OFFSET_CASES = _numbered([strip32_case(33, 128, 2), strip16_case(100, 192), row_blocks_case(129, 128)])
#: (b): shapes whose calls use a workspace (exact, exact, general values), and two that never do, run twice for determinism
WORKSPACE_CASES = _numbered([strip32_case(33, 128, 2), strip32_case(128, 512, 8), strip32_case(65, 512, 8)])
NO_WORKSPACE_TWICE_CASES = _numbered([strip16_case(100, 192), row_blocks_case(129, 128)])
#: (e): one exact case per family through functional.sym_layer (variants 1, 3, 5: ReLU; with, without, with a base)
WRAPPER_CASES = [Case(variant=v, **c) for v, c in ((1, strip32_case(33, 128, 2)), (3, strip16_case(17, 192)),
                                                   (5, row_blocks_case(129, 128)))]
OFFSET_RATIO = 100.0


def _round32(v):
    return v.float().double()


@functools.lru_cache(maxsize=None)
def general_layer(B, D, act, training, momentum=0.1, offset=False):
    """Seeded normal data generated in fp64 and rounded to fp32 once.  K = I + N(0, 1/4D): well conditioned, every
    column of P has a standard deviation near 1.1.  ``offset``: X gets a common row o with K o = +-100 |K_j| — the column
    means of P are then about 100 times their standard deviations."""
    gen = torch.Generator().manual_seed(4000 + 31 * B + D + (7 if offset else 0))
    rn = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    K = _round32(torch.eye(D, dtype=torch.float64) + (0.5 / D ** 0.5) * rn(D, D))
    X = rn(B, D)
    if offset:
        sign = 2.0 * torch.randint(0, 2, (D,), generator=gen).double() - 1.0
        X = X + torch.linalg.solve(K, OFFSET_RATIO * sign * K.norm(dim=1))
    gamma, beta = _round32(1 + 0.3 * rn(D)), _round32(0.2 * rn(D))
    rm, rv = _round32(0.3 * rn(D)), _round32(0.5 + torch.rand(D, generator=gen, dtype=torch.float64))
    return Layer(_round32(X), K, gamma, beta, rm, rv, _round32(rn(B, D)), 0.7, _round32(rn(B, D)), act, training, momentum,
                 eps=1e-5)


@functools.lru_cache(maxsize=None)
def general_case(B, D, act, training, momentum=0.1, offset=False):
    c = general_layer(B, D, act, training, momentum, offset)
    return c, reference(c)
