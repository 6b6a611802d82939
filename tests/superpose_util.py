"""Full-size layer calls against the fp64 oracle by superposition (tests/test_gpu_fullsize_oracle.py; the method itself is
tested in tests/test_superposition_oracle.py).

Every PDE layer of the benchmark's configurations is linear in its input u (the clamps act on the coefficients, the
channel operators and the skip blend are linear maps of each sample).  So a batch built as

    u_b = sum_k W[b,k] E_k,    gy_b = sum_l V[b,l] F_l          (K basis samples E, F of shape (C, N, N))

has    y_b = sum_k W[b,k] L(E_k),    gu_b = sum_l V[b,l] L^T(F_l),
and every parameter gradient is  sum_k d/dtheta <G_k, L_theta E_k>  with  G = (W^T V) F  (bilinear in u and gy).

The fp64 oracle then needs to see 2K samples at any batch size: one call on (E, F) for the basis outputs, one on (E, G)
per (W, V) for the parameter gradients.  The inputs are exact in the dtype the layer sees (multiples of 2^-10 and
integer weights for fp32, multiples of 1/8 and weights from {0, +-1, +-2, +-4} for bf16), so the superposition holds
exactly and the only distance left is the kernels' own rounding.

Rows of W (and of V) are distinct over any window of fewer than `distinct_rows(dtype)` samples (at least 342): a kernel
that reads or writes the plane of another sample, chunk or pass gets the wrong combination, and that shows."""
import itertools

import torch

from oracle import pde_oracle as O

# per dtype: basis size K, the values a weight may take, the grid of basis entries (scale) and their integer range
SETUP = {
    torch.float32: dict(K=4, weights=(-3, -2, -1, 0, 1, 2, 3), scale=2.0 ** -10, lo=-4096, hi=4095),
    torch.bfloat16: dict(K=3, weights=(-4, -2, -1, 0, 1, 2, 4), scale=1.0 / 8, lo=-16, hi=16),
}


def basis(dtype, C, N, seed, K=None):
    """(E, F): two float64 tensors (K, C, N, N) whose entries are exact in ``dtype`` (and every weighted sum of them is)."""
    s = SETUP[dtype]
    K = K or s["K"]
    g = torch.Generator().manual_seed(seed)
    draw = lambda: torch.randint(s["lo"], s["hi"] + 1, (K, C, N, N), generator=g).double() * s["scale"]
    return draw(), draw()


def distinct_rows(dtype, K=None):
    s = SETUP[dtype]
    return len(s["weights"]) ** (K or s["K"]) - 1


def weights(dtype, B, seed, K=None):
    """(B, K) float64 integer weights: the nonzero rows of the value grid in a seeded order, repeated with period
    ``distinct_rows`` — no two samples less than that many indices apart share a row."""
    s = SETUP[dtype]
    K = K or s["K"]
    rows = torch.tensor([r for r in itertools.product(s["weights"], repeat=K) if any(r)], dtype=torch.float64)
    g = torch.Generator().manual_seed(seed)
    rows = rows[torch.randperm(rows.shape[0], generator=g)]
    return rows[torch.arange(B) % rows.shape[0]]


def compose(E, W, dtype, device="cpu"):
    """sum_k W[:, k] E_k as a (B, C, N, N) tensor of ``dtype`` on ``device``: elementwise multiply-adds in fp32 (every
    product and partial sum is exact there), then one exact cast."""
    K = E.shape[0]
    Ed = E.to(device=device, dtype=torch.float32)
    Wd = W.to(device=device, dtype=torch.float32)
    u = torch.zeros((W.shape[0],) + tuple(E.shape[1:]), dtype=torch.float32, device=device)
    for k in range(K):
        u.addcmul_(Wd[:, k].view(-1, 1, 1, 1), Ed[k])
    del Ed
    return u if dtype == torch.float32 else u.to(dtype)


def exact_sum(E, W, rows=None):
    """float64 sum_k W[rows, k] E_k on E's device (the reference of ``compose`` and of the reconstruction)."""
    Wr = W if rows is None else W[rows]
    Wr = Wr.to(device=E.device, dtype=torch.float64)
    out = Wr[:, 0].view(-1, 1, 1, 1) * E[0]
    for k in range(1, E.shape[0]):
        out.addcmul_(Wr[:, k].view(-1, 1, 1, 1), E[k])
    return out


class Basis:
    """The oracle's view of one layer ``fn(u, params)`` (float64 parameters) on the basis (E, F): the basis outputs
    L(E_k) and L^T(F_l) once, the parameter gradients per weight pair (W, V) on demand."""

    def __init__(self, fn, params, E, F):
        self.fn, self.E, self.F = fn, E, F
        self.params = {k: v.detach().double().cpu() for k, v in params.items()}
        y, gu, _ = O.value_and_grads(fn, E, self.params, F)
        self.Y, self.GU = y.detach(), gu.detach()
        self._grads = {}
        self._dev = {}

    def grads(self, W, V):
        """{name: float64 gradient} of sum_b <gy_b, L(u_b)> (None where the layer does not use the parameter)."""
        key = (W.numpy().tobytes(), V.numpy().tobytes())
        if key not in self._grads:
            M = W.t() @ V                                             # (K, K), integers: exact
            G = torch.einsum("kl,lchw->kchw", M, self.F)
            self._grads[key] = O.value_and_grads(self.fn, self.E, self.params, G)[2]
        return self._grads[key]

    def on(self, device):
        """(Y, GU) as float64 tensors on ``device``."""
        if device not in self._dev:
            self._dev = {device: (self.Y.to(device), self.GU.to(device))}
        return self._dev[device]


def sliced_rel_err(got, W, Yb, rows=256):
    """golden_util.rel_err(got, sum_k W[:, k] Yb[k]) — max |a - b| / max |b| over the whole batch — with the float64
    reference built ``rows`` samples at a time on got's device."""
    num = den = 0.0
    for s in range(0, got.shape[0], rows):
        sl = slice(s, min(s + rows, got.shape[0]))
        ref = exact_sum(Yb, W, sl)
        num = max(num, float((got[sl].double() - ref).abs().max()))
        den = max(den, float(ref.abs().max()))
        del ref
    return num / den if den else num


def errors(basis_, W, V, y, gu, param_grads):
    """{"y", "gu", "g_<name>"}: rel_err of the layer's outputs against the superposed oracle.  ``param_grads``: {name:
    gradient} of the parameters that received one."""
    Yb, GUb = basis_.on(y.device)
    errs = {"y": sliced_rel_err(y, W, Yb), "gu": sliced_rel_err(gu, V, GUb)}
    ref = basis_.grads(W, V)
    assert set(param_grads) == {n for n, r in ref.items() if r is not None}, (sorted(param_grads), sorted(ref))
    for n, g in param_grads.items():
        r = ref[n]
        assert r is not None, n
        a = g.detach().double().cpu().reshape(r.shape)
        den = float(r.abs().max())
        d = float((a - r).abs().max())
        errs["g_" + n] = d / den if den else d
    return errs
