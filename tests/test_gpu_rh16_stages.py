"""Every kernel of the 16-bit Ruthotto-Haber symmetric layer (csrc/pde_rh.hip: rh_part16, rh_fwd16_epi, rh_out16_epi,
rh_bwd16_epi, rh_outer16, rh_k_to_f16) through the C ABI (pde_sym_layer_f16_* / pde_sym_layer_bf16_* / pde_sym_k_to_*), in both
types, against the header's contract written out in fp64 (tests/rh16_cases.py; tests/test_rh16_cases.py checks that ground,
and that its comparisons refuse subtly wrong evaluations, on the CPU).

Every call writes into NaN-patterned outputs and a NaN-filled workspace of exactly pde_sym_layer_*_workspace_bytes, and
every tensor the two entry points write is compared: P, H, mean, invstd, out, the running statistics, dP, gX, gK, g_gamma,
g_beta — and K16 from pde_sym_k_to_*, bitwise against K.to(dtype), in every case and at ties, fp16 subnormals, values
beyond 65504 and -0.

(a) Exact cases: the tensors of the case's bitwise set (all of them in the narrow grid) are equal to the contract — 16-bit
    ones as bit patterns, fp32 ones torch.equal; the others of a wide case are held by (b).  The backward runs once on the
    kernel's own saved P, H, mean, invstd and once on the contract's; the two give the same bits.  One fp16 case overflows
    one element of P: +-inf and non-finite values exactly where the contract has them.
(b) General values, stage by stage (rh16_cases.check_stages): each stage in fp64 from the kernel's own upstream tensors;
    16-bit outputs inside [r(v - m), r(v + m)], m = 4 x the largest deviation of plain fp32 torch on the GPU at that
    stage, at most a quarter of the elements of P, N, H and Q two-ended; fp32 outputs within max(3e-6, 2 x plain) of fp64.
(c) Protocol: the same calls twice with the workspace NaN-filled in between give the same bits; functional.sym_layer on
    both host paths equals the ABI bit for bit, on one exact case per wave count.

The 16-bit path has no environment switches.  Measured figures: DESIGN.md §5."""
import ctypes as C

import pytest
import torch

import rh16_cases as S
import rh_cases as R
import test_gpu_rh_paths as TP

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: S.TAG[d])
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from cnn_with_pde_amd import _lib as L
    return L.load()


def _fn(lib, dtype, what):
    return getattr(lib, f"pde_sym_layer_{S.TAG[dtype]}_{what}")


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _k16(lib, dtype, K):
    D = K.shape[0]
    K16 = _nan(D, D, dtype=dtype)
    rc = getattr(lib, f"pde_sym_k_to_{S.TAG[dtype]}")(D, _ptr(K), _ptr(K16), TP._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return K16


def _same_patterns(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


class Device:
    """The fp32 inputs of a layer on the GPU and K16 as the library makes it — compared with K.to(dtype) bit for bit."""

    def __init__(self, lib, dtype, c):
        up = lambda v: None if v is None else v.float().cuda().contiguous()
        self.c, self.dtype = c, dtype
        self.X, self.K, self.gamma, self.beta, self.base, self.g = up(c.X), up(c.K), up(c.gamma), up(c.beta), up(c.base), up(c.g)
        self.running_mean, self.running_var = up(c.running_mean), up(c.running_var)
        self.K16 = _k16(lib, dtype, self.K)
        assert _same_patterns(self.K16.cpu(), c.K.float().to(dtype)), "K16 is not r(K)"


def _workspace(lib, dtype, B, D):
    """NaN-filled, of exactly the size the library asks for"""
    n = _fn(lib, dtype, "workspace_bytes")(B, D)
    assert n == (D // 32) * S.split16(D) * (2 if B <= 64 else 4) * 1024 * 4
    return _nan(n // 4)


def _forward(lib, d, ws=None):
    c, dtype = d.c, d.dtype
    B, D = c.B, c.D
    ws = _workspace(lib, dtype, B, D) if ws is None else ws
    o = {"P": _nan(B, D, dtype=dtype), "H": _nan(B, D, dtype=dtype), "mean": _nan(D), "invstd": _nan(D),
         "out": _nan(B, D, dtype=dtype if c.base is None else torch.float32)}
    rm = None if d.running_mean is None else d.running_mean.clone()
    rv = None if d.running_var is None else d.running_var.clone()
    rc = _fn(lib, dtype, "forward")(B, D, R.ACT_CODE[c.act], 1 if c.training else 0, _ptr(d.X), _ptr(d.K16), _ptr(d.gamma),
                                    _ptr(d.beta), _ptr(rm), _ptr(rv), c.momentum, c.eps, _ptr(d.base), c.scale, _ptr(o["P"]),
                                    _ptr(o["H"]), _ptr(o["mean"]), _ptr(o["invstd"]), _ptr(o["out"]), _ptr(ws), ws.numel() * 4,
                                    TP._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    o["running_mean"], o["running_var"] = rm, rv
    return o


def _backward(lib, d, saved, ws=None):
    c, dtype = d.c, d.dtype
    B, D = c.B, c.D
    ws = _workspace(lib, dtype, B, D) if ws is None else ws
    o = {"dP": _nan(B, D, dtype=dtype), "gX": _nan(B, D), "gK": _nan(D, D), "g_gamma": _nan(D), "g_beta": _nan(D)}
    rc = _fn(lib, dtype, "backward")(B, D, R.ACT_CODE[c.act], 1 if c.training else 0, _ptr(d.g), c.scale, _ptr(d.X), _ptr(d.K16),
                                     _ptr(d.gamma), _ptr(saved["P"]), _ptr(saved["H"]), _ptr(saved["mean"]), _ptr(saved["invstd"]),
                                     _ptr(o["dP"]), _ptr(o["gX"]), _ptr(o["gK"]), _ptr(o["g_gamma"]), _ptr(o["g_beta"]), _ptr(ws),
                                     ws.numel() * 4, TP._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return o


def _run(lib, d):
    got = _forward(lib, d)
    got.update(_backward(lib, d, got))
    return got


def _bitwise(a, b, names, what):
    for name in names:
        if a[name] is None:
            assert b[name] is None, name
            continue
        view = torch.int16 if a[name].element_size() == 2 else torch.int32
        assert torch.equal(a[name].view(view), b[name].view(view)), f"{what}: {name}"


BACKWARD = ("dP", "gX", "gK", "g_gamma", "g_beta")


# =========================================================================================== K16
@DT
def test_k16_is_r_of_k_at_ties_subnormals_overflow_and_minus_zero(dtype, lib):
    D = 64
    gen = torch.Generator().manual_seed(16)
    K = torch.randn(D, D, generator=gen) * torch.exp2(torch.randint(-26, 18, (D, D), generator=gen).float())
    h, b = 2.0 ** -11, 2.0 ** -8                            # half a step of fp16 and of bf16 at 1
    special = [1 + h, 1 + 3 * h, -(1 + h), 1 + b, 1 + 3 * b, -(1 + b), 1 + h / 2, 1 + b / 2,            # ties and near them
               2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, -(2.0 ** -25), 3e-6, 6.2e-5, 2.0 ** -14 - 2.0 ** -25,
               65504.0, 65519.996, 65520.0, -65520.0, 65536.0, 7e4, -1e6, 3e38, -0.0, 0.0]
    K.view(-1)[:len(special)] = torch.tensor(special, dtype=torch.float32)
    want = K.to(dtype)
    if dtype == torch.float16:
        assert int(torch.isinf(want).sum()) > 5 and int(((want != 0) & (want.abs() < 2.0 ** -14)).sum()) > 100
    assert int((want.view(torch.int16) == -32768).sum()) >= 1                             # -0 keeps its sign
    got = _k16(lib, dtype, K.cuda())
    bad = got.cpu().view(torch.int16) != want.view(torch.int16)
    assert not bool(bad.any()), (int(bad.sum()), K[bad][:8].tolist(), got.cpu()[bad][:8].tolist(), want[bad][:8].tolist())


# =========================================================================================== (a) exact cases
def _saved_of(ref, dtype):
    return {"P": ref["P"].to(dtype).cuda(), "H": ref["H"].to(dtype).cuda(), "mean": ref["mean"].float().cuda(),
            "invstd": ref["invstd"].float().cuda()}


def _exact(lib, dtype, c, layer, ref, held, device="cpu"):
    d = Device(lib, dtype, layer)
    got = _run(lib, d)
    what = f"{S.TAG[dtype]} {S.case_id(c)}"
    S.compare_exact(layer, got, ref, held, dtype, what)
    assert {"P", "H", "mean", "invstd"} <= held             # then the contract's saved tensors are the kernel's own
    again = _backward(lib, d, _saved_of(ref, dtype))
    _bitwise(again, got, BACKWARD, what + ", backward on the contract's saved tensors")
    if held != frozenset(S.OUTPUTS):
        S.check_stages(layer, dtype, got, "cuda", what)
    return got


@DT
@pytest.mark.parametrize("c", S.narrow_cases(), ids=S.case_id)
def test_exact_narrow(c, dtype, lib):
    layer, ref, held = S.exact_case(c.family, c.B, c.D, c.variant, dtype)
    assert held == frozenset(S.OUTPUTS)
    _exact(lib, dtype, c, layer, ref, held)


@DT
@pytest.mark.parametrize("c", S.wide_cases(), ids=S.case_id)
def test_exact_wide(c, dtype, lib):
    layer, ref, held = S.exact_case(c.family, c.B, c.D, c.variant, dtype)
    _exact(lib, dtype, c, layer, ref, held)


@DT
def test_exact_at_the_workload_shape(dtype, lib):
    """(64, 3072): S = 8 with six slabs per slice; the fp64 products of the contract are taken on the GPU (exact either way)"""
    c = S.workload_case()
    layer = S.exact_layer(c.family, c.B, c.D, c.variant, dtype)
    ref = S.contract(layer, dtype, device="cuda")
    held = S.assert_exact(layer, ref, dtype)
    assert held == frozenset(S.OUTPUTS)
    _exact(lib, dtype, c, layer, ref, held)


def test_fp16_overflow_of_one_element_of_P(lib):
    """P and H carry +-inf exactly where the contract does; every other tensor is non-finite at exactly the contract's
    positions (0 inf is NaN on the matrix cores as in the contract) and equal elsewhere"""
    layer, ref, held = S.overflow_case()
    d = Device(lib, torch.float16, layer)
    got = _run(lib, d)
    S.compare_exact(layer, got, ref, held, torch.float16, "fp16 overflow")
    assert int(torch.isinf(got["P"]).sum()) == 1 and bool(torch.isinf(got["P"][S.OVERFLOW_ROW, S.OVERFLOW_COL]))
    again = _backward(lib, d, _saved_of(ref, torch.float16))
    S.compare_exact(layer, {**got, **again}, ref, held, torch.float16, "fp16 overflow, backward on the contract's saved tensors")


# =========================================================================================== (b) general values
@DT
@pytest.mark.parametrize("v", S.general_cases(), ids=S.general_id)
def test_general_values_stage_by_stage(v, dtype, lib):
    layer = S.general_layer(*v)
    d = Device(lib, dtype, layer)
    got = _run(lib, d)
    what = f"{S.TAG[dtype]} {S.general_id(v)}"
    fig = S.check_stages(layer, dtype, got, "cuda", what)
    print(what, " ".join(f"{k} m {a:.2e} two-ended {b:.2%};" for k, (a, b) in fig.items() if k in ("P", "N", "H", "Q", "dP")),
          " ".join(f"{k} {a:.2e}/{b:.2e};" for k, (a, b) in fig.items() if k not in ("P", "N", "H", "Q", "dP")))
    if not v[5]:
        assert got["running_mean"] is None and got["running_var"] is None
        tracked = _run(lib, Device(lib, dtype, S.general_layer(*v[:5], True)))
        _bitwise(got, tracked, [n for n in S.OUTPUTS if not n.startswith("running")], what + " against the tracked call")


# =========================================================================================== (c) protocol
TWICE = (("exact", 33, 128), ("exact", 128, 512), ("general", 65, 512), ("general", 100, 1024))


@DT
@pytest.mark.parametrize("kind,B,D", TWICE)
def test_nothing_is_read_from_the_workspace_before_it_is_written(kind, B, D, dtype, lib):
    layer = R.exact_layer(B, D, 1) if kind == "exact" else S.general_layer(B, D, "tanh", True)
    d = Device(lib, dtype, layer)
    ws = _workspace(lib, dtype, B, D)
    runs = []
    for _ in range(2):
        ws.fill_(NAN)
        got = _forward(lib, d, ws)
        ws.fill_(NAN)
        got.update(_backward(lib, d, got, ws))
        runs.append(got)
    for name in S.OUTPUTS:
        assert not bool(torch.isnan(runs[0][name]).any()), name
    _bitwise(runs[0], runs[1], S.OUTPUTS, "the same call twice")


WRAPPER = (("narrow", 33, 128), ("narrow", 65, 192))       # two waves, four waves


@DT
@pytest.mark.parametrize("host", ["ctypes", "host_ext"])
@pytest.mark.parametrize("family,B,D", WRAPPER)
def test_sym_layer_wrapper_equals_the_c_abi(family, B, D, host, dtype, lib, monkeypatch):
    from cnn_with_pde_amd import _lib as L
    from cnn_with_pde_amd import functional as F_
    (c,) = [c for c in S.narrow_cases() if (c.B, c.D) == (B, D)]
    assert c.waves == (2 if B <= 64 else 4)
    if host == "ctypes":
        monkeypatch.setattr(L, "host_ext", lambda: None)
    else:
        assert L.host_ext() is not None, "the native host path is not loaded in this process"
    layer, ref, held = S.exact_case(c.family, c.B, c.D, c.variant, dtype)
    d = Device(lib, dtype, layer)
    direct = _run(lib, d)
    bn = TP._bn(layer, D)
    X, K = d.X.clone().requires_grad_(True), d.K.clone().requires_grad_(True)
    base = None if d.base is None else d.base.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=dtype):
        K16 = F_.sym_k16(K, dtype)
        assert _same_patterns(K16, d.K16)
        out = F_.sym_layer(X, K, bn, layer.act, base=base, scale=layer.scale, K16=K16)
    assert out.dtype == (dtype if base is None else torch.float32)
    out.backward(d.g.to(out.dtype))
    torch.cuda.synchronize()
    got = {"out": out.detach(), "gX": X.grad, "gK": K.grad, "g_gamma": bn.weight.grad, "g_beta": bn.bias.grad,
           "running_mean": bn.running_mean, "running_var": bn.running_var}
    _bitwise(got, direct, list(got), f"sym_layer ({host})")
    S.compare_exact(layer, {**direct, **got}, ref, held, dtype, f"sym_layer ({host})")
    if base is not None:
        assert torch.equal(base.grad, d.g)
