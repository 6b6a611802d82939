"""The explicit family over plane SHAPES and I/O types: the 5-point layer (pde_explicit5_*: wave-per-plane kernels at
64x64 / 32x32 / 16x16, the generic float4 kernel at other widths that are multiples of 4, the scalar-column kernel at every
other width), the one-workgroup and the tiled Jacobi kernels, and the float64 entry points of both — non-square planes,
planes next to the dispatch thresholds, minimal planes, widths that are not a multiple of 4, against the CPU oracle
(oracle/pde_oracle.py: tiny_forward, jacobi_forward take any H x W in any dtype), bit for bit where the arithmetic is
exact, and the narrow types against the fp32 route.  Nothing here is meant to make a kernel fault: shapes the library
refuses are checked through the return code / PdeError, which come back before any launch."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import golden_util as G
import test_gpu_jacobi_tiled as JT
from oracle import pde_oracle as O
from test_gpu_f16 import _fn_runs, max_ulps
from test_gpu_f64 import TOL as TOL64       # the float64 layers' bar against the float64 oracle
from test_gpu_jacobi_tiled import _cabi, _ord16
from test_gpu_parity import TOL             # 1e-5

pytestmark = pytest.mark.gpu

# ---- 1. explicit 5-point layer ----------------------------------------------------------------------------------------
EX_SHAPES = [(8, 12), (12, 8), (4, 64), (64, 4), (20, 36), (1, 4), (4, 4),                                  # non-square
             (16, 16), (16, 32), (32, 16), (32, 32), (64, 32), (32, 64), (64, 64), (60, 64), (64, 68), (128, 128),  # dispatch
             (30, 30), (7, 9), (5, 1), (33, 31), (64, 62)]                                                  # W % 4 != 0
EX_IDS = [f"{h}x{w}" for h, w in EX_SHAPES]
# B x C ragged against the 4 planes a workgroup of the wave kernels takes: 7, 6 and 15 planes
EX_BC = [(1, 7), (1, 6), (3, 5)]
EX_DT, EX_EPS, EX_MAXC, EX_RELAX = 0.5, 1e-6, 0.125, 0.1      # max_coeff: the same number in every type
# exactly on max_coeff, below eps, above max_coeff, four inside: the clamp mask of explicit5_pgrad_kernel
EX_ALPHA = [0.125, 1e-7, 0.3, 0.05, 0.11, 0.124, 0.08]


def _ex_case(H, W, dtype=torch.float32):
    """(u, gy, alpha_base, channel_scaling), every value exact in fp16 and in bf16 where ``dtype`` is one of them"""
    B, Cc = EX_BC[EX_SHAPES.index((H, W)) % len(EX_BC)] if (H, W) in EX_SHAPES else (2, 5)
    g = torch.Generator().manual_seed(10000 * H + W)
    u = torch.randn(B, Cc, H, W, generator=g)
    gy = torch.randn(B, Cc, H, W, generator=g)
    a = torch.tensor(EX_ALPHA[:Cc])
    s = 1 + 0.3 * torch.randn(Cc, generator=g)
    if dtype in (torch.float16, torch.bfloat16):
        u, gy, a, s = (t.to(dtype).float() for t in (u, gy, a, s))
        assert float(a[0]) == EX_MAXC and float(a[1]) < EX_EPS
    return u, gy, a, s


def _ex_oracle(u, gy, a, s, steps, dtype, relax=EX_RELAX, dt=EX_DT, eps=EX_EPS, maxc=EX_MAXC):
    y, gu, gp = O.value_and_grads(
        lambda x, p: O.tiny_forward(x, p, dt=dt, num_steps=steps, eps=eps, max_coeff=maxc, relax=relax), u.to(dtype),
        {"alpha_base": a.to(dtype), "channel_scaling": s.to(dtype)}, gy.to(dtype))
    return y, gu, gp["alpha_base"], gp["channel_scaling"]


def _ex_fn(steps, relax=EX_RELAX, dt=EX_DT, eps=EX_EPS, maxc=EX_MAXC):
    import cnn_with_pde_amd as P
    return lambda u, a, s: P.explicit5_step(u, a, s, dt, eps, maxc, relax, steps)


def _ex_gpu(u, gy, a, s, steps, **kw):
    """through the module, in the tensors' own type: (y, gu, g_alpha_base, g_channel_scaling)"""
    y, gu, gp = _fn_runs(_ex_fn(steps, **kw), u.cuda(), [a.cuda(), s.cuda()], gy.cuda())
    return y, gu, gp[0], gp[1]


def _ex_cabi(io_dtype, u, gy, a, s, steps):
    """pde_explicit5_forward / _backward on tensors of any of the three I/O types (a, s and their gradients fp32)"""
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    B, Cc, H, W = u.shape
    p = lambda t: C.c_void_p(t.data_ptr())                                                  # noqa: E731
    fp = lambda t: C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_float))                   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out, gu = torch.empty_like(u), torch.empty_like(u)
    ga, gs = torch.empty_like(a), torch.empty_like(s)
    states = torch.empty((max(steps - 1, 1),) + tuple(u.shape), dtype=torch.float32, device="cuda")
    assert lib.pde_explicit5_forward(B, Cc, H, W, io_dtype, p(u), fp(a), fp(s), EX_DT, EX_EPS, EX_MAXC, EX_RELAX, steps,
                                     p(states), p(out), st) == 0
    nb = lib.pde_explicit5_backward_workspace_bytes(B, Cc, H, W, io_dtype, steps)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    assert lib.pde_explicit5_backward(B, Cc, H, W, io_dtype, p(u), p(states), p(gy), fp(a), fp(s), EX_DT, EX_EPS, EX_MAXC,
                                      EX_RELAX, steps, p(gu), fp(ga), fp(gs), p(ws), nb, st) == 0
    torch.cuda.synchronize()
    return out, gu, ga, gs


def _first_diff(got, want):
    """the first differing index of two tensors of one shape, with both values (for a failing exact comparison)"""
    bad = (got != want).nonzero()
    if bad.numel() == 0:
        return None
    i = tuple(int(x) for x in bad[0])
    return i, float(got[i]), float(want[i]), int(bad.shape[0])


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("H,W", EX_SHAPES, ids=EX_IDS)
def test_explicit_f32_vs_oracle(H, W, steps):
    u, gy, a, s = _ex_case(H, W)
    ref = _ex_oracle(u, gy, a, s, steps, torch.float32)
    got = [t.cpu() for t in _ex_gpu(u, gy, a, s, steps)]
    names = ("y", "gu", "g_alpha_base", "g_channel_scaling")
    errs = {n: G.rel_err(x, r) for n, x, r in zip(names, got, ref)}
    print((H, W, steps), errs)          # (5 to 7 channels; gradients of at most four entries: test_explicit_single_plane)
    bad = {n: v for n, v in errs.items() if not v <= TOL}
    assert not bad, (bad, errs)
    assert float(got[2][1]) == 0.0 and float(got[2][2]) == 0.0 and float(got[2][0]) != 0.0     # the clamp mask itself


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 4), (7, 9), (20, 36), (32, 32), (5, 1)], ids=lambda v: str(v))
def test_explicit_single_plane(H, W, steps):
    """B * C = 1: one plane in the whole call; its two gradients are single numbers, decided as test_gpu_fuzz.check_case
    decides gradients of at most four entries."""
    g = torch.Generator().manual_seed(77 * H + W)
    u, gy = torch.randn(1, 1, H, W, generator=g), torch.randn(1, 1, H, W, generator=g)
    a, s = torch.tensor([0.05]), torch.tensor([1.2])
    ref = _ex_oracle(u, gy, a, s, steps, torch.float32)
    ref64 = _ex_oracle(u, gy, a, s, steps, torch.float64)
    got = [t.cpu() for t in _ex_gpu(u, gy, a, s, steps)]
    errs = {"y": G.rel_err(got[0], ref[0]), "gu": G.rel_err(got[1], ref[1])}
    limits = {"y": TOL, "gu": TOL}
    for k, n in ((2, "g_alpha_base"), (3, "g_channel_scaling")):
        errs[n] = G.rel_err(got[k], ref64[k])
        limits[n] = max(2e-5, 4.0 * min(G.rel_err(ref[k], ref64[k]), 1e-4))
    print((H, W, steps), errs)
    bad = {n: (v, limits[n]) for n, v in errs.items() if not v <= limits[n]}
    assert not bad, (bad, errs)


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("H,W", EX_SHAPES, ids=EX_IDS)
def test_explicit_f16_vs_f32_route(H, W, steps):
    """fp16 through the module against the fp32 route on the same values: the gate of test_gpu_f16.py."""
    u, gy, a, s = _ex_case(H, W, torch.float16)
    y, gu, ga, gs = _ex_gpu(u.half(), gy.half(), a.half(), s.half(), steps)
    y32, gu32, ga32, gs32 = _ex_gpu(u, gy, a, s, steps)
    assert y.dtype == torch.float16 and gu.dtype == torch.float16 and y32.dtype == torch.float32
    print((H, W, steps), max_ulps(y, y32.half()), max_ulps(gu, gu32.half()))
    assert max_ulps(y, y32.half()) <= 1 and max_ulps(gu, gu32.half()) <= 1
    for g16, g32 in ((ga, ga32), (gs, gs32)):
        assert g16.dtype == torch.float16 and torch.equal(g16, g32.half()), (g16, g32)


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("H,W", EX_SHAPES, ids=EX_IDS)
def test_explicit_bf16_vs_f32_route(H, W, steps):
    """bf16 through the C ABI against the fp32 route on the same values: output and gu that route's rounded once (1 ulp);
    the parameter gradients are fp32 sums over the same widened values (what passes between the steps is fp32 in both
    routes), so they are that route's."""
    from cnn_with_pde_amd import _lib as L
    u, gy, a, s = (t.cuda() for t in _ex_case(H, W, torch.bfloat16))
    y, gu, ga, gs = _ex_cabi(L.PDE_IO_BF16, u.bfloat16(), gy.bfloat16(), a, s, steps)
    y32, gu32, ga32, gs32 = _ex_cabi(L.PDE_IO_F32, u, gy, a, s, steps)
    assert y.dtype == torch.bfloat16 and y32.dtype == torch.float32
    dy = int((_ord16(y) - _ord16(y32.bfloat16())).abs().max())
    dg = int((_ord16(gu) - _ord16(gu32.bfloat16())).abs().max())
    print((H, W, steps), dy, dg)
    assert dy <= 1 and dg <= 1
    assert torch.equal(ga, ga32) and torch.equal(gs, gs32), (ga, ga32, gs, gs32)
    # and the C ABI's fp32 route is the module's
    ym, gum, gam, gsm = _ex_gpu(u.cpu(), gy.cpu(), a.cpu(), s.cpu(), steps)
    assert torch.equal(ym, y32) and torch.equal(gum, gu32) and torch.equal(gam, ga32) and torch.equal(gsm, gs32)


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("H,W", EX_SHAPES, ids=EX_IDS)
def test_explicit_f64_vs_oracle(H, W, steps):
    u, gy, a, s = (t.double() for t in _ex_case(H, W))
    a = torch.tensor(EX_ALPHA[:a.numel()], dtype=torch.float64)        # 0.3, 0.05, ... as doubles, not widened floats
    ref = _ex_oracle(u, gy, a, s, steps, torch.float64)
    got = _ex_gpu(u, gy, a, s, steps)
    assert all(t.dtype == torch.float64 for t in got)
    errs = {n: G.rel_err(x.cpu(), r) for n, x, r in zip(("y", "gu", "g_alpha_base", "g_channel_scaling"), got, ref)}
    print((H, W, steps), errs)
    assert all(v <= TOL64 for v in errs.values()), errs
    assert float(got[2][1]) == 0.0 and float(got[2][2]) == 0.0 and float(got[2][0]) != 0.0


@pytest.mark.parametrize("H,W", [(20, 36), (32, 32), (33, 31), (7, 9)], ids=lambda v: str(v))
def test_explicit_exact(H, W):
    """Small integers in u and gy, channel_scaling 1, 2 and 1/2, alpha_base = 1/8 (the clamp inactive), dt = 1,
    relax = 1/2, three steps: every intermediate is a short dyadic number, fp32 is exact in any order of operations, so
    the results must equal the oracle's bit for bit on a non-square generic plane, a wave plane and two planes with
    W % 4 != 0 — a transposed index, a missed edge column or a ghost cell that is not zero fails whatever the tolerance."""
    steps, kw = 3, dict(relax=0.5, dt=1.0, eps=1e-6, maxc=1.0)
    g = torch.Generator().manual_seed(H * 1000 + W)
    u = torch.randint(-2, 3, (2, 3, H, W), generator=g).float()
    gy = torch.randint(-2, 3, (2, 3, H, W), generator=g).float()
    a, s = torch.full((3,), 0.125), torch.tensor([1.0, 2.0, 0.5])
    ref32 = _ex_oracle(u, gy, a, s, steps, torch.float32, **kw)
    ref64 = _ex_oracle(u, gy, a, s, steps, torch.float64, **kw)
    for r32, r64 in zip(ref32, ref64):                                  # the precondition
        assert torch.equal(r32.double(), r64)
    got = [t.cpu() for t in _ex_gpu(u, gy, a, s, steps, **kw)]
    for n, x, r in zip(("y", "gu", "g_alpha_base", "g_channel_scaling"), got, ref32):
        assert torch.equal(x, r), (n, "first (sample, channel, row, column), got, want, how many:", _first_diff(x, r))


@pytest.mark.parametrize("H,W", EX_SHAPES, ids=EX_IDS)
def test_explicit_dispatch_agreement(H, W):
    """Which planes stay in registers is decided twice: by the library (wave_plane_ok) and by the Python wrapper, which
    allocates `states` under torch.no_grad() only for planes it believes are NOT fused.  Three steps without gradients
    must succeed and equal the same call with gradients enabled, bit for bit."""
    u, _, a, s = _ex_case(H, W)
    fn = _ex_fn(3)
    ud, ad, sd = u.cuda(), a.cuda(), s.cuda()
    with torch.no_grad():
        y0 = fn(ud, ad, sd)
    y1 = fn(ud.clone().requires_grad_(True), ad.clone().requires_grad_(True), sd.clone().requires_grad_(True))
    torch.cuda.synchronize()
    assert not y0.requires_grad and y1.requires_grad
    assert torch.equal(y0, y1.detach()), _first_diff(y0.cpu(), y1.detach().cpu())


def test_explicit_refuses_empty_planes():
    """W = 0 or H = 0 come back as PDE_E_BADARG before any launch."""
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    t = torch.zeros(16, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())                                                  # noqa: E731
    fp = lambda x: C.cast(C.c_void_p(x.data_ptr()), C.POINTER(C.c_float))                   # noqa: E731
    for H, W in ((4, 0), (0, 4)):
        assert lib.pde_explicit5_forward(1, 1, H, W, L.PDE_IO_F32, p(t), fp(t), fp(t), 0.01, 1e-6, 0.15, 0.1, 1, None,
                                         p(t), None) == -1


# ---- 2. one-workgroup Jacobi kernels ----------------------------------------------------------------------------------
J_SMALL = [(4, 4), (4, 5), (5, 4), (4, 64), (64, 4), (7, 9), (33, 31), (63, 64), (64, 63), (64, 64)]


def _jacobi_case(B, H, W, nt, dtype=torch.float32):
    g = torch.Generator().manual_seed(1000 * H + W + nt)
    return (torch.randn(B, H, W, generator=g, dtype=dtype), torch.randn(B, H, W, generator=g, dtype=dtype),
            0.04 + 0.02 * torch.randn(H, generator=g, dtype=dtype), 0.05 + 0.02 * torch.randn(W, generator=g, dtype=dtype))


def _jacobi_parity(B, H, W, nt, path, dtype=torch.float32, tol=TOL):
    """as test_gpu_jacobi_tiled.test_oracle_parity, for a plane of either kernel family and either precision"""
    from cnn_with_pde_amd import _lib as L
    if path is not None:
        assert L.load().pde_jacobi_plane_path(H, W) == path
    u, gy, A, Bc = _jacobi_case(B, H, W, nt, dtype)
    y_ref, gu_ref, gp_ref = JT._oracle(u, A, Bc, gy, nt, dtype)
    if nt == 0:                                             # no step uses the coefficients: autograd reports None
        gp_ref = {"A": torch.zeros(H, dtype=dtype), "B": torch.zeros(W, dtype=dtype)}
    y, gu, gA, gB = JT._gpu(u, A, Bc, gy, nt)
    assert all(t.dtype == dtype for t in (y, gu, gA, gB))
    errs = {"y": G.rel_err(y.cpu(), y_ref), "gu": G.rel_err(gu.cpu(), gu_ref),
            "gA": G.rel_err(gA.cpu(), gp_ref["A"]), "gB": G.rel_err(gB.cpu(), gp_ref["B"])}
    print((B, H, W, nt), errs)
    if not all(v <= tol for v in errs.values()):
        d = (gu.cpu() - gu_ref).abs()
        where = tuple(int(x) for x in (d == d.max()).nonzero()[0])
        raise AssertionError((errs, "largest gu difference at (sample, row, column)", where))


def _jacobi_narrow(narrow, B, H, W, nt):
    """the gates of test_gpu_jacobi_tiled.test_narrow_io on another plane"""
    from cnn_with_pde_amd import _lib as L
    io_dtype = L.PDE_IO_BF16 if narrow == torch.bfloat16 else L.PDE_IO_F16
    u, gy, a, b = _jacobi_case(B, H, W, nt)
    u, gy, a, b = u.to(narrow).cuda(), gy.to(narrow).cuda(), a.cuda(), b.cuda()
    y, gu, ga, gb = _cabi(io_dtype, u, gy, a, b, nt)
    y32, gu32, ga32, gb32 = _cabi(L.PDE_IO_F32, u.float(), gy.float(), a, b, nt)
    assert y.dtype == narrow and y32.dtype == torch.float32
    assert int((_ord16(y) - _ord16(y32.to(narrow))).abs().max()) <= 1
    assert int((_ord16(gu) - _ord16(gu32.to(narrow))).abs().max()) <= 1
    assert G.rel_err(ga.cpu(), ga32.cpu()) <= 1e-6 and G.rel_err(gb.cpu(), gb32.cpu()) <= 1e-6


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("nt", [0, 1, 10])
@pytest.mark.parametrize("H,W", J_SMALL, ids=[f"{h}x{w}" for h, w in J_SMALL])
def test_jacobi_small_vs_oracle(H, W, nt, B):
    _jacobi_parity(B, H, W, nt, path=1)


@pytest.mark.parametrize("H,W", [(4, 4), (4, 64), (7, 9), (64, 64)], ids=lambda v: str(v))
def test_jacobi_small_exact(H, W):
    """test_exact_seams on the one-workgroup kernels: at H = 4 the rows the ring folds onto (1 and H-2) are neighbours."""
    from cnn_with_pde_amd import _lib as L
    assert L.load().pde_jacobi_plane_path(H, W) == 1
    JT.test_exact_seams(3, H, W)


@pytest.mark.parametrize("narrow", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H,W", [(4, 64), (7, 9), (64, 64)], ids=lambda v: str(v))
def test_jacobi_small_narrow_io(H, W, narrow):
    _jacobi_narrow(narrow, 4, H, W, 10)


@pytest.mark.parametrize("H,W", [(3, 8), (8, 3)], ids=lambda v: str(v))
def test_jacobi_refuses_planes_below_4(H, W):
    """rows 1 and H-2 coincide at H = 3: refused on the host, by the C ABI and by the wrapper"""
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    assert lib.pde_jacobi_plane_path(H, W) == 0
    u, a, b = torch.zeros(2, H, W, device="cuda"), torch.zeros(H, device="cuda"), torch.zeros(W, device="cuda")
    out = torch.full_like(u, 7.0)
    fp = lambda t: C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_float))                   # noqa: E731
    assert lib.pde_jacobi_forward(2, H, W, 1, fp(u), fp(a), fp(b), fp(out), None) == -1      # PDE_E_BADARG
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    assert lib.pde_jacobi_backward(2, H, W, 1, fp(u), fp(u), fp(a), fp(b), fp(out), fp(a), fp(b),
                                   C.c_void_p(ws.data_ptr()), ws.numel(), None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                         # nothing ran
    with pytest.raises(L.PdeError):
        P.jacobi_diffuse(u, a, b, 1)


# ---- 3. tiled Jacobi kernels ------------------------------------------------------------------------------------------
# a plane tiled in one dimension and minimal in the other; exact tile multiples (no partial tile); a last tile of one or
# two cells whose fold row lies in the previous tile, in W as well as in H; nt = K, K + 1, 2K (None: filled in below)
J_TILED = [(3, 4, 65, 7), (3, 65, 4, 7), (2, 4, 1024, 3), (2, 1024, 4, 3), (3, 64, 128, 7), (2, 128, 128, 7), (3, 66, 66, 7),
           (2, 129, 65, 7), (2, 65, 129, 7), (2, 97, 130, "K"), (2, 97, 130, "K+1"), (2, 97, 130, "2K")]


@pytest.mark.parametrize("B,H,W,nt", J_TILED, ids=lambda v: str(v))
def test_jacobi_tiled_vs_oracle(B, H, W, nt):
    if isinstance(nt, str):
        nt = {"K": JT._K(), "K+1": JT._K() + 1, "2K": 2 * JT._K()}[nt]
    _jacobi_parity(B, H, W, nt, path=2)


@pytest.mark.parametrize("H,W", [(4, 65), (66, 66), (129, 65), (128, 128)], ids=lambda v: str(v))
def test_jacobi_tiled_exact(H, W):
    from cnn_with_pde_amd import _lib as L
    assert L.load().pde_jacobi_plane_path(H, W) == 2
    JT.test_exact_seams(2, H, W)


@pytest.mark.parametrize("narrow", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H,W", [(4, 65), (129, 65)], ids=lambda v: str(v))
def test_jacobi_tiled_narrow_io(H, W, narrow):
    _jacobi_narrow(narrow, 3, H, W, 10)


# ---- 4. float64 Jacobi ------------------------------------------------------------------------------------------------
J_F64 = [(2, 2), (2, 5), (3, 3), (3, 7), (7, 3), (4, 64), (33, 31), (64, 64)]


def test_reflect_padding_is_defined_at_2_and_3():
    """the oracle's F.pad(mode="reflect") at H = 2 (the two fold rows swap) and H = 3 (they coincide)"""
    for H in (2, 3):
        u = torch.arange(float(H * 5)).view(1, H, 5)
        P = F.pad(u, (1, 1, 1, 1), mode="reflect")
        assert torch.equal(P[0, 0, 1:-1], u[0, 1]) and torch.equal(P[0, -1, 1:-1], u[0, H - 2])
        assert torch.equal(P.transpose(1, 2), F.pad(u.transpose(1, 2), (1, 1, 1, 1), mode="reflect"))


@pytest.mark.parametrize("nt", [1, 10])
@pytest.mark.parametrize("H,W", J_F64, ids=[f"{h}x{w}" for h, w in J_F64])
def test_jacobi_f64_vs_oracle(H, W, nt):
    """pde_jacobi_f64_* documents 2 <= H, W <= 64 and has a fold of its own; 64 x 64 needs more than 64 KB of LDS"""
    _jacobi_parity(3, H, W, nt, path=None, dtype=torch.float64, tol=TOL64)


def test_jacobi_f64_refuses_tiled_planes():
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L
    assert L.load().pde_jacobi_f64_backward_workspace_bytes(2, 65, 8, 1) == 0
    u = torch.zeros(2, 65, 8, dtype=torch.float64, device="cuda")
    with pytest.raises(L.PdeError):
        P.jacobi_diffuse(u, torch.zeros(65, dtype=torch.float64, device="cuda"),
                         torch.zeros(8, dtype=torch.float64, device="cuda"), 1)
