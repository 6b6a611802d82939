"""The emotion PDELayer on planes larger than 64x64: the tiled Jacobi kernels (a workgroup owns a 64x64 tile of one
sample and advances it PDE_JACOBI_TILED_K steps per launch on a halo) against the oracle, exactly at the tile seams,
at module level, with bf16 / fp16 tensors, twice, under graph capture — and the planes up to 64x64, which stay on the
one-workgroup kernels."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

import golden_util as G
from oracle import pde_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5               # tests/test_gpu_parity.py's bar for the coefficient vectors' gradients
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jacobi_small_path", "results.npz")


def _K():
    from cnn_with_pde_amd import _lib as L
    return L.PDE_JACOBI_TILED_K


def _oracle(u, A, Bc, gy, nt, dtype=torch.float64):
    return O.value_and_grads(lambda a, p: O.jacobi_forward(a, p["A"], p["B"], nt), u.to(dtype),
                             {"A": A.to(dtype), "B": Bc.to(dtype)}, gy.to(dtype))


def _gpu(u, A, Bc, gy, nt):
    import cnn_with_pde_amd as P
    ud, Ad, Bd = u.cuda().requires_grad_(True), A.cuda().requires_grad_(True), Bc.cuda().requires_grad_(True)
    y = P.jacobi_diffuse(ud, Ad, Bd, nt)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    return y.detach(), ud.grad, Ad.grad, Bd.grad


# nt = None: more steps than one launch takes — two full launches and a remainder
@pytest.mark.parametrize("B,H,W,nt", [(5, 65, 8, 3), (3, 8, 65, 3), (4, 96, 96, 10), (3, 100, 112, 10), (2, 129, 127, 7),
                                      (2, 224, 224, 10), (1, 1024, 1024, 2), (3, 97, 130, None), (3, 96, 96, 0),
                                      (3, 96, 96, 1)])
def test_oracle_parity(B, H, W, nt):
    from cnn_with_pde_amd import _lib as L
    if nt is None:
        nt = 2 * _K() + 3
        assert L.load().pde_jacobi_forward_workspace_bytes(B, H, W, nt) > 0
    assert L.load().pde_jacobi_plane_path(H, W) == 2
    g = torch.Generator().manual_seed(1000 * H + W + nt)
    u = torch.randn(B, H, W, generator=g)
    gy = torch.randn(B, H, W, generator=g)
    A = 0.04 + 0.02 * torch.randn(H, generator=g)
    Bc = 0.05 + 0.02 * torch.randn(W, generator=g)
    y_ref, gu_ref, gp_ref = _oracle(u, A, Bc, gy, nt)
    if nt == 0:                                             # no step uses the coefficients: autograd reports None
        gp_ref = {"A": torch.zeros(H, dtype=torch.float64), "B": torch.zeros(W, dtype=torch.float64)}
    y, gu, gA, gB = _gpu(u, A, Bc, gy, nt)
    errs = {"y": G.rel_err(y.cpu(), y_ref), "gu": G.rel_err(gu.cpu(), gu_ref),
            "gA": G.rel_err(gA.cpu(), gp_ref["A"]), "gB": G.rel_err(gB.cpu(), gp_ref["B"])}
    print((B, H, W, nt), errs)
    assert all(v <= TOL for v in errs.values()), errs


@pytest.mark.parametrize("B,H,W", [(3, 97, 130), (2, 224, 224), (2, 65, 8)])
def test_exact_seams(B, H, W):
    """a = b = 1/4 and small integers: every intermediate is a short dyadic number, fp32 is exact in any order, so the
    results must equal the oracle's bit for bit — one wrong halo cell, one gradient cell counted twice or one ring cell
    folded to the wrong place fails."""
    nt = 3
    g = torch.Generator().manual_seed(H * 1000 + W)
    u = torch.randint(-2, 3, (B, H, W), generator=g).float()
    gy = torch.randint(-2, 3, (B, H, W), generator=g).float()
    A, Bc = torch.full((H,), 0.25), torch.full((W,), 0.25)
    y32, gu32, gp32 = _oracle(u, A, Bc, gy, nt, torch.float32)
    y64, gu64, gp64 = _oracle(u, A, Bc, gy, nt, torch.float64)
    assert torch.equal(y32.double(), y64) and torch.equal(gu32.double(), gu64)           # the precondition
    assert torch.equal(gp32["A"].double(), gp64["A"]) and torch.equal(gp32["B"].double(), gp64["B"])
    y, gu, gA, gB = _gpu(u, A, Bc, gy, nt)
    assert torch.equal(y.cpu(), y32) and torch.equal(gu.cpu(), gu32)
    assert torch.equal(gA.cpu(), gp32["A"]) and torch.equal(gB.cpu(), gp32["B"])


def test_module_level():
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(77)
    pl = P.PDELayer(Nx=96, Ny=128, Lx=2.0, Ly=2.0, T=0.004)
    with torch.no_grad():
        for n, v in dict(alpha_w1=0.04, alpha_w2=0.01, alpha_w3=0.02, beta_w1=0.05, beta_w2=-0.01, beta_w3=0.01).items():
            getattr(pl, n).fill_(v)
    params = {k: v.detach().clone() for k, v in pl.named_parameters()}
    u = torch.randn(6, 1, 128, 96, generator=g)           # rows follow y (Ny), columns x (Nx)
    gy = torch.randn(6, 1, 128, 96, generator=g)
    y_ref, gu_ref, gp_ref = O.value_and_grads(lambda a, p: O.emotion_forward(a, p, Nx=96, Ny=128, Lx=2.0, Ly=2.0, T=0.004),
                                              u, params, gy)
    assert torch.isfinite(y_ref).all() and float(y_ref.abs().max()) < 10.0
    dl = pl.cuda()
    ud = u.cuda().requires_grad_(True)
    y = dl(ud)
    y.backward(gy.cuda())
    errs = {"y": G.rel_err(y.detach().cpu(), y_ref), "gu": G.rel_err(ud.grad.cpu(), gu_ref)}
    for n, p in dl.named_parameters():
        errs["g_" + n] = G.rel_err(p.grad.cpu(), gp_ref[n])
    print(errs)
    assert len(errs) == 8 and all(v <= 2e-4 for v in errs.values()), errs


def test_emotion_model_at_96():
    import cnn_with_pde_amd as P
    with contextlib.redirect_stdout(io.StringIO()):
        model = P.EmotionDiffusionClassifier(img_size=96).cuda()
    with torch.no_grad():                                   # the reference's initial weights are unstable at Nx = 96
        for p in model.pde.parameters():
            p.mul_(0.1)
    x = torch.randn(4, 1, 96, 96, device="cuda", requires_grad=True)
    out = model(x)
    assert out.shape == (4, 7)
    out.sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(x.grad).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def _ord16(t):
    """16-bit patterns (fp16 or bf16) as integers in value order."""
    i = t.detach().cpu().contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _cabi(io_dtype, u, gy, a, b, nt):
    """forward and backward through the typed C entry points on tensors of any of the three I/O types"""
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    B, H, W = u.shape
    p = lambda t: C.c_void_p(t.data_ptr())                                                  # noqa: E731
    fp = lambda t: C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_float))                   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out, gu = torch.empty_like(u), torch.empty_like(u)
    ga, gb = torch.empty_like(a), torch.empty_like(b)
    assert lib.pde_jacobi_io_forward(B, H, W, nt, io_dtype, p(u), fp(a), fp(b), p(out), st) == 0
    nb = lib.pde_jacobi_io_backward_workspace_bytes(B, H, W, nt, io_dtype)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    assert lib.pde_jacobi_io_backward(B, H, W, nt, io_dtype, p(u), p(gy), fp(a), fp(b), p(gu), fp(ga), fp(gb), p(ws), nb,
                                      st) == 0
    torch.cuda.synchronize()
    return out, gu, ga, gb


@pytest.mark.parametrize("narrow", [torch.bfloat16, torch.float16])
def test_narrow_io(narrow):
    """bf16 / fp16 tensors at 96x96 against the fp32 tiled route on the same values: the output and gu are that route's
    rounded once (1 ulp), the parameter gradients the same fp32 sums over the same widened values."""
    from cnn_with_pde_amd import _lib as L
    io_dtype = L.PDE_IO_BF16 if narrow == torch.bfloat16 else L.PDE_IO_F16
    B, H, W, nt = 4, 96, 96, 10
    g = torch.Generator().manual_seed(96)
    u = torch.randn(B, H, W, generator=g).to(narrow).cuda()
    gy = torch.randn(B, H, W, generator=g).to(narrow).cuda()
    a = (0.04 + 0.02 * torch.randn(H, generator=g)).cuda()
    b = (0.05 + 0.02 * torch.randn(W, generator=g)).cuda()
    y, gu, ga, gb = _cabi(io_dtype, u, gy, a, b, nt)
    y32, gu32, ga32, gb32 = _cabi(L.PDE_IO_F32, u.float(), gy.float(), a, b, nt)
    assert y.dtype == narrow and y32.dtype == torch.float32
    assert int((_ord16(y) - _ord16(y32.to(narrow))).abs().max()) <= 1
    assert int((_ord16(gu) - _ord16(gu32.to(narrow))).abs().max()) <= 1
    assert G.rel_err(ga.cpu(), ga32.cpu()) <= 1e-6 and G.rel_err(gb.cpu(), gb32.cpu()) <= 1e-6


def test_half_layer_at_96():
    import cnn_with_pde_amd as P
    layer = P.PDELayer(Nx=96, Ny=96, Lx=2.0, Ly=2.0, T=0.01, dt=0.001)
    with torch.no_grad():                                   # the stable weights of test_module_level
        for n, v in dict(alpha_w1=0.04, alpha_w2=0.01, alpha_w3=0.02, beta_w1=0.05, beta_w2=-0.01, beta_w3=0.01).items():
            getattr(layer, n).fill_(v)
    layer = layer.half().cuda()
    u = torch.randn(2, 1, 96, 96, device="cuda").half().requires_grad_(True)
    y = layer(u)
    y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    assert y.dtype == torch.float16 and u.grad.dtype == torch.float16 and torch.isfinite(y.float()).all()
    assert all(p.grad is not None and p.grad.dtype == torch.float16 for p in layer.parameters())


def test_repeatability():
    """No float atomics: two calls, with a large unrelated allocation between them, give the same bits."""
    g = torch.Generator().manual_seed(9)
    B, H, W, nt = 9, 100, 112, 10
    u = torch.randn(B, H, W, generator=g)
    gy = torch.randn(B, H, W, generator=g)
    A = 0.04 + 0.02 * torch.randn(H, generator=g)
    Bc = 0.05 + 0.02 * torch.randn(W, generator=g)
    first = _gpu(u, A, Bc, gy, nt)
    junk = torch.full((64 << 20,), 7.0, device="cuda")      # moves the next call's workspace somewhere else
    second = _gpu(u, A, Bc, gy, nt)
    del junk
    for x, y in zip(first, second):
        assert torch.equal(x, y)


def test_capture():
    """forward + autograd.grad as one captured graph: the tiled entry points allocate, copy and synchronise nothing."""
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(8)
    B, H, W, nt = 8, 96, 96, 10
    u = torch.randn(B, H, W, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(B, H, W, generator=g).cuda()
    A = (0.04 + 0.02 * torch.randn(H, generator=g)).cuda().requires_grad_(True)
    Bc = (0.05 + 0.02 * torch.randn(W, generator=g)).cuda().requires_grad_(True)

    def fn():
        y = P.jacobi_diffuse(u, A, Bc, nt)
        return (y,) + torch.autograd.grad(y, [u, A, Bc], gy)

    step = P.GraphedStep(fn)
    for trial in range(2):
        eager = [t.clone() for t in fn()]
        got = step()
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert torch.equal(a, b)
        with torch.no_grad():                               # new values, same buffers
            u.copy_(torch.randn(B, H, W, generator=g))
            gy.copy_(torch.randn(B, H, W, generator=g))
            A.mul_(1.1)


def small_path_case(N):
    """The inputs of the small-path fixture (tests/golden/jacobi_small_path/results.npz, written by tools/gen_jacobi_small_golden.py
    from the library as it was before the tiled kernels existed)."""
    g = torch.Generator().manual_seed(6400 + N)
    B, nt = 5, 10
    return (torch.randn(B, N, N, generator=g), torch.randn(B, N, N, generator=g), 0.04 + 0.02 * torch.randn(N, generator=g),
            0.05 + 0.02 * torch.randn(N, generator=g), nt)


@pytest.mark.parametrize("N", [48, 64])
def test_small_planes_unchanged(N):
    """Planes up to 64x64 stay on the one-workgroup kernels, bit for bit."""
    from cnn_with_pde_amd import _lib as L
    assert L.load().pde_jacobi_plane_path(N, N) == 1
    u, gy, A, Bc, nt = small_path_case(N)
    y, gu, gA, gB = _gpu(u, A, Bc, gy, nt)
    want = np.load(GOLDEN)
    for name, t in (("y", y), ("gu", gu), ("gA", gA), ("gB", gB)):
        assert torch.equal(t.cpu(), torch.from_numpy(want[f"{name}_{N}"])), name
