"""Helpers of the rectangle tests (tests/test_gpu_rect.py, tests/test_cabi_rect.py) and of
tools/gen_adi_gen_square_golden.py: seeded cases for the any-size implicit kernels and a raw ctypes driver of one
forward + backward through either the square entry points (pde_adi_forward / pde_adi_backward, PdeAdiDesc) or the
rectangle ones (pde_adi_rect_forward / pde_adi_rect_backward, PdeAdiRectDesc).  The driver talks to a CDLL handle it is
given and sets no argtypes, so it can be pointed at a library built from an older commit."""
import ctypes as C

import torch

#: N of the parent-commit fixture tests/golden/adi_gen_square_path/results.npz -> (B, C): 30 keeps the partial sums in
#: LDS (ALDS), 64 is one full wave per plane, 128 the longest line (two waves, 132 KB of LDS in the backward); two samples
#: at the large sizes so that the sum over workgroups is pinned there too (the file is 843 KiB, under the 1 MiB limit)
SQUARE_PATH_CASES = {30: (3, 2), 64: (2, 2), 128: (2, 1)}


def adi_case(B, Cc, H, W, seed, steps=2, dt=0.1, dx=1.0, dy=1.2, smooth3=True, clamp_max=3.0, eps=1e-6, ckpt=0b00100):
    """Seeded fp32 inputs of one call: Strang steps, smoothed coefficients that cross clamp_max and the floor while the
    time slopes move them (the pass-through mask differs from sweep to sweep), one checkpoint."""
    from cnn_with_pde_amd import functional as F_
    g = torch.Generator().manual_seed(seed)
    sweeps = tuple(s for st in F_.adi_schedule(dt, dx, dy, steps, "strang") for s in st)
    p = {"ab": 2.0 + 1.5 * torch.rand(Cc, H, W, generator=g), "bb": 0.4 * torch.randn(Cc, H, W, generator=g).abs(),
         "as": 3.0 * torch.randn(Cc, H, W, generator=g), "bs": 3.0 * torch.randn(Cc, H, W, generator=g)}
    return dict(B=B, C=Cc, H=H, W=W, sweeps=sweeps, smooth3=smooth3, clamp_max=clamp_max, eps=eps, ckpt=ckpt,
                u=torch.randn(B, Cc, H, W, generator=g), gy=torch.randn(B, Cc, H, W, generator=g), **p)


def square_path_case(N):
    B, Cc = SQUARE_PATH_CASES[N]
    return adi_case(B, Cc, N, N, 4000 + N)


def _fill(d, case):
    d.B, d.C, d.io_dtype, d.num_sweeps = case["B"], case["C"], 0, len(case["sweeps"])
    d.smooth3, d.has_clamp_max = int(case["smooth3"]), int(case["clamp_max"] is not None)
    d.clamp_max, d.eps = float(case["clamp_max"] or 0.0), case["eps"]
    for i, s in enumerate(case["sweeps"]):
        d.sweep[i].axis, d.sweep[i].delta, d.sweep[i].h2, d.sweep[i].t = int(s.axis), s.delta, s.h2, s.t
    return d


def run_entry(lib, case, rect):
    """y, gu and the four parameter gradients (alpha_base, beta_base, alpha_slope, beta_slope) of ``case`` on cuda:0 through
    the square (``rect=False``: needs H == W) or the rectangle entry points of the CDLL handle ``lib``."""
    from cnn_with_pde_amd import _lib as L
    if rect:
        d = _fill(L.PdeAdiRectDesc(), case)
        d.H, d.W = case["H"], case["W"]
        pre = "pde_adi_rect_"
    else:
        assert case["H"] == case["W"]
        d = _fill(L.PdeAdiDesc(), case)
        d.N = case["H"]
        pre = "pde_adi_"
    fwd_bytes, bwd_bytes = getattr(lib, pre + "forward_workspace_bytes"), getattr(lib, pre + "backward_workspace_bytes")
    fwd_bytes.restype = bwd_bytes.restype = C.c_size_t
    vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())                             # noqa: E731
    u, gy = case["u"].cuda(), case["gy"].cuda()
    p = [case[k].cuda().contiguous() for k in ("ab", "bb", "as", "bs")]
    y, gu = torch.empty_like(u), torch.empty_like(u)
    gp = [torch.empty_like(t) for t in p]
    bits = int(case["ckpt"])
    nf = fwd_bytes(C.byref(d))
    nb = bwd_bytes(C.byref(d), C.c_int32(bin(bits).count("1")))
    assert nf > 0 and nb > 0, (nf, nb)
    fws = torch.empty(nf, dtype=torch.uint8, device="cuda")
    bws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    rc = getattr(lib, pre + "forward")(C.byref(d), vp(u), vp(y), *[vp(t) for t in p], vp(None), vp(None), vp(None),
                                       vp(fws), C.c_size_t(nf), vp(None))
    assert rc == 0, rc
    mask = (C.c_uint64 * 2)(bits & (2 ** 64 - 1), bits >> 64)
    rc = getattr(lib, pre + "backward")(C.byref(d), vp(gy), vp(y), vp(u if bits else None), mask, vp(gu),
                                        *[vp(t) for t in p], *[vp(t) for t in gp], vp(fws), vp(bws), C.c_size_t(nb),
                                        vp(None))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {"y": y, "gu": gu, "g_ab": gp[0], "g_bb": gp[1], "g_as": gp[2], "g_bs": gp[3]}
