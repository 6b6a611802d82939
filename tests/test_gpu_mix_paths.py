"""Every kernel family of the channel operator out[b,i,p] = sum_j M[i,j] u[b,j,p] (csrc/pde_mix.hip, pde_mix_bf16.hip)
through the C ABI, against the same product in float64 on the CPU.

Each case names its family and first asserts that pde_channel_mix_path() — the function the entry points dispatch on —
returns it, and that pde_channel_mix_splits() gives the workload the case is meant to have:

    short        no walker (workgroup, or wave of the fp32-MFMA forward) takes more than one chunk
    long         more chunks than walkers and not a multiple of them: some walkers take one trip more than others, and
                 the prefetch of the chunk after the last runs past the end
    ragged       a plane that is no multiple of the 64-pixel chunk (partial last tile, or a plane smaller than one tile),
                 every walker on one trip as in short
    ragged+long  such a plane under a long workload: the uneven last trip meets partial tiles

(a) Exact cases, tolerance 0.  u and g are integers in -2..2 and M has entries in {-1, 0, 1}, so |out|, |gu| <= 2C and
|gM| <= 4 B HW.  Every partial sum, in any order, is then an integer below 2^24 and exact in fp32; one bf16 piece holds
each operand, so the three-piece products and the hi + lo split of M are exact; and the results survive the rounding to
bf16 (integers up to 256) or fp16 (up to 2048).  Each case checks those conditions on the CPU before it compares, so a
shape that breaks them fails there.  M is non-symmetric with no zero row or column: M in place of M^T fails.
(b) The accumulate / finalize protocol of pde_channel_mix_backward_steps on a NaN-filled workspace, exact as well.
(c) Random values at the bars tests/test_gpu_parity.py and tests/test_gpu_f16.py state for the same type and path.
(d) Refusals by return code, with nothing launched.

The PDE_MIX_* switches are read with getenv on every call, so monkeypatch.setenv selects a path in this process."""
import ctypes as C

import pytest
import torch

import golden_util as G

pytestmark = pytest.mark.gpu

IO = {"f32": (0, torch.float32), "bf16": (1, torch.bfloat16), "f16": (3, torch.float16)}
PATH = {"scalar": 0, "mfma32": 1, "mfma16": 2, "split3": 3, "fused": 4}
SWITCH = {"nosplit": "PDE_MIX_NO_SPLIT", "unfused": "PDE_MIX_UNFUSED", "nobf16": "PDE_MIX_NO_BF16_MFMA"}


def _id(case):
    path, Cc, B, HW, io = case[:5]
    sw = case[-1]
    return f"{path}-{Cc}-{B}-{HW}-{io}" + (f"-{sw}" if sw else "")


@pytest.fixture
def select(monkeypatch):
    """select("nosplit+unfused") sets exactly those switches and returns the library."""
    from cnn_with_pde_amd import _lib as L
    lib = L.load()

    def go(switches):
        for v in SWITCH.values():
            monkeypatch.delenv(v, raising=False)
        for s in filter(None, switches.split("+")):
            monkeypatch.setenv(SWITCH[s], "1")
        return lib
    return go


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _assert_plan(lib, path, B, Cc, HW, io, backward, kind):
    code = IO[io][0]
    got = lib.pde_channel_mix_path(B, Cc, HW, code, backward)
    assert got == PATH[path], f"the call takes path {got}, the case is named after {path} = {PATH[path]}"
    chunks = C.c_int64(0)
    walkers = lib.pde_channel_mix_splits(B, Cc, HW, code, backward, C.byref(chunks))
    assert walkers >= 1
    assert kind in ("short", "long", "ragged", "ragged+long")
    if "ragged" in kind:
        assert HW % 64 != 0
    if "long" in kind:
        assert chunks.value > walkers and chunks.value % walkers != 0, (chunks.value, walkers)
    else:
        assert chunks.value <= walkers, (chunks.value, walkers)


def _int_matrix(Cc, gen):
    M = torch.randint(-1, 2, (Cc, Cc), generator=gen).float()
    idx = torch.arange(Cc)
    M[idx, (idx + 1) % Cc] = 1.0                       # no zero row, no zero column
    if Cc >= 2:
        M[0, 1], M[1, 0] = 1.0, -1.0                   # not symmetric
        assert not torch.equal(M, M.t())
    assert bool((M != 0).any(dim=0).all()) and bool((M != 0).any(dim=1).all())
    return M


def _ints(B, Cc, HW, gen, dtype):
    return torch.randint(-2, 3, (B, Cc, HW), generator=gen).to(dtype)


def _gm_ref(g64, u64):
    Cc = g64.shape[1]
    return g64.transpose(0, 1).reshape(Cc, -1) @ u64.transpose(0, 1).reshape(Cc, -1).t()


def _assert_survives(ref, dtype, what):
    assert torch.equal(ref.to(dtype).double(), ref), f"{what}: the float64 reference is not exact in {dtype}"


def _assert_same(got, ref, what):
    got = got.double()
    if not torch.equal(got, ref):                      # NaN (never written) differs from everything
        bad = ~(got == ref)
        where = torch.nonzero(bad)[0].tolist()
        diff = float((got - ref).abs().nan_to_num(float("inf")).max())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, max |diff| {diff}, first at {where}")


def _forward(lib, B, Cc, HW, io, u, M):
    code, dt = IO[io]
    ud, Md = u.to(dt).cuda(), M.float().cuda()
    out = torch.full_like(ud, float("nan"))
    rc = lib.pde_channel_mix_forward(B, Cc, HW, code, _ptr(ud), _ptr(Md), _ptr(out), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out.cpu()


def _workspace(lib, B, Cc, HW):
    n = lib.pde_channel_mix_backward_workspace_bytes(B, Cc, HW)
    assert n > 0 and n % 4 == 0
    return torch.full((n // 4,), float("nan"), device="cuda")


def _backward_step(lib, B, Cc, HW, io, u, g, M, ws, gM, accumulate, finalize):
    code, dt = IO[io]
    ud, gd, Md = u.to(dt).cuda(), g.to(dt).cuda(), M.float().cuda()
    gu = torch.full_like(ud, float("nan"))
    rc = lib.pde_channel_mix_backward_steps(B, Cc, HW, code, _ptr(ud), _ptr(gd), _ptr(Md), _ptr(gu), _ptr(gM), _ptr(ws),
                                            ws.numel() * 4, accumulate, finalize, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return gu.cpu()


def _backward(lib, B, Cc, HW, io, u, g, M):
    """pde_channel_mix_backward on a NaN-filled workspace: (gu, gM) on the CPU."""
    code, dt = IO[io]
    ud, gd, Md = u.to(dt).cuda(), g.to(dt).cuda(), M.float().cuda()
    gu = torch.full_like(ud, float("nan"))
    gM = torch.full((Cc, Cc), float("nan"), device="cuda")
    ws = _workspace(lib, B, Cc, HW)
    rc = lib.pde_channel_mix_backward(B, Cc, HW, code, _ptr(ud), _ptr(gd), _ptr(Md), _ptr(gu), _ptr(gM), _ptr(ws),
                                      ws.numel() * 4, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return gu.cpu(), gM.cpu()


# ---- (a) exact cases -----------------------------------------------------------------------------------------------
# (family, C, B, HW, tensor type, workload, switches).  The B of a long case is the smallest odd-ish batch that puts
# B * ceil(HW / 64) past the family's walker count without dividing by it; _assert_plan checks that against the library.
BWD_EXACT = [
    # bf16 / fp16 products on their own MFMA: C = 64 / 128, whole 64-pixel tiles only (HW = 64: a plane of one tile)
    ("mfma16", 64, 1, 64, "bf16", "short", ""), ("mfma16", 128, 1, 64, "f16", "short", ""),
    ("mfma16", 64, 5, 128, "f16", "short", ""), ("mfma16", 128, 3, 1024, "bf16", "short", ""),
    ("mfma16", 64, 13, 4096, "bf16", "long", ""), ("mfma16", 64, 13, 4096, "f16", "long", ""),
    ("mfma16", 128, 5, 4096, "bf16", "long", ""), ("mfma16", 128, 5, 4096, "f16", "long", ""),
    # fp32 tensors as three bf16 pieces: C = 32 / 64 / 96
    ("split3", 32, 1, 64, "f32", "short", ""), ("split3", 64, 1, 4, "f32", "short", ""), ("split3", 96, 3, 1024, "f32", "short", ""),
    ("split3", 32, 17, 4096, "f32", "long", ""), ("split3", 64, 9, 4096, "f32", "long", ""), ("split3", 96, 5, 4096, "f32", "long", ""),
    ("split3", 96, 21, 784, "f32", "ragged+long", ""),
    ("split3", 32, 3, 4, "f32", "ragged", ""), ("split3", 64, 2, 36, "f32", "ragged", ""), ("split3", 96, 3, 100, "f32", "ragged", ""),
    ("split3", 64, 5, 196, "f32", "ragged", ""), ("split3", 32, 5, 784, "f32", "ragged", ""), ("split3", 96, 2, 196, "f32", "ragged", ""),
    # fused fp32 MFMA: fp32 at C = 128 (M^T fragments in the workspace) ...
    ("fused", 128, 1, 64, "f32", "short", ""), ("fused", 128, 3, 1024, "f32", "short", ""), ("fused", 128, 9, 4096, "f32", "long", ""),
    ("fused", 128, 3, 4, "f32", "ragged", ""), ("fused", 128, 2, 36, "f32", "ragged", ""), ("fused", 128, 3, 100, "f32", "ragged", ""),
    ("fused", 128, 3, 196, "f32", "ragged", ""), ("fused", 128, 2, 784, "f32", "ragged", ""),
    # ... fp32 at C = 32 / 64 / 96 behind PDE_MIX_NO_SPLIT (fragments in LDS) ...
    ("fused", 32, 1, 64, "f32", "short", "nosplit"), ("fused", 64, 3, 1024, "f32", "short", "nosplit"),
    ("fused", 96, 3, 64, "f32", "short", "nosplit"),
    ("fused", 32, 25, 4096, "f32", "long", "nosplit"), ("fused", 64, 13, 4096, "f32", "long", "nosplit"),
    ("fused", 96, 5, 4096, "f32", "long", "nosplit"),
    ("fused", 32, 3, 36, "f32", "ragged", "nosplit"), ("fused", 64, 5, 196, "f32", "ragged", "nosplit"),
    ("fused", 96, 2, 784, "f32", "ragged", "nosplit"), ("fused", 64, 3, 4, "f32", "ragged", "nosplit"),
    # ... and the bf16s / f16s instantiations: 16-bit tensors whose shape their own MFMA path does not take
    ("fused", 64, 5, 196, "bf16", "ragged", ""), ("fused", 128, 3, 196, "f16", "ragged", ""), ("fused", 128, 2, 100, "bf16", "ragged", ""),
    ("fused", 32, 2, 100, "f16", "ragged", ""), ("fused", 96, 2, 36, "bf16", "ragged", ""), ("fused", 64, 3, 4, "f16", "ragged", ""),
    ("fused", 32, 3, 1024, "bf16", "short", ""), ("fused", 96, 3, 1024, "f16", "short", ""),
    ("fused", 96, 5, 4096, "bf16", "long", ""), ("fused", 32, 25, 4096, "f16", "long", ""),
    ("fused", 64, 3, 1024, "bf16", "short", "nobf16"), ("fused", 128, 9, 4096, "bf16", "long", "nobf16"),
    ("fused", 64, 13, 4096, "f16", "long", "nobf16"),
    # unfused: transposed fp32-MFMA apply + mix_gm_mfma_kernel
    ("mfma32", 128, 1, 64, "f32", "short", "unfused"), ("mfma32", 128, 2, 256, "f32", "short", "unfused"),
    ("mfma32", 128, 9, 4096, "f32", "long", "unfused"), ("mfma32", 128, 3, 196, "f32", "ragged", "unfused"),
    ("mfma32", 32, 3, 4, "f32", "ragged", "nosplit+unfused"), ("mfma32", 64, 2, 36, "f32", "ragged", "nosplit+unfused"),
    ("mfma32", 96, 3, 100, "f32", "ragged", "nosplit+unfused"), ("mfma32", 32, 5, 784, "f32", "ragged", "nosplit+unfused"),
    ("mfma32", 64, 9, 4096, "f32", "long", "nosplit+unfused"), ("mfma32", 96, 3, 64, "f32", "short", "nosplit+unfused"),
    ("mfma32", 96, 3, 196, "bf16", "ragged", "unfused"), ("mfma32", 32, 3, 1024, "f16", "short", "unfused"),
    ("mfma32", 64, 9, 4096, "bf16", "long", "nobf16+unfused"), ("mfma32", 128, 2, 100, "f16", "ragged", "unfused"),
    # scalar transposed apply + mix_gm_kernel: any C (tile edges of 32; 160: 25 tiles), any HW
    ("scalar", 1, 1, 1, "f32", "short", ""), ("scalar", 2, 3, 3, "f32", "ragged", ""), ("scalar", 7, 5, 49, "f32", "ragged", ""),
    ("scalar", 33, 2, 49, "bf16", "ragged", ""), ("scalar", 160, 1, 49, "f16", "ragged", ""), ("scalar", 160, 2, 100, "f32", "ragged", ""),
    ("scalar", 32, 3, 49, "f32", "ragged", ""), ("scalar", 64, 2, 3, "bf16", "ragged", ""), ("scalar", 128, 2, 1, "f16", "ragged", ""),
    ("scalar", 1, 3, 64, "bf16", "short", ""), ("scalar", 2, 2, 1024, "f16", "short", ""), ("scalar", 33, 3, 64, "f32", "short", ""),
    ("scalar", 7, 17, 4096, "f32", "long", ""), ("scalar", 33, 5, 4096, "f32", "long", ""), ("scalar", 160, 3, 1024, "f32", "long", ""),
    ("scalar", 33, 5, 4096, "bf16", "long", ""), ("scalar", 160, 3, 1024, "f16", "long", ""),
]


@pytest.mark.parametrize("case", BWD_EXACT, ids=_id)
def test_backward_exact_on_integers(case, select):
    path, Cc, B, HW, io, kind, sw = case
    lib = select(sw)
    _assert_plan(lib, path, B, Cc, HW, io, 1, kind)
    dt = IO[io][1]
    gen = torch.Generator().manual_seed(7 * Cc + 3 * B + HW)
    u, g, M = _ints(B, Cc, HW, gen, torch.float64), _ints(B, Cc, HW, gen, torch.float64), _int_matrix(Cc, gen).double()
    gu_ref, gM_ref = torch.matmul(M.t(), g), _gm_ref(g, u)
    assert 4 * B * HW < 2 ** 24
    _assert_survives(gu_ref, dt, "gu")
    _assert_survives(gM_ref, torch.float32, "gM")
    gu, gM = _backward(lib, B, Cc, HW, io, u, g, M)
    _assert_same(gu, gu_ref, "gu")
    _assert_same(gM, gM_ref, "gM")


FWD_EXACT = [
    ("mfma16", 64, 1, 64, "bf16", "short", ""), ("mfma16", 128, 1, 64, "f16", "short", ""),
    ("mfma16", 128, 3, 1024, "bf16", "short", ""), ("mfma16", 64, 5, 128, "f16", "short", ""),
    ("mfma16", 64, 17, 4096, "bf16", "long", ""), ("mfma16", 64, 17, 4096, "f16", "long", ""),
    ("mfma16", 128, 5, 4096, "bf16", "long", ""), ("mfma16", 128, 5, 4096, "f16", "long", ""),
    ("mfma32", 32, 1, 4, "f32", "short", ""), ("mfma32", 64, 1, 64, "f32", "short", ""), ("mfma32", 96, 3, 1024, "f32", "short", ""),
    ("mfma32", 128, 5, 128, "f32", "short", ""),
    ("mfma32", 32, 33, 16384, "f32", "long", ""),      # 4224 blocks of 128 pixels on 4 x 1024 waves: the grid cap
    ("mfma32", 64, 3, 196, "f32", "ragged", ""), ("mfma32", 96, 2, 100, "f32", "ragged", ""), ("mfma32", 128, 3, 784, "f32", "ragged", ""),
    ("mfma32", 32, 5, 36, "f32", "ragged", ""), ("mfma32", 128, 2, 4, "f32", "ragged", ""),
    ("mfma32", 32, 3, 1024, "bf16", "short", ""), ("mfma32", 96, 3, 1024, "f16", "short", ""),
    ("mfma32", 64, 5, 196, "bf16", "ragged", ""), ("mfma32", 128, 3, 196, "f16", "ragged", ""), ("mfma32", 96, 2, 36, "bf16", "ragged", ""),
    ("mfma32", 64, 3, 1024, "bf16", "short", "nobf16"), ("mfma32", 64, 33, 16384, "bf16", "long", "nobf16"), ("mfma32", 32, 33, 16384, "bf16", "long", ""),
    ("scalar", 1, 1, 1, "f32", "short", ""), ("scalar", 2, 3, 3, "f32", "ragged", ""), ("scalar", 7, 5, 49, "f32", "ragged", ""),
    ("scalar", 33, 2, 49, "bf16", "ragged", ""), ("scalar", 160, 1, 49, "f16", "ragged", ""), ("scalar", 160, 2, 100, "f32", "ragged", ""),
    ("scalar", 32, 3, 49, "f32", "ragged", ""), ("scalar", 64, 2, 3, "bf16", "ragged", ""), ("scalar", 128, 2, 1, "f16", "ragged", ""),
    ("scalar", 7, 3, 1024, "f32", "short", ""), ("scalar", 33, 2, 300, "f16", "ragged", ""), ("scalar", 2, 2, 64, "bf16", "short", ""),
]


@pytest.mark.parametrize("case", FWD_EXACT, ids=_id)
def test_forward_exact_on_integers(case, select):
    path, Cc, B, HW, io, kind, sw = case
    lib = select(sw)
    _assert_plan(lib, path, B, Cc, HW, io, 0, kind)
    dt = IO[io][1]
    gen = torch.Generator().manual_seed(11 * Cc + 5 * B + HW)
    u, M = _ints(B, Cc, HW, gen, torch.float64), _int_matrix(Cc, gen).double()
    ref = torch.matmul(M, u)
    _assert_survives(ref, dt, "out")
    _assert_same(_forward(lib, B, Cc, HW, io, u, M), ref, "out")


# ---- (b) the multi-call protocol -----------------------------------------------------------------------------------
PROTOCOL = [
    ("mfma16", 128, 5, 4096, "bf16", ""), ("mfma16", 64, 3, 64, "f16", ""),
    ("split3", 96, 5, 4096, "f32", ""), ("split3", 32, 3, 100, "f32", ""), ("split3", 64, 2, 1024, "f32", ""),
    ("fused", 128, 9, 4096, "f32", ""), ("fused", 128, 3, 196, "f32", ""), ("fused", 64, 5, 196, "f32", "nosplit"),
    ("fused", 32, 3, 1024, "bf16", ""), ("fused", 96, 5, 4096, "f16", ""),
    ("mfma32", 128, 9, 4096, "f32", "unfused"), ("mfma32", 64, 3, 196, "f32", "nosplit+unfused"), ("mfma32", 96, 3, 196, "bf16", "unfused"),
    ("scalar", 33, 5, 4096, "f32", ""), ("scalar", 7, 5, 49, "f16", ""), ("scalar", 160, 3, 1024, "f32", ""),
]


@pytest.mark.parametrize("case", PROTOCOL, ids=_id)
def test_multi_call_protocol_exact(case, select):
    """accumulate = 0, 1, 1 with finalize on the last call only, on a workspace that starts as NaN: gM is the sum over
    the three calls and every gu_k is its own call's; finalize = 0 leaves gM alone; a later accumulate = 0 call on the
    same workspace gives its own gM with nothing left over."""
    path, Cc, B, HW, io, sw = case
    lib = select(sw)
    code, dt = IO[io]
    assert lib.pde_channel_mix_path(B, Cc, HW, code, 1) == PATH[path]
    K = 3
    assert 4 * K * B * HW < 2 ** 24
    gen = torch.Generator().manual_seed(13 * Cc + B + HW)
    M = _int_matrix(Cc, gen).double()
    ws = _workspace(lib, B, Cc, HW)
    sentinel = -12345.0
    gM = torch.full((Cc, Cc), sentinel, device="cuda")
    total = torch.zeros(Cc, Cc, dtype=torch.float64)
    for k in range(K):
        u, g = _ints(B, Cc, HW, gen, torch.float64), _ints(B, Cc, HW, gen, torch.float64)
        total += _gm_ref(g, u)
        gu_ref = torch.matmul(M.t(), g)
        _assert_survives(gu_ref, dt, "gu")
        gu = _backward_step(lib, B, Cc, HW, io, u, g, M, ws, gM, accumulate=int(k > 0), finalize=int(k == K - 1))
        _assert_same(gu, gu_ref, f"gu of call {k}")
        if k < K - 1:
            assert bool((gM == sentinel).all()), f"call {k} has finalize = 0 and wrote gM"
    _assert_survives(total, torch.float32, "gM")
    _assert_same(gM.cpu(), total, "gM over three calls")
    u, g = _ints(B, Cc, HW, gen, torch.float64), _ints(B, Cc, HW, gen, torch.float64)
    gM.fill_(sentinel)
    gu = _backward_step(lib, B, Cc, HW, io, u, g, M, ws, gM, accumulate=0, finalize=1)
    _assert_same(gu, torch.matmul(M.t(), g), "gu of the fresh call")
    _assert_same(gM.cpu(), _gm_ref(g, u), "gM of the fresh call on the used workspace")


# ---- (c) random values at the project's bars -----------------------------------------------------------------------
# (backward family, C, B, HW, type, forward family, switches): one long and one ragged shape per backward family (the
# 16-bit MFMA path takes whole tiles only: a plane of one tile stands in).  Bars, max-norm relative (golden_util.rel_err):
#   fp32 tensors 1e-5 (test_gpu_parity.TOL); three-piece path gu 5e-7, gM 2e-6, per channel 2e-6
#   (test_channel_mix_three_piece_products); a bf16 result 6e-3 (test_channel_mix_bf16_io), an fp16 result 5e-3
#   (test_gpu_f16); gM from 16-bit tensors 2e-5 on their MFMA path (test_channel_mix_bf16_io) and, on the fp32 kernels they
#   fall to, the fp32 bar 1e-5: products of two bf16 / fp16 numbers are exact in fp32, so that sum is an fp32 sum of exact
#   terms, no worse than the fp32 tensors' own.
RANDOM = [
    ("mfma16", 128, 5, 4096, "bf16", "mfma16", ""), ("mfma16", 64, 13, 4096, "f16", "mfma16", ""),
    ("mfma16", 64, 3, 64, "bf16", "mfma16", ""), ("mfma16", 128, 3, 64, "f16", "mfma16", ""),
    ("split3", 96, 5, 4096, "f32", "mfma32", ""), ("split3", 32, 17, 4096, "f32", "mfma32", ""), ("split3", 64, 5, 196, "f32", "mfma32", ""),
    ("fused", 128, 9, 4096, "f32", "mfma32", ""), ("fused", 128, 3, 196, "f32", "mfma32", ""),
    ("fused", 32, 25, 4096, "f32", "mfma32", "nosplit"), ("fused", 64, 5, 196, "f32", "mfma32", "nosplit"),
    ("fused", 96, 5, 4096, "bf16", "mfma32", ""), ("fused", 64, 5, 196, "f16", "mfma32", ""),
    ("mfma32", 128, 9, 4096, "f32", "mfma32", "unfused"), ("mfma32", 32, 3, 196, "f32", "mfma32", "nosplit+unfused"),
    ("mfma32", 96, 3, 196, "bf16", "mfma32", "unfused"),
    ("scalar", 33, 5, 4096, "f32", "scalar", ""), ("scalar", 7, 5, 49, "f32", "scalar", ""), ("scalar", 160, 2, 100, "bf16", "scalar", ""),
    ("scalar", 33, 3, 49, "f16", "scalar", ""),
]


def _bars(path, io):
    if io == "f32":
        if path == "split3":
            return dict(res=5e-7, gM=2e-6, per=2e-6)
        return dict(res=1e-5, gM=1e-5, per=1e-5 if path == "fused" else None)
    return dict(res=6e-3 if io == "bf16" else 5e-3, gM=2e-5 if path == "mfma16" else 1e-5, per=None)


@pytest.mark.parametrize("case", RANDOM, ids=_id)
def test_random_values_at_the_stated_bars(case, select):
    path, Cc, B, HW, io, fwd, sw = case
    lib = select(sw)
    code, dt = IO[io]
    assert lib.pde_channel_mix_path(B, Cc, HW, code, 1) == PATH[path]
    assert lib.pde_channel_mix_path(B, Cc, HW, code, 0) == PATH[fwd]
    gen = torch.Generator().manual_seed(17 * Cc + B + HW)
    u = torch.randn(B, Cc, HW, generator=gen).to(dt)
    g = torch.randn(B, Cc, HW, generator=gen)
    if io == "f32" and path in ("split3", "fused"):    # six decades across the channels of the incoming gradient
        g = g * torch.logspace(-3, 3, Cc).view(1, Cc, 1)
    g = g.to(dt)
    M = torch.eye(Cc) + 0.1 * torch.randn(Cc, Cc, generator=gen)
    if io == "f16":
        M = M.half().float()                           # the float16 route holds M in fp16 (include/pdecnn.h)
    assert not torch.equal(M, M.t()) or Cc == 1
    u64, g64, M64 = u.double(), g.double(), M.double()
    out_ref, gu_ref, gM_ref = torch.matmul(M64, u64), torch.matmul(M64.t(), g64), _gm_ref(g64, u64)
    out = _forward(lib, B, Cc, HW, io, u, M)
    gu, gM = _backward(lib, B, Cc, HW, io, u, g, M)
    bars = _bars(path, io)
    e_out, e_gu, e_gM = G.rel_err(out, out_ref), G.rel_err(gu, gu_ref), G.rel_err(gM, gM_ref)
    per = float(((gu.double() - gu_ref).abs().amax(dim=(0, 2)) / gu_ref.abs().amax(dim=(0, 2))).max())
    print(f"{_id(case)}: out {e_out:.2e} gu {e_gu:.2e} gM {e_gM:.2e} per-channel gu {per:.2e}")
    assert e_out <= (1e-5 if io == "f32" else bars["res"]), e_out
    assert e_gu <= bars["res"], e_gu
    assert e_gM <= bars["gM"], e_gM
    if bars["per"] is not None:
        assert per <= bars["per"], per


# ---- (d) refusals --------------------------------------------------------------------------------------------------
def test_refusals_by_return_code(select):
    """Bad dimensions, null pointers, an unknown tensor type, finalize without gM and a workspace one byte short come
    back as PDE_E_BADARG (-1) / PDE_E_WORKSPACE (-5) before anything is launched: the outputs keep their fill.  Every
    buffer passed here has its full size, so a check that let a call through would still run in bounds.  (The entry
    points do not check the workspace's alignment: there is no such refusal to test.)"""
    lib = select("")
    B, Cc, HW = 3, 64, 196
    fill = 777.0
    u, g = torch.zeros(B, Cc, HW, device="cuda"), torch.zeros(B, Cc, HW, device="cuda")
    M = torch.eye(Cc, device="cuda")
    out = torch.full((B, Cc, HW), fill, device="cuda")
    gM = torch.full((Cc, Cc), fill, device="cuda")
    need = lib.pde_channel_mix_backward_workspace_bytes(B, Cc, HW)
    ws = torch.full((need // 4,), fill, device="cuda")
    st = _stream()
    p = _ptr

    def fwd(B=B, Cc=Cc, HW=HW, io=0, u=u, M=M, out=out):
        return lib.pde_channel_mix_forward(B, Cc, HW, io, p(u), p(M), p(out), st)

    def bwd(B=B, Cc=Cc, HW=HW, io=0, u=u, g=g, M=M, gu=out, gM=gM, ws=ws, nbytes=need, acc=0, fin=1):
        return lib.pde_channel_mix_backward_steps(B, Cc, HW, io, p(u), p(g), p(M), p(gu), p(gM), p(ws), nbytes, acc, fin, st)

    for call in (fwd, bwd):
        for bad in (dict(B=0), dict(Cc=0), dict(HW=0), dict(B=-1), dict(Cc=-64), dict(HW=-196), dict(io=2), dict(io=7), dict(io=-1),
                    dict(u=None), dict(M=None)):
            assert call(**bad) == -1, (call.__name__, bad)
    assert fwd(out=None) == -1
    for bad in (dict(g=None), dict(gu=None), dict(ws=None), dict(gM=None, fin=1), dict(gM=None, fin=1, acc=1)):
        assert bwd(**bad) == -1, bad
    assert bwd(nbytes=need - 1) == -5 and bwd(nbytes=0) == -5
    assert lib.pde_channel_mix_backward(B, Cc, HW, 0, p(u), p(g), p(M), p(out), None, p(ws), need, st) == -1
    assert lib.pde_channel_mix_backward(B, Cc, HW, 0, p(u), p(g), p(M), p(out), p(gM), p(ws), need - 1, st) == -5
    assert lib.pde_channel_mix_backward_workspace_bytes(0, Cc, HW) == 0
    torch.cuda.synchronize()
    for t in (out, gM, ws):
        assert bool((t == fill).all()), "a refused call wrote to its outputs"
    # and the same arguments, put right, are served: gM may be absent when finalize = 0
    assert bwd(gM=None, fin=0) == 0 and bwd() == 0 and fwd() == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((gM == 0).all())
