"""The rectangle entry points of the C ABI (pde_adi_rect_*, include/pdecnn.h) on a machine without a GPU: header,
ctypes table and exports agree, the descriptors have the header's layout, and every refusal happens on the host before
anything touches the device.  The square descriptor and the square limits tests/test_cabi.py pins are still what they
were."""
import ctypes as C

import pytest

from test_cabi import declared_functions

RECT = ["pde_adi_rect_supported", "pde_adi_rect_forward_workspace_bytes", "pde_adi_rect_backward_workspace_bytes",
        "pde_adi_rect_kappa_max", "pde_adi_rect_forward", "pde_adi_rect_backward",
        "pde_adi_rect_f64_forward_workspace_bytes", "pde_adi_rect_f64_backward_workspace_bytes",
        "pde_adi_rect_f64_kappa_max", "pde_adi_rect_f64_forward", "pde_adi_rect_f64_backward"]


def test_header_table_and_exports_agree():
    from cnn_with_pde_amd import _lib
    names = declared_functions()
    lib = C.CDLL(_lib.LIB_PATH)
    for n in RECT:
        assert n in names, f"{n} missing in pdecnn.h"
        assert n in _lib.SIGNATURES, f"{n} missing in _lib.SIGNATURES"
        assert hasattr(lib, n), f"{n} not exported"
    assert sorted(_lib.SIGNATURES) == names
    _lib.load()


def test_struct_layouts():
    from cnn_with_pde_amd import _lib
    assert C.sizeof(_lib.PdeAdiRectDesc) == 10 * 4 + 16 * _lib.PDE_MAX_SWEEPS
    assert C.sizeof(_lib.PdeAdiRectDescF64) == 8 * 4 + 2 * 8 + 32 * _lib.PDE_MAX_SWEEPS
    assert _lib.PdeAdiRectDesc.W.offset == 12 and _lib.PdeAdiRectDesc.sweep.offset == 40
    assert _lib.PdeAdiRectDescF64.clamp_max.offset == 32 and _lib.PdeAdiRectDescF64.sweep.offset == 48
    # the square descriptors keep their layout (tests/test_cabi.py, tests/test_cabi_f64.py)
    assert C.sizeof(_lib.PdeAdiDesc) == 9 * 4 + 16 * _lib.PDE_MAX_SWEEPS and _lib.PdeAdiDesc.N.offset == 8


def test_supported_shapes():
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    got = [lib.pde_adi_rect_supported(h, w) for h, w in ((1, 8), (2, 2), (2, 128), (128, 2), (129, 8), (8, 129))]
    assert got == [0, 1, 1, 1, 0, 0]
    assert _lib.PDE_MAX_N_GENERIC == 128 and lib.pde_adi_rect_supported(128, 128) == 1 and lib.pde_adi_rect_supported(0, 0) == 0


def _desc(f64, H, W, B=2, Cc=3, S=3):
    from cnn_with_pde_amd import _lib
    d = _lib.PdeAdiRectDescF64() if f64 else _lib.PdeAdiRectDesc()
    d.B, d.C, d.H, d.W, d.num_sweeps = B, Cc, H, W, S
    d.io_dtype = _lib.PDE_IO_F64 if f64 else _lib.PDE_IO_F32
    d.eps = 1e-6
    for s in range(S):
        d.sweep[s].axis, d.sweep[s].delta, d.sweep[s].h2, d.sweep[s].t = s % 2, 0.01, 1.0, 0.0
    return d


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_workspace_queries(f64):
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    fam = "pde_adi_rect_f64_" if f64 else "pde_adi_rect_"
    fwd, bwd = getattr(lib, fam + "forward_workspace_bytes"), getattr(lib, fam + "backward_workspace_bytes")
    for hw in ((1, 8), (8, 129), (129, 8), (0, 5)):                       # refused descriptors: 0
        d = _desc(f64, *hw)
        assert fwd(C.byref(d)) == 0 and bwd(C.byref(d), 0) == 0
    assert fwd(None) == 0 and bwd(None, 0) == 0
    d = _desc(f64, 20, 36)
    d.io_dtype = _lib.PDE_IO_F32 if f64 else _lib.PDE_IO_F64              # the other family's type
    assert fwd(C.byref(d)) == 0
    d = _desc(f64, 20, 36)
    assert bwd(C.byref(d), -1) == 0 and bwd(C.byref(d), 3) == 0          # at most num_sweeps - 1 checkpoints
    # the factorisation is 4 arrays of H*W per (sweep, channel), a checkpoint B*C*H*W: both grow with H*W, not with a side
    sz = 8 if f64 else 4
    f1, f2 = fwd(C.byref(_desc(f64, 20, 36))), fwd(C.byref(_desc(f64, 40, 36)))
    assert f1 >= 3 * 3 * 4 * 20 * 36 * sz and f2 - f1 == 3 * 3 * 4 * 20 * 36 * sz
    assert fwd(C.byref(_desc(f64, 36, 20))) == f1                          # H*W alone
    b0, b1 = bwd(C.byref(_desc(f64, 20, 36)), 0), bwd(C.byref(_desc(f64, 20, 36)), 1)
    assert b0 > f1 and b1 - b0 >= 2 * 3 * 20 * 36 * sz
    assert bwd(C.byref(_desc(f64, 40, 36)), 1) > b1


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_refusal_codes_without_gpu(f64):
    """Descriptor checks come first, then pointers, then the workspace — all on the host."""
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    fam = "pde_adi_rect_f64_" if f64 else "pde_adi_rect_"
    fwd, bwd, kmax = getattr(lib, fam + "forward"), getattr(lib, fam + "backward"), getattr(lib, fam + "kappa_max")
    nf = 9 if f64 else 11                                                   # pointer arguments between d and the workspace size
    buf = (C.c_double * 4096)()
    p = C.cast(buf, C.c_void_p)
    misaligned = C.c_void_p(p.value + 4)
    mask = (C.c_uint64 * 2)(0, 0)

    def forward(d, ptr, ws, nbytes):
        mid = [ptr] * 6 + ([None] if f64 else [None, None, None])            # u, y, four parameters; no maxima
        return fwd(None if d is None else C.byref(d), *mid, ws, nbytes, None)

    def backward(d, ptr, ws, nbytes, m=mask, u=None):
        return bwd(C.byref(d), ptr, ptr, u, m, *([ptr] * 9), None, ws, nbytes, None)

    assert nf == len(_lib.SIGNATURES[fam + "forward"][1]) - 2
    for hw in ((1, 8), (8, 129), (129, 8)):
        d = _desc(f64, *hw)
        assert forward(d, None, None, 0) == -2 and backward(d, None, None, 0) == -2
        assert kmax(C.byref(d), None, None, None, None, None, None) == -2
    d = _desc(f64, 20, 36)
    assert forward(None, p, p, 1 << 40) == -1                                          # no descriptor
    assert forward(d, None, None, 0) == -1 and backward(d, None, None, 0) == -1      # null pointers
    assert kmax(C.byref(d), None, None, None, None, None, None) == -1
    assert forward(d, p, p, 16) == -5 and backward(d, p, p, 16) == -5                # short workspace
    big = 1 << 40
    assert forward(d, p, misaligned, big) == -5 and backward(d, p, misaligned, big) == -5
    d.num_sweeps = _lib.PDE_MAX_SWEEPS + 1
    assert forward(d, p, p, big) == -3
    d = _desc(f64, 20, 36)
    d.sweep[1].axis = 2
    assert forward(d, p, p, big) == -1
    d = _desc(f64, 20, 36)
    d.B = 0
    assert forward(d, p, p, big) == -1
    d = _desc(f64, 20, 36)
    assert backward(d, p, p, big, (C.c_uint64 * 2)(1, 0), None) == -1                 # a checkpoint needs u
    assert backward(d, p, p, big, (C.c_uint64 * 2)(0b100, 0), p) == -1                # the last state is y itself
    if not f64:
        d = _desc(f64, 20, 36)                                                         # host copy of the maxima needs the device buffer
        assert lib.pde_adi_rect_forward(C.byref(d), p, p, p, p, p, p, None, p, None, p, big, None) == -1


def test_square_pins_still_hold():
    """What tests/test_cabi.py and the GPU tests pin for squares: N = 130 is refused, 30 goes to the any-size path, 32 to
    the fused kernels, and the square any-size entry keeps sizing its workspace by N*N."""
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    assert [lib.pde_adi_line_length_path(n) for n in (1, 2, 6, 8, 28, 30, 32, 36, 64, 128, 129)] == \
        [0, 2, 2, 1, 1, 2, 1, 2, 2, 2, 0]
    d = _lib.PdeAdiDesc()
    d.B, d.C, d.N, d.num_sweeps = 1, 1, 130, 3
    assert lib.pde_adi_forward_workspace_bytes(C.byref(d)) == 0
    assert lib.pde_adi_forward(C.byref(d), None, None, None, None, None, None, None, None, None, None, 0, None) == -2
    d.B, d.C, d.N = 2, 3, 36
    r = _desc(False, 36, 36)
    assert lib.pde_adi_forward_workspace_bytes(C.byref(d)) == lib.pde_adi_rect_forward_workspace_bytes(C.byref(r)) > 0
    assert lib.pde_adi_backward_workspace_bytes(C.byref(d), 1) == lib.pde_adi_rect_backward_workspace_bytes(C.byref(r), 1) > 0
