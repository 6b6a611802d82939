"""The tiled Jacobi path (planes with H > 64 or W > 64, up to PDE_JACOBI_MAX_HW) as the C ABI shows it on a machine
without a GPU: the path query, the workspace sizes and the argument validation.  No compute calls."""
import ctypes as C

import pytest


def _lib():
    from cnn_with_pde_amd import _lib as L
    return L, L.load()


def test_plane_path_query():
    L, lib = _lib()
    cases = [(3, 8), (4, 4), (64, 64), (65, 8), (8, 65), (224, 224), (1024, 1024), (1025, 8)]
    assert [lib.pde_jacobi_plane_path(h, w) for h, w in cases] == [0, 1, 1, 2, 2, 2, 2, 0]
    assert L.PDE_JACOBI_MAX_HW == 1024


def test_header_states_the_limit_and_the_depth():
    import os
    import re
    L, _ = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pdecnn.h")).read()
    assert int(re.search(r"#define\s+PDE_JACOBI_MAX_HW\s+(\d+)", src).group(1)) == L.PDE_JACOBI_MAX_HW == 1024
    assert int(re.search(r"#define\s+PDE_JACOBI_TILED_K\s+(\d+)", src).group(1)) == L.PDE_JACOBI_TILED_K


def _align256(x):
    return (x + 255) // 256 * 256


def test_workspace_bytes():
    L, lib = _lib()
    assert lib.pde_jacobi_backward_workspace_bytes(2, 96, 96, 10) > 0
    assert lib.pde_jacobi_backward_workspace_bytes(1, 1024, 1024, 3) > 0
    assert lib.pde_jacobi_backward_workspace_bytes(1, 1025, 8, 3) == 0
    assert lib.pde_jacobi_backward_workspace_bytes(1, 8, 1025, 3) == 0
    # the one-workgroup path keeps its size: nt padded states per sample, then H + W partial sums per sample
    B, H, W, nt = 2, 48, 48, 10
    want = _align256(B * nt * (H + 2) * (W + 2) * 4) + _align256(B * (H + W) * 4)
    assert lib.pde_jacobi_backward_workspace_bytes(B, H, W, nt) == want
    for io in (L.PDE_IO_F32, L.PDE_IO_BF16, L.PDE_IO_F16):
        assert lib.pde_jacobi_io_backward_workspace_bytes(B, H, W, nt, io) == want
        assert lib.pde_jacobi_io_backward_workspace_bytes(2, 96, 96, 10, io) == lib.pde_jacobi_backward_workspace_bytes(2, 96, 96, 10)
    # the parked states are what grows with nt: nt - 1 interior images per sample
    d = lib.pde_jacobi_backward_workspace_bytes(2, 96, 96, 10) - lib.pde_jacobi_backward_workspace_bytes(2, 96, 96, 9)
    assert 2 * 96 * 96 * 4 <= d <= 2 * 96 * 96 * 4 + 256


def test_forward_workspace_bytes():
    L, lib = _lib()
    K = L.PDE_JACOBI_TILED_K
    assert lib.pde_jacobi_forward_workspace_bytes(2, 96, 96, K) == 0          # one launch: no image between launches
    assert lib.pde_jacobi_forward_workspace_bytes(2, 96, 96, K + 1) == 2 * _align256(2 * 96 * 96 * 4)
    assert lib.pde_jacobi_forward_workspace_bytes(2, 48, 48, 100) == 0        # the one-workgroup path never needs one
    assert lib.pde_jacobi_forward_workspace_bytes(2, 1025, 8, 100) == 0


def test_argument_validation_without_gpu():
    L, lib = _lib()
    for H, W in ((96, 96), (1025, 8)):
        assert lib.pde_jacobi_forward(1, H, W, 2, None, None, None, None, None) == -1
        assert lib.pde_jacobi_io_forward(1, H, W, 2, L.PDE_IO_F16, None, None, None, None, None) == -1
        assert lib.pde_jacobi_io_forward_ws(1, H, W, 2, L.PDE_IO_F32, None, None, None, None, None, 0, None) == -1
        assert lib.pde_jacobi_backward(1, H, W, 2, None, None, None, None, None, None, None, None, 0, None) == -1
        assert lib.pde_jacobi_io_backward(1, H, W, 2, L.PDE_IO_BF16, None, None, None, None, None, None, None, None, 0,
                                          None) == -1
    # valid pointers, a size no path serves / an I/O type that does not exist: still host-side refusals
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    fp = C.cast(buf, C.POINTER(C.c_float))
    assert lib.pde_jacobi_forward(1, 1025, 8, 2, fp, fp, fp, fp, None) == -1
    assert lib.pde_jacobi_io_forward(1, 96, 96, 2, 4, p, fp, fp, p, None) == -1
    assert lib.pde_jacobi_io_backward(1, 96, 96, 2, L.PDE_IO_F32, p, p, fp, fp, p, fp, fp, p, 16, None) == -5   # workspace
    # more steps than one launch takes, and no workspace to chain the launches through
    assert lib.pde_jacobi_io_forward(1, 96, 96, L.PDE_JACOBI_TILED_K + 1, L.PDE_IO_F32, p, fp, fp, p, None) == -5
