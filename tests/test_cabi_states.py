"""The trajectory entry points of the C ABI (pde_adi*_forward_states / pde_adi*_backward_states) without a GPU: the header,
the library's exports and the ctypes table agree, and every argument check runs on the host before any launch — the
pointers handed over here are host buffers no kernel may touch."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["pde_adi_", "pde_adi_rect_", "pde_adi_f64_", "pde_adi_rect_f64_"]
BADARG, UNSUPPORTED_N, TOO_MANY, WORKSPACE = -1, -2, -3, -5


def _header():
    src = open(os.path.join(ROOT, "include", "pdecnn.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_exports_and_table_agree():
    from cnn_with_pde_amd import _lib
    src = _header()
    lib = C.CDLL(_lib.LIB_PATH)
    for fam in FAMILIES:
        for name in (fam + "forward_states", fam + "backward_states"):
            assert re.search(r"\b%s\s*\(" % name, src), f"{name} not declared in pdecnn.h"
            assert hasattr(lib, name), f"{name} not exported"
            assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
            # the plain call's arguments plus the states tensor and the emission mask
            plain = _lib.SIGNATURES[name[:-len("_states")]][1]
            assert len(_lib.SIGNATURES[name][1]) == len(plain) + 2, name
    # the descriptors keep their layout
    assert C.sizeof(_lib.PdeAdiDesc) == 9 * 4 + 16 * _lib.PDE_MAX_SWEEPS


def _desc(fam, n, sweeps):
    from cnn_with_pde_amd import _lib
    f64 = "f64" in fam
    d = {"pde_adi_": _lib.PdeAdiDesc, "pde_adi_rect_": _lib.PdeAdiRectDesc, "pde_adi_f64_": _lib.PdeAdiDescF64,
         "pde_adi_rect_f64_": _lib.PdeAdiRectDescF64}[fam]()
    d.B, d.C, d.num_sweeps = 2, 1, sweeps
    if "rect" in fam:
        d.H, d.W = n, max(n - 1, 1) if n <= 128 else n
    else:
        d.N = n
    d.io_dtype = _lib.PDE_IO_F64 if f64 else _lib.PDE_IO_F32
    d.eps = 1e-6
    for s in range(min(sweeps, _lib.PDE_MAX_SWEEPS)):
        d.sweep[s].axis, d.sweep[s].delta, d.sweep[s].h2, d.sweep[s].t = s % 2, 0.01, 1.0, 0.0
    return d


def _calls(fam, d, states, mask, ws_bytes=0):
    """(forward_states rc, backward_states rc) with every other pointer a valid host buffer."""
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    em = (C.c_uint64 * 2)(mask & (2 ** 64 - 1), mask >> 64) if mask is not None else None
    ck = (C.c_uint64 * 2)(0, 0)
    st = p if states else None
    if "f64" in fam:
        fwd = getattr(lib, fam + "forward_states")(C.byref(d), p, p, st, em, p, p, p, p, None, p, ws_bytes, None)
    else:
        fwd = getattr(lib, fam + "forward_states")(C.byref(d), p, p, st, em, p, p, p, p, None, None, None, p, ws_bytes, None)
    bwd = getattr(lib, fam + "backward_states")(C.byref(d), p, st, em, p, None, ck, p, p, p, p, p, p, p, p, p, None, p,
                                                ws_bytes, None)
    return fwd, bwd


@pytest.mark.parametrize("fam", FAMILIES)
def test_argument_validation_without_gpu(fam):
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    # unsupported line lengths before anything else
    for n in (1, 130):
        assert _calls(fam, _desc(fam, n, 6), True, 0b1) == (UNSUPPORTED_N, UNSUPPORTED_N), n
    # both kernel families of the square fp32 entry points, the any-size kernels elsewhere
    for n in (32, 30):
        d = _desc(fam, n, 6)
        # a non-empty mask without a tensor
        assert _calls(fam, d, False, 0b00100) == (BADARG, BADARG), n
        # a bit at or above S-1: the last state is y itself; far above; in the high word
        for mask in (1 << 5, 1 << 6, 1 << 63, 1 << 64, 1 << 127, 0b100100):
            assert _calls(fam, d, True, mask) == (BADARG, BADARG), (n, mask)
        # everything in order up to the workspace: the checks above come before it, and nothing is launched
        assert _calls(fam, d, True, 0b10100, ws_bytes=0) == (WORKSPACE, WORKSPACE), n
        # an empty mask is the plain call: states is not looked at (null or not), the mask may be null
        assert _calls(fam, d, False, 0, ws_bytes=0) == (WORKSPACE, WORKSPACE), n
        assert _calls(fam, d, False, None, ws_bytes=0) == (WORKSPACE, WORKSPACE), n
        assert _calls(fam, d, True, 0, ws_bytes=0) == (WORKSPACE, WORKSPACE), n
        # null pointers of the plain call
        name = fam + "forward_states"
        nargs = len(_lib.SIGNATURES[name][1])
        assert getattr(lib, name)(C.byref(d), *([None] * (nargs - 3)), 0, None) == BADARG
        name = fam + "backward_states"
        nargs = len(_lib.SIGNATURES[name][1])
        assert getattr(lib, name)(C.byref(d), *([None] * (nargs - 3)), 0, None) == BADARG
    d = _desc(fam, 32, _lib.PDE_MAX_SWEEPS + 1)
    assert _calls(fam, d, True, 0b1) == (TOO_MANY, TOO_MANY)
    # the workspace queries are those of the plain calls
    d = _desc(fam, 32, 6)
    assert getattr(lib, fam + "forward_workspace_bytes")(C.byref(d)) > 0
    assert getattr(lib, fam + "backward_workspace_bytes")(C.byref(d), 0) > 0


def test_python_surface_exists():
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import functional as F_
    assert callable(F_.adi_diffuse_states) and callable(P.adi_diffuse_states)
    for cls in (P.MnistDiffusionLayer, P.FashionDiffusionLayer, P.SvhnDiffusionLayer, P.EnhancedDiffusionLayer,
                P.LearnableDiffusionLayer):
        assert callable(getattr(cls, "trajectory"))
    assert not hasattr(P.ImprovedDiffusionLayer, "trajectory") and not hasattr(P.PDELayer, "trajectory")


def test_step_selection_is_checked_before_any_launch():
    """``steps`` is validated on the host: these calls run on CPU tensors and must fail with ValueError, not with the
    PdeError a launch attempt on CPU tensors gives."""
    import contextlib
    import io

    import torch
    import cnn_with_pde_amd as P
    with contextlib.redirect_stdout(io.StringIO()):
        ly = P.EnhancedDiffusionLayer(8, 2, num_steps=4, channel_mixing_enabled=False)
    u = torch.zeros(1, 2, 8, 8)
    for bad in ([0], [3, 2], [5], [], [2, 2], [1.5], "ab"):
        with pytest.raises(ValueError):
            ly.trajectory(u, bad)
    with pytest.raises(P.PdeError):
        ly.trajectory(u, [1, 4])
    with pytest.raises(P.PdeError):
        ly.trajectory(u)
