"""The trajectory entry points of the explicit layers (pde_jacobi_io_*_states, pde_jacobi_f64_*_states,
pde_explicit5_*_states, pde_explicit5_f64_*_states) without a GPU, as test_cabi_states.py does for the ADI families: the
header, the library's exports and the ctypes table agree, and every argument check runs on the host before any launch —
the pointers handed over here are host buffers no kernel may touch, so every call below must come back refused."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# family -> the plain calls the two *_states entry points extend
FAMILIES = {"pde_jacobi_io_": ("pde_jacobi_io_forward_ws", "pde_jacobi_io_backward"),
            "pde_jacobi_f64_": ("pde_jacobi_f64_forward", "pde_jacobi_f64_backward"),
            "pde_explicit5_": ("pde_explicit5_forward", "pde_explicit5_backward"),
            "pde_explicit5_f64_": ("pde_explicit5_f64_forward", "pde_explicit5_f64_backward")}
OK, BADARG, TOO_MANY, WORKSPACE = 0, -1, -3, -5


def _header():
    src = open(os.path.join(ROOT, "include", "pdecnn.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_exports_and_table_agree():
    from cnn_with_pde_amd import _lib
    src = _header()
    lib = C.CDLL(_lib.LIB_PATH)
    for fam, plain in FAMILIES.items():
        for name, base in zip((fam + "forward_states", fam + "backward_states"), plain):
            assert re.search(r"\b%s\s*\(" % name, src), f"{name} not declared in pdecnn.h"
            assert hasattr(lib, name), f"{name} not exported"
            assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
            # the plain call's arguments plus the states tensor and the emission mask
            assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[base][1]) + 2, name
            assert _lib.SIGNATURES[name][1].count(C.POINTER(C.c_uint64)) == 1, name
            # and the header's parameter list is as long as the table's
            decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S).group(1)
            assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


def _mask(bits):
    return None if bits is None else (C.c_uint64 * 2)(bits & (2 ** 64 - 1), bits >> 64)


def _calls(fam, H, W, nt, states, bits, ws_bytes=0, B=2, only=None):
    """(forward_states rc, backward_states rc) with every other pointer a valid host buffer; ``only``: "fwd" / "bwd" makes
    that call alone and returns its code.  A call whose arguments are in order up to the workspace is only ever made where
    the workspace check (ws_bytes = 0) stops it: the backwards, and the tiled Jacobi forward beyond one launch."""
    if only is not None:
        return _calls_lazy(fam, H, W, nt, states, bits, ws_bytes, B)[0 if only == "fwd" else 1]()
    return tuple(c() for c in _calls_lazy(fam, H, W, nt, states, bits, ws_bytes, B))


def _calls_lazy(fam, H, W, nt, states, bits, ws_bytes, B):
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fp = C.cast(buf, C.POINTER(C.c_float))
    st = p if states else None
    em = _mask(bits)
    f, b = getattr(lib, fam + "forward_states"), getattr(lib, fam + "backward_states")
    if fam == "pde_jacobi_io_":
        return (lambda: f(B, H, W, nt, _lib.PDE_IO_F32, p, fp, fp, p, st, em, p, ws_bytes, None),
                lambda: b(B, H, W, nt, _lib.PDE_IO_F32, p, p, st, em, fp, fp, p, fp, fp, p, ws_bytes, None))
    if fam == "pde_jacobi_f64_":
        return (lambda: f(B, H, W, nt, p, p, p, p, st, em, None),
                lambda: b(B, H, W, nt, p, p, st, em, p, p, p, p, p, p, ws_bytes, None))
    if fam == "pde_explicit5_":
        return (lambda: f(B, 3, H, W, _lib.PDE_IO_F32, p, fp, fp, 0.5, 1e-6, 0.125, 0.1, nt, p, p, st, em, None),
                lambda: b(B, 3, H, W, _lib.PDE_IO_F32, p, p, p, st, em, fp, fp, 0.5, 1e-6, 0.125, 0.1, nt, p, fp, fp, p, ws_bytes,
                          None))
    return (lambda: f(B, 3, H, W, p, p, p, 0.5, 1e-6, 0.125, 0.1, nt, p, p, st, em, None),
            lambda: b(B, 3, H, W, p, p, p, st, em, p, p, 0.5, 1e-6, 0.125, 0.1, nt, p, p, p, p, ws_bytes, None))


# per family: planes of every kernel path it has (Jacobi: one-workgroup and tiled; explicit: wave and generic)
PLANES = {"pde_jacobi_io_": [(7, 9), (65, 8)], "pde_jacobi_f64_": [(7, 9)], "pde_explicit5_": [(16, 16), (7, 9)],
          "pde_explicit5_f64_": [(7, 9)]}


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_argument_validation_without_gpu(fam):
    for H, W in PLANES[fam]:
        nt = 6
        # a non-empty mask without a tensor
        assert _calls(fam, H, W, nt, False, 0b00100) == (BADARG, BADARG), (H, W)
        # a bit at or above nt-1: the last state is `out` itself; far above; in the high word
        for bits in (1 << 5, 1 << 6, 1 << 63, 1 << 64, 1 << 127, 0b100100):
            assert _calls(fam, H, W, nt, True, bits) == (BADARG, BADARG), (H, W, bits)
        # a single step has no state but `out`
        assert _calls(fam, H, W, 1, True, 0b1) == (BADARG, BADARG), (H, W)
        # more steps than the mask has bits, whatever the bits
        for bits in (0b1, 1 << 127):
            assert _calls(fam, H, W, 129, True, bits) == (TOO_MANY, TOO_MANY), (H, W, bits)
        # 128 steps are served: bit 127 is then the last state's, bit 126 passes on to the workspace check
        assert _calls(fam, H, W, 128, True, 1 << 127) == (BADARG, BADARG)
        assert _calls(fam, H, W, 128, True, 1 << 126, only="bwd") == WORKSPACE
        # everything in order up to the workspace: the checks above come before it, and nothing is launched
        assert _calls(fam, H, W, nt, True, 0b10100, only="bwd") == WORKSPACE, (H, W)
        # an empty mask is the plain call: the tensor is not looked at (null or not), the mask may be null
        for states, bits in ((False, 0), (False, None), (True, 0)):
            assert _calls(fam, H, W, nt, states, bits, only="bwd") == WORKSPACE, (H, W, states, bits)


def test_tiled_forward_reaches_its_workspace_check():
    """The tiled Jacobi forward is the one forward with a workspace (nt > PDE_JACOBI_TILED_K): the mask checks come first."""
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    nt = _lib.PDE_JACOBI_TILED_K + 2
    assert lib.pde_jacobi_plane_path(65, 8) == 2 and lib.pde_jacobi_forward_workspace_bytes(2, 65, 8, nt) > 0
    assert _calls("pde_jacobi_io_", 65, 8, nt, True, 0b101, only="fwd") == WORKSPACE
    assert _calls("pde_jacobi_io_", 65, 8, nt, False, 0, only="fwd") == WORKSPACE
    assert _calls("pde_jacobi_io_", 65, 8, nt, False, 0b101, only="fwd") == BADARG
    assert _calls("pde_jacobi_io_", 65, 8, nt, True, 1 << (nt - 1), only="fwd") == BADARG


@pytest.mark.parametrize("H,W", [(3, 8), (8, 3), (4, 1025), (0, 8)])
def test_unserved_jacobi_planes_are_badarg(H, W):
    from cnn_with_pde_amd import _lib
    assert _lib.load().pde_jacobi_plane_path(H, W) == 0
    assert _calls("pde_jacobi_io_", H, W, 6, True, 0b1, ws_bytes=1 << 30) == (BADARG, BADARG)
    assert _calls("pde_jacobi_io_", H, W, 6, False, 0, ws_bytes=1 << 30) == (BADARG, BADARG)


def test_null_pointers_of_the_plain_calls():
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    em = _mask(0b1)
    assert lib.pde_jacobi_io_forward_states(2, 7, 9, 6, _lib.PDE_IO_F32, *([None] * 6), None, 0, None) == BADARG
    assert lib.pde_jacobi_io_backward_states(2, 7, 9, 6, _lib.PDE_IO_F32, None, None, None, em, *([None] * 6), 0, None) == BADARG
    assert lib.pde_jacobi_f64_forward_states(2, 7, 9, 6, *([None] * 7)) == BADARG
    assert lib.pde_jacobi_f64_backward_states(2, 7, 9, 6, None, None, None, em, *([None] * 6), 0, None) == BADARG
    assert lib.pde_explicit5_forward_states(2, 3, 7, 9, _lib.PDE_IO_F32, None, None, None, 0.5, 1e-6, 0.125, 0.1, 3,
                                            *([None] * 5)) == BADARG
    assert lib.pde_explicit5_f64_forward_states(2, 3, 7, 9, None, None, None, 0.5, 1e-6, 0.125, 0.1, 3, *([None] * 5)) == BADARG
    # an I/O type the explicit kernels do not take, with everything else in order
    buf = (C.c_double * 64)()
    p, fp = C.cast(buf, C.c_void_p), C.cast(buf, C.POINTER(C.c_float))
    assert lib.pde_explicit5_forward_states(2, 3, 7, 9, _lib.PDE_IO_F64, p, fp, fp, 0.5, 1e-6, 0.125, 0.1, 3, p, p, p, em,
                                            None) == BADARG
    assert lib.pde_jacobi_io_forward_states(2, 7, 9, 6, _lib.PDE_IO_F64, p, fp, fp, p, p, em, None, 0, None) == BADARG


def test_python_surface_exists():
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import functional as F_
    for name in ("jacobi_diffuse_states", "explicit5_states"):
        assert callable(getattr(F_, name)) and callable(getattr(P, name))
        assert name in F_.__all__ and name in P.__all__
    # one validation of ``steps`` for the layers' trajectory method and the functional calls
    assert "check_steps" in P.MnistDiffusionLayer.trajectory.__code__.co_names
    assert "check_steps" in P.layer_trajectory.__code__.co_names
    assert F_.check_steps(None, 3) == [1, 2, 3] and F_.check_steps((2, 5), None) == [2, 5]
    assert callable(P.layer_trajectory) and "layer_trajectory" in P.__all__
    # the classes of compat/ are the classes layer_trajectory serves
    from cnn_with_pde_amd.compat import emotion_recognition, tiny_imagenet
    assert emotion_recognition.PDELayer is P.PDELayer and tiny_imagenet.ImprovedDiffusionLayer is P.ImprovedDiffusionLayer


def test_step_selection_is_checked_before_any_launch():
    """``steps`` is validated on the host: these calls run on CPU tensors and must fail with ValueError, not with the
    PdeError a launch attempt on CPU tensors gives."""
    import torch
    import cnn_with_pde_amd as P
    pl = P.PDELayer(Nx=24, Ny=20, Lx=2.0, Ly=2.0, T=0.004)
    ti = P.ImprovedDiffusionLayer(16, 3, num_steps=4)
    up, ut = torch.zeros(1, 20, 24), torch.zeros(1, 3, 16, 16)
    jac = lambda steps: P.jacobi_diffuse_states(up, pl.alpha(pl.y), pl.beta(pl.x), steps)                      # noqa: E731
    exp = lambda steps: P.explicit5_states(ut, ti.alpha_base, ti.channel_scaling, steps=steps)                # noqa: E731
    # empty, zero, not increasing, repeated, not whole, not numbers, no selection at all; beyond the 128 bits of the mask
    for bad in ([], [0], [3, 2], [2, 2], [1.5], "ab", None, [129], [1, 129], range(1, 201)):
        with pytest.raises(ValueError):
            jac(bad)
        with pytest.raises(ValueError):
            exp(bad)
    for call in (jac, exp):
        with pytest.raises(P.PdeError):
            call([1, 4])
        with pytest.raises(P.PdeError):
            call(range(1, 129))
    # the layer-level entry: None is every step, the layer's own time loop is the upper end
    long = P.PDELayer(Nx=24, Ny=20, T=0.2)
    assert pl.Nt == 4 and long.Nt > 128
    up4 = up.unsqueeze(1)
    for bad in ([0], [3, 2], [5], [], [2, 2], [1.5], "ab"):
        with pytest.raises(ValueError):
            P.layer_trajectory(pl, up4, bad)
        with pytest.raises(ValueError):
            P.layer_trajectory(ti, ut, bad)
    with pytest.raises(ValueError):
        P.layer_trajectory(pl, up)                              # (B,H,W): refused as forward refuses it
    for steps in ([129], [1, 129], None):
        with pytest.raises(ValueError):
            P.layer_trajectory(long, up4, steps)
    for layer, u in ((pl, up4), (ti, ut)):
        with pytest.raises(P.PdeError):
            P.layer_trajectory(layer, u, [1, 4])
        with pytest.raises(P.PdeError):
            P.layer_trajectory(layer, u)
    with pytest.raises(TypeError):
        P.layer_trajectory(torch.nn.Identity(), ut)
