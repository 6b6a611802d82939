"""The float64 entry points of the C ABI (include/pdecnn.h) on a machine without a GPU: struct layout, argument checks that
run on the host before any device work, and no CPU fallback for float64 tensors."""
import ctypes as C

import pytest
import torch


def _desc(B=2, Cc=3, N=8, S=3):
    from cnn_with_pde_amd import _lib as L
    d = L.PdeAdiDescF64()
    d.B, d.C, d.N, d.io_dtype, d.num_sweeps, d.eps = B, Cc, N, L.PDE_IO_F64, S, 1e-6
    for s in range(min(S, L.PDE_MAX_SWEEPS)):
        d.sweep[s].axis, d.sweep[s].delta, d.sweep[s].h2, d.sweep[s].t = s % 2, 0.001, 1.0, 0.0005 * s
    return d


def test_struct_sizes_match_header():
    from cnn_with_pde_amd import _lib as L
    assert C.sizeof(L.PdeSweepF64) == 32                           # int32 axis, int32 pad, 3 doubles
    assert C.sizeof(L.PdeAdiDescF64) == 8 * 4 + 2 * 8 + 32 * L.PDE_MAX_SWEEPS
    assert L.PdeAdiDescF64.clamp_max.offset == 32 and L.PdeAdiDescF64.sweep.offset == 48


def test_f64_symbols_are_declared_and_loaded():
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    for name in ("pde_adi_f64_forward", "pde_adi_f64_backward", "pde_channel_mix_f64_backward_steps",
                 "pde_skip_blend_f64_backward", "pde_explicit5_f64_backward", "pde_jacobi_f64_backward"):
        assert name in L.SIGNATURES and hasattr(lib, name)


def test_adi_f64_rejects_bad_descriptors_without_gpu():
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    d = _desc()
    assert lib.pde_adi_f64_forward_workspace_bytes(C.byref(d)) > 0
    assert lib.pde_adi_f64_backward_workspace_bytes(C.byref(d), 2) > 0
    assert lib.pde_adi_f64_forward(C.byref(d), None, None, None, None, None, None, None, None, 0, None) == -1   # nulls
    for N in (1, 129):
        d = _desc(N=N)
        assert lib.pde_adi_f64_forward_workspace_bytes(C.byref(d)) == 0
        assert lib.pde_adi_f64_forward(C.byref(d), None, None, None, None, None, None, None, None, 0, None) == -2
    for N in (2, 100, 101, 128):                                   # every length, both backward layouts
        assert lib.pde_adi_f64_backward_workspace_bytes(C.byref(_desc(N=N)), 0) > 0
    d = _desc(S=L.PDE_MAX_SWEEPS + 1)
    assert lib.pde_adi_f64_forward(C.byref(d), None, None, None, None, None, None, None, None, 0, None) == -3
    d = _desc(S=0)
    assert lib.pde_adi_f64_forward_workspace_bytes(C.byref(d)) == 0
    d = _desc()
    d.sweep[1].axis = 2                                            # bad axis
    assert lib.pde_adi_f64_forward_workspace_bytes(C.byref(d)) == 0
    assert lib.pde_adi_f64_forward(C.byref(d), None, None, None, None, None, None, None, None, 0, None) == -1
    d = _desc(B=0)
    assert lib.pde_adi_f64_forward_workspace_bytes(C.byref(d)) == 0
    assert lib.pde_adi_f64_backward_workspace_bytes(C.byref(d), 0) == 0
    d = _desc()
    d.io_dtype = L.PDE_IO_F32                                      # the float64 descriptor says so
    assert lib.pde_adi_f64_forward_workspace_bytes(C.byref(d)) == 0


def test_float32_entry_points_still_reject_an_unknown_io_dtype():
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    d = L.PdeAdiDesc()
    d.B, d.C, d.N, d.num_sweeps, d.io_dtype = 1, 1, 32, 3, L.PDE_IO_F64
    assert lib.pde_adi_forward_workspace_bytes(C.byref(d)) == 0
    assert lib.pde_adi_forward(C.byref(d), None, None, None, None, None, None, None, None, None, None, 0, None) == -1


def test_other_f64_entry_points_check_arguments_on_the_host():
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    assert lib.pde_channel_mix_f64_forward(0, 3, 16, None, None, None, None) == -1
    assert lib.pde_channel_mix_f64_forward(2, 129, 16, None, None, None, None) == -1
    assert lib.pde_channel_mix_f64_backward_workspace_bytes(2, 129, 16) == 0
    assert lib.pde_channel_mix_f64_backward_workspace_bytes(2, 128, 16) > 0
    assert lib.pde_channel_mix_f64_backward(2, 3, 16, None, None, None, None, None, None, 0, None) == -1
    assert lib.pde_skip_blend_f64_backward_workspace_bytes(0) == 0
    assert lib.pde_skip_blend_f64_forward(0, None, None, None, None, None) == -1
    assert lib.pde_explicit5_f64_forward(0, 1, 8, 8, None, None, None, 0.01, 1e-6, 0.15, 0.1, 1, None, None, None) == -1
    assert lib.pde_explicit5_f64_backward_workspace_bytes(1, 1, 8, 8, 0) == 0
    assert lib.pde_jacobi_f64_backward_workspace_bytes(1, 65, 8, 10) == 0
    assert lib.pde_jacobi_f64_backward_workspace_bytes(1, 64, 64, 10) > 0
    assert lib.pde_jacobi_f64_forward(1, 1, 8, 10, None, None, None, None, None) == -1


def test_float64_cpu_tensors_raise():
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib as L
    u = torch.randn(2, 1, 8, 8, dtype=torch.float64)
    p = torch.ones(8, 8, dtype=torch.float64)
    sweeps = [s for st in P.adi_schedule(0.01, 1.0, 1.0, 1) for s in st]
    with pytest.raises(L.PdeError):
        P.adi_diffuse(u, p, p, p * 0, p * 0, sweeps, smooth3=True)
    with pytest.raises(L.PdeError):
        P.channel_mix(u, torch.eye(1, dtype=torch.float64))
    with pytest.raises(L.PdeError):
        P.explicit5_step(u, torch.ones(1, dtype=torch.float64), torch.ones(1, dtype=torch.float64))
    with pytest.raises(L.PdeError):
        P.jacobi_diffuse(u[:, 0], torch.ones(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64), 2)
