"""The float16 tensor type of the C ABI (PDE_IO_F16) on a machine without a GPU: every family's workspace query takes it,
the host-side argument checks stay as strict as before, and the typed Jacobi twins are declared and exported."""
import ctypes as C


def _desc(B=2, Cc=3, N=32, S=9, io=3):
    from cnn_with_pde_amd import _lib as L
    d = L.PdeAdiDesc()
    d.B, d.C, d.N, d.io_dtype, d.num_sweeps, d.eps = B, Cc, N, io, S, 1e-6
    for s in range(S):                                             # Strang steps: x(dt/2) y(dt) x(dt/2)
        d.sweep[s].axis = 1 if s % 3 == 1 else 0
        d.sweep[s].delta = 0.002 if s % 3 == 1 else 0.001
        d.sweep[s].h2, d.sweep[s].t = 1.0, 0.001 * s
    return d


def test_header_value():
    from cnn_with_pde_amd import _lib as L
    assert L.PDE_IO_F16 == 3 and L.PDE_IO_F64 == 2


def test_workspace_queries_take_f16():
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    for N in (32, 28, 36):                                         # fused line lengths and one any-size length
        d = _desc(N=N)
        assert lib.pde_adi_forward_workspace_bytes(C.byref(d)) > 0, N
        assert lib.pde_adi_backward_workspace_bytes(C.byref(d), 2) > 0, N
    d = _desc()
    assert lib.pde_adi_steps_workspace_bytes(C.byref(d), 3) > 0
    assert lib.pde_adi_backward_step_workspace_bytes(C.byref(d), 3, 1) > 0
    assert lib.pde_adi_mixed_backward_workspace_bytes(C.byref(d), 3, 1) > 0
    assert lib.pde_adi_small_backward_workspace_bytes(C.byref(d), 3, 1) > 0
    assert lib.pde_adi_small_supported(C.byref(d), 3) == 1
    assert lib.pde_explicit5_backward_workspace_bytes(2, 3, 20, 20, L.PDE_IO_F16, 3) > 0
    assert lib.pde_jacobi_io_backward_workspace_bytes(2, 48, 48, 10, L.PDE_IO_F16) > 0
    assert lib.pde_jacobi_io_backward_workspace_bytes(2, 48, 48, 10, L.PDE_IO_F32) == \
        lib.pde_jacobi_backward_workspace_bytes(2, 48, 48, 10)


def test_kernel_choice_for_f16_descriptors():
    """fp16 takes the HIP kernels and the per-step path: the assembly backward and the one-launch wide forward are
    fp32-only."""
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    d = _desc(Cc=64, S=30)
    assert lib.pde_adi_backward_kernel(C.byref(d), 0) == 0
    assert lib.pde_adi_forward_kernel(C.byref(d)) == 0
    assert lib.pde_adi_mixed_one_launch(C.byref(d), 3) == 0
    assert lib.pde_adi_backward_kernel(C.byref(_desc(N=36)), 0) == 2      # any-size kernels


def test_null_pointers_still_rejected():
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    d = _desc()
    assert lib.pde_adi_forward(C.byref(d), None, None, None, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.pde_channel_mix_forward(2, 3, 16, L.PDE_IO_F16, None, None, None, None) == -1
    assert lib.pde_skip_blend_forward(16, L.PDE_IO_F16, None, None, None, None, None) == -1
    assert lib.pde_explicit5_forward(1, 1, 8, 8, L.PDE_IO_F16, None, None, None, 0.01, 1e-6, 0.15, 0.1, 1, None, None,
                                     None) == -1
    assert lib.pde_jacobi_io_forward(1, 8, 8, 2, L.PDE_IO_F16, None, None, None, None, None) == -1
    assert lib.pde_jacobi_io_backward(1, 8, 8, 2, L.PDE_IO_F16, None, None, None, None, None, None, None, None, 0,
                                      None) == -1


def test_unknown_io_dtype_rejected():
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    d = _desc(io=4)
    assert lib.pde_adi_forward_workspace_bytes(C.byref(d)) == 0
    assert lib.pde_adi_forward(C.byref(d), None, None, None, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.pde_adi_small_supported(C.byref(d), 3) == 0
    assert lib.pde_jacobi_io_backward_workspace_bytes(2, 48, 48, 10, 4) == 0
    p = C.c_void_p(16)                                             # never dereferenced: the type is checked first
    assert lib.pde_gate_combine_forward(1, 1, 1, 16, 4, (C.c_void_p * 1)(p), (C.c_void_p * 1)(p), p, p, None) == -1
    assert lib.pde_jacobi_io_forward(1, 8, 8, 2, 4, p, p, p, p, None) == -1


def test_typed_jacobi_entry_points_are_declared_and_exported():
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    for name in ("pde_jacobi_io_forward", "pde_jacobi_io_backward_workspace_bytes", "pde_jacobi_io_backward"):
        assert name in L.SIGNATURES and hasattr(lib, name)
