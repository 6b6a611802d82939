"""The fp16-operand Ruthotto-Haber entry points (include/pdecnn.h) reject bad arguments on the host, before touching the
device: null pointers, a width that is not a multiple of 64, an empty or too large batch, a missing workspace.  No GPU."""
import ctypes as C


def _lib():
    from cnn_with_pde_amd import _lib
    return _lib.load()


def test_f16_shape_rules():
    lib = _lib()
    assert lib.pde_sym_layer_f16_supported(64, 3072) == 1
    assert lib.pde_sym_layer_f16_supported(1, 64) == 1 and lib.pde_sym_layer_f16_supported(128, 192) == 1
    for B, D in [(0, 64), (-1, 64), (129, 3072), (64, 96), (64, 0), (64, 32)]:
        assert lib.pde_sym_layer_f16_supported(B, D) == 0
        assert lib.pde_sym_layer_f16_workspace_bytes(B, D) == 0
    assert lib.pde_sym_layer_f16_workspace_bytes(64, 3072) > 0


def test_f16_argument_validation_without_gpu():
    lib = _lib()
    fake = C.c_void_p(4096)                               # never dereferenced: validation fails before any launch
    n = lib.pde_sym_layer_f16_workspace_bytes(64, 3072)

    def fwd(B=64, D=3072, act=1, training=1, X=fake, K16=fake, P=fake, out=fake, ws=fake, nbytes=n, rm=fake):
        return lib.pde_sym_layer_f16_forward(B, D, act, training, X, K16, fake, fake, rm, rm, 0.1, 1e-5, None, -1.0,
                                             P, fake, fake, fake, out, ws, nbytes, None)

    def bwd(B=64, D=3072, act=1, g=fake, X=fake, dP=fake, gK=fake, ws=fake, nbytes=n):
        return lib.pde_sym_layer_f16_backward(B, D, act, 1, g, -1.0, X, fake, fake, fake, fake, fake, fake, dP, fake, gK,
                                              fake, fake, ws, nbytes, None)

    for kw in [dict(X=None), dict(K16=None), dict(P=None), dict(out=None), dict(B=0), dict(B=-3), dict(B=129),
               dict(D=96), dict(D=0), dict(act=3), dict(act=-1), dict(training=0, rm=None)]:
        assert fwd(**kw) == -1, kw
    for kw in [dict(g=None), dict(X=None), dict(dP=None), dict(gK=None), dict(B=0), dict(D=100), dict(act=7)]:
        assert bwd(**kw) == -1, kw
    # a workspace that is missing, too small or misaligned: PDE_E_WORKSPACE
    assert fwd(ws=None) == -5 and fwd(nbytes=n - 1) == -5 and fwd(ws=C.c_void_p(4100)) == -5
    assert bwd(ws=None) == -5 and bwd(nbytes=16) == -5
    assert lib.pde_sym_k_to_f16(96, fake, fake, None) == -1
    assert lib.pde_sym_k_to_f16(64, None, fake, None) == -1 and lib.pde_sym_k_to_f16(64, fake, None, None) == -1
    assert lib.pde_sym_k_to_f16(0, fake, fake, None) == -1
