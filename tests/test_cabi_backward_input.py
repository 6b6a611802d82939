"""The backward for the input alone (the *_backward_input entry points of include/pdecnn.h) on a machine without a GPU:
header, ctypes table and exports agree, and every refusal of the four sub-families happens on the host before anything
touches the device — with the workspace query 0 exactly where the call refuses its descriptor."""
import ctypes as C

import pytest

from test_cabi import declared_functions

FAMILIES = ["pde_adi_", "pde_adi_rect_", "pde_adi_f64_", "pde_adi_rect_f64_"]
NEW = [f + s for f in FAMILIES for s in ("backward_input_workspace_bytes", "backward_input", "backward_input_states")] + \
      ["pde_adi_backward_input_kernel"]


def test_header_table_and_exports_agree():
    from cnn_with_pde_amd import _lib
    names = declared_functions()
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n in names, f"{n} missing in pdecnn.h"
        assert n in _lib.SIGNATURES, f"{n} missing in _lib.SIGNATURES"
        assert hasattr(lib, n), f"{n} not exported"
    assert sorted(_lib.SIGNATURES) == names
    _lib.load()
    # the plain call is the _states call without (gstates, emit_mask)
    for f in FAMILIES:
        plain, states = _lib.SIGNATURES[f + "backward_input"][1], _lib.SIGNATURES[f + "backward_input_states"][1]
        assert len(states) == len(plain) + 2 and states[:2] == plain[:2] and states[4:] == plain[2:]


def _desc(fam, H, W, B=2, Cc=3, S=3):
    from cnn_with_pde_amd import _lib
    rect, f64 = "rect" in fam, "f64" in fam
    cls = {(False, False): _lib.PdeAdiDesc, (True, False): _lib.PdeAdiRectDesc, (False, True): _lib.PdeAdiDescF64,
           (True, True): _lib.PdeAdiRectDescF64}[rect, f64]
    d = cls()
    if rect:
        d.H, d.W = H, W
    else:
        d.N = H
    d.B, d.C, d.num_sweeps = B, Cc, S
    d.io_dtype = _lib.PDE_IO_F64 if f64 else _lib.PDE_IO_F32
    d.eps = 1e-6
    for s in range(S):
        # (sweeps of one axis with different delta / h2: the full backward's restriction is not this call's)
        d.sweep[s].axis, d.sweep[s].delta, d.sweep[s].h2, d.sweep[s].t = s % 2, 0.01 * (s + 1), 1.0, 0.0
    return d


def _bad_shapes(fam):
    if "rect" in fam:
        return [(1, 8), (8, 129), (129, 8), (0, 5)]
    return [(1, 1), (129, 129)]


def _good_shape(fam):
    return (20, 36) if "rect" in fam else (20, 20)


@pytest.mark.parametrize("fam", FAMILIES)
def test_workspace_query(fam):
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    q = getattr(lib, fam + "backward_input_workspace_bytes")
    fwd = getattr(lib, fam + "forward_workspace_bytes")
    assert q(None) == 0
    for hw in _bad_shapes(fam):
        assert q(C.byref(_desc(fam, *hw))) == 0
    d = _desc(fam, *_good_shape(fam))
    d.io_dtype = _lib.PDE_IO_F32 if "f64" in fam else _lib.PDE_IO_F64      # the other family's type
    assert q(C.byref(d)) == 0
    d = _desc(fam, *_good_shape(fam))
    d.num_sweeps = _lib.PDE_MAX_SWEEPS + 1
    assert q(C.byref(d)) == 0
    d = _desc(fam, *_good_shape(fam))
    d.B = 0
    assert q(C.byref(d)) == 0
    d = _desc(fam, *_good_shape(fam))
    # a factorisation and the sweep table: never more than the forward's workspace, which the call may read instead
    assert 0 < q(C.byref(d)) <= fwd(C.byref(d))
    if fam == "pde_adi_":                                                   # the any-size squares too
        d = _desc(fam, 50, 50)
        assert 0 < q(C.byref(d)) <= fwd(C.byref(d))


@pytest.mark.parametrize("fam", FAMILIES)
def test_refusal_codes_without_gpu(fam):
    """Descriptor checks come first, then pointers, then the mask, then the workspace — all on the host."""
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    plain, states = getattr(lib, fam + "backward_input"), getattr(lib, fam + "backward_input_states")
    query = getattr(lib, fam + "backward_input_workspace_bytes")
    buf = (C.c_double * 4096)()
    p = C.cast(buf, C.c_void_p)
    misaligned = C.c_void_p(p.value + 4)
    big = 1 << 40

    def call(d, ptr, ws, nbytes, fws=None):
        return plain(None if d is None else C.byref(d), ptr, ptr, ptr, ptr, ptr, ptr, fws, ws, nbytes, None)

    def call_states(d, ptr, gstates, mask, ws, nbytes, fws=None):
        return states(C.byref(d), ptr, gstates, mask, ptr, ptr, ptr, ptr, ptr, fws, ws, nbytes, None)

    empty = (C.c_uint64 * 2)(0, 0)
    for hw in _bad_shapes(fam):
        d = _desc(fam, *hw)
        want = -2
        assert call(d, None, None, 0) == want and call_states(d, None, None, None, None, 0) == want
        assert call(d, p, p, big) == want and query(C.byref(d)) == 0        # the query is 0 exactly where the call refuses
    d = _desc(fam, *_good_shape(fam))
    assert call(None, p, p, big) == -1                                       # no descriptor
    assert call(d, None, None, 0) == -1 and call_states(d, None, None, empty, None, 0) == -1     # null pointers
    assert call(d, p, None, big) == -1                                       # the workspace is required either way
    assert call(d, p, None, big, fws=p) == -1
    # each pointer on its own
    for i in range(6):
        args = [p] * 6
        args[i] = None
        assert plain(C.byref(d), *args, None, p, big, None) == -1
    assert call(d, p, p, 16) == -5 and call(d, p, p, query(C.byref(d)) - 1) == -5      # short workspace
    assert call(d, p, misaligned, big) == -5 and call(d, p, misaligned, big, fws=p) == -5
    assert call_states(d, p, None, None, p, 16) == -5 and call_states(d, p, p, empty, misaligned, big) == -5
    # the mask: S = 3, so bits 0 and 1 may be set; the state after the last sweep is the output itself
    assert call_states(d, p, None, (C.c_uint64 * 2)(1, 0), p, big) == -1     # non-empty with NULL gstates
    assert call_states(d, p, p, (C.c_uint64 * 2)(0b100, 0), p, big) == -1    # bit S-1
    assert call_states(d, p, p, (C.c_uint64 * 2)(1 << 40, 0), p, big) == -1
    assert call_states(d, p, p, (C.c_uint64 * 2)(0, 1), p, big) == -1        # bit 64
    assert call_states(d, p, p, (C.c_uint64 * 2)(1, 0), p, 16) == -5         # a good mask: the workspace is next
    d.num_sweeps = 1
    assert call_states(d, p, p, (C.c_uint64 * 2)(1, 0), p, big) == -1        # one sweep: nothing to emit
    d = _desc(fam, *_good_shape(fam))
    d.num_sweeps = _lib.PDE_MAX_SWEEPS + 1
    assert call(d, p, p, big) == -3 and query(C.byref(d)) == 0
    d = _desc(fam, *_good_shape(fam))
    d.sweep[1].axis = 2
    assert call(d, p, p, big) == -1 and query(C.byref(d)) == 0
    d = _desc(fam, *_good_shape(fam))
    d.io_dtype = _lib.PDE_IO_F32 if "f64" in fam else _lib.PDE_IO_F64
    assert call(d, p, p, big) == -1 and query(C.byref(d)) == 0


def test_kernel_query_and_old_answers():
    from cnn_with_pde_amd import _lib
    lib = _lib.load()
    k = lib.pde_adi_backward_input_kernel
    assert k(None) == -1
    got = []
    for n in (1, 2, 6, 8, 28, 30, 32, 36, 128, 129):
        got.append(k(C.byref(_desc("pde_adi_", n, n))))
    assert got == [-1, 2, 2, 0, 0, 2, 0, 2, 2, -1]
    # what the library answered before it knew this call
    assert [lib.pde_adi_line_length_path(n) for n in (1, 2, 6, 8, 28, 30, 32, 36, 64, 128, 129)] == \
        [0, 2, 2, 1, 1, 2, 1, 2, 2, 2, 0]
    d = _desc("pde_adi_", 30, 30)
    assert lib.pde_adi_backward_kernel(C.byref(d), 0) == 2 and lib.pde_adi_forward_kernel(C.byref(d)) == 2
    d = _desc("pde_adi_", 28, 28)
    assert lib.pde_adi_backward_kernel(C.byref(d), 0) == 0
