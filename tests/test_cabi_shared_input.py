"""The argument checks of pde_adi_multi_forward / pde_adi_multi_backward without a GPU.  Every call here is INVALID in
exactly one way and must be refused on the host before anything touches the device: the pointers handed over are host
buffers no kernel may see (a valid call would launch, so none is made)."""
import ctypes as C

import pytest

BADARG, WORKSPACE = -1, -5


def _desc(B=4, Cc=3, N=32, io=None, steps=2, split="strang", dt=0.02, dx=1.0):
    from cnn_with_pde_amd import _lib
    from cnn_with_pde_amd import functional as F_
    d = _lib.PdeAdiDesc()
    sweeps = [s for st in F_.adi_schedule(dt, dx, dx, steps, split) for s in st]
    d.B, d.C, d.N, d.num_sweeps = B, Cc, N, len(sweeps)
    d.io_dtype = _lib.PDE_IO_F32 if io is None else io
    d.has_clamp_max, d.clamp_max, d.eps = 1, 10.0, 1e-6
    for i, s in enumerate(sweeps):
        d.sweep[i].axis, d.sweep[i].delta, d.sweep[i].h2, d.sweep[i].t = s.axis, s.delta, s.h2, s.t
    return d


class Group:
    """A valid two-layer group (Strang, 2 and 3 steps) on host buffers; ``keep`` holds what the array points to."""

    def __init__(self, L=2, **kw):
        from cnn_with_pde_amd import _lib
        lib = _lib.load()
        self.lib = lib
        self.descs = [_desc(steps=2 + i, **kw) for i in range(L)]
        self.arr = (_lib.PdeSmallLayer * max(L, 1))()
        self.buf = (C.c_double * 64)()                    # 16-byte aligned dummy target of every other pointer
        base = C.addressof(self.buf)
        self.p = base + (-base % 16)
        self.masks = [(C.c_uint64 * 2)(0, 0) for _ in range(L)]
        self.ws = []
        for i in range(L):
            a, d = self.arr[i], self.descs[i]
            a.desc, a.sweeps_per_step, a.mode = C.pointer(d), 3, 1
            for f in ("M", "alpha_base", "beta_base", "alpha_slope", "beta_slope", "states", "steps_workspace",
                      "g_alpha_base", "g_beta_base", "g_alpha_slope", "g_beta_slope", "gM", "g_weight"):
                setattr(a, f, self.p)
            a.weight = 0.5
            a.steps_workspace_bytes = lib.pde_adi_steps_workspace_bytes(C.byref(d), 3)
            a.ckpt_mask = self.masks[i]
            n = lib.pde_adi_small_backward_workspace_bytes(C.byref(d), 3, 0)
            a.workspace, a.workspace_bytes = self.p, (n if n else 1 << 20)     # (0: a descriptor the query refuses)
        self.L = L

    def fwd(self, L=None, arr=True, u=True, out=True):
        p = C.c_void_p(self.p)
        return self.lib.pde_adi_multi_forward(self.L if L is None else L, self.arr if arr else None, p if u else None,
                                              p if out else None, None, None)

    def bwd(self, L=None, arr=True, u=True, gu=True):
        p = C.c_void_p(self.p)
        return self.lib.pde_adi_multi_backward(self.L if L is None else L, self.arr if arr else None, p,
                                               p if u else None, p if gu else None, None)

    def both(self, **kw):
        return self.fwd(**kw), self.bwd(**kw)


def test_number_of_layers_and_the_array():
    g = Group()
    assert g.both(L=0) == (BADARG, BADARG)
    assert g.both(L=5) == (BADARG, BADARG)
    assert g.both(L=-1) == (BADARG, BADARG)
    assert g.both(arr=False) == (BADARG, BADARG)


@pytest.mark.parametrize("layer", [0, 1])
def test_descriptor_faults(layer):
    """A null descriptor, C = 5, N = 20, four sweeps per step — in layer 0, and in layer 1 behind a valid layer 0."""
    from cnn_with_pde_amd import _lib
    g = Group()
    g.arr[layer].desc = C.POINTER(_lib.PdeAdiDesc)()
    assert g.both() == (BADARG, BADARG)
    for kw in (dict(Cc=5), dict(N=20)):
        g = Group(**kw)                                   # both layers: the group agrees, every layer is unsupported
        assert g.both() == (BADARG, BADARG), kw
        g = Group()
        bad = _desc(steps=2 + layer, **kw)                # one layer: unsupported AND different from the other
        g.arr[layer].desc = C.pointer(bad)
        assert g.both() == (BADARG, BADARG), kw
    g = Group()
    for a in g.arr:
        a.sweeps_per_step = 4
    assert g.both() == (BADARG, BADARG)
    g = Group()
    g.arr[layer].sweeps_per_step = 4
    assert g.both() == (BADARG, BADARG)


@pytest.mark.parametrize("what", ["B", "C", "N", "io_dtype", "sweeps_per_step"])
def test_layers_must_agree(what):
    """Each layer is valid on its own; the group is not."""
    from cnn_with_pde_amd import _lib
    g = Group()
    other = {"B": dict(B=5), "C": dict(Cc=2), "N": dict(N=28), "io_dtype": dict(io=_lib.PDE_IO_BF16),
             "sweeps_per_step": dict(split="lie")}[what]
    d1 = _desc(steps=3, **other)
    sps = 2 if what == "sweeps_per_step" else 3
    assert g.lib.pde_adi_small_supported(C.byref(d1), sps) == 1
    g.arr[1].desc, g.arr[1].sweeps_per_step = C.pointer(d1), sps
    g.arr[1].workspace_bytes = max(g.arr[1].workspace_bytes, g.lib.pde_adi_small_backward_workspace_bytes(C.byref(d1), sps, 0))
    assert g.both() == (BADARG, BADARG)


def test_modes():
    g = Group()
    g.arr[1].mode = 2                                     # coupling-after layers do not share an input
    assert g.both() == (BADARG, BADARG)
    g = Group()
    g.arr[0].mode = g.arr[1].mode = 2
    assert g.both() == (BADARG, BADARG)
    for mode in (0, 3):
        g = Group()
        g.arr[1].mode = mode
        assert g.both() == (BADARG, BADARG)
    g = Group()
    g.arr[1].skip_weight = g.p                            # a skip blend belongs to mode 2
    assert g.both() == (BADARG, BADARG)
    g = Group(L=1)
    g.arr[0].skip_weight = g.p
    assert g.both() == (BADARG, BADARG)


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("field", ["M", "alpha_base", "beta_base", "alpha_slope", "beta_slope", "steps_workspace"])
def test_null_pointers_both_passes(layer, field):
    g = Group()
    setattr(g.arr[layer], field, None)
    assert g.both() == (BADARG, BADARG)


def test_null_tensors():
    g = Group()
    assert g.fwd(u=False) == BADARG and g.fwd(out=False) == BADARG
    assert g.bwd(u=False) == BADARG and g.bwd(gu=False) == BADARG


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("field", ["states", "gM", "workspace", "g_alpha_base", "g_beta_base", "g_alpha_slope", "g_beta_slope"])
def test_backward_null_pointers(layer, field):
    g = Group()
    setattr(g.arr[layer], field, None)
    assert g.bwd() == BADARG


@pytest.mark.parametrize("layer", [0, 1])
def test_checkpoint_bits_are_step_local(layer):
    """Bits 0 .. sweeps_per_step - 2 only: the state after a step's last sweep is the step's output itself."""
    for lo, hi in ((0b100, 0), (0b1000, 0), (1 << 63, 0), (0, 1), (0b101, 0)):
        g = Group()
        g.masks[layer][0], g.masks[layer][1] = lo, hi
        g.arr[layer].workspace_bytes = 1 << 40            # large enough for any count: the mask itself is at fault
        assert g.bwd() == BADARG, (lo, hi)
    g = Group()                                           # Lie steps: bit 1 is already the step's output
    for i in range(2):
        d = _desc(steps=2 + i, split="lie")
        g.descs[i] = d
        g.arr[i].desc, g.arr[i].sweeps_per_step = C.pointer(d), 2
    g.masks[layer][0] = 0b10
    g.arr[layer].workspace_bytes = 1 << 40
    assert g.bwd() == BADARG


@pytest.mark.parametrize("layer", [0, 1])
def test_backward_workspace(layer):
    g = Group()
    assert g.arr[layer].workspace_bytes == g.lib.pde_adi_small_backward_workspace_bytes(C.byref(g.descs[layer]), 3, 0) > 0
    g.arr[layer].workspace_bytes -= 1                     # one byte short
    assert g.bwd() == WORKSPACE
    g = Group()
    g.arr[layer].workspace = g.p + 8                      # 8-byte aligned only
    assert g.bwd() == WORKSPACE
    g = Group()                                           # a parked state more than the workspace was sized for
    g.masks[layer][0] = 0b01
    assert g.bwd() == WORKSPACE
