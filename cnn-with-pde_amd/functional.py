"""Differentiable operators of the PDE-layer hot path, backed by libpdecnn_hip.so.

Each function is a ``torch.autograd.Function`` whose forward and backward enqueue the
hand-written HIP kernels on the current stream.  PyTorch is used only for device
memory, streams and autograd bookkeeping.  Nothing here has a CPU or eager fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading
import time
import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch
import torch.autograd.forward_ad as _fwad
from torch.autograd.function import once_differentiable

from . import _lib as L

__all__ = ["Sweep", "adi_schedule", "adi_diffuse", "adi_diffuse_states", "adi_diffuse_mixed", "adi_diffuse_small", "adi_diffuse_small_states", "adi_small_supported", "adi_diffuse_multi", "gate_combine", "plan_checkpoints", "kappa_max_async", "channel_mix", "skip_blend", "explicit5_step", "jacobi_diffuse", "explicit5_states", "jacobi_diffuse_states",
           "explicit5_tangent", "jacobi_diffuse_tangent", "linear_adjoint", "timing_enable", "timing_read", "Schedule", "sym_layer", "sym_layer_supported",
           "sym_layer_f16_supported", "sym_layer_bf16_supported", "sym_k16"]


@dataclass(frozen=True)
class Sweep:
    """One implicit sweep: a diffuse_x / diffuse_y call of the reference (mnist_test.py:55-63)."""
    axis: int        # 0: along W with alpha, 1: along H with beta
    delta: float     # dt/2 or dt
    h2: float        # dx**2 or dy**2
    t: float         # current_time at which alpha/beta are evaluated


class _HashedTuple(tuple):
    """A tuple whose hash is computed once: schedules are dictionary keys on every layer call (launch descriptors,
    support checks), and hashing 30 frozen dataclasses costs more host time than a kernel launch."""

    def __hash__(self):
        h = self.__dict__.get("_h")
        if h is None:
            h = self.__dict__["_h"] = tuple.__hash__(self)
        return h

    def __eq__(self, other):
        return self is other or tuple.__eq__(self, other)

    def __ne__(self, other):
        return not self.__eq__(other)


class Schedule(_HashedTuple):
    """Per-step sweep tuples of one layer call; ``.flat`` is the same sweeps as one flat tuple."""

    def __new__(cls, steps):
        self = super().__new__(cls, (_HashedTuple(st) for st in steps))
        self.flat = _HashedTuple(s for st in self for s in st)
        return self


def _as_schedule(steps) -> "Schedule":
    return steps if isinstance(steps, Schedule) else Schedule(steps)


def adi_schedule(dt: float, dx: float, dy: float, num_steps: int, split: str = "strang") -> List[List[Sweep]]:
    """Sweeps of every time step, with ``current_time`` accumulated in Python double exactly
    as the reference does (mnist_test.py:49-63 Strang; cifar_2version.py:79-101 Lie)."""
    steps, t = [], 0.0
    for _ in range(num_steps):
        s = [Sweep(0, dt / 2, dx ** 2, t)]
        t += dt / 2
        if split == "strang":
            s.append(Sweep(1, dt, dy ** 2, t))
            t += dt / 2
            s.append(Sweep(0, dt / 2, dx ** 2, t))
        elif split == "lie":
            s.append(Sweep(1, dt / 2, dy ** 2, t))
            t += dt / 2
        else:
            raise ValueError(f"unknown split {split!r}")
        steps.append(s)
    return steps


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


#: bytes the library asks of where a tensor, a coefficient plane or a matrix begins (include/pdecnn.h, "Alignment")
ALIGN = 16


def _aligned(t: Optional[torch.Tensor], align: int = ALIGN) -> Optional[torch.Tensor]:
    """``t`` as the library may be handed it: the SAME object when its storage begins on ``align`` bytes (no copy, no launch:
    every fresh allocation does), otherwise a contiguous copy in an allocation of its own.  ``align`` is what the header asks
    of the parameter in THIS call: 16 by default, 1 (never a copy: a tensor begins on its element's boundary) for a call
    served by element-wise kernels; the header's ELEMENT-ALIGNED parameters (skip_weight, weights, gates, gamma / beta,
    a_row / b_col, channel_scaling ...) do not come through here at all.  ``.contiguous()`` leaves a
    contiguous view where it is — a batch slice ``u[1:]``, a parameter cut from one flat buffer, a tensor that arrived
    through DLPack — and such a view begins wherever its storage offset puts it.  For read-only arguments; running
    statistics, which the kernels update in place one element at a time, need their element's alignment only and are
    passed as they are."""
    if t is None or align <= 1 or t.data_ptr() % align == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.PdeError("libpdecnn_hip operators need CUDA/HIP tensors (there is no CPU fallback)")


def _io_dtype(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return L.PDE_IO_F32
    if t.dtype == torch.bfloat16:
        return L.PDE_IO_BF16
    if t.dtype == torch.float16:
        return L.PDE_IO_F16
    raise L.PdeError(f"unsupported tensor dtype {t.dtype} (float32, bfloat16 or float16)")


#: tensor types the kernels take as they are (anything else is widened to fp32 first)
_IO_TYPES = (torch.float32, torch.bfloat16, torch.float16)


# float16: a call takes the float16 route only when its input AND every floating parameter it uses are float16 — the
# model.half() case, the only one where torch's type promotion gives float16.  Tensors in and out are then fp16, the
# arithmetic inside the kernels fp32, rounded to fp16 where the bf16 route rounds to bf16; parameter gradients are reduced
# in fp32 and rounded once (autograd casts them to the parameter's dtype).  Any other mix with an fp16 input keeps the
# behaviour from before the route existed: the input is widened to fp32 and the result is fp32 (autocast's fp32 layers).
def _is_f16(u, *params) -> bool:
    return (isinstance(u, torch.Tensor) and u.dtype == torch.float16 and
            all(p.dtype == torch.float16 for p in params if isinstance(p, torch.Tensor) and p.is_floating_point()))


def _io_in(u: torch.Tensor, *params) -> torch.Tensor:
    """``u`` as the kernels take it: fp32 and bf16 as given, fp16 on the float16 route, anything else widened to fp32."""
    if u.dtype in (torch.float32, torch.bfloat16) or (u.dtype == torch.float16 and _is_f16(u, *params)):
        return u
    return u.float()


def route_input(u: torch.Tensor, *params) -> torch.Tensor:
    """The input of a layer made of several calls, decided once for every parameter the layer uses (the float16 route needs
    them all fp16): float64 anywhere leaves it to the float64 route, otherwise ``_io_in``."""
    if _is_f64(u, *params):
        return u
    return _io_in(u, *params)


_M64 = (1 << 64) - 1


def _mask128(bits: int):
    """A 128-bit mask of the C ABI (the backward's checkpoints, a trajectory call's emitted sweeps or steps)."""
    return (C.c_uint64 * 2)(bits & _M64, bits >> 64)


_desc_cache = {}


def _fill_desc(cls, B, Cc, H, W, io, sweeps: Sequence[Sweep], smooth3, clamp_max, eps):
    """A new launch descriptor of type ``cls``: PdeAdiDesc / PdeAdiDescF64 for a square plane (N = H), PdeAdiRectDesc /
    PdeAdiRectDescF64 for (H, W)."""
    if len(sweeps) > L.PDE_MAX_SWEEPS:
        raise L.PdeError(f"{len(sweeps)} sweeps in one launch exceed PDE_MAX_SWEEPS={L.PDE_MAX_SWEEPS}")
    d = cls()
    if hasattr(cls, "N"):
        d.N = H
    else:
        d.H, d.W = H, W
    d.B, d.C, d.io_dtype, d.num_sweeps = B, Cc, io, len(sweeps)
    d.smooth3 = int(bool(smooth3))
    d.has_clamp_max = int(clamp_max is not None)
    d.clamp_max = float(clamp_max) if clamp_max is not None else 0.0
    d.eps = float(eps)
    for i, s in enumerate(sweeps):
        d.sweep[i].axis, d.sweep[i].delta, d.sweep[i].h2, d.sweep[i].t = int(s.axis), s.delta, s.h2, s.t
    return d


def _desc(cls, B, Cc, H, W, io, sweeps: Sequence[Sweep], smooth3, clamp_max, eps):
    """The launch descriptor (read-only for the library).  Cached: filling ~100 ctypes fields costs more host time than
    the kernels of a small layer take on the device."""
    if not isinstance(sweeps, tuple):
        sweeps = tuple(sweeps)
    key = (cls, B, Cc, H, W, io, sweeps, bool(smooth3), clamp_max, float(eps))
    d = _desc_cache.get(key)
    if d is None:
        d = _fill_desc(cls, B, Cc, H, W, io, sweeps, smooth3, clamp_max, eps)
        if len(_desc_cache) > 256:
            _desc_cache.clear()
        _desc_cache[key] = d
    return d


def _make_desc(B, Cc, N, io, sweeps: Sequence[Sweep], smooth3, clamp_max, eps) -> L.PdeAdiDesc:
    return _desc(L.PdeAdiDesc, B, Cc, N, N, io, sweeps, smooth3, clamp_max, eps)


def _build_desc(B, Cc, N, io, sweeps: Sequence[Sweep], smooth3, clamp_max, eps) -> L.PdeAdiDesc:
    """A square descriptor of the caller's own, not cached (bench.py asks the library about one)."""
    return _fill_desc(L.PdeAdiDesc, B, Cc, N, N, io, sweeps, smooth3, clamp_max, eps)


def _is_rect(u) -> bool:
    """A (B, C, H, W) input with H != W: served by the pde_adi_rect_* entry points (squares keep their own)."""
    return isinstance(u, torch.Tensor) and u.dim() == 4 and u.shape[2] != u.shape[3]


def _check_rect(u, *params):
    """Refuse, before any launch, a rectangle the library does not hold or parameters that are not (C, H, W) / (H, W)."""
    _require_cuda(u, *params)
    B, Cc, H, W = u.shape
    if not L.load().pde_adi_rect_supported(H, W):
        raise L.PdeError(f"plane {H}x{W}: both sides must be in [2, {L.PDE_MAX_N_GENERIC}] "
                         f"({L.ERRORS[-2]})")
    for p in params:
        q = tuple(p.shape)
        if q != (Cc, H, W) and not (len(q) == 2 and Cc == 1 and q == (H, W)):
            raise L.PdeError(f"coefficient of shape {q} does not match ({Cc},{H},{W})")


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# What the one node of a layer family (_AdiFn, _Explicit5Fn, _JacobiFn) needs to serve the plain call and the trajectory
# call alike.  ``sel`` None is the plain call; otherwise it lists what the call emits, the last sweep / step included.
def _kernel_input(u: torch.Tensor, f64: bool, io_types=_IO_TYPES, align: int = ALIGN) -> torch.Tensor:
    """``u`` as a family's kernels take it, contiguous: double on the float64 route, otherwise as it is when ``io_types``
    holds its type and widened to fp32 when not."""
    if f64:
        return u.to(torch.float64).contiguous()                 # every float64 entry point is element-wise: no requirement
    return _aligned((u if u.dtype in io_types else u.float()).contiguous(), align)


def _kernel_param(p: torch.Tensor, dtype) -> torch.Tensor:
    """A parameter cut from the graph, contiguous and in the kernels' type (no torch call for a type it has already)."""
    p = p.detach()
    return (p if p.dtype == dtype else p.to(dtype)).contiguous()     # per-channel / per-line vectors: ELEMENT-ALIGNED


def _out_and_traj(u, sel):
    """(what the node returns, the library's output, its trajectory tensor or None): a plain call returns the output, a
    tensor of its own; a trajectory call ONE tensor (K', ...) whose last slice is the library's output."""
    if sel is None:
        out = torch.empty_like(u)
        return out, out, None
    res = torch.empty((len(sel),) + tuple(u.shape), dtype=u.dtype, device=u.device)
    return res, res[-1], res


def _grad_as(g, dtype, shape=None):
    """A gradient in the type (and shape) of the tensor it belongs to; no torch call where it has them already (each costs
    the host more than a microsecond, and fp32 gradients of fp32 tensors are the common case)."""
    if shape is not None and g.shape != shape:
        g = g.reshape(shape)
    return g if g.dtype == dtype else g.to(dtype)


def _cotangent(g, dtype, align: int = ALIGN):
    """A cotangent as the library takes it: in the type of the tensor it belongs to, contiguous, aligned; None stays None."""
    return None if g is None else _aligned(_grad_as(g, dtype).contiguous(), align)


def _cotangents(g, dtype, sel, align: int = ALIGN):
    """(gradient of the library's output, gradient of the trajectory tensor or None) from the node's cotangent."""
    g = _cotangent(g, dtype, align)
    return (g, None) if sel is None else (g[-1], g)       # slots 0..K'-2 are the states' gradients, the last slice is gy


def _as_chw(p: torch.Tensor, Cc: int, N: int, W: Optional[int] = None, align: int = ALIGN) -> torch.Tensor:
    """The parameter as a contiguous fp32 (C, N, N) tensor — (C, N, W) on a rectangle."""
    W = N if W is None else W
    if p.dtype == torch.float32 and p.dim() == 3 and p.shape[0] == Cc and p.shape[1] == N and p.shape[2] == W \
            and p.is_contiguous():
        return _aligned(p.detach(), align)
    q = p.detach()
    if q.dim() == 2:
        q = q.unsqueeze(0)
    if tuple(q.shape) != (Cc, N, W):
        raise L.PdeError(f"coefficient of shape {tuple(p.shape)} does not match ({Cc},{N},{W})")
    return _aligned(q.to(torch.float32).contiguous(), align)


def _as_chw64(p: torch.Tensor, Cc: int, N: int, W: Optional[int] = None, align: int = 1) -> torch.Tensor:
    W = N if W is None else W
    q = p.detach()
    if q.dim() == 2:
        q = q.unsqueeze(0)
    if tuple(q.shape) != (Cc, N, W):
        raise L.PdeError(f"coefficient of shape {tuple(p.shape)} does not match ({Cc},{N},{W})")
    return q.to(torch.float64).contiguous()


#: (rect, f64) -> what tells the four sub-families of the implicit sweeps apart on the host: the prefix of their symbols,
#: their descriptor and the view their kernels take of a parameter.  Everything else is one body (``_AdiFn``).
_ADI_FAMILY = {(False, False): ("pde_adi_", L.PdeAdiDesc, _as_chw),
               (True, False): ("pde_adi_rect_", L.PdeAdiRectDesc, _as_chw),
               (False, True): ("pde_adi_f64_", L.PdeAdiDescF64, _as_chw64),
               (True, True): ("pde_adi_rect_f64_", L.PdeAdiRectDescF64, _as_chw64)}


#: amplification of rounding error tolerated when a state is rebuilt backwards from a later one
#: (x_{s-1} = (A_s + eps I) x_s grows high-frequency error by up to 1 + 4*coeff per sweep)
CKPT_AMAX = 8.0


def plan_checkpoints(kappa_max: Sequence[float], amax: float = CKPT_AMAX) -> int:
    """Bit s set: keep the state after sweep s as a checkpoint instead of rebuilding it.

    Walking back from the output, the error amplification of the rebuilt state is the product of
    (1 + 4*max coeff) over the sweeps undone since the last exact state; a checkpoint is placed
    whenever that product would pass ``amax``.  Small coefficients (mnist, cifar: 1e-3) need none;
    fashion-like ones (0.27 / 0.54) get one every two sweeps; very large ones one per sweep."""
    mask, amp = 0, 1.0
    for s in range(len(kappa_max) - 1, 0, -1):
        amp *= 1.0 + 4.0 * float(kappa_max[s])
        if amp > amax:
            mask |= 1 << (s - 1)
            amp = 1.0
    return mask


def kappa_max_async(u_like, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, sweeps: Sequence[Sweep],
                    smooth3=False, clamp_max=None, eps=1e-6):
    """Launch the per-sweep max-coefficient kernel and an asynchronous copy to pinned host memory.
    Returns an object with ``.host`` / ``.event``; the values are valid once ``event.query()`` is True."""
    lib = L.load()
    _require_cuda(u_like, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff)
    B, Cc, N, W = u_like.shape
    p = [_as_chw(t, Cc, N, W) for t in (alpha_base, beta_base, alpha_time_coeff, beta_time_coeff)]
    kdev = torch.empty(len(sweeps), dtype=torch.float32, device=u_like.device)
    with torch.cuda.device(u_like.device):
        if N != W:                                         # a rectangle: the pde_adi_rect_* entry points
            d = _desc(L.PdeAdiRectDesc, max(B, 1), Cc, N, W, L.PDE_IO_F32, sweeps, smooth3, clamp_max, eps)
            L.check(lib.pde_adi_rect_kappa_max(C.byref(d), *[_ptr(t) for t in p], _ptr(kdev), _stream()),
                    "pde_adi_rect_kappa_max")
        else:
            d = _make_desc(max(B, 1), Cc, N, L.PDE_IO_F32, sweeps, smooth3, clamp_max, eps)   # independent of the batch
            L.check(lib.pde_adi_kappa_max(C.byref(d), *[_ptr(t) for t in p], _ptr(kdev), _stream()), "pde_adi_kappa_max")
        host = torch.empty(len(sweeps), dtype=torch.float32, pin_memory=True)
        host.copy_(kdev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
    return _KmaxOwned(host, ev)


#: entries of the per-device ring of (pinned buffer, event) pairs through which the per-sweep coefficient maxima reach
#: the host; one entry is held from a forward to its backward, so this bounds the PDE-layer calls whose backward is
#: still outstanding (raise it for models with more PDE layers than this in one graph)
KMAX_RING = 256
_kmax_rings = {}


class _KmaxEntry:
    __slots__ = ("host", "event", "gen", "owner")


_kmax_lock = threading.Lock()


def _kmax_channel(n: int):
    """Pinned host buffer and an event for the early copy of the per-sweep coefficient maxima (pde_adi_forward copies
    and records, right behind the factorisation kernel).  Creating a pinned tensor and an event per call costs more
    host time than the launches of a small layer: they come from a ring.  An entry whose previous holder is still alive
    (its backward has not run: more than KMAX_RING PDE-layer calls outstanding — long step groups, activation
    checkpointing, many layers) is left alone and the call gets a buffer and an event of its own instead."""
    if n > L.PDE_MAX_SWEEPS * 4:
        raise L.PdeError(f"{n} coefficient maxima exceed the ring entry of {L.PDE_MAX_SWEEPS * 4}")
    dev = torch.cuda.current_device()
    with _kmax_lock:                                       # autograd threads of several devices, DataParallel replicas
        ring = _kmax_rings.get(dev)
        if ring is None:
            pool = torch.empty(KMAX_RING * L.PDE_MAX_SWEEPS * 4, dtype=torch.float32, pin_memory=True)
            ring = {"next": 0, "entries": []}
            for i in range(KMAX_RING):
                e = _KmaxEntry()
                e.host = pool[i * L.PDE_MAX_SWEEPS * 4:(i + 1) * L.PDE_MAX_SWEEPS * 4]
                e.event = torch.cuda.Event()
                e.event.record()        # creates the underlying hipEvent_t; the library re-records it
                e.gen = 0
                e.owner = None
                ring["entries"].append(e)
            _kmax_rings[dev] = ring
        # the first free entry from `next` on: one long-lived ticket (an output kept without a backward, activation
        # checkpointing) must not make every later call allocate pinned memory and an event of its own
        e = None
        for off in range(KMAX_RING):
            i = (ring["next"] + off) % KMAX_RING
            c = ring["entries"][i]
            if c.owner is None or c.owner() is None:
                e = c
                ring["next"] = (i + 1) % KMAX_RING
                break
        if e is None:                                      # every entry is held by a call whose backward is outstanding
            e = _KmaxEntry()
            e.host = torch.empty(L.PDE_MAX_SWEEPS * 4, dtype=torch.float32, pin_memory=True)
            e.event = torch.cuda.Event()
            e.event.record()
            e.gen = 0
        e.gen += 1
        t = _KmaxTicket(e, n)
        e.owner = weakref.ref(t)
    return t


class _KmaxOwned:
    """Coefficient maxima in a buffer of their own (kappa_max_async)."""
    __slots__ = ("host", "event")

    def __init__(self, host, event):
        self.host, self.event = host, event


def _wait_event(ev, budget=0.02):
    """Wait for an event that is expected within microseconds of the device reaching the factorisation kernel: poll it
    before blocking — a blocking hipEventSynchronize costs the host ~100-150 us to wake up, more than the whole backward
    of a small layer takes to launch.  The poll is bounded by time (in a device-bound loop the host arrives while the
    previous step's backward is still running), not by a number of queries."""
    q = ev.query
    t0 = time.perf_counter()
    while True:
        for _ in range(64):
            if q():
                return
        if time.perf_counter() - t0 > budget:
            break
    ev.synchronize()


class _KmaxTicket:
    """One use of a ring entry: ``host`` / ``event`` as long as the entry has not been handed out again."""
    __slots__ = ("entry", "gen", "n", "__weakref__")

    def __init__(self, entry, n):
        self.entry, self.gen, self.n = entry, entry.gen, n

    def _check(self):
        if self.entry.gen != self.gen:
            raise L.PdeError("the coefficient-maxima ring entry of this call was reused before its backward ran: "
                             "more than functional.KMAX_RING PDE-layer calls are outstanding; raise KMAX_RING")

    @property
    def host(self):
        self._check()
        return self.entry.host[:self.n]

    @property
    def event(self):
        self._check()
        return self.entry.event

    def wait(self):
        """Values once the copy has landed (waits for the factorisation kernel only)."""
        _wait_event(self.event)
        return self.host.tolist()


class _KmaxConcat:
    """The maxima of several calls in call order (a layer composed from per-step calls): ``host`` / ``event`` like a ticket."""
    __slots__ = ("parts",)

    def __init__(self, parts):
        self.parts = list(parts)

    class _Ev:
        def __init__(self, evs):
            self.evs = evs

        def query(self):
            return all(e.query() for e in self.evs)

        def synchronize(self):
            for e in self.evs:
                e.synchronize()

    @property
    def event(self):
        return _KmaxConcat._Ev([p.event for p in self.parts])

    @property
    def host(self):
        return torch.cat([p.host for p in self.parts])

    def wait(self):
        return [v for p in self.parts for v in p.wait()]


# ---- second order: the adjoint of a layer that is linear in its input --------------------------------------------------
# Every PDE layer family is linear in its input, so a node's backward output is gu = F(theta)^T g, and for a
# cotangent v on gu  <v, F^T g> = <F v, g>:  the gradient with respect to g is F v — the layer's FORWARD at input v — and the
# gradient with respect to theta is the parameter gradient of the layer's full backward at input v with cotangent g.  Both
# are calls the library makes anyway, so differentiating twice needs no kernel of its own: a node whose ``backward`` runs in
# grad mode (``create_graph=True``) wraps its usual backward body in ``linear_adjoint`` below, and otherwise runs it bare.
_NO_PARAM_TANGENT = ("the parameter gradients of a PDE layer's first backward are not differentiable: they are nonlinear in "
                     "the parameters, and their derivative with respect to the input or the cotangent is a coefficient "
                     "tangent the library has no kernel for (differentiate the input gradient instead, or detach them)")


# ---- forward mode (torch.autograd.forward_ad) -------------------------------------------------------------------------
# A node's ``jvp`` needs tensors its backward may not keep (the frozen route keeps neither y nor u), and the C++ nodes of
# csrc/host_ext.cpp cannot carry one.  So the public functions ask ``_has_tangent`` — one module attribute read outside a
# dual level — and only then go through ``_apply_dual``, which tells the ctypes node's forward to keep what its jvp reads.
_NO_TRAJ_JVP = ("forward-mode AD through a trajectory call (adi_diffuse_states, explicit5_states, jacobi_diffuse_states) is "
                "not implemented: the tangent kernels emit no intermediate states; differentiate the plain call, or chain "
                "one call per emitted state")
_NO_JVP_ROUTE = ("this node was not called through the library's public functions under forward_ad.dual_level(): it kept "
                 "nothing for a jvp")
_dual = threading.local()


def _has_tangent(*ts) -> bool:
    """True inside a ``forward_ad.dual_level()`` when one of the tensors carries a tangent."""
    if _fwad._current_level < 0:
        return False
    return any(isinstance(t, torch.Tensor) and _fwad.unpack_dual(t).tangent is not None for t in ts)


def _apply_dual(cls, *args):
    """``cls.apply`` with the mark that its forward takes (``_take_dual``): keep what the jvp needs."""
    _dual.on = True
    try:
        return cls.apply(*args)
    finally:
        _dual.on = False


def _take_dual(ctx) -> bool:
    """Read and clear the mark of ``_apply_dual`` (the calls a jvp makes itself are plain ones).  With the mark, absent
    tangents arrive as None instead of zeros."""
    on = getattr(_dual, "on", False)
    if on:
        _dual.on = False
        ctx.set_materialize_grads(False)
    return on


class _LinearAdjointFn(torch.autograd.Function):
    """``body(*cots)`` — a node's existing backward, run unchanged — as a differentiable function of the cotangents and of
    the original parameter tensors.  The first ``n_diff`` results are the gradients the layer is linear through (``gu``);
    every other result is a parameter gradient, handed through and NOT differentiable: a cotangent on one raises.
    ``primal(*vs)`` is the same layer call at input ``vs`` (one per differentiable result, None where no cotangent came)
    with the original parameters and the call's own configuration; it returns one output per cotangent of ``body``."""

    @staticmethod
    def forward(ctx, body, primal, n_cot, n_diff, *tensors):
        ctx.set_materialize_grads(False)
        ctx.primal, ctx.n_cot, ctx.n_diff = primal, n_cot, n_diff
        ctx.save_for_backward(*tensors)                       # the cotangents, then the parameters: inputs, no copy
        return body(*tensors[:n_cot])

    @staticmethod
    def backward(ctx, *gouts):
        n_cot, n_diff = ctx.n_cot, ctx.n_diff
        if any(g is not None for g in gouts[n_diff:]):
            raise NotImplementedError(_NO_PARAM_TANGENT)
        vs = gouts[:n_diff]
        saved = ctx.saved_tensors
        none = (None,) * (4 + len(saved))
        if all(v is None for v in vs):
            return none
        cots, params = saved[:n_cot], saved[n_cot:]
        need = [i for i, n in enumerate(ctx.needs_input_grad[4 + n_cot:]) if n and params[i] is not None]
        create = torch.is_grad_enabled()
        with torch.enable_grad() if need else contextlib.nullcontext():
            outs = ctx.primal(*vs)
            if not isinstance(outs, (tuple, list)):
                outs = (outs,)
            pairs = [(o, c) for o, c in zip(outs, cots) if c is not None and o is not None and o.requires_grad]
            gp = [None] * len(params)
            if need and pairs:
                gs = torch.autograd.grad([o for o, _ in pairs], [params[i] for i in need], [c for _, c in pairs],
                                         allow_unused=True, create_graph=create)
                for i, g in zip(need, gs):
                    gp[i] = g
        gc = [None if c is None or o is None else (o if create else o.detach()) for o, c in zip(outs, cots)]
        return (None, None, None, None, *gc, *gp)


def linear_adjoint(body, primal, cots, params, n_diff=1):
    """The results of ``body(*cots)``, differentiable once more (see ``_LinearAdjointFn``).  ``cots``: the cotangents the
    node's backward received (None where none came); ``params``: the original parameter tensors of the call (None allowed)."""
    return _LinearAdjointFn.apply(body, primal, len(cots), n_diff, *cots, *params)


def _second_order(cls, ctx, cots, n_diff=1):
    """A node's backward in grad mode: ``cls._backward`` under the core, the primal call ``cls.apply`` at the new input with
    the arguments the forward left in ``ctx.primal_args`` — (parameter tensors, non-tensor configuration)."""
    params, cfg = ctx.primal_args
    return linear_adjoint(lambda *g: cls._backward(ctx, *g), lambda v: cls.apply(v, *params, *cfg), cots, params, n_diff)


# ---- what the implicit-layer nodes below share: each decision is taken in one place (csrc/host_ext.cpp cuts its nodes the
# same way, and the two mirrors stay bitwise alike: tests/test_gpu_node_calls.py) --------------------------------------
def _grad_route(need_u, need_params) -> str:
    """"none" / "full" / "input_only" from what needs a gradient (``grad_mode_of`` in csrc/host_ext.cpp).  "input_only":
    the input does and no parameter does, so the backward is gu = F^T gy alone — unless ``PDE_BWD_INPUT=0`` keeps the
    full one."""
    if need_params:
        return "full"
    if not need_u:
        return "none"
    return "input_only" if L.bwd_input_enabled() else "full"


def _want_kmax(route: str, ckpt, kmax_sink) -> bool:
    """Whether the forward asks for its per-sweep coefficient maxima.  The full backward plans its checkpoints from them
    under "auto"; the input-only backward plans nothing, so there — as wherever an explicit mask was given — only a caller
    who handed in a sink gets them (``_AdiMultiFn`` has no sink: it never asks on the frozen route)."""
    if route == "none":
        return False
    return kmax_sink is not None or (route == "full" and ckpt == "auto")


def _kmax_request(want: bool, n: int, device, kmax_sink=None):
    """(device buffer, ticket, the entry points' three maxima arguments) of a forward that asks for ``n`` coefficient maxima
    — all NULL when it does not.  The maxima are a by-product of the factorisation kernel, copied to pinned host memory
    right behind it, so whoever plans checkpoints from them waits for the factorisation only.  The ticket goes to
    ``kmax_sink`` when there is one.  Call with the input's device current."""
    if not want:
        return None, None, (_ptr(None), _ptr(None), C.c_void_p(0))
    kdev = torch.empty(n, dtype=torch.float32, device=device)
    tk = _kmax_channel(n)
    if kmax_sink is not None:
        kmax_sink.append(tk)
    return kdev, tk, (_ptr(kdev), _ptr(tk.host), C.c_void_p(tk.event.cuda_event))


def _plan_steps(km: Sequence[float], K: int, sps: int) -> int:
    """One step-local checkpoint mask for all ``K`` steps of ``sps`` sweeps: the union of the steps' own plans
    (``plan_steps`` in csrc/host_ext.cpp)."""
    bits = 0
    for k in range(K):
        bits |= plan_checkpoints(km[k * sps:(k + 1) * sps])
    return bits


def _steps_prologue(lib, u, ab, bb, asl, bsl, M, steps, smooth3, clamp_max, eps):
    """What the forward of a layer with a channel operator between its steps builds from the kernel input ``u``: the four
    coefficient views, the operator in fp32, the descriptor, sweeps per step, steps, and the steps workspace (the
    factorisation, which the backward reuses)."""
    B, Cc, N, _ = u.shape
    sps, K = len(steps[0]), len(steps)
    sweeps = steps.flat if isinstance(steps, Schedule) else tuple(s for st in steps for s in st)
    p = [_as_chw(t, Cc, N) for t in (ab, bb, asl, bsl)]
    Mf = _aligned(M.detach().to(torch.float32).contiguous())
    d = _make_desc(B, Cc, N, _io_dtype(u), sweeps, smooth3, clamp_max, eps)
    sws = _workspace(lib.pde_adi_steps_workspace_bytes(C.byref(d), sps), u.device)
    return p, Mf, d, sps, K, sws


def _param_meta(*params):
    return [(t.shape, t.dtype) for t in params]


def _grads_like(p):
    """The library's parameter gradients: one fp32 (double on the float64 route) tensor per coefficient view."""
    return [torch.empty_like(t) for t in p]


def _grads_as(gp, meta):
    """... handed back in the callers' shapes — (N, N) at C = 1 — and types."""
    return [_grad_as(g, dt, s) for g, (s, dt) in zip(gp, meta)]


_SMALL_COEFFS = ("alpha_base", "beta_base", "alpha_slope", "beta_slope")


def _small_layer(a, i, d, sps, Mf, wdev, sws, p=None, gp=None, ws=None, mask=None, **tensors):
    """Fill ``a``, the PdeSmallLayer record of layer ``i`` of a shared-input group: what every pass sets, then what this
    pass has — coefficient views ``p``, their gradients ``gp``, the backward's workspace and checkpoint mask, and any
    other pointer field by name (a None stays NULL, as a fresh record has it)."""
    a.desc, a.sweeps_per_step, a.mode = C.pointer(d), sps, 1
    a.M = Mf.data_ptr()
    a.weight = 0.0
    a.weight_ptr = None if wdev is None else wdev.data_ptr() + 4 * i
    a.steps_workspace, a.steps_workspace_bytes = sws.data_ptr(), sws.numel()
    if p is not None:
        a.alpha_base, a.beta_base, a.alpha_slope, a.beta_slope = (t.data_ptr() for t in p)
    if gp is not None:
        a.g_alpha_base, a.g_beta_base, a.g_alpha_slope, a.g_beta_slope = (t.data_ptr() for t in gp)
    if ws is not None:
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    if mask is not None:
        a.ckpt_mask = mask
    for name, t in tensors.items():
        if t is not None:
            setattr(a, name, t.data_ptr())


class _AdiFn(torch.autograd.Function):
    """The implicit sweeps through ctypes, the general path: ``adi_diffuse`` and ``adi_diffuse_states`` of the four
    sub-families ``_ADI_FAMILY`` tells apart — squares and rectangles, fp32 / bf16 / fp16 tensors and float64 (every
    tensor in double, the checkpoint plan of ``_f64_ckpt_bits``, no coefficient maxima).

    One body, because the library has one: a plain call is the family's ``*_states`` call without a mask.  ``emit`` None is
    the plain call and returns ``y``, a tensor of its own.  Otherwise ``emit`` lists the sweeps whose state is returned
    (the last one included) and the result is ONE tensor (K', B, C, H, W) whose last slice is the library's ``y``.

    When the input needs a gradient and none of the four coefficient tensors does (a frozen layer, an attack, a saliency
    map), the backward is the family's ``*_backward_input_states``: gu = F^T gy alone, bitwise the full backward's gu.
    The node then keeps the coefficient views and the forward's workspace only — neither ``y`` nor ``u`` — and asks for no
    coefficient maxima unless a ``kmax_sink`` was handed in.  ``PDE_BWD_INPUT=0`` keeps the full backward for such calls."""

    @staticmethod
    def forward(ctx, u, ab, bb, asl, bsl, sweeps, smooth3, clamp_max, eps, ckpt, kmax_sink, emit=None, rect=False,
                f64=False):
        # the defaults are the plain square call below float64: what ``apply`` with the first eleven arguments has always
        # been (the backward's surplus trailing Nones are dropped by autograd)
        lib = L.load()
        if rect:
            _check_rect(u, ab, bb, asl, bsl)
        else:
            _require_cuda(u, ab, bb, asl, bsl)
            if u.dim() != 4 or u.shape[2] != u.shape[3]:
                raise L.PdeError(f"expected (B,C,N,N), got {tuple(u.shape)}")
        B, Cc, H, W = u.shape
        fam, desc_cls, as_chw = _ADI_FAMILY[rect, f64]
        # the fused kernels move tensors and coefficient planes 16 bytes wide; rectangles, float64 and the any-size path
        # one element at a time (include/pdecnn.h, "Alignment"): nothing to copy there
        ctx.align = al = ALIGN if not (rect or f64) and H % 4 == 0 and 8 <= H <= 32 else 1
        u = _kernel_input(u, f64, align=al)
        if f64:
            ckpt = _f64_ckpt_bits(ckpt, len(sweeps))
        p = [as_chw(t, Cc, H, W, al) for t in (ab, bb, asl, bsl)]
        d = _desc(desc_cls, B, Cc, H, W, L.PDE_IO_F64 if f64 else _io_dtype(u), sweeps, smooth3, clamp_max, eps)
        out, y, traj = _out_and_traj(u, emit)
        ebits = None if emit is None else sum(1 << s for s in emit[:-1])
        ws = _workspace(getattr(lib, fam + "forward_workspace_bytes")(C.byref(d)), u.device)
        # frozen coefficients: the backward (*_backward_input_states) reads neither y nor u and plans no checkpoints, so
        # nothing of u's shape is kept
        route = _grad_route(ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:5]))
        with torch.cuda.device(u.device):
            kdev, ctx.kmax, kargs = _kmax_request(not f64 and _want_kmax(route, ckpt, kmax_sink), len(sweeps), u.device,
                                                  kmax_sink)
            if f64:
                kargs = (None,)                      # the float64 entry points take the device pointer alone (never set)
            L.check(getattr(lib, fam + "forward_states")(C.byref(d), _ptr(u), _ptr(y), _ptr(traj),
                                                         None if emit is None else _mask128(ebits),
                                                         *[_ptr(t) for t in p], *kargs, _ptr(ws), ws.numel(), _stream()),
                    fam + "forward_states")
        ctx.fwd_ws = ws if route != "none" else None     # factorisation reused by the backward
        ctx.input_only = (out.shape, out.dtype, out.device) if route == "input_only" else None
        if route == "input_only":
            ctx.save_for_backward(*p)
        else:
            ctx.save_for_backward(out, u if (route == "full" and ckpt != 0) else None, *p)
        ctx.cfg = (d, fam, ckpt, ebits)
        ctx.param_meta = _param_meta(ab, bb, asl, bsl)
        ctx.primal_args = ((ab, bb, asl, bsl), (sweeps, smooth3, clamp_max, eps, ckpt, None, emit, rect, f64))
        ctx.dual = None
        if _take_dual(ctx):                              # a tangent came in (adi_diffuse decided): what the jvp reads
            ctx.save_for_forward(u, *p)
            ctx.dual = (tuple(t.detach() for t in (ab, bb, asl, bsl)), (sweeps, smooth3, clamp_max, eps), as_chw, f64)
        return out

    @staticmethod
    def jvp(ctx, ut, dab, dbb, das, dbs, *_):
        """Forward mode.  The layer is linear in ``u``: with no parameter tangent the output tangent is the layer's own
        forward at ``ut`` (``adi_diffuse``, the fused kernels at N <= 32).  Otherwise one ``*_tangent`` call through
        ``_tangent_call``: the fused tangent kernel at the fused sizes of the square family, the any-size kernels elsewhere."""
        d, fam, _, ebits = ctx.cfg
        if ebits is not None:
            raise NotImplementedError(_NO_TRAJ_JVP)
        if ctx.dual is None:
            raise NotImplementedError(_NO_JVP_ROUTE)
        params, cfg, as_chw, f64 = ctx.dual
        u, *p = ctx.saved_tensors
        dts = (dab, dbb, das, dbs)
        if all(t is None for t in dts):
            if ut is None:
                return torch.zeros_like(u)
            return adi_diffuse(ut.to(u.dtype), *params, *cfg).to(u.dtype)
        Cc, H, W = u.shape[1:]
        dp = [None if t is None else as_chw(t, Cc, H, W, 1) for t in dts]
        du = None if ut is None else _kernel_input(ut.to(u.dtype), f64, align=1)
        return _tangent_call(L.load(), fam, d, u, du, p, dp, False)[1]

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():                      # create_graph=True: differentiable once more
            return _second_order(_AdiFn, ctx, (g,))
        return _AdiFn._backward(ctx, g)

    @staticmethod
    def _backward(ctx, g):
        lib = L.load()
        if ctx.input_only is not None:
            return _AdiFn._backward_input(ctx, g)
        out, u, *p = ctx.saved_tensors
        d, fam, ckpt, ebits = ctx.cfg
        y = out if ebits is None else out[-1]
        gy, gtraj = _cotangents(g, out.dtype, ebits, ctx.align)
        gu = torch.empty_like(y)
        gp = _grads_like(p)
        bits = plan_checkpoints(ctx.kmax.wait()) if ckpt == "auto" else int(ckpt)
        ws = _workspace(getattr(lib, fam + "backward_workspace_bytes")(C.byref(d), bin(bits).count("1")), out.device)
        with torch.cuda.device(out.device):          # autograd thread: set device, fetch the stream here
            L.check(getattr(lib, fam + "backward_states")(C.byref(d), _ptr(gy), _ptr(gtraj),
                                                          None if ebits is None else _mask128(ebits), _ptr(y),
                                                          _ptr(u if bits else None), _mask128(bits), _ptr(gu),
                                                          *[_ptr(t) for t in p], *[_ptr(t) for t in gp],
                                                          _ptr(ctx.fwd_ws), _ptr(ws), ws.numel(), _stream()),
                    fam + "backward_states")
        ctx.fwd_ws = None
        return (gu, *_grads_as(gp, ctx.param_meta)) + (None,) * 9

    @staticmethod
    def _backward_input(ctx, g):
        """The backward of a call whose coefficients take no gradient: the family's ``*_backward_input_states``."""
        lib = L.load()
        p = ctx.saved_tensors
        d, fam, _, ebits = ctx.cfg
        shape, dtype, device = ctx.input_only
        gy, gtraj = _cotangents(g, dtype, ebits, ctx.align)
        gu = torch.empty(shape[-4:], dtype=dtype, device=device)
        ws = _workspace(getattr(lib, fam + "backward_input_workspace_bytes")(C.byref(d)), device)
        with torch.cuda.device(device):              # autograd thread: set device, fetch the stream here
            L.check(getattr(lib, fam + "backward_input_states")(C.byref(d), _ptr(gy), _ptr(gtraj),
                                                                None if ebits is None else _mask128(ebits), _ptr(gu),
                                                                *[_ptr(t) for t in p], _ptr(ctx.fwd_ws), _ptr(ws),
                                                                ws.numel(), _stream()),
                    fam + "backward_input_states")
        ctx.fwd_ws = None
        return (gu,) + (None,) * 13


class _AdiMixedFn(torch.autograd.Function):
    """One call of a layer whose time steps are separated by a channel operator: cifar10.py:84-112 (``mode``
    "pre": u <- M u, then the step's sweeps) and SVHN.py:55-72 ("post": the sweeps, then u <- K u).

    One factorisation for the whole schedule, then per step one mixing launch and one sweep launch; the
    backward walks the steps in reverse, accumulating the partial sums of the parameter gradients and of the
    matrix gradient on the device, and reduces them once at the end (instead of a torch autograd node, a
    factorisation, a reduction and a gradient-accumulation add per step).

    When the input needs a gradient and neither a coefficient tensor nor ``M`` does, the forward is
    ``pde_adi_mixed_forward_input`` — no ``states`` tensor, two scratch tensors at most — and the backward one
    ``pde_adi_mixed_backward_input``: per step M^T g and the transposed solves, bitwise the full backward's gu.  The node
    then keeps ``M`` and the steps workspace only, asks for no coefficient maxima unless a ``kmax_sink`` was handed in,
    ignores ``checkpoints`` and waits for nothing.  A call under ``no_grad`` runs the same forward.  ``PDE_BWD_INPUT=0``
    restores the full calls for both."""

    @staticmethod
    def forward(ctx, u, ab, bb, asl, bsl, M, steps, mode, smooth3, clamp_max, eps, ckpt, kmax_sink):
        lib = L.load()
        _require_cuda(u, ab, bb, asl, bsl, M)
        if u.dim() != 4 or u.shape[2] != u.shape[3]:
            raise L.PdeError(f"expected (B,C,N,N), got {tuple(u.shape)}")
        u = _kernel_input(u, False)
        p, Mf, d, sps, K, sws = _steps_prologue(lib, u, ab, bb, asl, bsl, M, steps, smooth3, clamp_max, eps)
        route = _grad_route(ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:6]))
        m = 1 if mode == "pre" else 2
        ctx.input_only = None
        ctx.primal_args = ((ab, bb, asl, bsl, M), (steps, mode, smooth3, clamp_max, eps, ckpt, None))
        if route != "full" and L.bwd_input_enabled():
            y = torch.empty_like(u)
            ws = _workspace(lib.pde_adi_mixed_forward_input_workspace_bytes(C.byref(d), sps), u.device)
            with torch.cuda.device(u.device):
                kdev, ctx.kmax, kargs = _kmax_request(_want_kmax(route, ckpt, kmax_sink), d.num_sweeps, u.device, kmax_sink)
                L.check(lib.pde_adi_mixed_forward_input(C.byref(d), sps, m, _ptr(u), _ptr(y), _ptr(Mf), *[_ptr(t) for t in p],
                                                        *kargs, _ptr(sws), sws.numel(), _ptr(ws), ws.numel(), _stream()),
                        "pde_adi_mixed_forward_input")
            if route == "input_only":
                ctx.save_for_backward(Mf)
                ctx.sws = sws
                ctx.input_only = (u.dtype, u.device)
                ctx.cfg = (d, sps, K, m, ckpt)
            return y
        # states[2k]: output of step k's first operator, states[2k+1]: of its second (= input of step k+1); the last of them
        # is the layer output and lives in a tensor of its own (no copy, and nobody can reach the kept states through it)
        states = torch.empty((2 * K - 1,) + tuple(u.shape), dtype=u.dtype, device=u.device)
        y = torch.empty_like(u)
        with torch.cuda.device(u.device):
            kdev, ctx.kmax, kargs = _kmax_request(_want_kmax(route, ckpt, kmax_sink), d.num_sweeps, u.device, kmax_sink)
            L.check(lib.pde_adi_mixed_forward(C.byref(d), sps, m, _ptr(u), _ptr(states), _ptr(y), _ptr(Mf),
                                              *[_ptr(t) for t in p], *kargs, _ptr(sws), sws.numel(), _stream()),
                    "pde_adi_mixed_forward")
        if route != "none":
            ctx.save_for_backward(u, states, y, Mf, *p)
            ctx.sws = sws
        ctx.cfg = (d, sps, K, m, ckpt)
        ctx.param_meta = _param_meta(ab, bb, asl, bsl)
        ctx.M_dtype = M.dtype
        return y

    @staticmethod
    def backward(ctx, gy):
        if torch.is_grad_enabled():                      # create_graph=True: differentiable once more
            return _second_order(_AdiMixedFn, ctx, (gy,))
        return _AdiMixedFn._backward(ctx, gy)

    @staticmethod
    def _backward(ctx, gy):
        lib = L.load()
        if ctx.input_only is not None:
            (Mf,) = ctx.saved_tensors
            d, sps, K, m, _ = ctx.cfg
            dtype, device = ctx.input_only
            g_in = _cotangent(gy, dtype)
            g_a = torch.empty_like(g_in)
            ws = _workspace(lib.pde_adi_mixed_backward_input_workspace_bytes(C.byref(d), sps), device)
            with torch.cuda.device(device):
                L.check(lib.pde_adi_mixed_backward_input(C.byref(d), sps, m, _ptr(g_in), _ptr(Mf), _ptr(g_a), _ptr(ctx.sws),
                                                         _ptr(ws), ws.numel(), _stream()), "pde_adi_mixed_backward_input")
            return (g_a,) + (None,) * 12
        u, states, y, Mf, *p = ctx.saved_tensors
        d, sps, K, m, ckpt = ctx.cfg
        bits = _plan_steps(ctx.kmax.wait(), K, sps) if ckpt == "auto" else int(ckpt)
        ws = _workspace(lib.pde_adi_mixed_backward_workspace_bytes(C.byref(d), sps, bin(bits).count("1")), u.device)
        g_in = _cotangent(gy, u.dtype)
        g_a = torch.empty_like(g_in)
        gp, gM = _grads_like(p), torch.empty_like(Mf)
        with torch.cuda.device(u.device):
            L.check(lib.pde_adi_mixed_backward(C.byref(d), sps, m, _ptr(g_in), _ptr(u), _ptr(states), _ptr(y), _ptr(Mf),
                                               _mask128(bits), _ptr(g_a), *[_ptr(t) for t in p], *[_ptr(t) for t in gp],
                                               _ptr(gM), _ptr(ctx.sws), _ptr(ws), ws.numel(), _stream()),
                    "pde_adi_mixed_backward")
        return (g_a, *_grads_as(gp, ctx.param_meta), _grad_as(gM, ctx.M_dtype)) + (None,) * 7


class _AdiSmallFn(torch.autograd.Function):
    """A layer with a channel operator between its time steps at C <= 4, whole time loop in ONE launch per pass
    (pde_adi_small_*): cifar10.py:84-112 ("pre"), SVHN.py:55-76 ("post", with the skip blend when ``skip_weight``
    is given).  The sweep output of every step is kept for the backward, as autograd keeps it in the reference.

    ``emit`` None is the plain call (``adi_diffuse_small``) and returns ``y``.  Otherwise (``adi_diffuse_small_states``:
    no skip blend) ``emit`` lists the time steps whose state is returned too, the last one included, out of the same
    launch per pass (pde_adi_small_forward_states / pde_adi_small_backward_states), and the result is ONE tensor
    (K', B, C, N, N) whose last slice is the library's ``y``.

    When ``u`` needs a gradient and neither a coefficient tensor, ``M`` nor ``skip_weight`` does, the forward keeps no
    states — ``pde_adi_small_forward_input``, or for a trajectory with a non-empty mask the emitting forward with ``states``
    NULL — and the backward is ``pde_adi_small_backward_input`` / ``_input_states``: gu = F^T gy alone, bitwise the full
    backward's gu.  No (K, B, C, N, N) tensor is allocated, ``u`` is not saved, ``checkpoints`` is ignored and no
    coefficient maxima are asked for unless a ``kmax_sink`` was handed in; ``M``, ``skip_weight`` and the steps workspace
    stay alive.  ``PDE_BWD_INPUT=0`` keeps the full backward for such calls."""

    @staticmethod
    def forward(ctx, u, ab, bb, asl, bsl, M, skip_weight, steps, mode, smooth3, clamp_max, eps, ckpt, kmax_sink, emit=None):
        lib = L.load()
        _require_cuda(u, ab, bb, asl, bsl, M, skip_weight)
        u = _kernel_input(u, False)
        p, Mf, d, sps, K, sws = _steps_prologue(lib, u, ab, bb, asl, bsl, M, steps, smooth3, clamp_max, eps)
        sw = None if skip_weight is None else skip_weight.detach().to(torch.float32).reshape(1).contiguous()
        route = _grad_route(ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:7]))
        out, y, traj = _out_and_traj(u, emit)
        ebits = None if emit is None else sum(1 << k for k in emit[:-1])
        # where the two public calls differ beyond the mask: an empty mask is the plain call, which goes on from the rounded
        # sweep outputs of 16-bit tensors only when it keeps them; a trajectory call keeps them under no_grad too, so that
        # its result is the same tensor in both grad modes — adi_diffuse_small under no_grad keeps none
        keep = route == "full" or (route == "none" and ebits == 0 and u.element_size() < 4)
        states = torch.empty((K,) + tuple(u.shape), dtype=u.dtype, device=u.device) if keep else None
        m = 1 if mode == "pre" else 2
        if route == "input_only" and not ebits:          # parks nothing, y as with states kept
            name, args = "pde_adi_small_forward_input", (_ptr(u), _ptr(y), _ptr(Mf), _ptr(sw))
        elif emit is None:
            name, args = "pde_adi_small_forward", (_ptr(u), _ptr(y), _ptr(states), _ptr(Mf), _ptr(sw))
        else:
            name, args = "pde_adi_small_forward_states", (_ptr(u), _ptr(y), _ptr(states), _ptr(traj), _mask128(ebits), _ptr(Mf))
        with torch.cuda.device(u.device):
            kdev, ctx.kmax, kargs = _kmax_request(_want_kmax(route, ckpt, kmax_sink), d.num_sweeps, u.device, kmax_sink)
            L.check(getattr(lib, name)(C.byref(d), sps, m, *args, *[_ptr(t) for t in p], *kargs, _ptr(sws), sws.numel(),
                                       _stream()), name)
        ctx.input_only = (u.shape, u.dtype, u.device) if route == "input_only" else None
        skip = (sw,) if emit is None else ()
        if route == "input_only":
            ctx.save_for_backward(Mf, *skip)
        elif route == "full":
            ctx.save_for_backward(u, states, Mf, *skip, *p)
        ctx.sws = sws if route != "none" else None
        ctx.cfg = (d, sps, K, m, ckpt, ebits)
        ctx.param_meta = _param_meta(ab, bb, asl, bsl)
        ctx.M_dtype = M.dtype
        ctx.skip_meta = None if skip_weight is None else (skip_weight.shape, skip_weight.dtype)
        ctx.primal_args = ((ab, bb, asl, bsl, M, skip_weight), (steps, mode, smooth3, clamp_max, eps, ckpt, None, emit))
        return out

    @staticmethod
    def _backward_input(ctx, g):
        """The backward of a call whose parameters take no gradient: ``pde_adi_small_backward_input`` / ``_input_states``."""
        lib = L.load()
        Mf, *skip = ctx.saved_tensors
        d, sps, _, m, _, ebits = ctx.cfg
        shape, dtype, device = ctx.input_only
        gy, gtraj = _cotangents(g, dtype, ebits)
        gu = torch.empty(shape, dtype=dtype, device=device)
        if ebits is None:
            name, args = "pde_adi_small_backward_input", (_ptr(gy), _ptr(Mf), _ptr(skip[0]), _ptr(gu))
        else:
            name, args = "pde_adi_small_backward_input_states", (_ptr(gy), _ptr(gtraj), _mask128(ebits), _ptr(Mf), _ptr(gu))
        with torch.cuda.device(device):
            L.check(getattr(lib, name)(C.byref(d), sps, m, *args, _ptr(ctx.sws), None, 0, _stream()), name)
        return (gu,) + (None,) * 14

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():                      # create_graph=True: differentiable once more
            return _second_order(_AdiSmallFn, ctx, (g,))
        return _AdiSmallFn._backward(ctx, g)

    @staticmethod
    def _backward(ctx, g):
        lib = L.load()
        if ctx.input_only is not None:
            return _AdiSmallFn._backward_input(ctx, g)
        d, sps, K, m, ckpt, ebits = ctx.cfg
        u, states, Mf, *rest = ctx.saved_tensors
        sw, p = (rest[0] if ebits is None else None), rest[-4:]
        bits = _plan_steps(ctx.kmax.wait(), K, sps) if ckpt == "auto" else int(ckpt)
        ws = _workspace(lib.pde_adi_small_backward_workspace_bytes(C.byref(d), sps, bin(bits).count("1")), u.device)
        gy, gtraj = _cotangents(g, u.dtype, ebits)
        gu = torch.empty_like(u)
        gp, gM = _grads_like(p), torch.empty_like(Mf)
        gsw = torch.empty(1, dtype=torch.float32, device=u.device) if sw is not None else None
        pp = (*[_ptr(t) for t in p], *[_ptr(t) for t in gp], _ptr(gM))
        if ebits is None:
            name = "pde_adi_small_backward"
            args = (_ptr(gy), _ptr(u), _ptr(states), _ptr(Mf), _ptr(sw), _mask128(bits), _ptr(gu), *pp, _ptr(gsw))
        else:
            name = "pde_adi_small_backward_states"
            args = (_ptr(gy), _ptr(gtraj), _mask128(ebits), _ptr(u), _ptr(states), _ptr(Mf), _mask128(bits), _ptr(gu), *pp)
        with torch.cuda.device(u.device):
            L.check(getattr(lib, name)(C.byref(d), sps, m, *args, _ptr(ctx.sws), _ptr(ws), ws.numel(), _stream()), name)
        gskip = None if sw is None else _grad_as(gsw, ctx.skip_meta[1], ctx.skip_meta[0])
        return (gu, *_grads_as(gp, ctx.param_meta), _grad_as(gM, ctx.M_dtype), gskip) + (None,) * 8


def _multi_cotangents(gout, gys, gsums, dtype):
    """The cotangents of a shared-input group as the library takes them; any of them may be missing, but not all."""
    gout = _cotangent(gout, dtype)
    gys = [_cotangent(g, dtype) for g in gys]
    gsums = [_cotangent(g, torch.float32) for g in gsums]
    if gout is None and all(g is None for g in gys) and all(g is None for g in gsums):
        raise L.PdeError("adi_diffuse_multi: no incoming gradient")
    return gout, gys, gsums


class _AdiMultiFn(torch.autograd.Function):
    """Several mixing-first layers (cifar10.EnhancedDiffusionLayer / cifar_2version.LearnableDiffusionLayer, C <= 4)
    on the SAME input in one launch per pass (pde_adi_multi_*): cifar10.py:272-280, cifar_2version.py:287-288.
    Returns (sum_i w_i y_i, y_1, ..., y_L); the y_i are the last sweep outputs the kernel keeps anyway.

    With frozen parameters (``u`` needs a gradient; no coefficient tensor, ``M`` or ``weights`` does) the backward is
    ``pde_adi_multi_backward_input``: one launch, plus the combine launch side by side — no pre-pass, no parameter-gradient
    epilogue, no wait for the coefficient maxima, which are not asked for.  The forward is unchanged: the ``y_i`` are the
    last kept states, so the states are written as before (the node just does not hold them).
    ``PDE_BWD_INPUT=0`` keeps the full backward."""

    @staticmethod
    def forward(ctx, u, weights, specs, want_sums, ckpt, *flat):
        lib = L.load()
        nl = len(specs)
        _require_cuda(u, weights, *flat)
        B, Cc = u.shape[:2]
        u = _kernel_input(u, False)
        route = _grad_route(ctx.needs_input_grad[0], ctx.needs_input_grad[1] or any(ctx.needs_input_grad[5:]))
        want_kmax = _want_kmax(route, ckpt, None)
        if ckpt != "auto" and not isinstance(ckpt, (tuple, list)):
            ckpt = (int(ckpt),) * nl                      # one step-local mask for every layer
        if ckpt != "auto" and len(ckpt) != nl:
            raise L.PdeError(f"adi_diffuse_multi: {len(ckpt)} checkpoint masks for {nl} layers")
        ctx.ckpt = ckpt
        ctx.set_materialize_grads(False)
        wdev = None if weights is None else weights.detach().to(torch.float32).contiguous()   # read by the kernels on the device
        arr = (L.PdeSmallLayer * nl)()
        layers, saved, views, ys, sums = [], [], [], [], []
        for i, (steps, smooth3, clamp_max, eps) in enumerate(specs):
            ab, bb, asl, bsl, M = flat[5 * i:5 * i + 5]
            p, Mf, d, sps, K, sws = _steps_prologue(lib, u, ab, bb, asl, bsl, M, steps, smooth3, clamp_max, eps)
            states = torch.empty((K,) + tuple(u.shape), dtype=u.dtype, device=u.device)
            with torch.cuda.device(u.device):
                kdev, tk, _ = _kmax_request(want_kmax, d.num_sweeps, u.device)
            psum = torch.empty((B, Cc), dtype=torch.float32, device=u.device) if want_sums else None
            _small_layer(arr[i], i, d, sps, Mf, wdev, sws, p=p, states=states, kappa_max=kdev,
                         kappa_max_host=tk.host if tk else None, plane_sums=psum)
            # workspaces, states and tickets stay on ctx — on the frozen route the factorisations alone
            layers.append((d, sps, K, sws, *((None,) * 3 if route == "input_only" else (states, kdev, tk)),
                           _param_meta(ab, bb, asl, bsl), M.dtype))
            saved += [Mf] if route == "input_only" else [*p, Mf]
            views.append(p)                                # (fp32 copies of 16-bit parameters: alive until the launch)
            ys.append(states[-1])                          # the last sweep output of every layer
            sums.append(psum)
        out = torch.empty_like(u)
        with torch.cuda.device(u.device):
            ev = tk.event if want_kmax else None               # recorded behind the last layer's copy
            L.check(lib.pde_adi_multi_forward(nl, arr, _ptr(u), _ptr(out), C.c_void_p(ev.cuda_event if ev is not None else 0),
                                              _stream()), "pde_adi_multi_forward")
        # the input, the parameter views and the operators go through save_for_backward (an in-place change of any of them
        # between forward and backward then raises torch's version-counter error instead of giving gradients that mix the
        # forward's factorisation with new parameter values); frozen: the operators and the weights only
        ctx.input_only = (u.shape, u.dtype, u.device) if route == "input_only" else None
        ctx.save_for_backward(*([] if route == "input_only" else [u]), *([wdev] if wdev is not None else []), *saved)
        ctx.layers = layers
        ctx.has_w = weights is not None
        ctx.want_sums = want_sums
        ctx.primal_args = ((weights, *flat), (specs, want_sums, ckpt))
        return (out, *ys, *sums) if want_sums else (out, *ys)

    @staticmethod
    def _backward_input(ctx, gout, gys, gsums):
        """The backward of a group whose parameters take no gradient: ``pde_adi_multi_backward_input``."""
        lib = L.load()
        nl = len(ctx.layers)
        shape, dtype, device = ctx.input_only
        saved = ctx.saved_tensors
        wdev = saved[0] if ctx.has_w else None
        Ms = saved[1 if ctx.has_w else 0:]
        gout, gys, gsums = _multi_cotangents(gout, gys, gsums, dtype)
        arr = (L.PdeSmallLayer * nl)()
        hold = []
        for i, (d, sps, _, sws, *_rest) in enumerate(ctx.layers):
            # (the slab of a side-by-side group; the query is what the library checks against, used or not)
            ws = _workspace(lib.pde_adi_small_backward_input_workspace_bytes(C.byref(d), sps), device) if nl > 1 else None
            _small_layer(arr[i], i, d, sps, Ms[i], wdev, sws, ws=ws, gys=gys[i], g_plane_sums=gsums[i])
            hold.append(ws)
        gu = torch.empty(shape, dtype=dtype, device=device)
        with torch.cuda.device(device):
            L.check(lib.pde_adi_multi_backward_input(nl, arr, _ptr(gout), _ptr(gu), _stream()),
                    "pde_adi_multi_backward_input")
        return (gu,) + (None,) * (4 + 5 * nl)

    @staticmethod
    def backward(ctx, gout, *gall):
        if torch.is_grad_enabled():                      # create_graph=True: differentiable once more
            params, cfg = ctx.primal_args
            return linear_adjoint(lambda *g: _AdiMultiFn._backward(ctx, *g),
                                  lambda v: _AdiMultiFn.apply(v, params[0], *cfg, *params[1:]), (gout, *gall), params)
        return _AdiMultiFn._backward(ctx, gout, *gall)

    @staticmethod
    def _backward(ctx, gout, *gall):
        lib = L.load()
        nl = len(ctx.layers)
        gys, gsums = gall[:nl], (gall[nl:] if ctx.want_sums else (None,) * nl)
        if ctx.input_only is not None:
            return _AdiMultiFn._backward_input(ctx, gout, gys, gsums)
        saved = ctx.saved_tensors
        u = saved[0]
        wdev = saved[1] if ctx.has_w else None
        pm = saved[2 if ctx.has_w else 1:]                 # per layer: four parameter views and the operator
        if ctx.ckpt == "auto":
            _wait_event(ctx.layers[-1][6].event)
        gout, gys, gsums = _multi_cotangents(gout, gys, gsums, u.dtype)
        arr = (L.PdeSmallLayer * nl)()
        outs, hold = [], []
        for i, (d, sps, K, sws, states, _, tk, meta, Mdt) in enumerate(ctx.layers):
            p, Mf = pm[5 * i:5 * i + 4], pm[5 * i + 4]
            bits = _plan_steps(tk.host.tolist(), K, sps) if ctx.ckpt == "auto" else int(ctx.ckpt[i])
            mask = _mask128(bits)
            ws = _workspace(lib.pde_adi_small_backward_workspace_bytes(C.byref(d), sps, bin(bits).count("1")), u.device)
            gp, gM = _grads_like(p), torch.empty_like(Mf)
            gw = torch.empty(1, dtype=torch.float32, device=u.device)
            _small_layer(arr[i], i, d, sps, Mf, wdev, sws, p=p, gp=gp, ws=ws, mask=mask, states=states, gys=gys[i],
                         g_plane_sums=gsums[i], gM=gM, g_weight=gw)
            hold.append((mask, ws))
            outs.append((gp, gM, gw, meta, Mdt))
        gu = torch.empty_like(u)
        with torch.cuda.device(u.device):
            L.check(lib.pde_adi_multi_backward(nl, arr, _ptr(gout), _ptr(u), _ptr(gu), _stream()), "pde_adi_multi_backward")
        flat = []
        for gp, gM, gw, meta, Mdt in outs:
            flat += _grads_as(gp, meta) + [_grad_as(gM, Mdt)]
        gweights = torch.cat([o[2] for o in outs]) if ctx.has_w else None
        return (gu, gweights, None, None, None, *flat)

def adi_diffuse_multi(u, layers, weights=None, plane_sums=False, checkpoints="auto"):
    """Run several mixing-first layers on the same ``u`` in one launch per pass.

    ``layers``: list of dicts with keys alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, steps and
    optionally smooth3, clamp_max, eps.  ``weights`` (L,): ``out = sum_i weights[i] * y_i`` (cifar10.py:277-280
    without the attention gates); None: ``out`` is not meaningful.  Returns ``(out, [y_1 .. y_L])``, and with
    ``plane_sums`` also ``[s_1 .. s_L]``, ``s_i[b,c] = sum_hw y_i`` — the adaptive average pool of
    cifar10.py:239 times H*W, a by-product of the kernel (differentiable like the ``y_i``).  ``checkpoints``: "auto",
    one step-local bit mask for every layer (an int) or one mask per layer (a tuple) — with masks there is no host wait
    at all and the call is hipGraph-capturable."""
    specs = tuple((_as_schedule(ly["steps"]), bool(ly.get("smooth3", False)), ly.get("clamp_max"),
                   float(ly.get("eps", 1e-6))) for ly in layers)
    flat = []
    for ly in layers:
        flat += [ly["alpha_base"], ly["beta_base"], ly["alpha_time_coeff"], ly["beta_time_coeff"], ly["M"]]
    if isinstance(checkpoints, list):
        checkpoints = tuple(checkpoints)
    nl = len(layers)
    if _is_f64(u, weights, *flat) or _is_rect(u):
        # float64, or a rectangular plane (H != W: no one-launch kernels): one layer after another (adi_diffuse_mixed),
        # the weighted sum and the plane sums in torch
        ys = []
        for i, ly in enumerate(layers):
            ck = checkpoints[i] if isinstance(checkpoints, tuple) else checkpoints
            ys.append(adi_diffuse_mixed(u, ly["alpha_base"], ly["beta_base"], ly["alpha_time_coeff"], ly["beta_time_coeff"],
                                        ly["M"], specs[i][0], "pre", smooth3=specs[i][1], clamp_max=specs[i][2],
                                        eps=specs[i][3], checkpoints=ck))
        out = sum(w * y for w, y in zip(weights, ys)) if weights is not None else ys[-1]
        if plane_sums:
            return out, ys, [y.sum(dim=(2, 3)) for y in ys]
        return out, ys
    u = _io_in(u, weights, *flat)
    f16 = u.dtype == torch.float16
    H = L.host_ext()
    if H is not None and u.dim() == 4 and u.is_cuda and u.shape[0] > 0 and len({len(sp[0][0]) for sp in specs}) == 1:
        # the native host path (csrc/host_ext.cpp): the same call of the C ABI from a C++ autograd node
        if checkpoints == "auto":
            mode, masks = 1, []
        else:
            masks = [int(checkpoints)] * nl if not isinstance(checkpoints, tuple) else [int(c) for c in checkpoints]
            if len(masks) != nl:
                raise L.PdeError(f"adi_diffuse_multi: {len(masks)} checkpoint masks for {nl} layers")
            mode = 0
        B, Cc, N, _ = u.shape
        io = _io_dtype(u)
        addrs = [C.addressof(_make_desc(B, Cc, N, io, st.flat, sm, cm, ep)) for st, sm, cm, ep in specs]
        res = H.multi(u, weights, flat, addrs, len(specs[0][0][0]), bool(plane_sums), mode, masks, CKPT_AMAX)
    else:
        res = _AdiMultiFn.apply(u, weights, specs, bool(plane_sums), checkpoints, *flat)
    if plane_sums:
        # the plane sums leave the kernel in fp32; on the float16 route they are fp16 like every other output
        sums = [s.half() for s in res[1 + nl:]] if f16 else list(res[1 + nl:])
        return res[0], list(res[1:1 + nl]), sums
    return res[0], list(res[1:])


_small_ok_cache = {}


def adi_small_supported(u, steps, smooth3=False, clamp_max=None, eps=1e-6) -> bool:
    """True when ``adi_diffuse_small`` can run this layer call (C <= 4, N in {16, 28, 32}, Strang or Lie steps; not
    float64)."""
    if u.dim() != 4 or u.shape[2] != u.shape[3] or not u.is_cuda or u.dtype == torch.float64:
        return False
    B, Cc, N, _ = u.shape
    if B == 0 or Cc > 4 or N > L.PDE_MAX_N or len(steps) * len(steps[0]) > L.PDE_MAX_SWEEPS:
        return False
    io = {torch.bfloat16: L.PDE_IO_BF16, torch.float16: L.PDE_IO_F16}.get(u.dtype, L.PDE_IO_F32)
    steps = _as_schedule(steps)
    key = (B, Cc, N, io, steps.flat, bool(smooth3), clamp_max, float(eps), len(steps[0]))
    ok = _small_ok_cache.get(key)
    if ok is None:
        if len(_small_ok_cache) > 256:
            _small_ok_cache.clear()
        d = _make_desc(B, Cc, N, io, steps.flat, smooth3, clamp_max, eps)
        ok = _small_ok_cache[key] = bool(L.load().pde_adi_small_supported(C.byref(d), len(steps[0])))
    return ok


def adi_diffuse_small(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, steps, mode: str, skip_weight=None,
                      smooth3: bool = False, clamp_max: Optional[float] = None, eps: float = 1e-6, checkpoints="auto",
                      kmax_sink: Optional[list] = None):
    """``adi_diffuse_mixed`` (plus the SVHN skip blend when ``skip_weight`` is given) for C <= 4 channels: the whole
    time loop in one launch forward and one backward.  Check ``adi_small_supported`` first."""
    if mode not in ("pre", "post"):
        raise ValueError(mode)
    steps = _as_schedule(steps)
    every = (u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, skip_weight)
    if _is_f64(*every) or (_fwad._current_level >= 0 and _has_tangent(*every)):
        # float64: no one-launch kernels; the layer out of its pieces (adi_diffuse_mixed composes it per step).  Forward
        # mode (a tangent on an argument inside a dual level) too: the one-launch node has no jvp, the pieces have one
        y = adi_diffuse_mixed(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, steps, mode, smooth3=smooth3,
                              clamp_max=clamp_max, eps=eps, checkpoints=checkpoints)
        return y if skip_weight is None else skip_blend(u, y, skip_weight)
    u = _io_in(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, skip_weight)
    if kmax_sink is None and (checkpoints == "auto" or isinstance(checkpoints, int)) and u.shape[0] > 0:
        H = L.host_ext()
        if H is not None and u.dim() == 4 and u.is_cuda:
            # the native host path (csrc/host_ext.cpp): the same call of the C ABI from a C++ autograd node
            B, Cc, N, _ = u.shape
            d = _make_desc(B, Cc, N, _io_dtype(u), steps.flat, smooth3, clamp_max, eps)
            return H.small(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, skip_weight, C.addressof(d),
                           len(steps[0]), 1 if mode == "pre" else 2, 1 if checkpoints == "auto" else 0,
                           0 if checkpoints == "auto" else int(checkpoints), CKPT_AMAX)
    return _AdiSmallFn.apply(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, skip_weight, steps, mode,
                             bool(smooth3), clamp_max, float(eps), checkpoints, kmax_sink)


def adi_diffuse_mixed(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, steps, mode: str,
                      smooth3: bool = False, clamp_max: Optional[float] = None, eps: float = 1e-6, checkpoints="auto",
                      kmax_sink: Optional[list] = None):
    """All time steps of a layer with a channel operator ``M`` between them, as one autograd node.

    ``steps``: list of per-step sweep lists (``adi_schedule``); ``mode`` "pre": ``u <- M u`` before every
    step (cifar10.py:91), "post": after every step (SVHN.py:71).  ``checkpoints``: "auto" or a bit mask
    relative to a step (bit 0 = state after the step's first sweep), applied to every step."""
    if mode not in ("pre", "post"):
        raise ValueError(mode)
    if u.shape[0] == 0:
        return _empty_passthrough(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M)
    steps = tuple(tuple(st) for st in steps)
    if len({len(st) for st in steps}) != 1:
        raise ValueError("every step must have the same number of sweeps")
    if not _is_f64(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M):
        u = _io_in(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M)
    if _is_rect(u):
        _check_rect(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff)   # before the first operator launch
    dual = _fwad._current_level >= 0 and _has_tangent(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M)
    if u.dim() == 4 and u.is_cuda and (dual or _is_rect(u) or L.load().pde_adi_line_length_path(int(u.shape[-1])) == 2 or
                                       _is_f64(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M)):
        # forward mode (a tangent on an argument inside a dual level: the per-step nodes carry the jvp), or
        # a rectangle (H != W: no per-step entry points either), or
        # a line length without fused kernels (pde_adi_line_length_path: any size up to PDE_MAX_N_GENERIC): the per-step
        # entry points do not exist there; compose the layer from its own pieces — the channel operator and the sweeps of
        # one step per call, chained by autograd (the step-local checkpoint mask applies to every step unchanged).  float64
        # takes this route at every line length: its sweeps are the any-size kernels instantiated for double
        return adi_diffuse_mixed_per_step(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, steps, mode,
                                          smooth3=smooth3, clamp_max=clamp_max, eps=eps, checkpoints=checkpoints,
                                          kmax_sink=kmax_sink)
    if kmax_sink is None and (checkpoints == "auto" or isinstance(checkpoints, int)):
        H = L.host_ext()
        if H is not None and u.dim() == 4 and u.is_cuda and u.shape[2] == u.shape[3]:
            # the native host path (csrc/host_ext.cpp): the same two calls of the C ABI from a C++ autograd node
            B, Cc, N, _ = u.shape
            flat = tuple(s for st in steps for s in st)
            d = _make_desc(B, Cc, N, _io_dtype(u), flat, smooth3, clamp_max, eps)
            return H.mixed(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, C.addressof(d), len(steps[0]),
                           1 if mode == "pre" else 2, 1 if checkpoints == "auto" else 0,
                           0 if checkpoints == "auto" else int(checkpoints), CKPT_AMAX)
    return _AdiMixedFn.apply(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, steps, mode, bool(smooth3),
                             clamp_max, float(eps), checkpoints, kmax_sink)


def adi_diffuse_mixed_per_step(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, steps, mode: str,
                               smooth3: bool = False, clamp_max: Optional[float] = None, eps: float = 1e-6,
                               checkpoints="auto", kmax_sink: Optional[list] = None, states: Optional[list] = None):
    """A layer with a channel operator composed from its own pieces, at every C and every plane: the operator and the sweeps
    of one step per call, chained by autograd (the step-local checkpoint mask applies to every step unchanged).  This is
    how ``adi_diffuse_mixed`` runs rectangles, line lengths without fused kernels and float64.  ``states``: a list that
    receives the state after every step — after the step's sweeps and, in "post" mode, after its operator; each one is a
    node of the autograd graph, so a loss may be put on any of them."""
    tickets = [] if kmax_sink is not None else None
    for st in steps:
        if mode == "pre":
            u = channel_mix(u, M)
        u = adi_diffuse(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, st, smooth3=smooth3,
                        clamp_max=clamp_max, eps=eps, checkpoints=checkpoints, kmax_sink=tickets)
        if mode == "post":
            u = channel_mix(u, M)
        if states is not None:
            states.append(u)
    if tickets and len(tickets) == len(steps):           # the whole layer's maxima, step after step (lagged plans)
        kmax_sink.append(_KmaxConcat(tickets))
    return u


def _empty_passthrough(u, *params):
    """Empty batch: nothing to launch.  Like the reference's torch ops, pass the empty tensor through and
    keep it connected to the parameters (their gradients are zeros, not None)."""
    _require_cuda(u, *params)
    if _is_f64(u, *params):
        u = u.to(torch.float64)
    tie = sum((p.sum() for p in params if isinstance(p, torch.Tensor)), u.new_zeros(()))
    return u + 0 * tie.to(u.dtype)


def adi_diffuse(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, sweeps: Sequence[Sweep],
                smooth3: bool = False, clamp_max: Optional[float] = None, eps: float = 1e-6, checkpoints="auto",
                kmax_sink: Optional[list] = None):
    """Run ``sweeps`` (a flat list) of implicit diffusion on ``u`` (B,C,N,N) in one fused launch; a rectangular
    ``u`` (B,C,H,W) with (C,H,W) parameters, both sides in [2, 128], runs on the any-size kernels (pde_adi_rect_*).

    Replaces the reference's time loop over diffuse_x/diffuse_y/thomas_solver_batch
    (mnist_test.py:44-198, cifar10.py:74-211) and its autograd backward.

    ``checkpoints``: "auto" (default) chooses the backward's checkpoints from the coefficients
    (``plan_checkpoints``); an int is an explicit bit mask (0: rebuild every state from the output).
    ``kmax_sink``: a list that receives an object with ``.host`` (pinned tensor) and ``.event``: the per-sweep
    maximum coefficient of this call (valid once the event has completed).
    """
    if u.shape[0] == 0:
        return _empty_passthrough(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff)
    if not isinstance(sweeps, tuple):
        sweeps = tuple(sweeps)
    # the sub-family, decided here once: a rectangle (H != W) and float64 run through the ctypes node only (no
    # host-extension path); float64 and float16 by the same rules on a rectangle as on a square
    rect = _is_rect(u)
    f64 = _is_f64(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff)
    if not f64:
        u = _io_in(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff)
    if _fwad._current_level >= 0 and _has_tangent(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff):
        # forward mode: the ctypes node carries the jvp (the C++ nodes cannot), and is told to keep what it reads
        return _apply_dual(_AdiFn, u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff,
                           sweeps, bool(smooth3), clamp_max, float(eps), checkpoints, kmax_sink, None, rect, f64)
    if not (rect or f64) and (isinstance(checkpoints, int) or (kmax_sink is None and checkpoints == "auto")):
        H = L.host_ext()
        if H is not None and u.dim() == 4 and u.is_cuda and u.dtype in _IO_TYPES:
            # the native host path (csrc/host_ext.cpp): the same two calls of the C ABI from a C++ autograd node
            B, Cc, N, _ = u.shape
            d = _make_desc(B, Cc, N, _io_dtype(u), sweeps, smooth3, clamp_max, eps)
            if checkpoints == "auto":
                mode, lo, hi = 1, 0, 0
            else:
                bits = int(checkpoints)
                mode, lo, hi = 0, bits & _M64, (bits >> 64) & _M64
                lo, hi = (lo - (1 << 64) if lo >> 63 else lo), (hi - (1 << 64) if hi >> 63 else hi)
            if kmax_sink is not None:                         # "lagged": an explicit mask now, the maxima for the next plan
                y, tk = H.adi_lagged(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, C.addressof(d), lo, hi)
                if tk is not None:
                    kmax_sink.append(tk)
                return y
            return H.adi(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, C.addressof(d), mode, lo, hi, CKPT_AMAX)
    return _AdiFn.apply(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff,
                        sweeps, bool(smooth3), clamp_max, float(eps), checkpoints, kmax_sink, None, rect, f64)


def adi_diffuse_states(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, sweeps: Sequence[Sweep], emit,
                       smooth3: bool = False, clamp_max: Optional[float] = None, eps: float = 1e-6, checkpoints="auto",
                       kmax_sink: Optional[list] = None):
    """``adi_diffuse`` that returns the trajectory: the state after every sweep listed in ``emit`` (strictly increasing
    0-based sweep indices; the last sweep is always included) as ONE tensor (K', B, C, H, W), out of the same single
    launch per pass.  With 16-bit tensors an emitted state is the fp32 state rounded once; the time loop goes on
    unrounded, so the last slice is bit for bit what ``adi_diffuse`` returns.  Differentiable: ``u`` and the four
    coefficient tensors receive the gradient of a loss on any of the returned states.  Squares and rectangles, fp32 /
    bf16 / fp16 tensors and float64 by the rules of ``adi_diffuse``; always the ctypes path (the native host extension
    does not know this call).  ``checkpoints`` / ``kmax_sink`` as in ``adi_diffuse``."""
    if not isinstance(sweeps, tuple):
        sweeps = tuple(sweeps)
    S = len(sweeps)
    emit = [int(s) for s in emit]
    if any(s < 0 or s >= S for s in emit) or any(b <= a for a, b in zip(emit, emit[1:])):
        raise ValueError(f"emit must be strictly increasing sweep indices in 0..{S - 1}, got {emit}")
    if S == 0:
        raise ValueError("no sweeps")
    if not emit or emit[-1] != S - 1:
        emit.append(S - 1)
    emit = tuple(emit)
    f64 = _is_f64(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff)
    if u.shape[0] == 0:
        y = _empty_passthrough(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff)
        return torch.stack([y] * len(emit))
    if not f64:
        u = _io_in(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff)
    if u.dim() != 4:
        raise L.PdeError(f"expected (B,C,H,W), got {tuple(u.shape)}")
    return _AdiFn.apply(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, sweeps, bool(smooth3), clamp_max,
                        float(eps), checkpoints, kmax_sink, emit, _is_rect(u), f64)


def _tangent_call(lib, fam, d, u, du, p, dp, want_y):
    """One ``*_tangent`` call of family ``fam`` (include/pdecnn_tangent.h) on kernel-ready tensors: (y or None, dy).
    The square fp32-parameter family at a line length that has fused kernels (N = 8 .. 32) takes
    ``pde_adi_tangent_fused`` (include/pdecnn_tangent_fused.h) instead, whose kernels read 16 bytes wide: a misaligned
    view is copied first.  ``PDE_TANGENT_FUSED=0`` keeps every size on the any-size kernels."""
    name = fam + "tangent"
    if fam == "pde_adi_" and L.tangent_fused_enabled():
        nbytes = lib.pde_adi_tangent_fused_workspace_bytes(C.byref(d))
        if nbytes > 0:
            name = "pde_adi_tangent_fused"
            u, du = _aligned(u), _aligned(du)
            p, dp = [_aligned(t) for t in p], [_aligned(t) for t in dp]
    if name == fam + "tangent":
        nbytes = getattr(lib, fam + "tangent_workspace_bytes")(C.byref(d))
    y = torch.empty_like(u) if want_y else None
    dy = torch.empty_like(u)
    ws = _workspace(nbytes, u.device)
    with torch.cuda.device(u.device):
        L.check(getattr(lib, name)(C.byref(d), _ptr(u), _ptr(du), *[_ptr(t) for t in p], *[_ptr(t) for t in dp],
                                   _ptr(y), _ptr(dy), _ptr(ws), ws.numel(), _stream()), name)
    return y, dy


def adi_diffuse_tangent(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, sweeps: Sequence[Sweep], *, du=None,
                        d_alpha_base=None, d_beta_base=None, d_alpha_time_coeff=None, d_beta_time_coeff=None,
                        smooth3: bool = False, clamp_max: Optional[float] = None, eps: float = 1e-6):
    """``(y, ydot)``: ``adi_diffuse`` and its directional derivative along the input tangent ``du`` and the four parameter
    tangents (None: zero; at least one must be given), in one pass of the tangent-linear kernel (pde_adi*_tangent).  Plain
    tensors, no autograd graph.  Squares and rectangles up to 128, fp32 / bf16 / fp16 tensors and float64 by the rules of
    ``adi_diffuse``.  Squares of N = 8, 12, ..., 32 that are not float64 run on the fused two-sided solver
    (pde_adi_tangent_fused: ``y`` is ``adi_diffuse``'s bit for bit); every other size, rectangles and float64 on the
    any-size kernels, and ``PDE_TANGENT_FUSED=0`` sends the fused sizes there too.  At a kink of the clamp the one-sided
    derivative of the forward's own mask is taken."""
    params = (alpha_base, beta_base, alpha_time_coeff, beta_time_coeff)
    dparams = (d_alpha_base, d_beta_base, d_alpha_time_coeff, d_beta_time_coeff)
    if du is None and all(t is None for t in dparams):
        raise ValueError("adi_diffuse_tangent needs du or a parameter tangent (use adi_diffuse for the value alone)")
    if not isinstance(sweeps, tuple):
        sweeps = tuple(sweeps)
    if u.dim() != 4:
        raise L.PdeError(f"expected (B,C,H,W), got {tuple(u.shape)}")
    if du is not None and du.shape != u.shape:
        raise L.PdeError(f"du of shape {tuple(du.shape)} does not match u {tuple(u.shape)}")
    rect = _is_rect(u)
    f64 = _is_f64(u, *params)
    with torch.no_grad():
        if not f64:
            u = _io_in(u, *params)
        if rect:
            _check_rect(u, *params)
        else:
            _require_cuda(u, *params)
        _require_cuda(du, *dparams)
        if u.shape[0] == 0:
            y = u.to(torch.float64) if f64 else u.clone()
            return y, torch.zeros_like(y)
        B, Cc, H, W = u.shape
        fam, desc_cls, as_chw = _ADI_FAMILY[rect, f64]
        u = _kernel_input(u.detach(), f64, align=1)          # the tangent kernels read one element at a time
        du = None if du is None else _kernel_input(du.detach().to(u.dtype), f64, align=1)
        p = [as_chw(t, Cc, H, W, 1) for t in params]
        dp = [None if t is None else as_chw(t, Cc, H, W, 1) for t in dparams]
        d = _desc(desc_cls, B, Cc, H, W, L.PDE_IO_F64 if f64 else _io_dtype(u), sweeps, smooth3, clamp_max, eps)
        return _tangent_call(L.load(), fam, d, u, du, p, dp, True)


def adi_diffuse_small_states(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, steps, mode: str, emit,
                             smooth3: bool = False, clamp_max: Optional[float] = None, eps: float = 1e-6, checkpoints="auto",
                             kmax_sink: Optional[list] = None):
    """``adi_diffuse_small`` (no skip blend) that returns the trajectory: the state after every time step listed in
    ``emit`` (strictly increasing 0-based step indices; the last step is always included) as ONE tensor
    (K', B, C, N, N), out of the same single launch per pass.  The state after a step is what the reference's loop holds
    at the end of that iteration: "pre" the step's sweep output, "post" the sweep output after the operator.  With 16-bit
    tensors the time loop goes on from the rounded sweep output of every step in grad mode and under ``no_grad`` alike,
    and a "post" state is the fp32 value rounded once.  Differentiable: ``u``, the four coefficient tensors and ``M``
    receive the gradient of a loss on any of the returned states.  Check ``adi_small_supported`` first; always the
    ctypes path.  ``checkpoints`` / ``kmax_sink`` as in ``adi_diffuse_small``."""
    if mode not in ("pre", "post"):
        raise ValueError(mode)
    steps = _as_schedule(steps)
    K = len(steps)
    emit = [int(k) for k in emit]
    if any(k < 0 or k >= K for k in emit) or any(b <= a for a, b in zip(emit, emit[1:])):
        raise ValueError(f"emit must be strictly increasing step indices in 0..{K - 1}, got {emit}")
    if K == 0:
        raise ValueError("no steps")
    if not emit or emit[-1] != K - 1:
        emit.append(K - 1)
    emit = tuple(emit)
    if u.shape[0] == 0:
        y = _empty_passthrough(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M)
        return torch.stack([y] * len(emit))
    u = _io_in(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M)
    return _AdiSmallFn.apply(u, alpha_base, beta_base, alpha_time_coeff, beta_time_coeff, M, None, steps, mode,
                             bool(smooth3), clamp_max, float(eps), checkpoints, kmax_sink, emit)


# --------------------------------------------------------------------------- channel mixing
class _MixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, M):
        lib = L.load()
        _require_cuda(u, M)
        B, Cc = u.shape[0], u.shape[1]
        HW = u[0, 0].numel()
        u_in = u
        if u.dtype not in _IO_TYPES:
            u = u.float()
        u = _aligned(u.contiguous())
        Mf = _aligned(M.detach().to(torch.float32).contiguous())
        out = torch.empty_like(u)
        with torch.cuda.device(u.device):
            L.check(lib.pde_channel_mix_forward(B, Cc, HW, _io_dtype(u), _ptr(u), _ptr(Mf), _ptr(out), _stream()),
                    "pde_channel_mix_forward")
        # M frozen (the operator is linear in u): the backward is gu = M^T gout alone and reads no u
        ctx.input_only = None
        if _grad_route(ctx.needs_input_grad[0], ctx.needs_input_grad[1]) == "input_only":
            ctx.input_only = (B, Cc, HW, u.dtype)
            ctx.save_for_backward(Mf)
        else:
            ctx.save_for_backward(u, Mf)
        ctx.primal_args = (u_in if ctx.input_only is None else None, M)
        ctx.dual = _take_dual(ctx)
        if ctx.dual:
            ctx.save_for_forward(u, M.detach())
        return out

    @staticmethod
    def jvp(ctx, ut, Mt):
        return _mix_jvp(_MixFn, ctx, ut, Mt)

    @staticmethod
    def backward(ctx, gout):
        if torch.is_grad_enabled():                      # create_graph=True: differentiable once more
            return _mix_second_order(_MixFn, ctx, gout)
        return _MixFn._backward(ctx, gout)

    @staticmethod
    def _backward(ctx, gout):
        lib = L.load()
        if ctx.input_only is not None:
            (Mf,) = ctx.saved_tensors
            B, Cc, HW, dtype = ctx.input_only
            gout = _aligned(gout.to(dtype).contiguous())
            gu = torch.empty_like(gout)
            ws = _workspace(lib.pde_channel_mix_backward_input_workspace_bytes(B, Cc, HW), gout.device)
            with torch.cuda.device(gout.device):
                L.check(lib.pde_channel_mix_backward_input(B, Cc, HW, _io_dtype(gout), _ptr(gout), _ptr(Mf), _ptr(gu), _ptr(ws),
                                                           ws.numel(), _stream()), "pde_channel_mix_backward_input")
            return gu, None
        u, Mf = ctx.saved_tensors
        B, Cc = u.shape[0], u.shape[1]
        HW = u[0, 0].numel()
        gout = _aligned(gout.to(u.dtype).contiguous())
        gu = torch.empty_like(u)
        gM = torch.empty_like(Mf)
        ws = _workspace(lib.pde_channel_mix_backward_workspace_bytes(B, Cc, HW), u.device)
        with torch.cuda.device(u.device):
            L.check(lib.pde_channel_mix_backward(B, Cc, HW, _io_dtype(u), _ptr(u), _ptr(gout), _ptr(Mf), _ptr(gu),
                                                 _ptr(gM), _ptr(ws), ws.numel(), _stream()),
                    "pde_channel_mix_backward")
        return gu, gM


def _mix_second_order(cls, ctx, gout):
    """``y = M u`` is bilinear, so both results of its backward are differentiable:
    <v, M^T g> + <W, g u^T> = <channel_mix(v, M) + channel_mix(u, W), g>."""
    u, M = ctx.primal_args

    def primal(v, W):
        out = None if v is None else cls.apply(v, M)
        if W is not None:
            t = cls.apply(u, W)
            out = t if out is None else out + t
        return out
    return linear_adjoint(lambda g: cls._backward(ctx, g), primal, (gout,), (u, M), n_diff=2)


def _mix_jvp(cls, ctx, ut, Mt):
    """Forward mode of ``y = M u``: ``M ut + Mt u``, each term the node's own forward kernel."""
    if not ctx.dual:
        raise NotImplementedError(_NO_JVP_ROUTE)
    u, M = ctx.saved_tensors
    out = None if ut is None else cls.apply(ut.to(u.dtype), M)
    if Mt is not None:
        t = cls.apply(u, Mt)
        out = t if out is None else out + t
    return torch.zeros_like(u) if out is None else out


def channel_mix(u, M):
    """out[b,i,p] = sum_j M[i,j] u[b,j,p] — cifar10.py:65-72 and SVHN.py:78-86."""
    if u.shape[0] == 0:
        return _empty_passthrough(u, M)
    f64 = _is_f64(u, M)
    if not f64:
        u = _io_in(u, M)
    if _fwad._current_level >= 0 and _has_tangent(u, M):
        return _apply_dual(_MixF64Fn if f64 else _MixFn, u, M)
    return _MixF64Fn.apply(u, M) if f64 else _MixFn.apply(u, M)


# --------------------------------------------------------------------------- BatchNorm2d + 4x4 avg/max pooling
# The nodes that are NOT linear in their input (this one, the symmetric layers, the gate combination) are differentiable
# once: their backwards are marked ``once_differentiable``, so differentiating through them twice raises instead of
# treating the first gradient as a constant.
class _BnPoolFn(torch.autograd.Function):
    """cifar10.py:346-353 in two passes over the activation (pde_tail.hip): statistics, then normalise + pool."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps):
        lib = L.load()
        _require_cuda(x, gamma, beta)
        B, Cc, N, _ = x.shape
        xf = _aligned(x.contiguous())
        gm = None if gamma is None else gamma.detach().to(torch.float32).contiguous()
        bt = None if beta is None else beta.detach().to(torch.float32).contiguous()
        mean = torch.empty(Cc, dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        out = torch.empty((B, 2 * Cc, 4, 4), dtype=torch.float32, device=x.device)
        amax = torch.empty((B, Cc, 4, 4), dtype=torch.int32, device=x.device)
        ws = _workspace(lib.pde_bn_pool_workspace_bytes(B, Cc), x.device)
        with torch.cuda.device(x.device):
            L.check(lib.pde_bn_pool_forward(B, Cc, N, _ptr(xf), _ptr(gm), _ptr(bt), float(eps), 1 if training else 0,
                                            float(momentum), _ptr(running_mean), _ptr(running_var), _ptr(mean), _ptr(invstd),
                                            _ptr(out), _ptr(amax), _ptr(ws), ws.numel(), _stream()), "pde_bn_pool_forward")
        ctx.save_for_backward(xf, gm, mean, invstd, amax)
        ctx.training = bool(training)
        ctx.has = (gamma is not None, beta is not None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        lib = L.load()
        xf, gm, mean, invstd, amax = ctx.saved_tensors
        B, Cc, N, _ = xf.shape
        g = _aligned(gout.to(torch.float32).contiguous())
        gx = torch.empty_like(xf)
        gg = torch.empty(Cc, dtype=torch.float32, device=xf.device)
        gb = torch.empty_like(gg)
        ws = _workspace(lib.pde_bn_pool_workspace_bytes(B, Cc), xf.device)
        with torch.cuda.device(xf.device):
            L.check(lib.pde_bn_pool_backward(B, Cc, N, _ptr(xf), _ptr(gm), _ptr(mean), _ptr(invstd), _ptr(amax), _ptr(g),
                                             1 if ctx.training else 0, _ptr(gx), _ptr(gg), _ptr(gb), _ptr(ws), ws.numel(),
                                             _stream()), "pde_bn_pool_backward")
        return gx, (gg if ctx.has[0] else None), (gb if ctx.has[1] else None), None, None, None, None, None


def bn_pool_supported(x, bn) -> bool:
    """Whether ``bn_pool`` takes (x, bn): fp32 CUDA tensor (B,C,N,N), N a multiple of 4 up to 64, a BatchNorm2d with a
    fixed momentum (or no running statistics).  A module without running statistics is taken in eval mode too: torch
    normalises with the batch statistics there, and so does ``bn_pool``."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[2] == x.shape[3] and x.shape[2] % 4 == 0
            and 4 <= x.shape[2] <= 64 and x.shape[0] > 0 and not torch.is_autocast_enabled()
            and (bn.momentum is not None or not bn.track_running_stats))


def bn_pool(x, bn):
    """``cat([adaptive_avg_pool2d(bn(x), 4), adaptive_max_pool2d(bn(x), 4)], dim=1)`` for a ``torch.nn.BatchNorm2d``
    module ``bn`` (cifar10.py:346-353) without materialising ``bn(x)``: (B,C,N,N) -> (B,2C,4,4).  Updates the module's
    running statistics in training mode exactly as the module would."""
    training = bn.training or bn.running_mean is None
    rm = bn.running_mean if (bn.track_running_stats and bn.training) or not training else None
    rv = bn.running_var if (bn.track_running_stats and bn.training) or not training else None
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return _BnPoolFn.apply(x, bn.weight, bn.bias, rm, rv, training, bn.momentum if bn.momentum is not None else 0.0, bn.eps)


# --------------------------------------------------------------------------- Ruthotto-Haber symmetric layer (MFMA)
_ACT_CODE = {"identity": 0, "relu": 1, "tanh": 2}


_sym_ws = {}


def _sym_workspace(B, D, dev):
    """Scratch for the partial tiles of the symmetric layer's split strip products: kept per (device, stream, width) —
    calls on one stream are ordered, calls on different streams get different buffers (and a captured graph keeps pointing
    at memory that stays allocated)."""
    n = L.load().pde_sym_layer_workspace_bytes(B, D)
    if n == 0:
        return None
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, D, n)
    ws = _sym_ws.get(key)
    if ws is None:
        if len(_sym_ws) > 64:
            _sym_ws.clear()
        ws = _sym_ws[key] = torch.empty(n, dtype=torch.uint8, device=dev)
    return ws


class _SymLayerFn(torch.autograd.Function):
    """out = base + scale * (act(BatchNorm1d(X K^T)) K) — cifar_2version.py:190-258 — on the fp32 matrix cores (pde_rh.hip)."""

    @staticmethod
    def forward(ctx, X, K, gamma, beta, base, running_mean, running_var, training, momentum, eps, scale, act):
        lib = L.load()
        _require_cuda(X, K, gamma, beta, base)
        B, D = X.shape
        Xf = _aligned(X.to(torch.float32).contiguous())
        Kf = _aligned(K.detach().to(torch.float32).contiguous())
        gm = gamma.detach().to(torch.float32).contiguous()
        bt = beta.detach().to(torch.float32).contiguous()
        bs = None if base is None else _aligned(base.to(torch.float32).contiguous())
        dev = X.device
        P = torch.empty((B, D), dtype=torch.float32, device=dev)
        H = torch.empty_like(P)
        out = torch.empty_like(P)
        mean = torch.empty(D, dtype=torch.float32, device=dev)
        invstd = torch.empty_like(mean)
        with torch.cuda.device(dev):
            ws = _sym_workspace(B, D, dev)
            L.check(lib.pde_sym_layer_forward(B, D, act, 1 if training else 0, _ptr(Xf), _ptr(Kf), _ptr(gm), _ptr(bt),
                                              _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), _ptr(bs),
                                              float(scale), _ptr(P), _ptr(H), _ptr(mean), _ptr(invstd), _ptr(out),
                                              _ptr(ws), 0 if ws is None else ws.numel(), _stream()),
                    "pde_sym_layer_forward")
        ctx.save_for_backward(Xf, Kf, gm, P, H, mean, invstd)
        ctx.cfg = (bool(training), float(scale), int(act), base is not None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        lib = L.load()
        Xf, Kf, gm, P, H, mean, invstd = ctx.saved_tensors
        training, scale, act, has_base = ctx.cfg
        B, D = Xf.shape
        g = _aligned(gout.to(torch.float32).contiguous())
        dev = Xf.device
        dP = torch.empty_like(Xf)
        gX = torch.empty_like(Xf)
        gK = torch.empty_like(Kf)
        gg = torch.empty(D, dtype=torch.float32, device=dev)
        gb = torch.empty_like(gg)
        with torch.cuda.device(dev):
            ws = _sym_workspace(B, D, dev)
            L.check(lib.pde_sym_layer_backward(B, D, act, 1 if training else 0, _ptr(g), float(scale), _ptr(Xf), _ptr(Kf),
                                               _ptr(gm), _ptr(P), _ptr(H), _ptr(mean), _ptr(invstd), _ptr(dP), _ptr(gX),
                                               _ptr(gK), _ptr(gg), _ptr(gb), _ptr(ws), 0 if ws is None else ws.numel(),
                                               _stream()), "pde_sym_layer_backward")
        return gX, gK, gg, gb, (g if has_base else None), None, None, None, None, None, None, None


SYM_LAYER_MAX_ROWS = 128      # one strip workgroup owns all rows of its 16 features up to here (the reference trains at 64)


def sym_layer_supported(X, bn) -> bool:
    """Whether ``sym_layer`` takes this input: an fp32 CUDA batch whose feature count is a multiple of
    64, outside autocast, and a BatchNorm1d with affine parameters and a fixed momentum."""
    if not (X.is_cuda and X.dtype == torch.float32 and X.dim() >= 2 and X.shape[0] > 0) or torch.is_autocast_enabled():
        return False
    D = X[0].numel()
    if bn.weight is None or bn.bias is None or (bn.momentum is None and bn.track_running_stats):
        return False
    if not bn.training and bn.running_mean is None:
        pass                                              # eval without running statistics = batch statistics: supported
    B = X.shape[0]
    # Policy, not capability (``sym_layer`` itself takes any batch): above SYM_LAYER_MAX_ROWS rows the row-block kernels
    # are 1.6-1.9x behind rocBLAS, so the module-level callers keep plain torch there; a training-mode
    # batch of one row is refused by torch.nn.BatchNorm1d ("Expected more than 1 value per channel") and must stay so.
    if B > SYM_LAYER_MAX_ROWS or (B == 1 and (bn.training or bn.running_mean is None)):
        return False
    return bool(L.load().pde_sym_layer_supported(B, D))


def sym_k16(K, dtype=torch.float16):
    """``K16 = r(K)``: the 16-bit copy of a symmetric layer's (D, D) weight that autocast makes once per region — fp16
    (the default) or ``torch.bfloat16``; the 16-bit-operand ``sym_layer`` takes it and picks its route by the copy's
    dtype.  Not differentiable (the layer's gradient goes to K)."""
    if dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"sym_k16 makes an fp16 or a bf16 copy, not {dtype}")
    bf = dtype == torch.bfloat16
    H_ = L.host_ext()
    if H_ is not None and K.is_cuda:
        return H_.sym_kbf16(K) if bf else H_.sym_k16(K)
    _require_cuda(K)
    Kf = _aligned(K.detach().to(torch.float32).contiguous())
    K16 = torch.empty(K.shape, dtype=dtype, device=K.device)
    with torch.cuda.device(K.device):
        if bf:
            L.check(L.load().pde_sym_k_to_bf16(K.shape[0], _ptr(Kf), _ptr(K16), _stream()), "pde_sym_k_to_bf16")
        else:
            L.check(L.load().pde_sym_k_to_f16(K.shape[0], _ptr(Kf), _ptr(K16), _stream()), "pde_sym_k_to_f16")
    return K16


def sym_layer_f16_supported(X, bn) -> bool:
    """Whether the fp16-operand ``sym_layer`` takes this input under ``torch.autocast("cuda", torch.float16)``: the
    rules of ``sym_layer_supported`` (fp32 X, D a multiple of 64, at most SYM_LAYER_MAX_ROWS rows, no one-row training
    batch) with autocast on for CUDA in fp16.  bf16 autocast and calls outside autocast are not taken."""
    dtype = torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype()
    if not (torch.is_autocast_enabled() and dtype == torch.float16):
        return False
    if not (X.is_cuda and X.dtype == torch.float32 and X.dim() >= 2 and X.shape[0] > 0):
        return False
    if bn.weight is None or bn.bias is None or (bn.momentum is None and bn.track_running_stats):
        return False
    B = X.shape[0]
    if B > SYM_LAYER_MAX_ROWS or (B == 1 and (bn.training or bn.running_mean is None)):
        return False
    return bool(L.load().pde_sym_layer_f16_supported(B, X[0].numel()))


def sym_layer_bf16_supported(X, bn) -> bool:
    """Whether the bf16-operand ``sym_layer`` takes this input under ``torch.autocast("cuda", torch.bfloat16)``: the
    rules of ``sym_layer_f16_supported`` with autocast on for CUDA in bf16."""
    dtype = torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype()
    if not (torch.is_autocast_enabled() and dtype == torch.bfloat16):
        return False
    if not (X.is_cuda and X.dtype == torch.float32 and X.dim() >= 2 and X.shape[0] > 0):
        return False
    if bn.weight is None or bn.bias is None or (bn.momentum is None and bn.track_running_stats):
        return False
    B = X.shape[0]
    if B > SYM_LAYER_MAX_ROWS or (B == 1 and (bn.training or bn.running_mean is None)):
        return False
    return bool(L.load().pde_sym_layer_bf16_supported(B, X[0].numel()))


def _sym16_forward(ctx, tag, dtype, X, K16, gamma, beta, base, running_mean, running_var, training, momentum, eps, scale, act):
    """Forward of the 16-bit-operand symmetric layer through ``pde_sym_layer_<tag>_forward`` (tag "f16" or "bf16")."""
    lib = L.load()
    _require_cuda(X, K16, gamma, beta, base)
    B, D = X.shape
    Xf = _aligned(X.to(torch.float32).contiguous())
    gm = gamma.detach().to(torch.float32).contiguous()
    bt = beta.detach().to(torch.float32).contiguous()
    bs = None if base is None else _aligned(base.to(torch.float32).contiguous())
    K16 = _aligned(K16)
    dev = X.device
    P = torch.empty((B, D), dtype=dtype, device=dev)
    H = torch.empty_like(P)
    out = torch.empty((B, D), dtype=dtype if bs is None else torch.float32, device=dev)
    mean = torch.empty(D, dtype=torch.float32, device=dev)
    invstd = torch.empty_like(mean)
    name = f"pde_sym_layer_{tag}_forward"
    with torch.cuda.device(dev):
        ws = torch.empty(getattr(lib, f"pde_sym_layer_{tag}_workspace_bytes")(B, D), dtype=torch.uint8, device=dev)
        L.check(getattr(lib, name)(B, D, act, 1 if training else 0, _ptr(Xf), _ptr(K16), _ptr(gm), _ptr(bt),
                                   _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), _ptr(bs),
                                   float(scale), _ptr(P), _ptr(H), _ptr(mean), _ptr(invstd), _ptr(out), _ptr(ws),
                                   ws.numel(), _stream()), name)
    ctx.save_for_backward(Xf, K16, gm, P, H, mean, invstd)
    ctx.cfg = (bool(training), float(scale), int(act), base is not None)
    return out


def _sym16_backward(ctx, tag, gout):
    lib = L.load()
    Xf, K16, gm, P, H, mean, invstd = ctx.saved_tensors
    training, scale, act, has_base = ctx.cfg
    B, D = Xf.shape
    g = _aligned(gout.to(torch.float32).contiguous())
    dev = Xf.device
    dP = torch.empty_like(P)
    gX = torch.empty_like(Xf)
    gK = torch.empty((D, D), dtype=torch.float32, device=dev)
    gg = torch.empty(D, dtype=torch.float32, device=dev)
    gb = torch.empty_like(gg)
    name = f"pde_sym_layer_{tag}_backward"
    with torch.cuda.device(dev):
        ws = torch.empty(getattr(lib, f"pde_sym_layer_{tag}_workspace_bytes")(B, D), dtype=torch.uint8, device=dev)
        L.check(getattr(lib, name)(B, D, act, 1 if training else 0, _ptr(g), float(scale), _ptr(Xf), _ptr(K16), _ptr(gm),
                                   _ptr(P), _ptr(H), _ptr(mean), _ptr(invstd), _ptr(dP), _ptr(gX), _ptr(gK), _ptr(gg),
                                   _ptr(gb), _ptr(ws), ws.numel(), _stream()), name)
    return gX, gK, None, gg, gb, (g if has_base else None), None, None, None, None, None, None, None


class _SymLayerF16Fn(torch.autograd.Function):
    """The fp16-operand symmetric layer (pde_rh.hip: fp16 autocast's rounding points on the fp16 matrix cores): ctypes twin
    of the C++ node ``sym_f16`` (csrc/host_ext.cpp), same calls in the same order.  Scratch from the caching allocator
    for every call."""

    @staticmethod
    def forward(ctx, X, K, K16, gamma, beta, base, running_mean, running_var, training, momentum, eps, scale, act):
        return _sym16_forward(ctx, "f16", torch.float16, X, K16, gamma, beta, base, running_mean, running_var, training,
                              momentum, eps, scale, act)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        return _sym16_backward(ctx, "f16", gout)


class _SymLayerBf16Fn(torch.autograd.Function):
    """The same under bf16 autocast (bf16 rounding points on the bf16 matrix cores): ctypes twin of the C++ node
    ``sym_bf16``."""

    @staticmethod
    def forward(ctx, X, K, K16, gamma, beta, base, running_mean, running_var, training, momentum, eps, scale, act):
        return _sym16_forward(ctx, "bf16", torch.bfloat16, X, K16, gamma, beta, base, running_mean, running_var, training,
                              momentum, eps, scale, act)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        return _sym16_backward(ctx, "bf16", gout)


def sym_layer(X, K, bn, activation: str = "relu", base=None, scale: float = -1.0, K16=None):
    """``base + scale * (act(bn(X @ K.T)) @ K)`` for a dense (D, D) weight ``K`` and a ``torch.nn.BatchNorm1d`` ``bn``
    (cifar_2version.py:210-219; ``F_sym`` itself is ``base=None, scale=-1``; ParabolicBlock's step is ``base=Y, scale=-dt``,
    HamiltonianBlock's ``base=Y, scale=+dt`` on Z and ``base=Z, scale=+dt`` on Y).  X: (B, ...) flattened to (B, D); the result
    has X's shape.  Updates the module's running statistics in training mode exactly as the module would.

    ``K16`` (``sym_k16(K)`` or ``sym_k16(K, torch.bfloat16)``): the 16-bit-operand form, with CUDA fp16 or bf16 autocast's
    rounding points (include/pdecnn.h) on the matrix cores of that type, chosen by ``K16.dtype``; the result has
    K16's dtype without ``base`` (as autocast's ``F_sym``) and is fp32 with one (``base + r(scale Q)``, as
    ``Y + dt * F_sym``).  The gradient reaches ``K`` (fp32), not ``K16``.  X must be fp32 and
    ``sym_layer_f16_supported`` / ``sym_layer_bf16_supported`` hold."""
    shape = X.shape
    B = shape[0]
    X2 = X.reshape(B, -1)
    training = bn.training or bn.running_mean is None
    track = bn.track_running_stats and bn.running_mean is not None
    rm = bn.running_mean if (track and bn.training) or not training else None
    rv = bn.running_var if (track and bn.training) or not training else None
    if bn.training and track and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    b2 = None if base is None else base.reshape(B, -1)
    mom = bn.momentum if bn.momentum is not None else 0.0
    H_ = L.host_ext()
    if K16 is not None:
        if X2.dtype != torch.float32 or K16.dtype not in (torch.float16, torch.bfloat16):
            raise TypeError("sym_layer(K16=...) takes an fp32 X and an fp16 or bf16 K16")
        bf = K16.dtype == torch.bfloat16
        if H_ is not None and X2.is_cuda:
            out = (H_.sym_bf16 if bf else H_.sym_f16)(X2, K, K16, bn.weight, bn.bias, b2, rm, rv, bool(training), float(mom),
                                                      float(bn.eps), float(scale), _ACT_CODE[activation])
        else:
            out = (_SymLayerBf16Fn if bf else _SymLayerF16Fn).apply(X2, K, K16, bn.weight, bn.bias, b2, rm, rv, training, mom,
                                                                    bn.eps, scale, _ACT_CODE[activation])
        return out.view(shape)
    if H_ is not None and X2.is_cuda:
        # the native host path (csrc/host_ext.cpp): the same two calls of the C ABI from a C++ autograd node
        out = H_.sym(X2, K, bn.weight, bn.bias, b2, rm, rv, bool(training), float(mom), float(bn.eps), float(scale),
                     _ACT_CODE[activation])
    else:
        out = _SymLayerFn.apply(X2, K, bn.weight, bn.bias, b2, rm, rv, training, mom, bn.eps, scale, _ACT_CODE[activation])
    return out.view(shape)


# --------------------------------------------------------------------------- attention gates + weighted combination
class _GateCombineFn(torch.autograd.Function):
    """combined = sum_i w_i gate_i[b,c] y_i — cifar10.py:242 (x * attention_weights) and :277-280 in one pass; the
    backward in one pass too (scaled gradients of the y_i and the per-plane dots the gate/weight gradients need)."""

    @staticmethod
    def forward(ctx, weights, nl, *rest):
        lib = L.load()
        ys, gates = rest[:nl], rest[nl:]
        _require_cuda(weights, *rest)
        y0 = ys[0]
        dt = y0.dtype if y0.dtype in (torch.float32, torch.bfloat16) or _is_f16(*ys, *gates, weights) else torch.float32
        ys_c = [_aligned(y.to(dt).contiguous()) for y in ys]
        B, Cc = y0.shape[:2]
        HW = y0[0, 0].numel()
        g_c = [g.detach().to(torch.float32).reshape(B, Cc).contiguous() for g in gates]
        w_c = weights.detach().to(torch.float32).contiguous()
        out = torch.empty_like(ys_c[0])
        yp = (C.c_void_p * nl)(*[y.data_ptr() for y in ys_c])
        gp = (C.c_void_p * nl)(*[g.data_ptr() for g in g_c])
        with torch.cuda.device(y0.device):
            L.check(lib.pde_gate_combine_forward(nl, B, Cc, HW, _io_dtype(ys_c[0]), yp, gp, _ptr(w_c), _ptr(out), _stream()),
                    "pde_gate_combine_forward")
        ctx.save_for_backward(w_c, *ys_c, *g_c)
        ctx.nl = nl
        ctx.meta = (weights.dtype, [y.dtype for y in ys], [(g.dtype, g.shape) for g in gates])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lib = L.load()
        nl = ctx.nl
        w_c, *rest = ctx.saved_tensors
        ys_c, g_c = rest[:nl], rest[nl:]
        B, Cc = ys_c[0].shape[:2]
        HW = ys_c[0][0, 0].numel()
        g = _aligned(g.to(ys_c[0].dtype).contiguous())
        gys = [torch.empty_like(y) for y in ys_c]
        dots = [torch.empty((B, Cc), dtype=torch.float32, device=g.device) for _ in range(nl)]
        yp = (C.c_void_p * nl)(*[y.data_ptr() for y in ys_c])
        gp = (C.c_void_p * nl)(*[t.data_ptr() for t in g_c])
        gyp = (C.c_void_p * nl)(*[t.data_ptr() for t in gys])
        dp = (C.c_void_p * nl)(*[t.data_ptr() for t in dots])
        with torch.cuda.device(g.device):
            L.check(lib.pde_gate_combine_backward(nl, B, Cc, HW, _io_dtype(g), _ptr(g), yp, gp, _ptr(w_c), gyp, dp, _stream()),
                    "pde_gate_combine_backward")
        wdt, ydts, gmeta = ctx.meta
        gw = torch.stack([(g_c[i] * dots[i]).sum() for i in range(nl)]).to(wdt)
        ggates = [(w_c[i] * dots[i]).to(gmeta[i][0]).reshape(gmeta[i][1]) for i in range(nl)]
        return (gw, None, *[t.to(d) for t, d in zip(gys, ydts)], *ggates)


def gate_combine(ys, gates, weights):
    """``sum_i weights[i] * gates[i][:, :, None, None] * ys[i]`` in one pass over the tensors (cifar10.py:242,277-280)."""
    return _GateCombineFn.apply(weights, len(ys), *ys, *gates)


# --------------------------------------------------------------------------- explicit layers
# One node per family, as for the implicit sweeps: a plain call is the family's ``*_states`` call without a mask.  ``steps``
# None is the plain call of ``num_steps`` / ``nt`` steps (any count the library takes) and returns ``out``, a tensor of its
# own; otherwise ``steps`` are the emitted step numbers (the last one is the step count), ``bits`` their mask without the
# last, and the result is ONE tensor (K', ...) whose last slice is the library's ``out``.  ``f64`` picks the
# pde_*_f64_* entry points: every tensor in double, no tensor-type argument.
class _Explicit5Fn(torch.autograd.Function):
    dual = None                  # set on the ctx by a forward that _apply_dual marked: (alpha_base, channel_scaling) for the jvp

    @staticmethod
    def forward(ctx, u, alpha_base, channel_scaling, dt, eps, max_coeff, relax, num_steps, steps, bits, f64):
        lib = L.load()
        _require_cuda(u, alpha_base, channel_scaling)
        fam, kt = ("pde_explicit5_f64_", torch.float64) if f64 else ("pde_explicit5_", torch.float32)
        u = _kernel_input(u, f64, align=1)
        B, Cc, H, W = u.shape
        # rows of whole groups of four columns move four elements wide (16 bytes of fp32, 8 of 16-bit values); every other
        # plane, and float64, one element at a time
        ctx.align = 1 if (f64 or W % 4) else 4 * u.element_size()
        u = _aligned(u, ctx.align)
        a, s = _kernel_param(alpha_base, kt), _kernel_param(channel_scaling, kt)
        res, out, traj = _out_and_traj(u, steps)
        # alpha_base and channel_scaling frozen: the backward is the adjoint walk alone and reads neither u nor a state
        route = _grad_route(ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:3]))
        need_grad = route == "full"
        fused = not f64 and (H, W) in ((64, 64), (32, 32), (16, 16))     # planes that stay in registers over all steps
        # inputs of steps 2..num_steps: what the backward reads (and what chains the steps for generic plane sizes): fp32
        # whatever the tensors' type, or doubles
        states = torch.empty((num_steps - 1,) + tuple(u.shape), dtype=kt, device=u.device) \
            if num_steps > 1 and (need_grad or not fused) else None
        io = () if f64 else (_io_dtype(u),)
        with torch.cuda.device(u.device):
            L.check(getattr(lib, fam + "forward_states")(B, Cc, H, W, *io, _ptr(u), _ptr(a), _ptr(s), dt, eps, max_coeff,
                                                         relax, num_steps, _ptr(states), _ptr(out), _ptr(traj),
                                                         None if steps is None else _mask128(bits), _stream()),
                    fam + "forward_states")
        ctx.input_only = None
        if route == "input_only":
            ctx.input_only = (tuple(u.shape), u.dtype, u.device)
            ctx.save_for_backward(a, s)
        else:
            ctx.save_for_backward(u, states if need_grad else None, a, s)
        ctx.cfg = (dt, eps, max_coeff, relax, num_steps, steps, bits, f64)
        ctx.p_dtypes = (alpha_base.dtype, channel_scaling.dtype)
        ctx.primal_args = ((alpha_base, channel_scaling), ctx.cfg)
        if getattr(_dual, "on", False) and _take_dual(ctx):     # a tangent came in (explicit5_step decided): what the jvp reads
            ctx.save_for_forward(u, a, s)
            ctx.dual = (alpha_base.detach(), channel_scaling.detach())
        return res

    @staticmethod
    def jvp(ctx, ut, dat, dst, *_):
        """Forward mode.  The layer is linear in ``u``: with no parameter tangent the output tangent is the layer's own
        forward at ``ut``.  Otherwise one ``pde_explicit5[_f64]_tangent`` call."""
        dt, eps, max_coeff, relax, num_steps, steps, _, f64 = ctx.cfg
        if steps is not None:
            raise NotImplementedError(_NO_TRAJ_JVP)
        if ctx.dual is None:
            raise NotImplementedError(_NO_JVP_ROUTE)
        u, a, s = ctx.saved_tensors
        if dat is None and dst is None:
            if ut is None:
                return torch.zeros_like(u)
            return explicit5_step(ut.to(u.dtype), *ctx.dual, dt, eps, max_coeff, relax, num_steps).to(u.dtype)
        du = None if ut is None else _aligned(_kernel_input(ut.to(u.dtype), f64, align=1), ctx.align)
        da, ds = (None if t is None else _kernel_param(t, a.dtype) for t in (dat, dst))
        return _explicit5_tangent_call(L.load(), f64, u, du, a, s, da, ds, (dt, eps, max_coeff, relax, num_steps), False)[1]

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():                      # create_graph=True: differentiable once more
            return _second_order(_Explicit5Fn, ctx, (g,))
        return _Explicit5Fn._backward(ctx, g)

    @staticmethod
    def _backward(ctx, g):
        lib = L.load()
        dt, eps, max_coeff, relax, num_steps, steps, bits, f64 = ctx.cfg
        fam = "pde_explicit5_f64_" if f64 else "pde_explicit5_"
        if ctx.input_only is not None:
            a, s = ctx.saved_tensors
            shape, dtype, device = ctx.input_only
            B, Cc, H, W = shape
            gout, gtraj = _cotangents(g, dtype, steps, ctx.align)
            gu = torch.empty(shape, dtype=dtype, device=device)
            io = () if f64 else (_io_dtype(gu),)
            n = getattr(lib, fam + "backward_input_workspace_bytes")(B, Cc, H, W, *io, num_steps)
            ws = _workspace(n, device) if n else None
            with torch.cuda.device(device):
                L.check(getattr(lib, fam + "backward_input_states")(B, Cc, H, W, *io, _ptr(gout), _ptr(gtraj),
                                                                    None if steps is None else _mask128(bits), _ptr(a),
                                                                    _ptr(s), dt, eps, max_coeff, relax, num_steps, _ptr(gu),
                                                                    _ptr(ws), n, _stream()), fam + "backward_input_states")
            return (gu,) + (None,) * 10
        u, states, a, s = ctx.saved_tensors
        B, Cc, H, W = u.shape
        gout, gtraj = _cotangents(g, u.dtype, steps, ctx.align)
        gu, ga, gs = torch.empty_like(u), torch.empty_like(a), torch.empty_like(s)
        io = () if f64 else (_io_dtype(u),)
        ws = _workspace(getattr(lib, fam + "backward_workspace_bytes")(B, Cc, H, W, *io, num_steps), u.device)
        with torch.cuda.device(u.device):
            L.check(getattr(lib, fam + "backward_states")(B, Cc, H, W, *io, _ptr(u), _ptr(states), _ptr(gout), _ptr(gtraj),
                                                          None if steps is None else _mask128(bits), _ptr(a), _ptr(s), dt,
                                                          eps, max_coeff, relax, num_steps, _ptr(gu), _ptr(ga), _ptr(gs),
                                                          _ptr(ws), ws.numel(), _stream()), fam + "backward_states")
        return (gu, _grad_as(ga, ctx.p_dtypes[0]), _grad_as(gs, ctx.p_dtypes[1])) + (None,) * 8


def explicit5_step(u, alpha_base, channel_scaling, dt=0.01, eps=1e-6, max_coeff=0.15, relax=0.1, num_steps=1):
    """``num_steps`` relaxed explicit 5-point steps in one call — tiny_imagenet.py:38-49,53-72."""
    if u.shape[0] == 0 or num_steps < 1:
        return _empty_passthrough(u, alpha_base, channel_scaling)
    f64 = _is_f64(u, alpha_base, channel_scaling)
    if not f64:
        u = _io_in(u, alpha_base, channel_scaling)
    if _fwad._current_level >= 0 and _has_tangent(u, alpha_base, channel_scaling):
        # forward mode: the node is told to keep what its jvp reads
        return _apply_dual(_Explicit5Fn, u, alpha_base, channel_scaling, float(dt), float(eps), float(max_coeff),
                           float(relax), int(num_steps), None, None, f64)
    return _Explicit5Fn.apply(u, alpha_base, channel_scaling, float(dt), float(eps), float(max_coeff), float(relax),
                              int(num_steps), None, None, f64)


def _explicit5_tangent_call(lib, f64, u, du, a, s, da, ds, cfg, want_y):
    """One ``pde_explicit5[_f64]_tangent`` call (include/pdecnn_explicit_tangent.h) on kernel-ready tensors: (y or None, dy)."""
    dt, eps, max_coeff, relax, num_steps = cfg
    fam = "pde_explicit5_f64_" if f64 else "pde_explicit5_"
    B, Cc, H, W = u.shape
    io = () if f64 else (_io_dtype(u),)
    y = torch.empty_like(u) if want_y else None
    dy = torch.empty_like(u)
    n = getattr(lib, fam + "tangent_workspace_bytes")(B, Cc, H, W, *io, num_steps)
    ws = _workspace(n, u.device) if n else None
    with torch.cuda.device(u.device):
        L.check(getattr(lib, fam + "tangent")(B, Cc, H, W, *io, _ptr(u), _ptr(du), _ptr(a), _ptr(s), _ptr(da), _ptr(ds), dt,
                                              eps, max_coeff, relax, num_steps, _ptr(y), _ptr(dy), _ptr(ws), n, _stream()),
                fam + "tangent")
    return y, dy


def explicit5_tangent(u, alpha_base, channel_scaling, *, du=None, d_alpha_base=None, d_channel_scaling=None, dt=0.01, eps=1e-6,
                      max_coeff=0.15, relax=0.1, num_steps=1):
    """``(y, ydot)``: ``explicit5_step`` and its directional derivative along the input tangent ``du`` and the tangents of
    ``alpha_base`` and ``channel_scaling`` (None: zero; at least one must be given), the primal and the tangent state
    advanced together (pde_explicit5[_f64]_tangent: one launch for 64x64, 32x32 and 16x16 planes, one per step otherwise).
    Plain tensors, no autograd graph.  fp32, bf16, the float16 route and float64 by the rules of ``explicit5_step``; ``y``
    is bit for bit its result.  Where ``alpha_base`` sits on a bound of the clamp the derivative passes, as torch's does."""
    dparams = (d_alpha_base, d_channel_scaling)
    if du is None and all(t is None for t in dparams):
        raise ValueError("explicit5_tangent needs du or a parameter tangent (use explicit5_step for the value alone)")
    if u.dim() != 4:
        raise L.PdeError(f"expected (B,C,H,W), got {tuple(u.shape)}")
    if du is not None and du.shape != u.shape:
        raise L.PdeError(f"du of shape {tuple(du.shape)} does not match u {tuple(u.shape)}")
    if num_steps < 1:
        raise ValueError(f"num_steps must be at least 1, got {num_steps}")
    f64 = _is_f64(u, alpha_base, channel_scaling)
    with torch.no_grad():
        if not f64:
            u = _io_in(u, alpha_base, channel_scaling)
        _require_cuda(u, alpha_base, channel_scaling, du, *dparams)
        if u.shape[0] == 0:
            y = u.to(torch.float64) if f64 else u.clone()
            return y, torch.zeros_like(y)
        kt = torch.float64 if f64 else torch.float32
        u = _kernel_input(u.detach(), f64, align=1)
        align = 1 if (f64 or u.shape[3] % 4) else 4 * u.element_size()
        u = _aligned(u, align)
        du = None if du is None else _aligned(_kernel_input(du.detach().to(u.dtype), f64, align=1), align)
        a, s = _kernel_param(alpha_base, kt), _kernel_param(channel_scaling, kt)
        da, ds = (None if t is None else _kernel_param(t, kt) for t in dparams)
        return _explicit5_tangent_call(L.load(), f64, u, du, a, s, da, ds,
                                       (float(dt), float(eps), float(max_coeff), float(relax), int(num_steps)), True)


class _JacobiFn(torch.autograd.Function):
    """fp32 tensors, fp16 ones on the float16 route (pde_jacobi_io_*: the same kernels with fp16 I/O; anything else is
    widened to fp32), or float64 (pde_jacobi_f64_*)."""
    dual = None                  # set on the ctx by a forward that _apply_dual marked: (a_row, b_col) for the jvp

    @staticmethod
    def forward(ctx, u, a_row, b_col, nt, steps, bits, f64):
        lib = L.load()
        _require_cuda(u, a_row, b_col)
        fam, kt = ("pde_jacobi_f64_", torch.float64) if f64 else ("pde_jacobi_io_", torch.float32)
        ctx.align = 1                                            # the Jacobi kernels move one element at a time
        u = _kernel_input(u, f64, (torch.float32, torch.float16), align=1)
        B, H, W = u.shape
        a, b = _kernel_param(a_row, kt), _kernel_param(b_col, kt)
        res, out, traj = _out_and_traj(u, steps)
        with torch.cuda.device(u.device):
            if f64:
                io, fws = (), ()
            else:
                # a tiled plane with more steps than one launch takes: the launches chain through a workspace
                n = lib.pde_jacobi_forward_workspace_bytes(B, H, W, nt)
                ws = _workspace(n, u.device) if n else None
                io, fws = (_io_dtype(u),), (_ptr(ws), ws.numel() if n else 0)
            L.check(getattr(lib, fam + "forward_states")(B, H, W, nt, *io, _ptr(u), _ptr(a), _ptr(b), _ptr(out), _ptr(traj),
                                                         None if steps is None else _mask128(bits), *fws, _stream()),
                    fam + "forward_states")
        # a_row and b_col frozen: the backward is the adjoint walk alone and reads no u
        ctx.input_only = None
        if _grad_route(ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:3])) == "input_only":
            ctx.input_only = (tuple(u.shape), u.dtype, u.device)
            ctx.save_for_backward(a, b)
        else:
            ctx.save_for_backward(u, a, b)
        ctx.cfg = (nt, steps, bits, f64)
        ctx.p_dtypes = (a_row.dtype, b_col.dtype)
        ctx.primal_args = ((a_row, b_col), ctx.cfg)
        if getattr(_dual, "on", False) and _take_dual(ctx):     # a tangent came in (jacobi_diffuse decided): what the jvp reads
            ctx.save_for_forward(u, a, b)
            ctx.dual = (a_row.detach(), b_col.detach())
        return res

    @staticmethod
    def jvp(ctx, ut, dat, dbt, *_):
        """Forward mode.  The layer is linear in ``u``: with no coefficient tangent the output tangent is the layer's own
        forward at ``ut``.  Otherwise one ``pde_jacobi_io_tangent`` / ``pde_jacobi_f64_tangent`` call."""
        nt, steps, _, f64 = ctx.cfg
        if steps is not None:
            raise NotImplementedError(_NO_TRAJ_JVP)
        if ctx.dual is None:
            raise NotImplementedError(_NO_JVP_ROUTE)
        u, a, b = ctx.saved_tensors
        if dat is None and dbt is None:
            if ut is None:
                return torch.zeros_like(u)
            return jacobi_diffuse(ut.to(u.dtype), *ctx.dual, nt).to(u.dtype)
        du = None if ut is None else _kernel_input(ut.to(u.dtype), f64, (torch.float32, torch.float16), align=1)
        da, db = (None if t is None else _kernel_param(t, a.dtype) for t in (dat, dbt))
        return _jacobi_tangent_call(L.load(), f64, u, du, a, b, da, db, nt, False)[1]

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():                      # create_graph=True: differentiable once more
            return _second_order(_JacobiFn, ctx, (g,))
        return _JacobiFn._backward(ctx, g)

    @staticmethod
    def _backward(ctx, g):
        lib = L.load()
        nt, steps, bits, f64 = ctx.cfg
        fam = "pde_jacobi_f64_" if f64 else "pde_jacobi_io_"
        if ctx.input_only is not None:
            a, b = ctx.saved_tensors
            shape, dtype, device = ctx.input_only
            B, H, W = shape
            gout, gtraj = _cotangents(g, dtype, steps, ctx.align)
            gu = torch.empty(shape, dtype=dtype, device=device)
            with torch.cuda.device(device):
                if f64:
                    io, bws = (), ()
                else:
                    io = (_io_dtype(gu),)
                    n = lib.pde_jacobi_io_backward_input_workspace_bytes(B, H, W, nt, *io)
                    ws = _workspace(n, device) if n else None
                    bws = (_ptr(ws), n)
                L.check(getattr(lib, fam + "backward_input_states")(B, H, W, nt, *io, _ptr(gout), _ptr(gtraj),
                                                                    None if steps is None else _mask128(bits), _ptr(a),
                                                                    _ptr(b), _ptr(gu), *bws, _stream()),
                        fam + "backward_input_states")
            return gu, None, None, None, None, None, None
        u, a, b = ctx.saved_tensors
        B, H, W = u.shape
        gout, gtraj = _cotangents(g, u.dtype, steps, ctx.align)
        gu, ga, gb = torch.empty_like(u), torch.empty_like(a), torch.empty_like(b)
        io = () if f64 else (_io_dtype(u),)
        with torch.cuda.device(u.device):
            ws = _workspace(getattr(lib, fam + "backward_workspace_bytes")(B, H, W, nt, *io), u.device)
            L.check(getattr(lib, fam + "backward_states")(B, H, W, nt, *io, _ptr(u), _ptr(gout), _ptr(gtraj),
                                                          None if steps is None else _mask128(bits), _ptr(a), _ptr(b),
                                                          _ptr(gu), _ptr(ga), _ptr(gb), _ptr(ws), ws.numel(), _stream()),
                    fam + "backward_states")
        return gu, _grad_as(ga, ctx.p_dtypes[0]), _grad_as(gb, ctx.p_dtypes[1]), None, None, None, None


def jacobi_diffuse(u, a_row, b_col, nt: int):
    """emotion_recognition.py:82-97 on (B,H,W): reflect-pad once, ``nt`` Jacobi updates."""
    if u.shape[0] == 0:
        return _empty_passthrough(u, a_row, b_col)
    f64 = _is_f64(u, a_row, b_col)
    if not f64:
        u = _io_in(u, a_row, b_col)
    if _fwad._current_level >= 0 and _has_tangent(u, a_row, b_col):
        # forward mode: the node is told to keep what its jvp reads
        return _apply_dual(_JacobiFn, u, a_row, b_col, int(nt), None, None, f64)
    return _JacobiFn.apply(u, a_row, b_col, int(nt), None, None, f64)


def _jacobi_tangent_call(lib, f64, u, du, a, b, da, db, nt, want_y):
    """One ``pde_jacobi_io_tangent`` / ``pde_jacobi_f64_tangent`` call (include/pdecnn_explicit_tangent.h) on kernel-ready
    tensors: (y or None, dy)."""
    B, H, W = u.shape
    y = torch.empty_like(u) if want_y else None
    dy = torch.empty_like(u)
    with torch.cuda.device(u.device):
        if f64:
            L.check(lib.pde_jacobi_f64_tangent(B, H, W, nt, _ptr(u), _ptr(du), _ptr(a), _ptr(b), _ptr(da), _ptr(db), _ptr(y),
                                               _ptr(dy), _stream()), "pde_jacobi_f64_tangent")
        else:
            io = _io_dtype(u)
            # a tiled plane with more steps than one launch takes: the launches chain through a workspace
            n = lib.pde_jacobi_io_tangent_workspace_bytes(B, H, W, nt, io)
            ws = _workspace(n, u.device) if n else None
            L.check(lib.pde_jacobi_io_tangent(B, H, W, nt, io, _ptr(u), _ptr(du), _ptr(a), _ptr(b), _ptr(da), _ptr(db),
                                              _ptr(y), _ptr(dy), _ptr(ws), n, _stream()), "pde_jacobi_io_tangent")
    return y, dy


def jacobi_diffuse_tangent(u, a_row, b_col, nt: int, *, du=None, d_a_row=None, d_b_col=None):
    """``(y, ydot)``: ``jacobi_diffuse`` and its directional derivative along the input tangent ``du`` and the tangents of
    ``a_row`` and ``b_col`` (None: zero; at least one must be given), the padded plane and its tangent advanced together
    (pde_jacobi_io_tangent: one workgroup per sample up to 64x64, the tiled kernel above; pde_jacobi_f64_tangent).  Plain
    tensors, no autograd graph.  fp32, the float16 route and float64 by the rules of ``jacobi_diffuse``; ``y`` is bit for
    bit its result."""
    dparams = (d_a_row, d_b_col)
    if du is None and all(t is None for t in dparams):
        raise ValueError("jacobi_diffuse_tangent needs du or a coefficient tangent (use jacobi_diffuse for the value alone)")
    if u.dim() != 3:
        raise L.PdeError(f"expected (B,H,W), got {tuple(u.shape)}")
    if du is not None and du.shape != u.shape:
        raise L.PdeError(f"du of shape {tuple(du.shape)} does not match u {tuple(u.shape)}")
    f64 = _is_f64(u, a_row, b_col)
    with torch.no_grad():
        if not f64:
            u = _io_in(u, a_row, b_col)
        _require_cuda(u, a_row, b_col, du, *dparams)
        if u.shape[0] == 0:
            y = u.to(torch.float64) if f64 else u.clone()
            return y, torch.zeros_like(y)
        kt = torch.float64 if f64 else torch.float32
        io_types = (torch.float32, torch.float16)
        u = _kernel_input(u.detach(), f64, io_types, align=1)
        du = None if du is None else _kernel_input(du.detach().to(u.dtype), f64, io_types, align=1)
        a, b = _kernel_param(a_row, kt), _kernel_param(b_col, kt)
        da, db = (None if t is None else _kernel_param(t, kt) for t in dparams)
        return _jacobi_tangent_call(L.load(), f64, u, du, a, b, da, db, int(nt), True)


# --------------------------------------------------------------------------- trajectories of the explicit layers
MAX_EMIT_STEPS = 128        # the emission mask of the C ABI is 128 bits


def check_steps(steps, last: int, what: str = "steps"):
    """The step selection of every ``trajectory`` / ``*_states`` call: None (every step of 1..last) or whole, strictly
    increasing 1-based step numbers within 1..last (None: no upper end).  Returns them as a list; ValueError otherwise."""
    if steps is None:
        if last is None:
            raise ValueError(f"{what} must be a sequence of step numbers")
        sel = list(range(1, int(last) + 1))
    else:
        try:
            raw = list(steps)
            sel = [int(k) for k in raw]
            exact = all(float(k) == int(k) for k in raw)
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be None or a sequence of step numbers, got {steps!r}") from None
        if not exact:
            raise ValueError(f"{what} must be whole step numbers, got {steps!r}")
    if not sel or sel[0] < 1 or (last is not None and sel[-1] > last) or any(b <= a for a, b in zip(sel, sel[1:])):
        end = "" if last is None else f" in 1..{last}"
        raise ValueError(f"{what} must be strictly increasing step numbers{end}, got {steps!r}")
    return sel


def _emit_steps(steps):
    """(steps as a tuple, the C ABI's emission mask without the last step) of a ``*_states`` call."""
    sel = tuple(check_steps(steps, None))
    if sel[-1] > MAX_EMIT_STEPS:
        raise ValueError(f"a trajectory call takes at most {MAX_EMIT_STEPS} time steps, got {sel[-1]}")
    return sel, sum(1 << (k - 1) for k in sel[:-1])


def jacobi_diffuse_states(u, a_row, b_col, steps):
    """``jacobi_diffuse`` that returns the trajectory: the state after every time step listed in ``steps`` (strictly
    increasing 1-based step numbers; ``max(steps)`` steps are run, at most 128) as ONE tensor ``(len(steps),) + u.shape``,
    out of the launches the plain call of ``max(steps)`` steps makes.  Slice ``i`` is bit for bit
    ``jacobi_diffuse(u, a_row, b_col, steps[i])`` — the reflect-padded ring keeps the input's values over the whole time
    loop, which chained one-step calls would not; with fp16 tensors it is the fp32 state rounded once while the time loop
    goes on unrounded.  Differentiable in ``u`` and both coefficient vectors for a loss on any of the returned states.
    fp32, the float16 route and float64 by the rules of ``jacobi_diffuse``."""
    sel, bits = _emit_steps(steps)
    if u.dim() != 3:
        raise L.PdeError(f"expected (B,H,W), got {tuple(u.shape)}")
    if u.shape[0] == 0:
        return torch.stack([_empty_passthrough(u, a_row, b_col)] * len(sel))
    f64 = _is_f64(u, a_row, b_col)
    if not f64:
        u = _io_in(u, a_row, b_col)
    return _JacobiFn.apply(u, a_row, b_col, sel[-1], sel, bits, f64)


def explicit5_states(u, alpha_base, channel_scaling, dt=0.01, eps=1e-6, max_coeff=0.15, relax=0.1, steps=(1,)):
    """``explicit5_step`` that returns the trajectory: the state after every step listed in ``steps`` (strictly increasing
    1-based step numbers; ``max(steps)`` steps are run, at most 128) as ONE tensor ``(len(steps),) + u.shape``, out of the
    launches the plain call of ``max(steps)`` steps makes (one for 64x64, 32x32 and 16x16 planes).  Slice ``i`` is bit for
    bit ``explicit5_step(..., num_steps=steps[i])``; with 16-bit tensors it is the fp32 state rounded once while the time
    loop goes on unrounded.  Differentiable in ``u``, ``alpha_base`` and ``channel_scaling`` for a loss on any of the
    returned states.  fp32, bf16, the float16 route and float64 by the rules of ``explicit5_step``."""
    sel, bits = _emit_steps(steps)
    if u.dim() != 4:
        raise L.PdeError(f"expected (B,C,H,W), got {tuple(u.shape)}")
    if u.shape[0] == 0:
        return torch.stack([_empty_passthrough(u, alpha_base, channel_scaling)] * len(sel))
    f64 = _is_f64(u, alpha_base, channel_scaling)
    if not f64:
        u = _io_in(u, alpha_base, channel_scaling)
    return _Explicit5Fn.apply(u, alpha_base, channel_scaling, float(dt), float(eps), float(max_coeff), float(relax),
                              sel[-1], sel, bits, f64)


# --------------------------------------------------------------------------- SVHN skip connection
class _SkipBlendFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u0, u, skip_weight):
        lib = L.load()
        _require_cuda(u0, u, skip_weight)
        if u0.shape != u.shape:
            raise L.PdeError(f"shapes differ: {tuple(u0.shape)} vs {tuple(u.shape)}")
        dt = u.dtype if u.dtype in (torch.float32, torch.bfloat16) or _is_f16(u, u0, skip_weight) else torch.float32
        a, b = _aligned(u0.to(dt).contiguous()), _aligned(u.to(dt).contiguous())
        w = skip_weight.detach().to(torch.float32).reshape(1).contiguous()
        out = torch.empty_like(b)
        with torch.cuda.device(b.device):
            L.check(lib.pde_skip_blend_forward(b.numel(), _io_dtype(b), _ptr(a), _ptr(b), _ptr(w), _ptr(out), _stream()),
                    "pde_skip_blend_forward")
        # skip_weight frozen: the backward is the split g_u0 = s g, g_u = (1 - s) g alone and reads neither u0 nor u
        ctx.input_only = None
        if _grad_route(any(ctx.needs_input_grad[:2]), ctx.needs_input_grad[2]) == "input_only":
            ctx.input_only = b.dtype
            ctx.save_for_backward(w)
        else:
            ctx.save_for_backward(a, b, w)
        ctx.in_dtypes = (u0.dtype, u.dtype, skip_weight.dtype, skip_weight.shape)
        ctx.primal_args = skip_weight
        ctx.dual = _take_dual(ctx)
        if ctx.dual:
            ctx.save_for_forward(a, b, w, skip_weight.detach())
        return out

    @staticmethod
    def jvp(ctx, u0t, ut, wt):
        return _blend_jvp(_SkipBlendFn, ctx, u0t, ut, wt)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():                      # create_graph=True: differentiable once more
            return _blend_second_order(_SkipBlendFn, ctx, g)
        return _SkipBlendFn._backward(ctx, g)

    @staticmethod
    def _backward(ctx, g):
        lib = L.load()
        if ctx.input_only is not None:
            (w,) = ctx.saved_tensors
            g = _aligned(g.to(ctx.input_only).contiguous())
            g_a, g_b = torch.empty_like(g), torch.empty_like(g)
            with torch.cuda.device(g.device):
                L.check(lib.pde_skip_blend_backward_input(g.numel(), _io_dtype(g), _ptr(g), _ptr(w), _ptr(g_a), _ptr(g_b),
                                                          _stream()), "pde_skip_blend_backward_input")
            d0, d1, _, _ = ctx.in_dtypes
            return g_a.to(d0), g_b.to(d1), None
        a, b, w = ctx.saved_tensors
        g = _aligned(g.to(b.dtype).contiguous())
        g_a, g_b = torch.empty_like(a), torch.empty_like(b)
        g_w = torch.empty(1, dtype=torch.float32, device=b.device)
        ws = _workspace(lib.pde_skip_blend_backward_workspace_bytes(b.numel()), b.device)
        with torch.cuda.device(b.device):
            L.check(lib.pde_skip_blend_backward(b.numel(), _io_dtype(b), _ptr(g), _ptr(a), _ptr(b), _ptr(w), _ptr(g_a), _ptr(g_b),
                                                _ptr(g_w), _ptr(ws), ws.numel(), _stream()), "pde_skip_blend_backward")
        d0, d1, dw, shw = ctx.in_dtypes
        return g_a.to(d0), g_b.to(d1), g_w.to(dw).reshape(shw)


def _blend_second_order(cls, ctx, g):
    """The blend is linear in (u0, u): <v0, s g> + <v1, (1 - s) g> = <skip_blend(v0, v1, w), g>.  Its ``skip_weight``
    gradient is a parameter gradient like any other: not differentiable."""
    w = ctx.primal_args

    def primal(v0, v1):
        return cls.apply(torch.zeros_like(v1) if v0 is None else v0, torch.zeros_like(v0) if v1 is None else v1, w)
    return linear_adjoint(lambda c: cls._backward(ctx, c), primal, (g,), (w,), n_diff=2)


def _blend_jvp(cls, ctx, u0t, ut, wt):
    """Forward mode of ``s u0 + (1 - s) u``, s = sigmoid(w): the blend of the tangents (the node's own forward kernel)
    plus ``s (1 - s) wt (u0 - u)``."""
    if not ctx.dual:
        raise NotImplementedError(_NO_JVP_ROUTE)
    a, b, w, w_in = ctx.saved_tensors                      # w_in: as the caller gave it (it takes part in the type routing)
    out = None
    if u0t is not None or ut is not None:
        out = cls.apply(torch.zeros_like(a) if u0t is None else u0t.to(a.dtype),
                        torch.zeros_like(b) if ut is None else ut.to(b.dtype), w_in)
    if wt is not None:
        s = torch.sigmoid(w)
        t = ((s * (1 - s) * wt.reshape(1).to(w.dtype)) * (a.to(w.dtype) - b.to(w.dtype))).to(b.dtype)
        out = t if out is None else out + t
    return torch.zeros_like(b) if out is None else out


def skip_blend(u0, u, skip_weight):
    """``sigmoid(skip_weight) * u0 + (1 - sigmoid(skip_weight)) * u`` — SVHN.py:73-74, one pass."""
    f64 = _is_f64(u0, u, skip_weight)
    if u.numel() == 0:
        if f64:
            u0, u, skip_weight = u0.double(), u.double(), skip_weight.double()
        s = torch.sigmoid(skip_weight)
        return s * u0 + (1 - s) * u
    cls = _SkipBlendF64Fn if f64 else _SkipBlendFn
    if _fwad._current_level >= 0 and _has_tangent(u0, u, skip_weight):
        return _apply_dual(cls, u0, u, skip_weight)
    return cls.apply(u0, u, skip_weight)


# --------------------------------------------------------------------------- float64
# A call takes the float64 path when its input or any floating parameter is float64 (torch's type promotion, which the
# reference's ops follow): the output is float64 and every gradient comes back in its own tensor's dtype.  The layer
# families' nodes (_AdiFn, _Explicit5Fn, _JacobiFn) take it as their ``f64`` switch; the functions below run the other
# pde_*_f64_* entry points (double arithmetic throughout).  There is no float64 host-extension path.
def _is_f64(*ts) -> bool:
    return any(isinstance(t, torch.Tensor) and t.dtype == torch.float64 for t in ts)


def _d64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float64).contiguous()


def _f64_ckpt_bits(ckpt, num_sweeps: int) -> int:
    """The backward's checkpoint mask in float64: an int is honoured; "auto" / "lagged" keep the state after every sweep
    (nothing is rebuilt, so no rounding is amplified: the plan needs no coefficient maxima)."""
    if isinstance(ckpt, int) and not isinstance(ckpt, bool):
        return int(ckpt)
    return (1 << max(num_sweeps - 1, 0)) - 1


class _MixF64Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, M):
        lib = L.load()
        _require_cuda(u, M)
        B, Cc = u.shape[0], u.shape[1]
        HW = u[0, 0].numel()
        u_in = u
        u = u.to(torch.float64).contiguous()
        Md = _d64(M)
        out = torch.empty_like(u)
        with torch.cuda.device(u.device):
            L.check(lib.pde_channel_mix_f64_forward(B, Cc, HW, _ptr(u), _ptr(Md), _ptr(out), _stream()),
                    "pde_channel_mix_f64_forward")
        ctx.input_only = None
        if _grad_route(ctx.needs_input_grad[0], ctx.needs_input_grad[1]) == "input_only":
            ctx.input_only = (B, Cc, HW)
            ctx.save_for_backward(Md)
        else:
            ctx.save_for_backward(u, Md)
        ctx.m_dtype = M.dtype
        ctx.primal_args = (u_in if ctx.input_only is None else None, M)
        ctx.dual = _take_dual(ctx)
        if ctx.dual:
            ctx.save_for_forward(u, M.detach())
        return out

    @staticmethod
    def jvp(ctx, ut, Mt):
        return _mix_jvp(_MixF64Fn, ctx, ut, Mt)

    @staticmethod
    def backward(ctx, gout):
        if torch.is_grad_enabled():                      # create_graph=True: differentiable once more
            return _mix_second_order(_MixF64Fn, ctx, gout)
        return _MixF64Fn._backward(ctx, gout)

    @staticmethod
    def _backward(ctx, gout):
        lib = L.load()
        if ctx.input_only is not None:
            (Md,) = ctx.saved_tensors
            B, Cc, HW = ctx.input_only
            gout = gout.to(torch.float64).contiguous()
            gu = torch.empty_like(gout)
            with torch.cuda.device(gout.device):
                L.check(lib.pde_channel_mix_f64_backward_input(B, Cc, HW, _ptr(gout), _ptr(Md), _ptr(gu), _stream()),
                        "pde_channel_mix_f64_backward_input")
            return gu, None
        u, Md = ctx.saved_tensors
        B, Cc = u.shape[0], u.shape[1]
        HW = u[0, 0].numel()
        gout = gout.to(torch.float64).contiguous()
        gu, gM = torch.empty_like(u), torch.empty_like(Md)
        ws = _workspace(lib.pde_channel_mix_f64_backward_workspace_bytes(B, Cc, HW), u.device)
        with torch.cuda.device(u.device):
            L.check(lib.pde_channel_mix_f64_backward(B, Cc, HW, _ptr(u), _ptr(gout), _ptr(Md), _ptr(gu), _ptr(gM), _ptr(ws),
                                                     ws.numel(), _stream()), "pde_channel_mix_f64_backward")
        return gu, gM.to(ctx.m_dtype)


class _SkipBlendF64Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u0, u, skip_weight):
        lib = L.load()
        _require_cuda(u0, u, skip_weight)
        if u0.shape != u.shape:
            raise L.PdeError(f"shapes differ: {tuple(u0.shape)} vs {tuple(u.shape)}")
        a, b = u0.to(torch.float64).contiguous(), u.to(torch.float64).contiguous()
        w = _d64(skip_weight).reshape(1)
        out = torch.empty_like(b)
        with torch.cuda.device(b.device):
            L.check(lib.pde_skip_blend_f64_forward(b.numel(), _ptr(a), _ptr(b), _ptr(w), _ptr(out), _stream()),
                    "pde_skip_blend_f64_forward")
        ctx.input_only = False
        if _grad_route(any(ctx.needs_input_grad[:2]), ctx.needs_input_grad[2]) == "input_only":
            ctx.input_only = True
            ctx.save_for_backward(w)
        else:
            ctx.save_for_backward(a, b, w)
        ctx.in_meta = (u0.dtype, u.dtype, skip_weight.dtype, skip_weight.shape)
        ctx.primal_args = skip_weight
        ctx.dual = _take_dual(ctx)
        if ctx.dual:
            ctx.save_for_forward(a, b, w, skip_weight.detach())
        return out

    @staticmethod
    def jvp(ctx, u0t, ut, wt):
        return _blend_jvp(_SkipBlendF64Fn, ctx, u0t, ut, wt)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():                      # create_graph=True: differentiable once more
            return _blend_second_order(_SkipBlendF64Fn, ctx, g)
        return _SkipBlendF64Fn._backward(ctx, g)

    @staticmethod
    def _backward(ctx, g):
        lib = L.load()
        if ctx.input_only:
            (w,) = ctx.saved_tensors
            g = g.to(torch.float64).contiguous()
            g_a, g_b = torch.empty_like(g), torch.empty_like(g)
            with torch.cuda.device(g.device):
                L.check(lib.pde_skip_blend_f64_backward_input(g.numel(), _ptr(g), _ptr(w), _ptr(g_a), _ptr(g_b), _stream()),
                        "pde_skip_blend_f64_backward_input")
            d0, d1, _, _ = ctx.in_meta
            return g_a.to(d0), g_b.to(d1), None
        a, b, w = ctx.saved_tensors
        g = g.to(torch.float64).contiguous()
        g_a, g_b = torch.empty_like(a), torch.empty_like(b)
        g_w = torch.empty(1, dtype=torch.float64, device=b.device)
        ws = _workspace(lib.pde_skip_blend_f64_backward_workspace_bytes(b.numel()), b.device)
        with torch.cuda.device(b.device):
            L.check(lib.pde_skip_blend_f64_backward(b.numel(), _ptr(g), _ptr(a), _ptr(b), _ptr(w), _ptr(g_a), _ptr(g_b),
                                                    _ptr(g_w), _ptr(ws), ws.numel(), _stream()), "pde_skip_blend_f64_backward")
        d0, d1, dw, shw = ctx.in_meta
        return g_a.to(d0), g_b.to(d1), g_w.to(dw).reshape(shw)


# --------------------------------------------------------------------------- timing
def timing_enable(on: bool = True):
    L.check(L.load().pde_timing_enable(int(on)), "pde_timing_enable")


def timing_read() -> Tuple[float, int, float, int]:
    """(sum of forward-kernel ms, launches, sum of backward-kernel ms, launches) since enable."""
    f, b = C.c_double(), C.c_double()
    nf, nb = C.c_int64(), C.c_int64()
    L.check(L.load().pde_timing_read(C.byref(f), C.byref(nf), C.byref(b), C.byref(nb)), "pde_timing_read")
    return f.value, nf.value, b.value, nb.value
