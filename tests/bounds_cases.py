"""The case table of tests/test_gpu_bounds.py: every entry point of include/pdecnn.h that writes device memory, at the
smallest shapes at which its stores go ragged, with the role of every pointer it takes.

A case is a family, a dict of dimensions and (optionally) an environment switch.  Its family's builder turns it into a
sequence of C ABI calls over named buffers; the builder talks to a context, never to torch.cuda, so the same code

  * runs on the CPU with a recording context (``SpecCtx``: shapes, roles and workspace sizes only — the size queries are
    host functions), which is what tests/test_bounds_cases.py checks against the header;
  * runs on the GPU twice, on ordinary tensors and inside a ``guard_util.Arena`` (tests/test_gpu_bounds.py).

Roles of a buffer:
    in      read only; its guards are checked
    out     the header says it is overwritten: pre-filled with 0xFF, every element must have been stored
    inout   holds values on entry that the call updates (running statistics)
    carry   carried between the calls of the sequence and poisoned only before the first of them (the per-step workspace,
            the partial sums of a *_steps backward), or an output the header says is written in part (``states`` of the
            one-launch wide forward: ``written_slots`` names the slices that are, and those are held like an output)
    ws      scratch of exactly the queried size, 0xFF on entry

Every buffer also carries the alignment the header's "Alignment" section asks of the pointer it is bound to (``ctx.aligns``,
bytes): 16 by default and for every workspace, the element's own for the names of ``ELEMENT_ALIGNED`` and, when the builder
says that its calls are served by element-wise kernels (``ctx.vec_elems = 1``), for every other tensor too; ``vec_elems = 4``
is the explicit layer on float4 rows (16-bit tensors then begin on 8 bytes).  tests/test_bounds_cases.py holds the table to
the header; tests/test_alignment_refusal.py and tests/test_gpu_alignment.py run it.

Arguments of a call are looked up by the parameter NAMES the header declares, so a builder only says where a name differs
from the buffer it is bound to ({"workspace": "bws"}); kappa_max_host and kappa_event are NULL in every case."""
import ctypes as C
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IO = {"f32": (0, torch.float32), "bf16": (1, torch.bfloat16), "f16": (3, torch.float16), "f64": (2, torch.float64)}
IO3 = ("f32", "bf16", "f16")
NULL_BY_DEFAULT = ("kappa_max_host", "kappa_event")

DEFAULT_ALIGN = 16
#: parameters (and PdeSmallLayer fields) the kernels read and write one element at a time: the ELEMENT-ALIGNED list of pdecnn.h
ELEMENT_ALIGNED = frozenset((
    "kappa_max", "kappa_max_host", "skip_weight", "g_skip_weight", "weight_ptr", "g_weight", "plane_sums", "weights", "gates", "dots",
    "gamma", "beta", "mean", "invstd", "running_mean", "running_var", "ggamma", "gbeta", "argmax", "bn_weight", "bn_bias",
    "g_bn_weight", "g_bn_bias", "a_row", "b_col", "g_a_row", "g_b_col", "channel_scaling", "g_channel_scaling"))


def header_element_aligned():
    """The names behind ``ELEMENT-ALIGNED:`` in the Alignment section of pdecnn.h."""
    src = open(os.path.join(ROOT, "include", "pdecnn.h")).read()
    m = re.search(r"ELEMENT-ALIGNED:(.*?)\n \*\s+\(", src, flags=re.S)
    return frozenset(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", m.group(1).replace("*", " ")))


#: function prefix -> names that are element-aligned in those functions only (the ELEMENT-ALIGNED IN lines of pdecnn.h)
ELEMENT_ALIGNED_IN = {"pde_explicit5_": frozenset(("alpha_base", "g_alpha_base")), "pde_bn_pool_": frozenset(("out", "gout"))}


def header_element_aligned_in():
    src = open(os.path.join(ROOT, "include", "pdecnn.h")).read()
    return {m.group(1): frozenset(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", m.group(2).split("(")[0]))
            for m in re.finditer(r"ELEMENT-ALIGNED IN (pde_[a-z0-9_]+): ([^\n]*)", src)}


def param_of(buffer):
    """The parameter (or struct field) a buffer is named after: per-layer and per-slot suffixes dropped (gates_0, kappa_max_2)."""
    return re.sub(r"_\d+$", "", buffer)


def fused_line_length(n):
    return 8 <= n <= 32 and n % 4 == 0


# ---------------------------------------------------------------------------------------------------- the header
def header_functions():
    """{name: [(name of the parameter, is a pointer, its pointee is const)]} for every function pdecnn.h declares."""
    src = open(os.path.join(ROOT, "include", "pdecnn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(pde_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            if p in ("", "void"):
                continue
            name = re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(\[\d*\])?$", p).group(1)
            params.append((name, "*" in p or "[" in p, p.startswith("const ")))
        out[m.group(1)] = params
    return out


def writing_functions():
    """The functions the table must cover: a pointer to non-const memory, or a workspace."""
    return sorted(f for f, ps in header_functions().items()
                  if any((ptr and not const) or "workspace" in name for name, ptr, const in ps))


#: functions of ``writing_functions()`` that no case calls, and why
EXCLUDED = {
    "pde_sym_layer_path": "writes three host integers (split, waves, row_blocks); no device memory",
    "pde_channel_mix_splits": "writes one host integer (chunks); no device memory",
    "pde_timing_read": "writes four host scalars; no device memory",
}

#: environment switches a case may name; each must be a getenv string of csrc/
SWITCHES = ("PDE_ASM_FWD=1", "PDE_ASM_BWD=0", "PDE_FWD_SCHED=0", "PDE_WIDE=0", "PDE_MIX_UNFUSED=1", "PDE_MIX_NO_SPLIT=1",
            "PDE_MIX_NO_BF16_MFMA=1", "PDE_RH_NO_STRIP32=1", "PDE_RH_NO_SPLIT=1")


# ---------------------------------------------------------------------------------------------------- contexts
class SpecCtx:
    """Records what a builder declares; allocates no output.  ``ptr`` is 0 for everything."""
    device = "cpu"

    def __init__(self):
        self.roles, self.shapes, self.dtypes, self.values, self.t = {}, {}, {}, {}, {}
        self.written_slots = {}                  # carry buffer written in part -> the slices (first axis) the header says are written
        self.aligns = {}                         # buffer -> bytes its base must be a multiple of (pdecnn.h, "Alignment")
        self.vec_elems = None                    # None: the default rule; k: tensors of this case begin on k elements (at most 16 bytes)
        self.also_element = frozenset()          # names that are element-aligned in this case's functions only

    def _align_of(self, name, role, dtype, param):
        item = torch.empty((), dtype=dtype).element_size()
        if dtype == torch.uint8 and role in ("ws", "carry"):
            return DEFAULT_ALIGN                                     # every workspace
        if (param or param_of(name)) in ELEMENT_ALIGNED or (param or param_of(name)) in self.also_element:
            return item
        return DEFAULT_ALIGN if self.vec_elems is None else min(DEFAULT_ALIGN, self.vec_elems * item)

    def _add(self, name, role, shape, dtype, fill=None, param=None):
        assert name not in self.roles and name not in self.values, f"{name} declared twice"
        self.roles[name], self.shapes[name], self.dtypes[name] = role, tuple(int(s) for s in shape), dtype
        self.aligns[name] = self._align_of(name, role, dtype, param)
        self.t[name] = self._alloc(name, role, self.shapes[name], dtype, fill)
        return self.t[name]

    def _alloc(self, name, role, shape, dtype, fill):
        return None

    def inp(self, name, t, dtype=None):
        t = t.to(dtype) if dtype is not None else t
        return self._add(name, "in", t.shape, t.dtype, t)

    def inout(self, name, t):
        return self._add(name, "inout", t.shape, t.dtype, t)

    def out(self, name, shape, dtype, param=None):
        """``param``: the parameter whose alignment rule applies, where the buffer is not named after it."""
        return self._add(name, "out", shape, dtype, param=param)

    def carry(self, name, shape, dtype):
        return self._add(name, "carry", shape, dtype)

    def ws(self, name, nbytes, role="ws"):
        self._add(name, role, (int(nbytes),), torch.uint8)
        return int(nbytes)

    def val(self, name, v):
        assert name not in self.roles and name not in self.values, f"{name} declared twice"
        self.values[name] = v
        return v

    def ptr(self, name, byte_offset=0):
        return 0

    def stream(self):
        return None

    def nbytes(self, name):
        n = torch.empty((), dtype=self.dtypes[name]).element_size()
        for s in self.shapes[name]:
            n *= s
        return n


def call_args(ctx, params, amap):
    """The ctypes arguments of one call: every parameter the header declares, looked up by its name — in ``amap`` first
    (a buffer or value name, a literal, or None for NULL), then among the context's buffers and values."""
    args = []
    for name, is_ptr, const in params:
        if name in amap:
            v = amap[name]
        elif name == "stream":
            args.append(ctx.stream())
            continue
        elif name in NULL_BY_DEFAULT:
            v = None
        else:
            v = name
        if isinstance(v, str):
            if v in ctx.roles:
                args.append(C.c_void_p(ctx.ptr(v)))
                continue
            v = ctx.values[v]                        # KeyError: the builder left a parameter of the header unbound
        args.append(C.byref(v) if isinstance(v, C.Structure) else v)
    return args


def bound_buffers(ctx, params, amap):
    """[(parameter, buffer, pointee is const)] for the pointer parameters of a call that are bound to a buffer."""
    out = []
    for name, is_ptr, const in params:
        v = amap.get(name, name)
        if is_ptr and isinstance(v, str) and v in ctx.roles:
            out.append((name, v, const))
    return out


def lib():
    from cnn_with_pde_amd import _lib
    return _lib.load()


def _gen(p, salt=0):
    return torch.Generator().manual_seed(1234567 + 7919 * salt + sum(ord(c) for c in repr(sorted(p.items(), key=str))))


def mask128(bits):
    return (C.c_uint64 * 2)(bits & (2 ** 64 - 1), bits >> 64)


def popcount(bits):
    return bin(bits).count("1")


# ---------------------------------------------------------------------------------------------------- ADI, whole schedule
def _sweeps(p):
    from cnn_with_pde_amd.functional import adi_schedule
    return [s for st in adi_schedule(p.get("dt", 0.02), 1.0, 1.0, p["steps"], p.get("split", "strang")) for s in st]


def _adi_desc(p):
    from cnn_with_pde_amd import _lib as L
    from cnn_with_pde_amd.functional import _fill_desc
    f64, rect = p["io"] == "f64", p.get("rect", False)
    cls = {(False, False): L.PdeAdiDesc, (False, True): L.PdeAdiDescF64, (True, False): L.PdeAdiRectDesc,
           (True, True): L.PdeAdiRectDescF64}[rect, f64]
    return _fill_desc(cls, p["B"], p["C"], p["H"], p["W"], IO[p["io"]][0], _sweeps(p), False, 10.0, 1e-6)


def _adi_params(ctx, p, g, suffix=""):
    """alpha / beta (C,H,W): base 1 +- 15 %, slope 0.5 N(0,1); with ``clampmove`` base + slope t crosses the clamp floor
    inside the time window at some points of every channel (the factor kernel then flags the channel and the masked body
    owns it: tests/test_gpu_asm_bwd.py::test_channels_with_moving_clamp_masks_share_the_call)."""
    pt = torch.float64 if p["io"] == "f64" else torch.float32
    shape = (p["C"], p["H"], p["W"])
    T = p["steps"] * p.get("dt", 0.02)
    low = torch.zeros(shape, dtype=torch.bool)
    for k in ("alpha_base", "beta_base"):
        v = 1 + 0.15 * torch.randn(shape, generator=g)
        if p.get("clampmove"):
            low = torch.rand(shape, generator=g) < 0.25
            v = torch.where(low, 0.5 * T * torch.rand(shape, generator=g), v)
        ctx.inp(k + suffix, v, pt)
        s = 0.5 * torch.randn(shape, generator=g)
        ctx.inp(k.replace("base", "slope") + suffix, torch.where(low, -torch.ones(shape), s), pt)


def _adi_fam(p):
    return "pde_adi_" + ("rect_" if p.get("rect") else "") + ("f64_" if p["io"] == "f64" else "")


def build_adi(ctx, p):
    l = lib()
    g = _gen(p)
    dt = IO[p["io"]][1]
    kt = torch.float64 if p["io"] == "f64" else torch.float32
    d = ctx.val("d", _adi_desc(p))
    shape = (p["B"], p["C"], p["H"], p["W"])
    S, fam = d.num_sweeps, _adi_fam(p)
    if fam != "pde_adi_" or not fused_line_length(p["H"]):       # rectangles, float64, the any-size path: element-wise kernels
        ctx.vec_elems = 1
    ckpt, emit = p.get("ckpt", 0), p.get("emit", 0)
    ctx.inp("u", torch.randn(shape, generator=g), dt)
    ctx.inp("gy", torch.randn(shape, generator=g), dt)
    _adi_params(ctx, p, g)
    ctx.out("y", shape, dt)
    ctx.out("gu", shape, dt)
    ctx.out("kappa_max", (S,), kt)
    for k in ("g_alpha_base", "g_beta_base", "g_alpha_slope", "g_beta_slope"):
        ctx.out(k, shape[1:], kt)
    ctx.val("ckpt_mask", mask128(ckpt))
    nf = ctx.ws("fws", getattr(l, fam + "forward_workspace_bytes")(C.byref(d)))
    nb = ctx.ws("bws", getattr(l, fam + "backward_workspace_bytes")(C.byref(d), popcount(ckpt)))
    assert nf > 0 and nb > 0, (nf, nb)
    st = "_states" if emit else ""
    if emit:
        ctx.val("emit_mask", mask128(emit))
        ctx.out("states", (popcount(emit),) + shape, dt)
        ctx.inp("gstates", torch.randn((popcount(emit),) + shape, generator=g), dt)
    calls = [(fam + "forward" + st, {"workspace": "fws", "workspace_bytes": nf}),
             (fam + "backward" + st, {"fwd_workspace": "fws" if p.get("reuse", True) else None, "workspace": "bws",
                                      "workspace_bytes": nb})]
    if fam != "pde_adi_f64_":                          # the square float64 family has no kappa_max entry point
        ctx.out("kappa2", (S,), kt, param="kappa_max")
        calls.append((fam + "kappa_max", {"kappa_max": "kappa2"}))
    expect = []
    if "fwd_kernel" in p:
        expect.append(("pde_adi_forward_kernel", (C.byref(d),), p["fwd_kernel"]))
    if "bwd_kernel" in p:
        expect.append(("pde_adi_backward_kernel", (C.byref(d), popcount(ckpt)), p["bwd_kernel"]))
    return calls, expect


# ---------------------------------------------------------------------------------------------------- ADI per step
def build_steps(ctx, p):
    l = lib()
    g = _gen(p)
    dt = IO[p["io"]][1]
    d = ctx.val("d", _adi_desc(p))
    sps, K = 3, p["steps"]
    shape = (p["B"], p["C"], p["H"], p["W"])
    ckpt = p.get("ckpt", 0)
    ctx.val("sweeps_per_step", sps)
    ctx.inp("x0", torch.randn(shape, generator=g), dt)
    ctx.inp("gK", torch.randn(shape, generator=g), dt)
    _adi_params(ctx, p, g)
    ctx.out("kappa_max", (d.num_sweeps,), torch.float32)
    ctx.val("ckpt_mask", mask128(ckpt))
    ns = ctx.ws("sws", l.pde_adi_steps_workspace_bytes(C.byref(d), sps), "carry")
    nb = ctx.ws("bws", l.pde_adi_backward_step_workspace_bytes(C.byref(d), sps, popcount(ckpt)), "carry")
    assert ns > 0 and nb > 0
    for k in range(K):
        ctx.out(f"x{k + 1}", shape, dt)
        ctx.out(f"g{k}", shape, dt)
    for k in ("g_alpha_base", "g_beta_base", "g_alpha_slope", "g_beta_slope"):
        ctx.out(k, shape[1:], torch.float32)
    calls = [("pde_adi_factor_steps", {"steps_workspace": "sws", "workspace_bytes": ns})]
    for k in range(K):
        calls.append(("pde_adi_forward_step", {"step": k, "u": f"x{k}", "y": f"x{k + 1}", "steps_workspace": "sws"}))
    for k in reversed(range(K)):
        calls.append(("pde_adi_backward_step", {"step": k, "gy": f"g{k + 1}" if k + 1 < K else "gK", "y": f"x{k + 1}",
                                                "u": f"x{k}", "gu": f"g{k}", "steps_workspace": "sws", "workspace": "bws",
                                                "workspace_bytes": nb, "accumulate": 0 if k == K - 1 else 1}))
    calls.append(("pde_adi_param_grads", {"steps_workspace": "sws", "workspace": "bws"}))
    return calls, []


# ---------------------------------------------------------------------------------------------------- ADI, C <= 4, one launch
def _matrix(Cc, g):
    return torch.eye(Cc) + 0.2 * torch.randn(Cc, Cc, generator=g)


def build_small(ctx, p):
    l = lib()
    g = _gen(p)
    dt = IO[p["io"]][1]
    d = ctx.val("d", _adi_desc(p))
    sps = 3 if p.get("split", "strang") == "strang" else 2
    K = p["steps"]
    shape = (p["B"], p["C"], p["H"], p["W"])
    ckpt, emit, skip = p.get("ckpt", 0), p.get("emit", 0), p.get("skip", False)
    assert l.pde_adi_small_supported(C.byref(d), sps) == 1
    ctx.val("sweeps_per_step", sps)
    ctx.val("mode", p["mode"])
    ctx.inp("u", torch.randn(shape, generator=g), dt)
    ctx.inp("gy", torch.randn(shape, generator=g), dt)
    ctx.inp("M", _matrix(p["C"], g))
    _adi_params(ctx, p, g)
    ctx.out("y", shape, dt)
    ctx.out("states", (K,) + shape, dt)
    ctx.out("gu", shape, dt)
    ctx.out("kappa_max", (d.num_sweeps,), torch.float32)
    for k in ("g_alpha_base", "g_beta_base", "g_alpha_slope", "g_beta_slope"):
        ctx.out(k, shape[1:], torch.float32)
    ctx.out("gM", (p["C"], p["C"]), torch.float32)
    ctx.val("ckpt_mask", mask128(ckpt))
    ns = ctx.ws("sws", l.pde_adi_steps_workspace_bytes(C.byref(d), sps), "carry")
    nb = ctx.ws("bws", l.pde_adi_small_backward_workspace_bytes(C.byref(d), sps, popcount(ckpt)))
    assert ns > 0 and nb > 0
    fa = {"steps_workspace": "sws", "workspace_bytes": ns}
    ba = {"steps_workspace": "sws", "workspace": "bws", "workspace_bytes": nb}
    if emit:
        ctx.val("emit_mask", mask128(emit))
        ctx.out("traj", (popcount(emit),) + shape, dt)
        ctx.inp("gtraj", torch.randn((popcount(emit),) + shape, generator=g), dt)
        return [("pde_adi_small_forward_states", fa), ("pde_adi_small_backward_states", ba)], []
    if skip:
        ctx.inp("skip_weight", torch.tensor([0.3]))
        ctx.out("g_skip_weight", (1,), torch.float32)
    else:
        fa["skip_weight"] = ba["skip_weight"] = ba["g_skip_weight"] = None
    return [("pde_adi_small_forward", fa), ("pde_adi_small_backward", ba)], []


# ---------------------------------------------------------------------------------------------------- ADI, wide layers
def build_mixed(ctx, p):
    l = lib()
    g = _gen(p)
    dt = IO[p["io"]][1]
    d = ctx.val("d", _adi_desc(p))
    sps, K = 3, p["steps"]
    shape = (p["B"], p["C"], p["H"], p["W"])
    ckpt = p.get("ckpt", 0)
    one = l.pde_adi_mixed_one_launch(C.byref(d), sps)
    ctx.val("sweeps_per_step", sps)
    ctx.val("mode", p["mode"])
    ctx.inp("u", torch.randn(shape, generator=g), dt)
    ctx.inp("gy", torch.randn(shape, generator=g), dt)
    ctx.inp("M", torch.eye(p["C"]) + 0.3 / p["C"] ** 0.5 * torch.randn(p["C"], p["C"], generator=g))
    _adi_params(ctx, p, g)
    ctx.out("y", shape, dt)
    # the one-launch forward writes only the sweep output of every step (pdecnn.h): part of `states` stays as it was
    (ctx.carry if one else ctx.out)("states", (2 * K - 1,) + shape, dt)
    if one:                                               # states[2k+1] (mode 1) / states[2k] (mode 2); states[2K-1] is `y` here
        ctx.written_slots["states"] = [s for s in range(2 * K - 1) if s % 2 == (1 if p["mode"] == 1 else 0)]
    ctx.out("gu", shape, dt)
    ctx.out("kappa_max", (d.num_sweeps,), torch.float32)
    for k in ("g_alpha_base", "g_beta_base", "g_alpha_slope", "g_beta_slope"):
        ctx.out(k, shape[1:], torch.float32)
    ctx.out("gM", (p["C"], p["C"]), torch.float32)
    ctx.val("ckpt_mask", mask128(ckpt))
    ns = ctx.ws("sws", l.pde_adi_steps_workspace_bytes(C.byref(d), sps), "carry")
    nb = ctx.ws("bws", l.pde_adi_mixed_backward_workspace_bytes(C.byref(d), sps, popcount(ckpt)))
    assert ns > 0 and nb > 0
    calls = [("pde_adi_mixed_forward", {"steps_workspace": "sws", "workspace_bytes": ns}),
             ("pde_adi_mixed_backward", {"steps_workspace": "sws", "workspace": "bws", "workspace_bytes": nb})]
    return calls, [("pde_adi_mixed_one_launch", (C.byref(d), sps), p["one_launch"])]


# ---------------------------------------------------------------------------------------------------- shared-input group
MULTI_LAYERS = ((0.02, 1), (0.04, 3), (0.05, 2))        # dt, steps of the three layers (cifar10.py:272-274 in small)


def build_multi(ctx, p):
    from cnn_with_pde_amd import _lib as L
    l = lib()
    g = _gen(p)
    dt = IO[p["io"]][1]
    shape = (p["B"], p["C"], p["H"], p["W"])
    nl, sps = len(MULTI_LAYERS), 3
    ctx.inp("u", torch.randn(shape, generator=g), dt)
    ctx.inp("gy", torch.randn(shape, generator=g), dt)
    ctx.inp("weights", torch.softmax(torch.randn(nl, generator=g), 0))
    ctx.out("out", shape, dt)
    ctx.out("gu", shape, dt)
    arr = (L.PdeSmallLayer * nl)()
    keep = []
    for i, (ldt, steps) in enumerate(MULTI_LAYERS):
        q = dict(p, dt=ldt, steps=steps)
        d = _adi_desc(q)
        keep.append((d, mask128(0)))
        s = f"_{i}"
        ctx.inp("M" + s, _matrix(p["C"], g))
        _adi_params(ctx, q, g, s)
        ctx.out("states" + s, (steps,) + shape, dt)
        ctx.out("plane_sums" + s, shape[:2], torch.float32)
        ctx.out("kappa_max" + s, (d.num_sweeps,), torch.float32)
        ctx.inp("gys" + s, torch.randn(shape, generator=g), dt)
        ctx.inp("g_plane_sums" + s, torch.randn(shape[:2], generator=g))
        for k in ("g_alpha_base", "g_beta_base", "g_alpha_slope", "g_beta_slope"):
            ctx.out(k + s, shape[1:], torch.float32)
        ctx.out("gM" + s, (p["C"], p["C"]), torch.float32)
        ctx.out("g_weight" + s, (1,), torch.float32)
        ns = ctx.ws("sws" + s, l.pde_adi_steps_workspace_bytes(C.byref(d), sps), "carry")
        nb = ctx.ws("bws" + s, l.pde_adi_small_backward_workspace_bytes(C.byref(d), sps, 0))
        assert ns > 0 and nb > 0
        a = arr[i]
        a.desc, a.sweeps_per_step, a.mode = C.pointer(d), sps, 1
        for k in ("M", "alpha_base", "beta_base", "alpha_slope", "beta_slope", "states", "plane_sums", "kappa_max", "gys",
                  "g_plane_sums", "g_alpha_base", "g_beta_base", "g_alpha_slope", "g_beta_slope", "gM", "g_weight"):
            setattr(a, k, ctx.ptr(k + s) or None)
        a.weight, a.weight_ptr = 0.0, (ctx.ptr("weights", 4 * i) or None)
        a.steps_workspace, a.steps_workspace_bytes = ctx.ptr("sws" + s) or None, ns
        a.workspace, a.workspace_bytes = ctx.ptr("bws" + s) or None, nb
        a.ckpt_mask = keep[-1][1]
    ctx.val("num_layers", nl)
    ctx.val("layers", arr)
    ctx.val("_keep", keep)
    return [("pde_adi_multi_forward", {}), ("pde_adi_multi_backward", {})], []


# ---------------------------------------------------------------------------------------------------- channel operator
MIX_PATH = {"scalar": 0, "mfma32": 1, "mfma16": 2, "split3": 3, "fused": 4}


def build_mix(ctx, p):
    l = lib()
    g = _gen(p)
    B, Cc, HW, f64 = p["B"], p["C"], p["HW"], p["io"] == "f64"
    code, dt = IO[p["io"]]
    pt = torch.float64 if f64 else torch.float32
    if f64:
        ctx.vec_elems = 1
    for k in ("B", "C", "HW"):
        ctx.val(k, p[k])
    ctx.val("io_dtype", code)
    ctx.inp("u", torch.randn(B, Cc, HW, generator=g), dt)
    ctx.inp("gout", torch.randn(B, Cc, HW, generator=g), dt)
    M = torch.randn(Cc, Cc, generator=g) / Cc ** 0.5
    ctx.inp("M", M.half().float() if p["io"] == "f16" else M, pt)      # the float16 route expects fp16 values in M
    ctx.out("out", (B, Cc, HW), dt)
    ctx.out("gu", (B, Cc, HW), dt)
    ctx.out("gM", (Cc, Cc), pt)
    ctx.out("gu2", (B, Cc, HW), dt)
    ctx.out("gu3", (B, Cc, HW), dt)
    ctx.out("gM2", (Cc, Cc), pt)
    f = "pde_channel_mix_f64_" if f64 else "pde_channel_mix_"
    n = getattr(l, f + "backward_workspace_bytes")(B, Cc, HW)
    assert n > 0
    ctx.ws("ws", n)
    ctx.ws("acc", n, "carry")
    w = {"workspace": "ws", "workspace_bytes": n}
    a = {"workspace": "acc", "workspace_bytes": n}
    calls = [(f + "forward", {}), (f + "backward", w),
             # gM spread over two calls that share `acc`: the first starts the partial sums, the second adds and reduces
             (f + "backward_steps", dict(a, gu="gu2", gM=None, accumulate=0, finalize=0)),
             (f + "backward_steps", dict(a, gu="gu3", gM="gM2", accumulate=1, finalize=1))]
    expect = []
    if not f64:
        expect = [("pde_channel_mix_path", (B, Cc, HW, code, 0), MIX_PATH[p["fwd_path"]]),
                  ("pde_channel_mix_path", (B, Cc, HW, code, 1), MIX_PATH[p["bwd_path"]])]
    return calls, expect


def build_blend(ctx, p):
    l = lib()
    g = _gen(p)
    n, f64 = p["n"], p["io"] == "f64"
    code, dt = IO[p["io"]]
    pt = torch.float64 if f64 else torch.float32
    if f64:
        ctx.vec_elems = 1
    ctx.val("n", n)
    ctx.val("io_dtype", code)
    ctx.inp("u0", torch.randn(n, generator=g), dt)
    ctx.inp("u", torch.randn(n, generator=g), dt)
    ctx.inp("g", torch.randn(n, generator=g), dt)
    ctx.inp("skip_weight", torch.tensor([0.4]), pt)
    ctx.out("out", (n,), dt)
    ctx.out("g_u0", (n,), dt)
    ctx.out("g_u", (n,), dt)
    ctx.out("g_skip_weight", (1,), pt)
    f = "pde_skip_blend_f64_" if f64 else "pde_skip_blend_"
    nb = ctx.ws("ws", getattr(l, f + "backward_workspace_bytes")(n))
    assert nb > 0
    return [(f + "forward", {}), (f + "backward", {"workspace": "ws", "workspace_bytes": nb})], []


def build_gate(ctx, p):
    g = _gen(p)
    Lr, B, Cc, (H, W) = p["L"], p["B"], p["C"], p["hw"]
    code, dt = IO[p["io"]]
    for k, v in (("L", Lr), ("B", B), ("C", Cc), ("HW", H * W), ("io_dtype", code)):
        ctx.val(k, v)
    ctx.inp("g", torch.randn(B, Cc, H * W, generator=g), dt)
    ctx.inp("weights", torch.softmax(torch.randn(Lr, generator=g), 0))
    ctx.out("out", (B, Cc, H * W), dt)
    arrs = {k: (C.c_void_p * Lr)() for k in ("ys", "gates", "gys", "dots")}
    for i in range(Lr):
        ctx.inp(f"ys_{i}", torch.randn(B, Cc, H * W, generator=g), dt)
        ctx.inp(f"gates_{i}", torch.rand(B, Cc, generator=g))
        ctx.out(f"gys_{i}", (B, Cc, H * W), dt)
        ctx.out(f"dots_{i}", (B, Cc), torch.float32)
        for k in arrs:
            arrs[k][i] = ctx.ptr(f"{k}_{i}") or None
    for k, a in arrs.items():
        ctx.val(k, a)
    return [("pde_gate_combine_forward", {}), ("pde_gate_combine_backward", {})], []


def build_bn_pool(ctx, p):
    l = lib()
    g = _gen(p)
    B, Cc, N = p["B"], p["C"], p["N"]
    ctx.also_element = ELEMENT_ALIGNED_IN["pde_bn_pool_"]
    for k in ("B", "C", "N"):
        ctx.val(k, p[k])
    ctx.val("eps", 1e-5)
    ctx.val("training", p["training"])
    ctx.val("momentum", 0.1)
    ctx.inp("x", torch.randn(B, Cc, N, N, generator=g))
    ctx.inp("gamma", 1 + 0.2 * torch.randn(Cc, generator=g))
    ctx.inp("beta", 0.2 * torch.randn(Cc, generator=g))
    ctx.inp("gout", torch.randn(B, 2 * Cc, 4, 4, generator=g))
    ctx.inout("running_mean", 0.1 * torch.randn(Cc, generator=g))
    ctx.inout("running_var", 1 + 0.1 * torch.rand(Cc, generator=g))
    ctx.out("mean", (Cc,), torch.float32)
    ctx.out("invstd", (Cc,), torch.float32)
    ctx.out("out", (B, 2 * Cc, 4, 4), torch.float32)
    ctx.out("argmax", (B, Cc, 4, 4), torch.int32)
    ctx.out("gx", (B, Cc, N, N), torch.float32)
    ctx.out("ggamma", (Cc,), torch.float32)
    ctx.out("gbeta", (Cc,), torch.float32)
    n = l.pde_bn_pool_workspace_bytes(B, Cc)
    assert n > 0
    ctx.ws("fws", n)
    ctx.ws("bws", n)
    return [("pde_bn_pool_forward", {"workspace": "fws", "workspace_bytes": n}),
            ("pde_bn_pool_backward", {"workspace": "bws", "workspace_bytes": n})], []


# ---------------------------------------------------------------------------------------------------- explicit and Jacobi
def build_explicit(ctx, p):
    l = lib()
    g = _gen(p)
    B, Cc, H, W, nt, f64 = p["B"], p["C"], p["H"], p["W"], p["nt"], p["io"] == "f64"
    code, dt = IO[p["io"]]
    pt = torch.float64 if f64 else torch.float32
    emit = p.get("emit", 0)
    ctx.vec_elems = 1 if (f64 or W % 4) else 4                   # float4 rows: four elements per access, 8 bytes of 16-bit ones
    ctx.also_element = ELEMENT_ALIGNED_IN["pde_explicit5_"]
    for k, v in (("B", B), ("C", Cc), ("H", H), ("W", W), ("io_dtype", code), ("num_steps", nt), ("dt", 0.01), ("eps", 1e-6),
                 ("max_coeff", 0.15), ("relax", 0.1)):
        ctx.val(k, v)
    shape = (B, Cc, H, W)
    ctx.inp("u", torch.randn(shape, generator=g), dt)
    ctx.inp("gout", torch.randn(shape, generator=g), dt)
    ctx.inp("alpha_base", 0.05 + 0.1 * torch.rand(Cc, generator=g), pt)
    ctx.inp("channel_scaling", 1 + 0.1 * torch.randn(Cc, generator=g), pt)
    ctx.out("out", shape, dt)
    ctx.out("gu", shape, dt)
    ctx.out("g_alpha_base", (Cc,), pt)
    ctx.out("g_channel_scaling", (Cc,), pt)
    if nt > 1:
        # the inputs of steps 2..num_steps, fp32 whatever the I/O type: the forward may go without them on the wave-per-plane
        # sizes, but writes all of them when they are given, and the backward asks for them at every size
        ctx.out("states", (nt - 1,) + shape, pt)
    f = "pde_explicit5_f64_" if f64 else "pde_explicit5_"
    nb = ctx.ws("ws", getattr(l, f + "backward_workspace_bytes")(*((B, Cc, H, W) + (() if f64 else (code,)) + (nt,))))
    st = {} if nt > 1 else {"states": None}
    ba = dict(st, workspace="ws", workspace_bytes=nb)
    if emit:
        ctx.val("emit_mask", mask128(emit))
        ctx.out("traj", (popcount(emit),) + shape, dt)
        ctx.inp("gtraj", torch.randn((popcount(emit),) + shape, generator=g), dt)
        return [(f + "forward_states", st), (f + "backward_states", ba)], []
    return [(f + "forward", st), (f + "backward", ba)], []


def build_jacobi(ctx, p):
    """api: "plain" (pde_jacobi_forward / _backward, fp32), "io", "ws" (pde_jacobi_io_forward_ws), "states", or the float64
    forms "f64" / "f64_states"."""
    l = lib()
    g = _gen(p)
    B, H, W, nt, api = p["B"], p["H"], p["W"], p["nt"], p["api"]
    f64 = api.startswith("f64")
    code, dt = IO["f64" if f64 else p["io"]]
    pt = torch.float64 if f64 else torch.float32
    emit = p.get("emit", 0)
    ctx.vec_elems = 1                                            # the Jacobi kernels move one element at a time
    for k, v in (("B", B), ("H", H), ("W", W), ("nt", nt), ("io_dtype", code)):
        ctx.val(k, v)
    ctx.inp("u", torch.randn(B, H, W, generator=g), dt)
    ctx.inp("gout", torch.randn(B, H, W, generator=g), dt)
    ctx.inp("a_row", 0.05 + 0.15 * torch.rand(H, generator=g), pt)
    ctx.inp("b_col", 0.05 + 0.15 * torch.rand(W, generator=g), pt)
    ctx.out("out", (B, H, W), dt)
    ctx.out("gu", (B, H, W), dt)
    ctx.out("g_a_row", (H,), pt)
    ctx.out("g_b_col", (W,), pt)
    expect = [("pde_jacobi_plane_path", (H, W), p["path"])]
    if f64:
        nb = l.pde_jacobi_f64_backward_workspace_bytes(B, H, W, nt)
    elif api == "plain":
        nb = l.pde_jacobi_backward_workspace_bytes(B, H, W, nt)
    else:
        nb = l.pde_jacobi_io_backward_workspace_bytes(B, H, W, nt, code)
    ctx.ws("bws", nb)
    ba = {"workspace": "bws", "workspace_bytes": nb}
    if emit:
        ctx.val("emit_mask", mask128(emit))
        ctx.out("states", (popcount(emit), B, H, W), dt)
        ctx.inp("gstates", torch.randn(popcount(emit), B, H, W, generator=g), dt)
    if api in ("ws", "states"):
        nf = ctx.ws("fws", l.pde_jacobi_forward_workspace_bytes(B, H, W, nt))
        assert (nf > 0) == (p["path"] == 2 and nt > 10), nf
        fa = {"workspace": "fws", "workspace_bytes": nf}
    names = {"plain": ("pde_jacobi_forward", "pde_jacobi_backward"), "io": ("pde_jacobi_io_forward", "pde_jacobi_io_backward"),
             "ws": ("pde_jacobi_io_forward_ws", "pde_jacobi_io_backward"),
             "states": ("pde_jacobi_io_forward_states", "pde_jacobi_io_backward_states"),
             "f64": ("pde_jacobi_f64_forward", "pde_jacobi_f64_backward"),
             "f64_states": ("pde_jacobi_f64_forward_states", "pde_jacobi_f64_backward_states")}[api]
    calls = [(names[0], fa if api in ("ws", "states") else {}), (names[1], ba)]
    if p.get("plain_slices"):
        # the emitted slices against the plain call of that many steps, bit for bit: one more forward per emitted step
        k = 0
        for bit in range(nt - 1):
            if emit >> bit & 1:
                ctx.out(f"plain{k}", (B, H, W), dt)
                n = ctx.ws(f"pws{k}", l.pde_jacobi_forward_workspace_bytes(B, H, W, bit + 1))
                calls.append(("pde_jacobi_io_forward_ws", {"nt": bit + 1, "out": f"plain{k}", "workspace": f"pws{k}",
                                                           "workspace_bytes": n}))
                k += 1
    return calls, expect


# ---------------------------------------------------------------------------------------------------- symmetric layer
RH_PATH = {"strip32": 0, "strip16": 1, "row_blocks": 2}


def build_sym(ctx, p):
    """kind: "f32", "f16" or "bf16" (the 16-bit-operand layers: K16 made by pde_sym_k_to_*, B <= 128, a workspace always)."""
    l = lib()
    g = _gen(p)
    B, D, kind, with_ws = p["B"], p["D"], p["kind"], p.get("ws", True)
    t16 = {"f16": torch.float16, "bf16": torch.bfloat16}.get(kind)
    for k, v in (("B", B), ("D", D), ("act", p.get("act", 1)), ("training", 1), ("momentum", 0.1), ("eps", 1e-5),
                 ("scale", -1.0)):
        ctx.val(k, v)
    ctx.inp("X", torch.randn(B, D, generator=g))
    ctx.inp("K", torch.randn(D, D, generator=g) / D ** 0.5)
    ctx.inp("bn_weight", 1 + 0.2 * torch.randn(D, generator=g))
    ctx.inp("bn_bias", 0.2 * torch.randn(D, generator=g))
    ctx.inp("g_out", torch.randn(B, D, generator=g))
    has_base = p.get("base", True)
    if has_base:
        ctx.inp("base", torch.randn(B, D, generator=g))
    ctx.inout("running_mean", 0.1 * torch.randn(D, generator=g))
    ctx.inout("running_var", 1 + 0.1 * torch.rand(D, generator=g))
    ht = t16 or torch.float32
    ctx.out("P", (B, D), ht)
    ctx.out("H", (B, D), ht)
    ctx.out("mean", (D,), torch.float32)
    ctx.out("invstd", (D,), torch.float32)
    ctx.out("out", (B, D), torch.float32 if (has_base or t16 is None) else t16)
    ctx.out("dP", (B, D), ht)
    ctx.out("gX", (B, D), torch.float32)
    ctx.out("gK", (D, D), torch.float32)
    ctx.out("g_bn_weight", (D,), torch.float32)
    ctx.out("g_bn_bias", (D,), torch.float32)
    nobase = {} if has_base else {"base": None}
    expect = []
    if t16 is None:
        assert l.pde_sym_layer_supported(B, D) == 1
        n = l.pde_sym_layer_workspace_bytes(B, D) if with_ws else 0
        if n:
            ctx.ws("fws", n)
            ctx.ws("bws", n)
        fa = {"workspace": "fws" if n else None, "workspace_bytes": n}
        ba = {"workspace": "bws" if n else None, "workspace_bytes": n}
        if "path" in p:
            expect.append(("pde_sym_layer_path", (B, D, int(n > 0), None, None, None), RH_PATH[p["path"]]))
        if "dk_path" in p:
            expect.append(("pde_sym_layer_dk_path", (B, D), p["dk_path"]))
        return [("pde_sym_layer_forward", dict(fa, **nobase)), ("pde_sym_layer_backward", ba)], expect
    assert getattr(l, f"pde_sym_layer_{kind}_supported")(B, D) == 1
    n = getattr(l, f"pde_sym_layer_{kind}_workspace_bytes")(B, D)
    assert n > 0
    ctx.ws("fws", n)
    ctx.ws("bws", n)
    ctx.out("K16", (D, D), t16)
    return [(f"pde_sym_k_to_{kind}", {}),
            (f"pde_sym_layer_{kind}_forward", dict(nobase, workspace="fws", workspace_bytes=n)),
            (f"pde_sym_layer_{kind}_backward", {"workspace": "bws", "workspace_bytes": n})], expect


BUILDERS = {"adi": build_adi, "steps": build_steps, "small": build_small, "mixed": build_mixed, "multi": build_multi,
            "mix": build_mix, "blend": build_blend, "gate": build_gate, "bn_pool": build_bn_pool, "explicit": build_explicit,
            "jacobi": build_jacobi, "sym": build_sym}


# ---------------------------------------------------------------------------------------------------- the table
class Case:
    def __init__(self, id, family, p, switch=None, note=""):
        self.id, self.family, self.p, self.switch, self.note = id, family, p, switch, note

    def build(self, ctx):
        return BUILDERS[self.family](ctx, dict(self.p))

    def __repr__(self):
        return self.id


def _bits(*bs):
    return sum(1 << b for b in bs)


def _all_but_last(n):
    """Bits 0 .. n-2: every sweep (step) of n but the last — the whole range a checkpoint or emission mask may set."""
    return (1 << (n - 1)) - 1


def _sched_id(steps, split):
    return f"{steps}{split}"


SCHEDULES = ((1, "strang"), (2, "strang"), (2, "lie"))


def _adi_cases():
    out = []

    def add(tag, sw=None, **p):
        H, W = p["H"], p["W"]
        size = f"n{H}" if H == W and not p.get("rect") else f"{H}x{W}"
        cid = (f"adi-{tag}-{size}-b{p['B']}c{p['C']}-{p['io']}-{_sched_id(p['steps'], p.get('split', 'strang'))}"
               f"-ck{p.get('ckpt', 0):x}-em{p.get('emit', 0):x}" + (f"-{sw}" if sw else ""))
        out.append(Case(cid, "adi", p, sw))

    # fused line lengths
    for N in (8, 12, 28, 32):
        for B, Cc in ((1, 1), (3, 5), (37, 5)):
            for io in IO3:
                for steps, split in SCHEDULES:
                    kern = {}
                    if N == 32 and io == "f32" and (steps, split) == (2, "strang"):
                        kern = dict(fwd_kernel=3, bwd_kernel=1)      # the hand-over forward, the assembly backward
                    add("fused", B=B, C=Cc, H=N, W=N, io=io, steps=steps, split=split, **kern)
        for io in IO3:
            S = 6
            for ck in (_bits(2), _all_but_last(S)):                  # the pre-pass and the parked states in the workspace
                add("fused", B=3, C=5, H=N, W=N, io=io, steps=2, ckpt=ck)
            for em in (_bits(0), _all_but_last(S)):                  # {first sweep}, {every sweep but the last}
                add("fused", B=3, C=5, H=N, W=N, io=io, steps=2, emit=em)
            add("fused", B=37, C=5, H=N, W=N, io=io, steps=2, ckpt=_bits(1), emit=_all_but_last(S))
    add("clampmove", B=37, C=1, H=32, W=32, io="f32", steps=2, dt=0.05, clampmove=True, bwd_kernel=1)
    add("norefactor", B=3, C=5, H=32, W=32, io="f32", steps=2, reuse=False, bwd_kernel=1)
    add("norefactor", B=3, C=5, H=28, W=28, io="bf16", steps=2, reuse=False, ckpt=_bits(2))
    # kernels behind a switch: the same N = 32 fp32 Strang cases, one child interpreter per value
    for sw, kern in (("PDE_ASM_FWD=1", dict(fwd_kernel=1)), ("PDE_ASM_BWD=0", dict(bwd_kernel=0)),
                     ("PDE_FWD_SCHED=0", dict(fwd_kernel=0))):
        for B, Cc in ((1, 1), (3, 5), (37, 5)):
            add("fused", sw, B=B, C=Cc, H=32, W=32, io="f32", steps=2, **kern)
    # the any-size path: layout changes at N = 44 / 82 / 100
    for N in (2, 5, 33, 44, 45, 82, 84, 100, 104, 128):
        for io in IO3:
            add("any", B=3, C=2, H=N, W=N, io=io, steps=1, fwd_kernel=2, bwd_kernel=2)
            add("any", B=3, C=2, H=N, W=N, io=io, steps=2, ckpt=_bits(1, 4), fwd_kernel=2)
            add("any", B=3, C=2, H=N, W=N, io=io, steps=2, emit=_bits(0, 3))
            add("any", B=3, C=2, H=N, W=N, io=io, steps=2, emit=_all_but_last(6))
    for H, W in ((5, 9), (2, 128), (128, 2), (100, 128)):
        for io in IO3:
            add("rect", B=3, C=2, H=H, W=W, io=io, steps=1, rect=True)
            add("rect", B=3, C=2, H=H, W=W, io=io, steps=2, rect=True, ckpt=_bits(1, 4))
            add("rect", B=3, C=2, H=H, W=W, io=io, steps=2, rect=True, emit=_bits(0, 3))
            add("rect", B=3, C=2, H=H, W=W, io=io, steps=2, rect=True, emit=_all_but_last(6))
    # float64: at 128 x 128 the backward keeps its state plane in the workspace
    for N in (5, 100, 128):
        add("f64", B=3, C=2, H=N, W=N, io="f64", steps=1)
        add("f64", B=3, C=2, H=N, W=N, io="f64", steps=2, ckpt=_bits(1, 4))
        add("f64", B=3, C=2, H=N, W=N, io="f64", steps=2, emit=_bits(0, 3))
        add("f64", B=3, C=2, H=N, W=N, io="f64", steps=2, emit=_all_but_last(6))
    add("rect", B=3, C=2, H=100, W=128, io="f64", steps=1, rect=True)
    add("rect", B=3, C=2, H=100, W=128, io="f64", steps=2, rect=True, ckpt=_bits(1, 4))
    add("rect", B=3, C=2, H=100, W=128, io="f64", steps=2, rect=True, emit=_bits(0, 3))
    add("rect", B=3, C=2, H=100, W=128, io="f64", steps=2, rect=True, emit=_all_but_last(6))
    return out


def _layer_cases():
    out = []
    for io in IO3:
        for ck in (0, _bits(0)):
            out.append(Case(f"steps-n16-c5-{io}-ck{ck}", "steps", dict(B=3, C=5, H=16, W=16, io=io, steps=2, ckpt=ck)))
    for Cc in (1, 3, 4):
        for N in (16, 28):
            for B in (1, 5):
                for mode, skip in ((1, False), (2, False), (2, True)):
                    io = IO3[(Cc + N // 4 + B + mode) % 3]
                    p = dict(B=B, C=Cc, H=N, W=N, io=io, steps=2, mode=mode, skip=skip)
                    out.append(Case(f"small-c{Cc}-n{N}-b{B}-{io}-m{mode}{'s' if skip else ''}", "small", p))
                io = IO3[(Cc + B) % 3]
                out.append(Case(f"small-states-c{Cc}-n{N}-b{B}-{io}", "small",
                                dict(B=B, C=Cc, H=N, W=N, io=io, steps=3, mode=1 + (Cc + B) % 2, emit=_all_but_last(3) if (B == 5 or N == 28) else _bits(0),
                                     ckpt=_bits(0) if N == 28 else 0)))
    for Cc in (32, 64):
        for mode in (1, 2):
            p = dict(B=3, C=Cc, H=8, W=8, io="f32", steps=2, mode=mode, one_launch=0)
            # N = 8 has no one-launch kernel (N = 28 or 32): these run per step; the one-launch forward is the N = 28 case
            out.append(Case(f"mixed-c{Cc}-n8-f32-m{mode}", "mixed", p))
        out.append(Case(f"mixed-one-launch-c{Cc}-n28-f32", "mixed",
                        dict(B=3, C=Cc, H=28, W=28, io="f32", steps=2, mode=1 + Cc // 64, one_launch=1)))
        out.append(Case(f"mixed-c{Cc}-n28-f32-PDE_WIDE=0", "mixed",
                        dict(B=3, C=Cc, H=28, W=28, io="f32", steps=2, mode=1 + Cc // 64, one_launch=0), "PDE_WIDE=0"))
    for Cc in (96, 128):
        for io in ("f32", "bf16"):
            out.append(Case(f"mixed-c{Cc}-n8-{io}", "mixed",
                            dict(B=3, C=Cc, H=8, W=8, io=io, steps=2, mode=1 if io == "f32" else 2, one_launch=0,
                                 ckpt=_bits(0) if Cc == 96 else 0)))
    for io in IO3:
        out.append(Case(f"multi-n16-c3-b3-{io}", "multi", dict(B=3, C=3, H=16, W=16, io=io)))
    return out


def _side_cases():
    out = []
    # (C, B, HW, io, forward path, backward path): one ragged and one whole-tile case per path (tests/test_gpu_mix_paths.py)
    mix = [(1, 1, 1, "f32", "scalar", "scalar"), (33, 2, 49, "bf16", "scalar", "scalar"), (160, 1, 49, "f16", "scalar", "scalar"),
           (33, 3, 64, "f32", "scalar", "scalar"), (160, 2, 196, "f32", "scalar", "scalar"),
           (64, 1, 64, "f32", "mfma32", "split3"), (64, 5, 196, "f32", "mfma32", "split3"),
           (128, 1, 64, "f32", "mfma32", "fused"), (128, 3, 196, "f32", "mfma32", "fused"),
           (64, 5, 196, "bf16", "mfma32", "fused"), (128, 3, 196, "f16", "mfma32", "fused"),
           (64, 1, 64, "bf16", "mfma16", "mfma16"), (128, 1, 64, "f16", "mfma16", "mfma16"),
           (64, 2, 49, "f32", "scalar", "scalar"), (128, 2, 1, "f16", "scalar", "scalar")]
    for Cc, B, HW, io, fp, bp in mix:
        out.append(Case(f"mix-c{Cc}-b{B}-hw{HW}-{io}", "mix", dict(B=B, C=Cc, HW=HW, io=io, fwd_path=fp, bwd_path=bp)))
    for sw, rows in (("PDE_MIX_NO_SPLIT=1", [(64, 1, 64, "f32", "mfma32", "fused"), (64, 5, 196, "f32", "mfma32", "fused")]),
                     ("PDE_MIX_UNFUSED=1", [(128, 1, 64, "f32", "mfma32", "mfma32"), (128, 3, 196, "f32", "mfma32", "mfma32"),
                                            (64, 5, 196, "bf16", "mfma32", "mfma32")]),
                     ("PDE_MIX_NO_BF16_MFMA=1", [(64, 1, 64, "bf16", "mfma32", "fused"), (128, 1, 64, "f16", "mfma32", "fused")])):
        for Cc, B, HW, io, fp, bp in rows:
            out.append(Case(f"mix-c{Cc}-b{B}-hw{HW}-{io}-{sw}", "mix",
                            dict(B=B, C=Cc, HW=HW, io=io, fwd_path=fp, bwd_path=bp), sw))
    for Cc, B, HW in ((1, 1, 1), (33, 2, 49), (64, 1, 64), (128, 3, 196), (128, 2, 49)):      # float64: C <= 128
        out.append(Case(f"mix-c{Cc}-b{B}-hw{HW}-f64", "mix", dict(B=B, C=Cc, HW=HW, io="f64")))
    for n in (1, 255, 256 * 512 + 3):
        for io in IO3 + ("f64",):
            out.append(Case(f"blend-n{n}-{io}", "blend", dict(n=n, io=io)))
    for io in IO3:
        out.append(Case(f"gate-l1-2x2-b1c1-{io}", "gate", dict(L=1, B=1, C=1, hw=(2, 2), io=io)))
        out.append(Case(f"gate-l3-7x36-b5c1-{io}", "gate", dict(L=3, B=5, C=1, hw=(7, 36), io=io)))
        out.append(Case(f"gate-l4-2x2-b1c3-{io}", "gate", dict(L=4, B=1, C=3, hw=(2, 2), io=io)))
    for B, Cc, N in ((2, 1, 4), (3, 5, 12), (65, 2, 8)):
        for tr in (1, 0):
            out.append(Case(f"bn_pool-b{B}c{Cc}n{N}-{'train' if tr else 'eval'}", "bn_pool", dict(B=B, C=Cc, N=N, training=tr)))
    return out


def _explicit_cases():
    out = []
    for H, W in ((16, 16), (32, 32), (64, 64), (60, 64), (5, 7), (4, 65)):
        for io in IO3 + ("f64",):
            for nt in (1, 3):
                out.append(Case(f"explicit-{H}x{W}-{io}-nt{nt}", "explicit", dict(B=3, C=2, H=H, W=W, io=io, nt=nt)))
            for em in (_bits(0), _all_but_last(4)):
                out.append(Case(f"explicit-states-{H}x{W}-{io}-em{em:x}", "explicit",
                                dict(B=3, C=2, H=H, W=W, io=io, nt=4, emit=em)))
    for H, W in ((4, 4), (5, 7), (64, 64), (65, 8), (97, 130)):
        path = 2 if max(H, W) > 64 else 1
        for io in IO3:
            for nt in (1, 10):
                out.append(Case(f"jacobi-io-{H}x{W}-{io}-nt{nt}", "jacobi", dict(B=3, H=H, W=W, nt=nt, io=io, api="io", path=path)))
            for em in (_bits(0), _all_but_last(10)):
                out.append(Case(f"jacobi-states-{H}x{W}-{io}-em{em:x}", "jacobi",
                                dict(B=3, H=H, W=W, nt=10, io=io, api="states", emit=em, path=path)))
        out.append(Case(f"jacobi-plain-{H}x{W}-nt10", "jacobi", dict(B=3, H=H, W=W, nt=10, io="f32", api="plain", path=path)))
        if path == 1:
            out.append(Case(f"jacobi-f64-{H}x{W}-nt10", "jacobi", dict(B=3, H=H, W=W, nt=10, io="f64", api="f64", path=path)))
            out.append(Case(f"jacobi-f64-states-{H}x{W}", "jacobi",
                            dict(B=3, H=H, W=W, nt=10, io="f64", api="f64_states", emit=_all_but_last(10), path=path)))
    for H, W in ((65, 8), (97, 130)):
        for io in IO3:
            out.append(Case(f"jacobi-ws-{H}x{W}-{io}-nt12", "jacobi", dict(B=3, H=H, W=W, nt=12, io=io, api="ws", path=2)))
            out.append(Case(f"jacobi-states-{H}x{W}-{io}-nt12", "jacobi",
                            dict(B=3, H=H, W=W, nt=12, io=io, api="states", emit=_bits(0, 9, 10), path=2)))
    # the only case of the suite that sends a slot index through the high word of emit_slot (pde_common.h) on a kernel;
    # its slices are also compared bit for bit with the plain call of that many steps
    hi = _bits(0, 63, 64, 68)
    out.append(Case("jacobi-states-5x7-f32-nt70-high-word", "jacobi",
                    dict(B=2, H=5, W=7, nt=70, io="f32", api="states", emit=hi, path=1, plain_slices=True)))
    out.append(Case("jacobi-states-65x8-bf16-nt70-high-word", "jacobi",
                    dict(B=2, H=65, W=8, nt=70, io="bf16", api="states", emit=hi, path=2, plain_slices=True)))
    out.append(Case("jacobi-f64-states-5x7-nt70-high-word", "jacobi",
                    dict(B=2, H=5, W=7, nt=70, io="f64", api="f64_states", emit=hi, path=1)))
    out.append(Case("explicit-states-5x7-f32-nt70-high-word", "explicit", dict(B=2, C=2, H=5, W=7, io="f32", nt=70, emit=hi)))
    out.append(Case("explicit-states-16x16-f16-nt70-high-word", "explicit", dict(B=2, C=2, H=16, W=16, io="f16", nt=70, emit=hi)))
    return out


def _sym_cases():
    out = []
    # the ragged batches of tests/rh_cases.py, one case per path of pde_sym_layer_path / _dk_path
    # (D = 192 has no split of its contraction: the workspace query answers 0 and the 16-column strips run either way;
    # (100, 256) is the four-wave form of the 32-column strips)
    for B, D, ws, path in ((33, 128, True, "strip32"), (33, 128, False, "strip16"), (100, 192, True, "strip16"),
                           (100, 192, False, "strip16"), (100, 256, True, "strip32"), (129, 128, True, "row_blocks"),
                           (129, 128, False, "row_blocks")):
        out.append(Case(f"sym-f32-b{B}-d{D}-{'ws' if ws else 'null'}", "sym",
                        dict(B=B, D=D, kind="f32", ws=ws, path=path, dk_path=0, act=1 + (B + D) % 2, base=B != 100)))
    for sw, rows in (("PDE_RH_NO_STRIP32=1", [(33, 128, "strip16", 0), (100, 256, "strip16", 0)]),
                     ("PDE_RH_NO_SPLIT=1", [(33, 128, "strip32", 1), (129, 128, "row_blocks", 1)])):
        for B, D, path, dk in rows:
            out.append(Case(f"sym-f32-b{B}-d{D}-ws-{sw}", "sym", dict(B=B, D=D, kind="f32", ws=True, path=path, dk_path=dk), sw))
    for kind in ("f16", "bf16"):
        for B, D in ((33, 128), (100, 192), (128, 64)):
            out.append(Case(f"sym-{kind}-b{B}-d{D}", "sym", dict(B=B, D=D, kind=kind, base=B != 100, act=1 + B % 2)))
    return out


CASES = _adi_cases() + _layer_cases() + _side_cases() + _explicit_cases() + _sym_cases()
BY_ID = {c.id: c for c in CASES}
