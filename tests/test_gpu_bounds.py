"""Every C entry point held to its buffers (tests/bounds_cases.py, tests/guard_util.py).

Each case runs its sequence of C ABI calls twice, through ctypes with every pointer owned by the test:

  (b) guarded: every device pointer comes from a ``guard_util.Arena`` — 1 MiB of 0xFF on both sides of every buffer, the
      tail guard at the buffer's exact last byte + 1; every overwritten output pre-filled with 0xFF (a NaN in every
      floating type); every workspace exactly ``*_workspace_bytes(...)`` bytes and 0xFF-filled;
  (a) plain: the same values in ordinary torch tensors from the caching allocator, outputs and workspaces zero-filled (a
      workspace is at least 256 bytes long so that its pointer is never NULL; the size passed is the queried one).

and asserts: every return code 0 and every guard byte intact (a store past either end of a buffer); no element of an
overwritten output still all-ones (a ragged tail that is skipped); every output of (b) finite where (a) is and bitwise
equal to (a) (scratch or partial sums read before the call wrote them).  The guarded run goes first, and the plain run
follows only when its guards held.  No reference is needed but the call itself.

Kernels behind an environment switch the library reads once per process run in one child interpreter per switch value
(this file run as a script), which writes a report the parent asserts on.  A last child runs the smallest case of every
public function family of ``functional`` with the wrappers' own scratch (``functional._workspace``, the symmetric layer's
``_sym_workspace``) replaced by arena buffers of exactly the requested size.  The 16-bit-operand symmetric layers take
their workspace from ``torch.empty`` directly (``functional._sym16_forward`` / ``_sym16_backward``): that patch does not
reach them, their C ABI cases in the table do.

After a fault of the device nothing more is started on it: a ``RuntimeError`` from torch that is not the library's own
``PdeError``, a child's exit code 3 or a child that ran into its time limit ends the whole pytest session."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bounds_cases as BC  # noqa: E402
import guard_util as GU  # noqa: E402

pytestmark = pytest.mark.gpu

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class GpuFault(RuntimeError):
    pass


class PlainCtx(BC.SpecCtx):
    device = "cuda"

    def _alloc(self, name, role, shape, dtype, fill):
        if fill is not None:
            return fill.to(dtype).contiguous().to("cuda")
        if dtype == torch.uint8 and role in ("ws", "carry"):
            return torch.zeros(max(shape[0], 256), dtype=torch.uint8, device="cuda")      # never NULL; the size passed stays
        return torch.zeros(shape, dtype=dtype, device="cuda")

    def ptr(self, name, byte_offset=0):
        return self.t[name].data_ptr() + byte_offset

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class ArenaCtx(PlainCtx):
    skew = False                                 # tests/test_gpu_alignment.py: every buffer at exactly the alignment the header asks

    def __init__(self):
        super().__init__()
        self.arena = GU.Arena("cuda", skew=self.skew)

    def _alloc(self, name, role, shape, dtype, fill):
        if self.skew:
            return self.arena.tensor(shape, dtype, fill=fill, name=name, align=self.aligns[name])
        return self.arena.tensor(shape, dtype, fill=fill, name=name)

    def ptr(self, name, byte_offset=0):
        return self.arena.ptr(self.t[name]) + byte_offset


def _is_fault(e):
    """torch reports a HIP error of the device as a plain RuntimeError, from whichever call meets it first; the library's
    own refusals are PdeError."""
    from cnn_with_pde_amd._lib import PdeError
    return isinstance(e, GpuFault) or (isinstance(e, RuntimeError) and not isinstance(e, PdeError))


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                    # a fault: nothing more may be started on this device
        raise GpuFault(str(e)) from e


def _run(case, ctx, lib, hdr):
    calls, expect = case.build(ctx)
    for fn, args, want in expect:
        got = getattr(lib, fn)(*args)
        assert got == want, f"{case.id}: {fn} answers {got}, the case is meant for {want}"
    for i, (fn, amap) in enumerate(calls):
        rc = getattr(lib, fn)(*BC.call_args(ctx, hdr[fn], amap))
        assert rc == 0, f"{case.id}: call {i} ({fn}) returned {rc}"
    _sync()
    return calls


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def _finite(t):
    return torch.isfinite(t) if t.is_floating_point() else torch.ones_like(t, dtype=torch.bool)


def check_case(case, lib=None, hdr=None, guarded_ctx=None):
    """Both runs of one case and the assertions; returns the line it prints.  ``guarded_ctx``: the context of the guarded run
    (``ArenaCtx``, or a subclass that places its buffers differently)."""
    lib = lib or BC.lib()
    hdr = hdr or BC.header_functions()
    guarded = (guarded_ctx or ArenaCtx)()
    _run(case, guarded, lib, hdr)
    guarded.arena.check()                                        # 1. every guard byte of every buffer
    outs = [n for n, r in guarded.roles.items() if r == "out"]
    for n in outs:                                               # 2. no element of an overwritten output was skipped
        left = GU.Arena.unwritten(guarded.t[n])
        assert left == 0, f"{case.id}: {left} of {guarded.t[n].numel()} elements of {n} were never written"
    plain = PlainCtx()
    _run(case, plain, lib, hdr)
    compared = outs + [n for n, r in guarded.roles.items() if r == "inout"] + list(guarded.written_slots)
    for n in compared:
        a, b = plain.t[n], guarded.t[n]
        if n in guarded.written_slots:                           # written in part: the slices the header names, held like
            a, b = a[guarded.written_slots[n]], b[guarded.written_slots[n]]      # an output (2. as well)
            left = GU.Arena.unwritten(b)
            assert left == 0, f"{case.id}: {left} elements of the written slices {guarded.written_slots[n]} of {n} were never written"
        bad = _finite(a) & ~_finite(b)                           # 3. poison that reached a result
        assert not bool(bad.any()), f"{case.id}: {int(bad.sum())} elements of {n} are not finite in the guarded run only"
        same = _bits(a) == _bits(b)                              # 4. bitwise the plain run
        assert bool(same.all()), (f"{case.id}: {int((~same).sum())} of {a.numel()} elements of {n} differ between the plain "
                                  f"and the guarded run, first at flat index {int((~same).flatten().nonzero()[0])}")
    if case.p.get("plain_slices"):                               # emitted slices = the plain call of that many steps
        for ctx in (guarded, plain):
            k = 0
            while f"plain{k}" in ctx.t:
                assert torch.equal(_bits(ctx.t["states"][k]), _bits(ctx.t[f"plain{k}"])), (case.id, "slot", k)
                k += 1
            assert k == BC.popcount(case.p["emit"])
    guarded.arena.check()
    line = (f"{case.id}: {len(guarded.roles)} buffers guarded ({guarded.arena.guarded_bytes() >> 20} MiB of guard bytes), "
            f"{len(outs)} outputs checked for unwritten elements, {len(compared)} compared bitwise: " + " ".join(compared))
    return line


def test_the_arena_sees_a_stray_store_on_the_device():
    """The arena's own check on device memory: stores planted with torch one element before a tensor, one element behind
    its odd-sized end and at the far end of the tail guard are reported where they are; nothing else is."""
    a = GU.Arena("cuda")
    t = a.tensor((37, 3), torch.bfloat16, fill=torch.zeros(37, 3), name="t")
    other = a.raw(1001, name="other")
    assert t.is_cuda and t.data_ptr() % 256 == 0 and other.data_ptr() % 256 == 0 and a.unwritten(t) == 0
    a.check()
    r = a.bufs[0]
    end = r.off + r.nbytes
    r.buf[end:end + 2] = 0
    assert a.damage() == [("t", "tail", 0, 1, 2)]
    r.buf[end:end + 2] = GU.POISON
    r.buf[r.off - 2:r.off] = 0
    r.buf[-1] = 0
    assert a.damage() == [("t", "head", -2, -1, 2), ("t", "tail", r.buf.numel() - 1 - end, r.buf.numel() - 1 - end, 1)]
    with pytest.raises(GU.GuardError):
        a.check()
    p = a.tensor((5, 9), torch.float16)
    p[:, :4] = 1.0
    assert a.unwritten(p) == 25


IN_PROCESS = [c for c in BC.CASES if c.switch is None]


@pytest.fixture(scope="module")
def library():
    return BC.lib(), BC.header_functions()


@pytest.mark.parametrize("case", IN_PROCESS, ids=[c.id for c in IN_PROCESS])
def test_bounds(case, library):
    try:
        print(check_case(case, *library))
    except RuntimeError as e:
        if not _is_fault(e):
            raise
        pytest.exit(f"GPU fault in {case.id}: {e}", returncode=3)


# ---------------------------------------------------------------------------------------------------- children
def _child(mode, env, tmp_path):
    report = str(tmp_path / "report.json")
    keep = {k: v for k, v in os.environ.items() if k.partition("=")[0] not in {s.partition("=")[0] for s in BC.SWITCHES}}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, report], env=dict(keep, **env),
                           capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired as e:       # a hang: the next child must not start on this device
        pytest.exit(f"the child {mode} ran into its time limit: {str(e.stderr)[-1500:]}", returncode=3)
    if r.returncode == 3:
        pytest.exit(f"GPU fault in the child {mode}: {r.stderr[-1500:]}", returncode=3)
    assert r.returncode == 0, (mode, r.stdout[-1500:], r.stderr[-3000:])
    print(r.stdout)
    return json.load(open(report))


@pytest.mark.parametrize("switch", BC.SWITCHES)
def test_bounds_behind_a_switch(switch, tmp_path):
    name, _, value = switch.partition("=")
    want = [c.id for c in BC.CASES if c.switch == switch]
    assert want
    rep = _child(switch, {name: value}, tmp_path)
    assert sorted(rep) == sorted(want)
    bad = {k: v for k, v in rep.items() if v != "ok"}
    assert not bad, bad


def test_the_wrappers_own_scratch(tmp_path):
    """functional.py sizes the scratch that the C ABI cases size by hand: the smallest case of every public function family
    with ``_workspace`` / ``_sym_workspace`` handing out arena buffers of exactly the requested size, 0xFF-filled — guards
    intact, results bitwise those of the unpatched call."""
    rep = _child("wrappers", {"PDE_HOST_EXT": "0"}, tmp_path)
    assert set(rep) == set(WRAPPER_FAMILIES), set(rep) ^ set(WRAPPER_FAMILIES)
    bad = {k: v for k, v in rep.items() if v != "ok"}
    assert not bad, bad


# ---- the wrapper families: name -> callable(P, F, gen) returning the tensors to compare (outputs and gradients) ----------
def _grads(out, inputs, gen):
    outs = out if isinstance(out, (tuple, list)) else [out]
    outs = [o for o in outs if o is not None and o.requires_grad]
    gs = [torch.randn(o.shape, generator=gen).to(o.dtype).cuda() for o in outs]
    got = torch.autograd.grad(outs, [t for t in inputs if t.requires_grad], gs, allow_unused=True)
    return [o.detach() for o in outs] + [g for g in got if g is not None]


def _adi_inputs(gen, B, Cc, H, W, dtype=torch.float32):
    u = torch.randn(B, Cc, H, W, generator=gen).to(dtype).cuda().requires_grad_(True)
    ps = [(1 + 0.15 * torch.randn(Cc, H, W, generator=gen)).cuda().requires_grad_(True) for _ in range(2)]
    ps += [(0.5 * torch.randn(Cc, H, W, generator=gen)).cuda().requires_grad_(True) for _ in range(2)]
    return u, [ps[0], ps[1], ps[2], ps[3]]


def _w_adi(P, F, gen, states=False, N=12, dtype=torch.float32):
    u, ps = _adi_inputs(gen, 3, 5, N, N, dtype)
    sweeps = [s for st in P.adi_schedule(0.02, 1.0, 1.0, 2) for s in st]
    if states:
        y = P.adi_diffuse_states(u, *ps, sweeps, [0, 3, 5], clamp_max=10.0, checkpoints=0b10)
    else:
        y = P.adi_diffuse(u, *ps, sweeps, clamp_max=10.0, checkpoints=0b10)
    return _grads(y, [u] + ps, gen)


def _w_layer(P, F, gen, which):
    Cc, N = {"small": (3, 16), "mixed": (32, 8)}[which]
    u, ps = _adi_inputs(gen, 3, Cc, N, N)
    M = (torch.eye(Cc) + 0.2 / Cc ** 0.5 * torch.randn(Cc, Cc, generator=gen)).cuda().requires_grad_(True)
    steps = P.adi_schedule(0.02, 1.0, 1.0, 2)
    fn = P.adi_diffuse_small if which == "small" else P.adi_diffuse_mixed
    y = fn(u, *ps, M, steps, "pre", clamp_max=10.0, checkpoints=0)
    return _grads(y, [u, M] + ps, gen)


def _w_multi(P, F, gen):
    u, _ = _adi_inputs(gen, 3, 3, 16, 16)
    layers, leaves = [], [u]
    for dt, k in BC.MULTI_LAYERS:
        _, ps = _adi_inputs(gen, 1, 3, 16, 16)
        M = (torch.eye(3) + 0.2 * torch.randn(3, 3, generator=gen)).cuda().requires_grad_(True)
        layers.append(dict(alpha_base=ps[0], beta_base=ps[1], alpha_time_coeff=ps[2], beta_time_coeff=ps[3], M=M,
                           steps=P.adi_schedule(dt, 1.0, 1.0, k), clamp_max=10.0))
        leaves += ps + [M]
    w = torch.softmax(torch.randn(3, generator=gen), 0).cuda().requires_grad_(True)
    out, ys = P.adi_diffuse_multi(u, layers, weights=w, checkpoints=0)
    return _grads([out] + list(ys), leaves + [w], gen)


def _w_mix(P, F, gen):
    u = torch.randn(2, 33, 7, 7, generator=gen).cuda().requires_grad_(True)
    M = (torch.randn(33, 33, generator=gen) / 6).cuda().requires_grad_(True)
    return _grads(P.channel_mix(u, M), [u, M], gen)


def _w_blend(P, F, gen):
    u0, u = (torch.randn(255, generator=gen).cuda().requires_grad_(True) for _ in range(2))
    w = torch.tensor(0.4).cuda().requires_grad_(True)
    return _grads(F.skip_blend(u0, u, w), [u0, u, w], gen)


def _w_explicit(P, F, gen, states=False):
    u = torch.randn(3, 2, 5, 7, generator=gen).cuda().requires_grad_(True)
    a = (0.05 + 0.1 * torch.rand(2, generator=gen)).cuda().requires_grad_(True)
    s = (1 + 0.1 * torch.randn(2, generator=gen)).cuda().requires_grad_(True)
    y = P.explicit5_states(u, a, s, steps=(1, 3)) if states else P.explicit5_step(u, a, s, num_steps=3)
    return _grads(y, [u, a, s], gen)


def _w_jacobi(P, F, gen, states=False):
    u = torch.randn(3, 65, 8, generator=gen).cuda().requires_grad_(True)
    a = (0.05 + 0.15 * torch.rand(65, generator=gen)).cuda().requires_grad_(True)
    b = (0.05 + 0.15 * torch.rand(8, generator=gen)).cuda().requires_grad_(True)
    y = P.jacobi_diffuse_states(u, a, b, (1, 11, 12)) if states else P.jacobi_diffuse(u, a, b, 12)
    return _grads(y, [u, a, b], gen)


def _w_sym(P, F, gen):
    B, D = 33, 128
    X = torch.randn(B, D, generator=gen).cuda().requires_grad_(True)
    K = (torch.randn(D, D, generator=gen) / D ** 0.5).cuda().requires_grad_(True)
    bn = torch.nn.BatchNorm1d(D).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(D, generator=gen))
        bn.bias.copy_(0.2 * torch.randn(D, generator=gen))
    y = F.sym_layer(X, K, bn, "relu", base=X, scale=-1.0)
    return _grads(y, [X, K, bn.weight, bn.bias], gen) + [bn.running_mean.clone(), bn.running_var.clone()]


WRAPPER_FAMILIES = {
    "adi_diffuse": _w_adi, "adi_diffuse_states": lambda P, F, g: _w_adi(P, F, g, states=True),
    "adi_diffuse_any_size_bf16": lambda P, F, g: _w_adi(P, F, g, N=33, dtype=torch.bfloat16),
    "adi_diffuse_small": lambda P, F, g: _w_layer(P, F, g, "small"),
    "adi_diffuse_mixed": lambda P, F, g: _w_layer(P, F, g, "mixed"),
    "adi_diffuse_multi": _w_multi, "channel_mix": _w_mix, "skip_blend": _w_blend,
    "explicit5_step": _w_explicit, "explicit5_states": lambda P, F, g: _w_explicit(P, F, g, states=True),
    "jacobi_diffuse": _w_jacobi, "jacobi_diffuse_states": lambda P, F, g: _w_jacobi(P, F, g, states=True),
    "sym_layer": _w_sym,
}


def _wrappers_child():
    import cnn_with_pde_amd as P
    import cnn_with_pde_amd.functional as F
    from cnn_with_pde_amd import _lib as L
    assert L.host_ext() is None, "PDE_HOST_EXT=0 keeps every call on the ctypes path"
    real_ws, real_sym = F._workspace, F._sym_workspace
    rep = {}
    for name, fn in WRAPPER_FAMILIES.items():
        try:
            want = fn(P, F, torch.Generator().manual_seed(99))
            _sync()
            arena, asked = GU.Arena("cuda"), []

            def ws(nbytes, device):
                asked.append(int(nbytes))
                return arena.raw(int(nbytes), name=f"{name}:workspace{len(asked)}")

            def sym_ws(B, D, dev):
                n = L.load().pde_sym_layer_workspace_bytes(B, D)
                asked.append(int(n))
                return arena.raw(n, name=f"{name}:sym_workspace{len(asked)}") if n else None

            F._workspace, F._sym_workspace = ws, sym_ws
            try:
                got = fn(P, F, torch.Generator().manual_seed(99))
                _sync()
            finally:
                F._workspace, F._sym_workspace = real_ws, real_sym
            arena.check()
            assert len(got) == len(want) and len(got) >= 2
            for i, (a, b) in enumerate(zip(want, got)):
                assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), f"result {i} differs from the unpatched call"
                assert bool(_finite(b).all()), f"result {i} is not finite"
            print(f"{name}: {len(asked)} scratch buffers of {asked} bytes, {arena.guarded_bytes() >> 20} MiB of guard bytes, "
                  f"{len(got)} results bitwise equal")
            rep[name] = "ok"
        except Exception as e:  # noqa: BLE001  (the parent asserts on the report)
            if _is_fault(e):
                raise GpuFault(str(e)) from e
            rep[name] = f"{type(e).__name__}: {e}"[:600]
    return rep


def _main(mode, report):
    try:
        if mode == "wrappers":
            rep = _wrappers_child()
        else:
            lib, hdr = BC.lib(), BC.header_functions()
            rep = {}
            for c in BC.CASES:
                if c.switch == mode:
                    t0 = time.time()
                    try:
                        print(check_case(c, lib, hdr), f"[{time.time() - t0:.2f} s]")
                        rep[c.id] = "ok"
                    except Exception as e:  # noqa: BLE001  (the parent names the case from the report)
                        if _is_fault(e):
                            raise GpuFault(str(e)) from e
                        rep[c.id] = f"{type(e).__name__}: {e}"[:600]
    except GpuFault as e:
        print(f"GPU fault: {e}", file=sys.stderr)
        return 3
    json.dump(rep, open(report, "w"))
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv[1], sys.argv[2]))
