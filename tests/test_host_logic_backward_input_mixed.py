"""Host logic of the input-only route of the channel-operator nodes (functional._AdiMixedFn, _MixFn, _MixF64Fn,
_SkipBlendFn, _SkipBlendF64Fn), without a device: the nodes run on CPU tensors against a library stand-in that records
which entry point is called and answers PDE_OK.  Held here: which route ``_grad_route`` picks from what needs a gradient,
which C calls each route makes, what the node saves (nothing of the input's size when frozen), which gradients come back,
that ``checkpoints`` and the coefficient maxima play no part on the frozen route, and that ``PDE_BWD_INPUT=0`` restores
the full calls.  The numbers the stand-in leaves behind mean nothing; tests/test_gpu_backward_input_mixed.py holds the bits."""
import contextlib

import pytest
import torch


class FakeLib:
    """Every ``pde_*`` entry point: records its name; a size query answers 256, anything else PDE_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("pde_"):
            raise AttributeError(name)

        def fn(*a):
            self.calls.append(name)
            return 256 if name.endswith("_bytes") else 0
        return fn

    def take(self):
        got, self.calls = [c for c in self.calls if not c.endswith("_bytes")], []
        return got


@pytest.fixture
def fake(monkeypatch):
    import cnn_with_pde_amd.functional as F
    from cnn_with_pde_amd import _lib as L
    lib = FakeLib()
    monkeypatch.setattr(L, "load", lambda: lib)
    monkeypatch.setattr(L, "_host", False)
    monkeypatch.setattr(L, "_bwd_input", True)
    monkeypatch.setattr(F, "_require_cuda", lambda *ts: None)
    monkeypatch.setattr(F, "_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    return lib


def test_grad_route():
    import cnn_with_pde_amd.functional as F
    from cnn_with_pde_amd import _lib as L
    old = L._bwd_input
    try:
        L._bwd_input = True
        assert [F._grad_route(u, p) for u, p in ((False, False), (True, False), (False, True), (True, True))] == \
            ["none", "input_only", "full", "full"]
        L._bwd_input = False
        assert F._grad_route(True, False) == "full" and F._grad_route(False, False) == "none"
    finally:
        L._bwd_input = old
    assert F._want_kmax("input_only", "auto", None) is False and F._want_kmax("input_only", 0, []) is True
    assert F._want_kmax("full", "auto", None) is True and F._want_kmax("none", "auto", []) is False


def _mixed_args(frozen, need_u=True, m_grad=None, K=2):
    import cnn_with_pde_amd as P
    B, Cc, N = 2, 5, 8
    u = torch.randn(B, Cc, N, N).requires_grad_(need_u)
    ps = [torch.rand(Cc, N, N).requires_grad_(not frozen) for _ in range(4)]
    M = torch.eye(Cc).requires_grad_((not frozen) if m_grad is None else m_grad)
    return u, ps, M, tuple(tuple(st) for st in P.adi_schedule(0.02, 1.0, 1.0, K, "strang"))


def _big(y, n):
    return [t for t in y.grad_fn.saved_tensors if t is not None and t.numel() >= n]


@pytest.mark.parametrize("ck", ["auto", 0, 1])
def test_mixed_node_frozen(fake, ck):
    import cnn_with_pde_amd.functional as F
    u, ps, M, steps = _mixed_args(True)
    y = F._AdiMixedFn.apply(u, *ps, M, steps, "pre", False, None, 1e-6, ck, None)
    assert fake.take() == ["pde_adi_mixed_forward_input"]
    assert not _big(y, u.numel()) and [tuple(t.shape) for t in y.grad_fn.saved_tensors] == [(5, 5)]
    (gu,) = torch.autograd.grad(y, u, torch.randn_like(y))
    assert fake.take() == ["pde_adi_mixed_backward_input"] and gu.shape == u.shape


def test_mixed_node_other_routes(fake, monkeypatch):
    import cnn_with_pde_amd.functional as F
    from cnn_with_pde_amd import _lib as L
    # nothing needs a gradient: the forward that keeps nothing, and no node
    u, ps, M, steps = _mixed_args(True, need_u=False)
    y = F._AdiMixedFn.apply(u, *ps, M, steps, "post", False, None, 1e-6, "auto", None)
    assert fake.take() == ["pde_adi_mixed_forward_input"] and y.grad_fn is None
    # a coefficient or the operator needs one: the full calls, states kept
    for kw in (dict(frozen=False), dict(frozen=True, m_grad=True), dict(frozen=False, need_u=False)):
        u, ps, M, steps = _mixed_args(**kw)
        y = F._AdiMixedFn.apply(u, *ps, M, steps, "pre", False, None, 1e-6, 0, None)
        assert fake.take() == ["pde_adi_mixed_forward"], kw
        assert len(_big(y, u.numel())) == 3                   # u, states, y
        wanted = [t for t in (u, *ps, M) if t.requires_grad]
        grads = torch.autograd.grad(y, wanted, torch.randn_like(y))
        assert fake.take() == ["pde_adi_mixed_backward"] and len(grads) == len(wanted)
    # the switch: a frozen call and a call under no_grad are back on the full forward
    monkeypatch.setattr(L, "_bwd_input", False)
    u, ps, M, steps = _mixed_args(True)
    y = F._AdiMixedFn.apply(u, *ps, M, steps, "pre", False, None, 1e-6, 0, None)
    assert fake.take() == ["pde_adi_mixed_forward"] and len(_big(y, u.numel())) == 3
    torch.autograd.grad(y, u, torch.randn_like(y))
    assert fake.take() == ["pde_adi_mixed_backward"]
    with torch.no_grad():
        F._AdiMixedFn.apply(u, *ps, M, steps, "pre", False, None, 1e-6, 0, None)
    assert fake.take() == ["pde_adi_mixed_forward"]


@pytest.mark.parametrize("f64", [False, True])
def test_mix_node(fake, f64):
    import cnn_with_pde_amd.functional as F
    fn, pre = (F._MixF64Fn, "pde_channel_mix_f64_") if f64 else (F._MixFn, "pde_channel_mix_")
    dt = torch.float64 if f64 else torch.float32
    for m_grad, u_grad in ((False, True), (True, True), (True, False)):
        u = torch.randn(2, 5, 8, 8, dtype=dt).requires_grad_(u_grad)
        M = torch.eye(5, dtype=dt).requires_grad_(m_grad)
        y = fn.apply(u, M)
        assert fake.take() == [pre + "forward"]
        assert bool(_big(y, u.numel())) == m_grad
        wanted = [t for t in (u, M) if t.requires_grad]
        got = torch.autograd.grad(y, wanted, torch.randn_like(y))
        assert fake.take() == [pre + ("backward" if m_grad else "backward_input")]
        assert [g.shape for g in got] == [t.shape for t in wanted] and [g.dtype for g in got] == [t.dtype for t in wanted]


@pytest.mark.parametrize("f64", [False, True])
def test_skip_blend_node(fake, f64):
    import cnn_with_pde_amd.functional as F
    fn, pre = (F._SkipBlendF64Fn, "pde_skip_blend_f64_") if f64 else (F._SkipBlendFn, "pde_skip_blend_")
    dt = torch.float64 if f64 else torch.float32
    for w_grad, grads in ((False, (True, True)), (False, (False, True)), (True, (True, True)), (True, (False, False))):
        u0 = torch.randn(2, 5, 8, 8, dtype=dt).requires_grad_(grads[0])
        u = torch.randn(2, 5, 8, 8, dtype=dt).requires_grad_(grads[1])
        w = torch.tensor(0.3, dtype=dt).requires_grad_(w_grad)
        y = fn.apply(u0, u, w)
        assert fake.take() == [pre + "forward"]
        assert bool(_big(y, u.numel())) == w_grad
        wanted = [t for t in (u0, u, w) if t.requires_grad]
        got = torch.autograd.grad(y, wanted, torch.randn_like(y))
        assert fake.take() == [pre + ("backward" if w_grad else "backward_input")]
        assert [g.shape for g in got] == [t.shape for t in wanted] and [g.dtype for g in got] == [t.dtype for t in wanted]


def test_the_switch_keeps_mix_and_blend_on_the_full_calls(fake, monkeypatch):
    import cnn_with_pde_amd.functional as F
    from cnn_with_pde_amd import _lib as L
    monkeypatch.setattr(L, "_bwd_input", False)
    u = torch.randn(2, 5, 8, 8).requires_grad_(True)
    y = F._MixFn.apply(u, torch.eye(5))
    torch.autograd.grad(y, u, torch.randn_like(y))
    assert fake.take() == ["pde_channel_mix_forward", "pde_channel_mix_backward"]
    y = F._SkipBlendFn.apply(u, u.detach().clone(), torch.tensor(0.3))
    torch.autograd.grad(y, u, torch.randn_like(y))
    assert fake.take() == ["pde_skip_blend_forward", "pde_skip_blend_backward"]
