"""The Ruthotto-Haber symmetric layer under CUDA bf16 autocast on the bf16 matrix cores (pde_rh.hip).

The rule of test_gpu_rh_amp.py with r() = round to nearest even to bf16: truth is an fp64 evaluation of autocast's contract
(include/pdecnn.h), every rounding point applied straight-through; the fused path must be within
max(FLOOR_BF16, 2 x e_torch) of it for every output, gradient and running statistic, e_torch being plain
``torch.autocast("cuda", torch.bfloat16)``'s own error against the same truth, measured in the same test
(rel = max |a - t| / max |t|).

FLOOR_BF16 = 8e-3: the largest plain-autocast error over the 14 entry-point cases of the first MI355X run (7.19e-3: gX at
B = 64, D = 128, tanh), rounded up to one significant digit.  Measured there (fused / plain bf16 autocast, each against the
truth): entry points, outputs 0-3.2e-3 / 0-3.9e-3 (the small widths give the truth's own bits on both paths), gX
1.5e-3-5.2e-3 / 2.4e-3-7.2e-3, gK 1.2e-3-3.5e-3 / 3.1e-3-5.7e-3 (the fp32 sum of K's two terms), g_gamma 9.2e-4-7.2e-3 /
1.6e-3-6.8e-3 (the largest fused error: B = 64, D = 128, tanh, with a base; plain 6.7e-3 there), g_beta 1.4e-3-2.5e-3 /
1.9e-3-5.3e-3, running statistics up to 3.3e-5 / 1.1e-4; fused never above 2 x plain.  Modules at D = 192, B = 33
(two steps of dt = 0.5): outputs at most 4.5e-8 on both paths, parameter gradients 1.1e-3-6.7e-3 fused against
1.7e-3-1.2e-2 plain (the largest of each: beta of the HamiltonianBlock's F_Z).
"""
import pytest
import torch

import test_gpu_rh_amp as A
from test_gpu_rh_amp import ACTS, _node_names, quiet, rel

FLOOR_BF16 = 8e-3

BF16 = torch.bfloat16
DIMS = {64: (1, 8), 128: (2, 8), 192: (3, 8), 512: (8, 8), 3072: (3, 32)}     # D = channels x side x side


def _r(x):
    """bf16 rounding (to nearest even), straight-through for autograd."""
    return x + (x.to(BF16).to(x.dtype) - x).detach()


def truth_layer(X, K, gamma, beta, rm, rv, base, scale, act, training, momentum, eps):
    """fp64: out = base + r(scale r(r(act(r(BN(r(r(X) r(K)^T))))) r(K))), running statistics updated in place."""
    X16, K16 = _r(X), _r(K)
    P = _r(X16 @ K16.T)
    if training:
        mu, var = P.mean(0), P.var(0, unbiased=False)
        if rm is not None:
            B = P.shape[0]
            with torch.no_grad():
                rm.mul_(1 - momentum).add_(momentum * mu.detach())
                rv.mul_(1 - momentum).add_(momentum * var.detach() * B / max(B - 1, 1))
    else:
        mu, var = rm, rv
    N = _r(gamma * (P - mu) / torch.sqrt(var + eps) + beta)
    H = _r(ACTS[act](N))
    Q = _r(H @ K16)
    S = _r(scale * Q)
    return S if base is None else base + S


def _perturb(l, seed):
    D = l.feature_dim
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        l.K.weight.add_(0.02 * torch.randn(D, D, generator=g).cuda())
        l.norm.weight.copy_(1 + 0.2 * torch.randn(D, generator=g))
        l.norm.bias.copy_(0.1 * torch.randn(D, generator=g))
        l.norm.running_mean.copy_(0.1 * torch.randn(D, generator=g))
        l.norm.running_var.copy_(0.5 + torch.rand(D, generator=g))
    return l


def _layer(D, act, training, seed):
    import cnn_with_pde_amd as P
    torch.manual_seed(seed)
    return _perturb(P.models.SymmetricLayer(*DIMS[D], act).cuda().train(training), seed)


def _bf16_ran(t):
    return any("SymBf16Fn" in n or "SymLayerBf16Fn" in n for n in _node_names(t))


def _fp32_ran(t):
    return any("SymFn" in n or "SymLayerFn" in n for n in _node_names(t))


def _any_fused(t):
    return _bf16_ran(t) or _fp32_ran(t) or A._fused_ran(t)


def _leaves(mods):
    """fp64 copies of (K, gamma, beta) of every layer, as autograd leaves."""
    return [[p.detach().double().requires_grad_(True) for p in (m.K.weight, m.norm.weight, m.norm.bias)] for m in mods]


def _run_layer(l, X, base, scale, gy, mode):
    """mode: "fused" (functional.sym_layer with a bf16 K16), "torch" (plain bf16 autocast) or "truth" (fp64)."""
    from cnn_with_pde_amd import functional as F_
    rm0, rv0 = l.norm.running_mean.clone(), l.norm.running_var.clone()
    if mode == "truth":
        (K, gm, bt), = _leaves([l])
        Xd = X.double().requires_grad_(True)
        rm, rv = rm0.double(), rv0.double()
        out = truth_layer(Xd, K, gm, bt, rm, rv, None if base is None else base.double(), scale, l.act_name, l.training,
                          l.norm.momentum, l.norm.eps)
        out.backward(gy.double())
        return dict(out=out.detach(), gX=Xd.grad, gK=K.grad, gg=gm.grad, gb=bt.grad, rm=rm, rv=rv)
    Xp = X.clone().requires_grad_(True)
    l.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=BF16):
        if mode == "fused":
            K16 = F_.sym_k16(l.K.weight, BF16)
            assert K16.dtype == BF16 and torch.equal(K16, l.K.weight.detach().to(BF16))
            out = F_.sym_layer(Xp, l.K.weight, l.norm, l.act_name, base=base, scale=scale, K16=K16)
            assert _bf16_ran(out)
        else:
            l.fused = False
            out = l.residual(base, Xp, scale) if base is not None else l(Xp)
            l.fused = True
            assert not _any_fused(out)
    out.backward(gy.to(out.dtype))
    torch.cuda.synchronize()
    res = dict(out=out.detach(), gX=Xp.grad, gK=l.K.weight.grad, gg=l.norm.weight.grad, gb=l.norm.bias.grad,
               rm=l.norm.running_mean.clone(), rv=l.norm.running_var.clone())
    with torch.no_grad():
        l.norm.running_mean.copy_(rm0)
        l.norm.running_var.copy_(rv0)
    return res


def _check(fused, plain, truth, label):
    report = {k: (rel(fused[k], truth[k]), rel(plain[k], truth[k])) for k in truth}
    print(label, {k: f"{a:.2e}/{b:.2e}" for k, (a, b) in report.items()})
    for k in truth:
        assert torch.isfinite(fused[k]).all(), (label, k)
    for k, (ef, et) in report.items():
        assert ef <= max(FLOOR_BF16, 2 * et), (label, k, ef, et)


#        B    D    act       training   edge reached
CASES = [(1, 64, "relu", False),        # one row, split 1
         (5, 64, "identity", True),     # partial 32-row block
         (33, 192, "relu", True),       # two row blocks, split 1, 2 waves
         (64, 128, "tanh", True),       # split 2, the 2-wave limit
         (65, 512, "relu", True),       # first 4-wave size, split 8
         (128, 512, "tanh", True),      # row limit
         (64, 3072, "relu", True)]      # the reference's own shape


def _case_tensors(B, D, with_base):
    g = torch.Generator().manual_seed(B * 7 + D)
    X = torch.randn(B, D, generator=g).cuda()
    base = torch.randn(B, D, generator=g).cuda() if with_base else None
    gy = torch.randn(B, D, generator=g).cuda()
    return X, base, gy


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,act,training", CASES)
@pytest.mark.parametrize("with_base", [True, False])
def test_entry_points_against_truth(B, D, act, training, with_base):
    l = _layer(D, act, training, seed=B + D)
    X, base, gy = _case_tensors(B, D, with_base)
    scale = -0.5 if with_base else -1.0
    fused = _run_layer(l, X, base, scale, gy, "fused")
    assert fused["out"].dtype == (torch.float32 if with_base else BF16)
    assert fused["gK"].dtype == torch.float32 and fused["gX"].dtype == X.dtype
    plain = _run_layer(l, X, base, scale, gy, "torch")
    assert plain["out"].dtype == fused["out"].dtype
    truth = _run_layer(l, X, base, scale, gy, "truth")
    _check(fused, plain, truth, f"B={B} D={D} {act} train={training} base={with_base}")


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,act,with_base", [(33, 192, "relu", True), (128, 512, "tanh", False)])
def test_host_paths_match_bitwise(B, D, act, with_base):
    """The C++ node (host_ext.cpp SymBf16Fn) against its ctypes twin (functional._SymLayerBf16Fn)."""
    from cnn_with_pde_amd import _lib as L
    from cnn_with_pde_amd import functional as F_
    ext = L.host_ext()
    if ext is None:
        pytest.skip("the native host extension is switched off")
    l = _layer(D, act, True, seed=5)
    X, base, gy = _case_tensors(B, D, with_base)
    rm0, rv0 = l.norm.running_mean.clone(), l.norm.running_var.clone()

    def fn(native):
        with torch.no_grad():
            l.norm.running_mean.copy_(rm0)
            l.norm.running_var.copy_(rv0)
        l.zero_grad(set_to_none=True)
        Xp = X.clone().requires_grad_(True)
        bp = None if base is None else base.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF16):
            K16 = F_.sym_k16(l.K.weight, BF16)
            y = F_.sym_layer(Xp, l.K.weight, l.norm, act, base=bp, scale=0.7, K16=K16)
        node = y.grad_fn.next_functions[0][0]
        assert ("SymBf16Fn" in node.name()) == native and ("SymLayerBf16Fn" in node.name()) != native, node.name()
        y.backward(gy.to(y.dtype))
        torch.cuda.synchronize()
        return [K16, y.detach().clone(), Xp.grad, l.K.weight.grad, l.norm.weight.grad, l.norm.bias.grad,
                l.norm.running_mean.clone(), l.norm.running_var.clone(), None if bp is None else bp.grad]

    a = fn(True)
    L._host = False
    try:
        b = fn(False)
    finally:
        L._host = ext
    for i, (s, t) in enumerate(zip(a, b)):
        assert (s is None) == (t is None), i
        if s is not None:
            assert s.dtype == t.dtype and torch.equal(s, t), (i, float((s.float() - t.float()).abs().max()))


# ---- modules at D = 192 (3 x 8 x 8), B = 33 ----
MB, MC, MS = 33, 3, 8


def _module(kind, seed=3):
    import cnn_with_pde_amd as P
    torch.manual_seed(seed)
    if kind == "forward":
        blk = P.models.SymmetricLayer(MC, MS, "relu").cuda().train()
        mods = [blk]
    elif kind == "parabolic":
        blk = quiet(P.models.ParabolicBlock, MC, MS, num_steps=2, dt=0.5).cuda().train()
        mods = [blk.symmetric_layer]
    else:
        blk = quiet(P.models.HamiltonianBlock, MC, MS, num_steps=2, dt=0.5).cuda().train()
        mods = [blk.F_Y, blk.F_Z]
    for i, m in enumerate(mods):
        _perturb(m, seed + i)
    g = torch.Generator().manual_seed(seed)
    Y = torch.randn(MB, MC, MS, MS, generator=g).cuda()
    gy = torch.randn(MB, MC, MS, MS, generator=g).cuda()
    return blk, mods, Y, gy


def _steps(kind, blk, Y, step):
    """The block written out: step(i, base, X, scale) = base + scale * (act(BN(X K_i^T)) K_i), base None = F_sym's sign."""
    if kind == "forward":
        return step(0, None, Y, -1.0)
    if kind == "parabolic":
        for _ in range(blk.num_steps):
            Y = step(0, Y, Y, -blk.dt)
        return Y
    Z = torch.zeros_like(Y)
    for _ in range(blk.num_steps):
        Y = step(0, Y, Z, blk.dt)
        Z = step(1, Z, Y, blk.dt)
    return Y


def _truth_module(kind, blk, mods, Y, gy):
    leaves = _leaves(mods)
    stats = [(m.norm.running_mean.double().clone(), m.norm.running_var.double().clone()) for m in mods]

    def step(i, base, X, scale):
        (K, gm, bt), (rm, rv), m = leaves[i], stats[i], mods[i]
        b2 = None if base is None else base.reshape(X.shape[0], -1)
        return truth_layer(X.reshape(X.shape[0], -1), K, gm, bt, rm, rv, b2, scale, m.act_name, True, m.norm.momentum,
                           m.norm.eps).view_as(X)

    out = _steps(kind, blk, Y.double(), step)
    out.backward(gy.double())
    return out.detach(), [p.grad for ls in leaves for p in ls]


def _plain_module(kind, blk, mods, Y):
    """The reference's own ops (cifar_2version.py:210-258) on the modules' parameters, under the caller's autocast."""
    def step(i, base, X, scale):
        m = mods[i]
        h = m.activation(m.norm(m.K(X.reshape(X.shape[0], -1))))
        f = (-(h @ m.K.weight)).view_as(X)
        return f if base is None else base + scale * (-f)

    return _steps(kind, blk, Y, step)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["forward", "parabolic", "hamiltonian"])
def test_modules_under_bf16_autocast(kind):
    blk, mods, Y, gy = _module(kind)
    params = [p for m in mods for p in (m.K.weight, m.norm.weight, m.norm.bias)]
    stats0 = [(m.norm.running_mean.clone(), m.norm.running_var.clone()) for m in mods]

    def reset(fused):
        for m, (a, b) in zip(mods, stats0):
            m.fused = fused
            with torch.no_grad():
                m.norm.running_mean.copy_(a)
                m.norm.running_var.copy_(b)
        blk.zero_grad(set_to_none=True)

    def run(fused, f=None):
        reset(fused)
        with torch.autocast("cuda", dtype=BF16):
            out = blk(Y) if f is None else f()
        assert _bf16_ran(out) == fused and (fused or not _any_fused(out))
        out.backward(gy.to(out.dtype))
        torch.cuda.synchronize()
        return out.detach(), [p.grad.clone() for p in params]

    of, gf = run(True)
    op, gp = run(False)
    assert of.dtype == op.dtype == (BF16 if kind == "forward" else torch.float32)
    # fused = False is plain torch, bit for bit
    ow, gw = run(False, lambda: _plain_module(kind, blk, mods, Y))
    assert ow.dtype == op.dtype and torch.equal(ow, op)
    for a, b in zip(gw, gp):
        assert torch.equal(a, b)
    reset(True)
    ot, gt = _truth_module(kind, blk, mods, Y, gy)
    fused = {"out": of, **{f"g{i}": t for i, t in enumerate(gf)}}
    plain = {"out": op, **{f"g{i}": t for i, t in enumerate(gp)}}
    truth = {"out": ot, **{f"g{i}": t for i, t in enumerate(gt)}}
    _check(fused, plain, truth, f"{kind} B={MB} D={MC * MS * MS}")


@pytest.mark.gpu
def test_the_other_routes_did_not_move():
    from cnn_with_pde_amd import functional as F_
    l = _layer(192, "relu", True, seed=2)
    X, base, _ = _case_tensors(33, 192, True)
    with torch.autocast("cuda", dtype=torch.float16):
        assert F_.sym_layer_f16_supported(X, l.norm) and not F_.sym_layer_bf16_supported(X, l.norm)
        out = l.residual(base, X, -0.5)
        assert A._fused_ran(out) and not _bf16_ran(out) and not _fp32_ran(out)
        assert F_.sym_k16(l.K.weight).dtype == torch.float16
    assert not F_.sym_layer_f16_supported(X, l.norm) and not F_.sym_layer_bf16_supported(X, l.norm)
    out = l.residual(base, X, -0.5)
    assert _fp32_ran(out) and not _bf16_ran(out) and not A._fused_ran(out)
    with torch.autocast("cuda", dtype=BF16):
        assert F_.sym_layer_bf16_supported(X, l.norm) and not F_.sym_layer_f16_supported(X, l.norm)
        assert not F_.sym_layer_bf16_supported(X.to(BF16), l.norm)
        K16 = F_.sym_k16(l.K.weight, BF16)
        for half in (torch.float16, BF16):
            with pytest.raises(TypeError):
                F_.sym_layer(X.to(half), l.K.weight, l.norm, "relu", K16=K16)
        with pytest.raises(TypeError):
            F_.sym_layer(X, l.K.weight, l.norm, "relu", K16=l.K.weight.detach())          # an fp32 "K16"
    with pytest.raises(TypeError):
        F_.sym_k16(l.K.weight, torch.float32)


@pytest.mark.gpu
def test_graph_capture_replays_the_eager_bits():
    """ParabolicBlock forward + backward under bf16 autocast at D = 64, B = 5, captured; K changed in place; the replay
    equals eager."""
    import cnn_with_pde_amd as P
    torch.manual_seed(21)
    blk = quiet(P.models.ParabolicBlock, 1, 8, num_steps=3, dt=0.5).cuda().train()
    blk.symmetric_layer.norm.track_running_stats = False          # replays must not move state the eager run reads
    blk.symmetric_layer.norm.running_mean = None
    blk.symmetric_layer.norm.running_var = None
    g = torch.Generator().manual_seed(21)
    Y = torch.randn(5, 1, 8, 8, generator=g).cuda()
    gy = torch.randn(5, 1, 8, 8, generator=g).cuda()
    params = list(blk.parameters())
    Ys = Y.clone().requires_grad_(True)

    def fn():
        with torch.autocast("cuda", dtype=BF16):
            out = blk(Ys)
        assert _bf16_ran(out)
        return (out,) + torch.autograd.grad(out, [Ys] + params, gy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fn()
    with torch.no_grad():
        blk.symmetric_layer.K.weight.add_(0.05 * torch.randn(64, 64, generator=g).cuda())
    graph.replay()
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in static]
    ref = [t.detach() for t in fn()]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))
