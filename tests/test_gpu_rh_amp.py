"""The Ruthotto-Haber symmetric layer under CUDA fp16 autocast on the fp16 matrix cores (pde_rh.hip).

Truth is an fp64 evaluation of autocast's contract (include/pdecnn.h): every rounding point r() applied straight-through,
so that autograd gives the gradients autocast's casts pass back.  The fused path must be within
max(FLOOR, 2 x e_torch) of it for every output, gradient and running statistic, e_torch being plain-torch autocast's own
error against the same truth, measured in the same test (rel = max |a - t| / max |t|).

FLOOR = 2e-3, from the first MI355X run.  Measured there (fused / plain autocast, each against the truth): entry points,
12 cases, largest fused error 8.0e-4 (g_gamma, B = 128 tanh; plain 9.1e-4), outputs 3.4e-4-4.9e-4 where plain has the
same, gX 3.5e-4-5.1e-4 (plain 4.3e-4-9.4e-4), gK 2.2e-4-3.9e-4 (plain 4.8e-4-1.1e-3), running statistics 1e-5 (plain
5e-6-1.3e-5); modules: F_sym output 5e-4 on both, the four-step ParabolicBlock's parameter gradients 0.06-0.15 on both
(the straight-through truth does not round gradients; four steps of dt = 0.5 amplify that), HamiltonianBlock 3e-3-0.12
fused against 3e-3-0.16 plain.
"""
import contextlib
import io

import pytest
import torch

FLOOR = 2e-3

ACTS = {"relu": torch.relu, "tanh": torch.tanh, "identity": lambda x: x}


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def _r(x):
    """fp16 rounding, straight-through for autograd."""
    return x + (x.to(torch.float16).to(x.dtype) - x).detach()


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


def rel(a, t):
    return float((a.double() - t.double()).abs().max() / t.double().abs().max().clamp_min(1e-30))


def _dims(D):
    return {3072: (3, 32), 1024: (1, 32), 192: (3, 8), 64: (1, 8)}[D]


def _layer(D, act, training, seed):
    import cnn_with_pde_amd as P
    c, s = _dims(D)
    torch.manual_seed(seed)
    l = P.models.SymmetricLayer(c, s, act).cuda().train(training)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        l.K.weight.add_(0.02 * torch.randn(D, D, generator=g).cuda())
        l.norm.weight.copy_(1 + 0.2 * torch.randn(D, generator=g))
        l.norm.bias.copy_(0.1 * torch.randn(D, generator=g))
        l.norm.running_mean.copy_(0.1 * torch.randn(D, generator=g))
        l.norm.running_var.copy_(0.5 + torch.rand(D, generator=g))
    return l


def _node_names(t):
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        names.append(n.name())
        todo.extend(f for f, _ in n.next_functions)
    return names


def _fused_ran(t):
    return any("SymF16Fn" in n or "SymLayerF16Fn" in n for n in _node_names(t))


def _run_layer(l, X, base, scale, gy, mode):
    """mode: "fused" (functional.sym_layer with K16), "torch" (plain autocast) or "truth" (fp64)."""
    from cnn_with_pde_amd import functional as F_
    D = X.shape[1]
    rm0, rv0 = l.norm.running_mean.clone(), l.norm.running_var.clone()
    if mode == "truth":
        K = l.K.weight.detach().double().requires_grad_(True)
        gm = l.norm.weight.detach().double().requires_grad_(True)
        bt = l.norm.bias.detach().double().requires_grad_(True)
        Xd = X.double().requires_grad_(True)
        rm, rv = rm0.double(), rv0.double()
        out = truth_layer(Xd, K, gm, bt, rm, rv, None if base is None else base.double(), scale, l.act_name, l.training,
                          l.norm.momentum, l.norm.eps)
        out.backward(gy.double())
        return dict(out=out.detach(), gX=Xd.grad, gK=K.grad, gg=gm.grad, gb=bt.grad, rm=rm, rv=rv)
    Xp = X.clone().requires_grad_(True)
    l.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        if mode == "fused":
            out = F_.sym_layer(Xp, l.K.weight, l.norm, l.act_name, base=base, scale=scale, K16=F_.sym_k16(l.K.weight))
            assert _fused_ran(out)
        else:
            l.fused = False
            out = l.residual(base, Xp, scale) if base is not None else l(Xp)
            l.fused = True
            assert not _fused_ran(out)
    out.backward(gy.to(out.dtype))
    torch.cuda.synchronize()
    res = dict(out=out.detach(), gX=Xp.grad, gK=l.K.weight.grad, gg=l.norm.weight.grad, gb=l.norm.bias.grad,
               rm=l.norm.running_mean.clone(), rv=l.norm.running_var.clone())
    with torch.no_grad():
        l.norm.running_mean.copy_(rm0)
        l.norm.running_var.copy_(rv0)
    return res


CASES = [(64, 3072, "relu", True), (128, 3072, "tanh", True), (33, 192, "relu", True), (5, 64, "identity", True),
         (1, 64, "relu", False), (100, 1024, "relu", False)]


def _check(fused, plain, truth, label):
    report = {}
    for k in truth:
        ef, et = rel(fused[k], truth[k]), rel(plain[k], truth[k])
        report[k] = (ef, et)
        assert torch.isfinite(fused[k]).all(), (label, k)
    print(label, {k: f"{a:.2e}/{b:.2e}" for k, (a, b) in report.items()})
    for k, (ef, et) in report.items():
        assert ef <= max(FLOOR, 2 * et), (label, k, ef, et)
    return report


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,act,training", CASES)
@pytest.mark.parametrize("with_base", [True, False])
def test_entry_points_against_truth(B, D, act, training, with_base):
    l = _layer(D, act, training, seed=B + D)
    g = torch.Generator().manual_seed(B * 7 + D)
    X = torch.randn(B, D, generator=g).cuda()
    base = torch.randn(B, D, generator=g).cuda() if with_base else None
    gy = torch.randn(B, D, generator=g).cuda()
    scale = -0.5 if with_base else -1.0
    fused = _run_layer(l, X, base, scale, gy, "fused")
    assert fused["out"].dtype == (torch.float32 if with_base else torch.float16)
    plain = _run_layer(l, X, base, scale, gy, "torch")
    assert plain["out"].dtype == fused["out"].dtype
    truth = _run_layer(l, X, base, scale, gy, "truth")
    _check(fused, plain, truth, f"B={B} D={D} {act} train={training} base={with_base}")


def _truth_block(kind, mods, Y, gy):
    """fp64 evaluation of a block under the contract; returns the output and the parameter gradients."""
    ps = []
    layers = []
    for m in mods:
        K = m.K.weight.detach().double().requires_grad_(True)
        gm = m.norm.weight.detach().double().requires_grad_(True)
        bt = m.norm.bias.detach().double().requires_grad_(True)
        rm, rv = m.norm.running_mean.detach().double().clone(), m.norm.running_var.detach().double().clone()
        ps += [K, gm, bt]
        layers.append((K, gm, bt, rm, rv, m))

    def step(i, base, X, scale):
        K, gm, bt, rm, rv, m = layers[i]
        return truth_layer(X.reshape(X.shape[0], -1), K, gm, bt, rm, rv, base.reshape(X.shape[0], -1), scale, m.act_name,
                           m.training, m.norm.momentum, m.norm.eps).view_as(X)

    Yd = Y.double()
    if kind == "parabolic":
        blk = mods[0]._blk
        for _ in range(blk.num_steps):
            Yd = step(0, Yd, Yd, -blk.dt)
    else:
        blk = mods[0]._blk
        Z = torch.zeros_like(Yd)
        for _ in range(blk.num_steps):
            Yd = step(0, Yd, Z, blk.dt)
            Z = step(1, Z, Yd, blk.dt)
    Yd.backward(gy.double())
    return Yd.detach(), [p.grad for p in ps]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [64, 128])
@pytest.mark.parametrize("kind", ["forward", "parabolic", "hamiltonian"])
def test_modules_under_autocast(kind, B):
    import cnn_with_pde_amd as P
    torch.manual_seed(B)
    if kind == "forward":
        blk = _layer(3072, "relu", True, seed=B)
        mods = [blk]
    elif kind == "parabolic":
        blk = quiet(P.models.ParabolicBlock, 3, 32, num_steps=4, dt=0.5).cuda().train()
        mods = [blk.symmetric_layer]
    else:
        blk = quiet(P.models.HamiltonianBlock, 3, 32, num_steps=3, dt=0.8).cuda().train()
        mods = [blk.F_Y, blk.F_Z]
    for m in mods:
        m._blk = blk
    g = torch.Generator().manual_seed(3 * B)
    Y = torch.randn(B, 3, 32, 32, generator=g).cuda()
    gy = torch.randn(B, 3, 32, 32, generator=g).cuda()
    params = [p for m in mods for p in (m.K.weight, m.norm.weight, m.norm.bias)]
    stats0 = [(m.norm.running_mean.clone(), m.norm.running_var.clone()) for m in mods]

    def run(fused):
        for m, (a, b) in zip(mods, stats0):
            m.fused = fused
            with torch.no_grad():
                m.norm.running_mean.copy_(a)
                m.norm.running_var.copy_(b)
        blk.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = blk(Y)
        assert _fused_ran(out) == fused
        out.backward(gy.to(out.dtype))
        torch.cuda.synchronize()
        return out.detach(), [p.grad.clone() for p in params]

    of, gf = run(True)
    op, gp = run(False)
    assert of.dtype == op.dtype == (torch.float16 if kind == "forward" else torch.float32)
    for m, (a, b) in zip(mods, stats0):
        m.fused = True
        with torch.no_grad():
            m.norm.running_mean.copy_(a)
            m.norm.running_var.copy_(b)
    if kind == "forward":
        ot, gt = _truth_forward(blk, Y, gy)
    else:
        ot, gt = _truth_block(kind, mods, Y, gy)
    fused = {"out": of, **{f"g{i}": t for i, t in enumerate(gf)}}
    plain = {"out": op, **{f"g{i}": t for i, t in enumerate(gp)}}
    truth = {"out": ot, **{f"g{i}": t for i, t in enumerate(gt)}}
    _check(fused, plain, truth, f"{kind} B={B}")


def _truth_forward(l, Y, gy):
    K = l.K.weight.detach().double().requires_grad_(True)
    gm = l.norm.weight.detach().double().requires_grad_(True)
    bt = l.norm.bias.detach().double().requires_grad_(True)
    rm, rv = l.norm.running_mean.double().clone(), l.norm.running_var.double().clone()
    out = truth_layer(Y.double().reshape(Y.shape[0], -1), K, gm, bt, rm, rv, None, -1.0, l.act_name, True,
                      l.norm.momentum, l.norm.eps).view_as(Y)
    out.backward(gy.double())
    return out.detach(), [K.grad, gm.grad, bt.grad]


@pytest.mark.gpu
@pytest.mark.parametrize("with_base", [True, False])
def test_host_paths_match_bitwise(with_base):
    """The C++ node (host_ext.cpp SymF16Fn) against its ctypes twin (functional._SymLayerF16Fn)."""
    from cnn_with_pde_amd import _lib as L
    from cnn_with_pde_amd import functional as F_
    B, D = 64, 3072
    l = _layer(D, "tanh", True, seed=5)
    g = torch.Generator().manual_seed(5)
    X = torch.randn(B, D, generator=g).cuda()
    base = torch.randn(B, D, generator=g).cuda() if with_base else None
    gy = torch.randn(B, D, generator=g).cuda()
    rm0, rv0 = l.norm.running_mean.clone(), l.norm.running_var.clone()

    def fn(native):
        with torch.no_grad():
            l.norm.running_mean.copy_(rm0)
            l.norm.running_var.copy_(rv0)
        l.zero_grad(set_to_none=True)
        Xp = X.clone().requires_grad_(True)
        bp = None if base is None else base.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            K16 = F_.sym_k16(l.K.weight)
            y = F_.sym_layer(Xp, l.K.weight, l.norm, "tanh", base=bp, scale=0.7, K16=K16)
        node = y.grad_fn.next_functions[0][0]
        assert ("SymF16Fn" in node.name()) == native and ("SymLayerF16Fn" in node.name()) != native, node.name()
        y.backward(gy.to(y.dtype))
        torch.cuda.synchronize()
        return [K16, y.detach().clone(), Xp.grad, l.K.weight.grad, l.norm.weight.grad, l.norm.bias.grad,
                l.norm.running_mean.clone(), l.norm.running_var.clone(), None if bp is None else bp.grad]

    ext = L.host_ext()
    assert ext is not None
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


@pytest.mark.gpu
def test_deterministic():
    from cnn_with_pde_amd import functional as F_
    B, D = 128, 3072
    l = _layer(D, "relu", True, seed=9)
    g = torch.Generator().manual_seed(9)
    X = torch.randn(B, D, generator=g).cuda()
    gy = torch.randn(B, D, generator=g).cuda()

    def once():
        l.zero_grad(set_to_none=True)
        Xp = X.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = F_.sym_layer(Xp, l.K.weight, l.norm, "relu", base=Xp, scale=-0.5, K16=F_.sym_k16(l.K.weight))
        y.backward(gy)
        torch.cuda.synchronize()
        return [y.detach().clone(), Xp.grad, l.K.weight.grad.clone(), l.norm.weight.grad.clone(), l.norm.bias.grad.clone()]

    for s, t in zip(once(), once()):
        assert torch.equal(s, t)


@pytest.mark.gpu
def test_grad_scaler_overflow_in_gQ_skips_the_step_on_both_paths():
    """A loss scale whose gradient is finite in fp16 (gS) but overflows once multiplied by the step (gQ = r(2 gS))."""
    B, D = 64, 3072
    g = torch.Generator().manual_seed(11)
    X = torch.randn(B, D, generator=g).cuda()
    for fused in (True, False):
        l = _layer(D, "relu", True, seed=11)
        l.fused = fused
        opt = torch.optim.SGD(l.parameters(), lr=0.1)
        scaler = torch.amp.GradScaler("cuda", init_scale=40000.0)
        before = [p.detach().clone() for p in l.parameters()]
        with torch.autocast("cuda", dtype=torch.float16):
            out = l.residual(X, X, 2.0)
            assert _fused_ran(out) == fused
            loss = out.float().sum()
        scaler.scale(loss).backward()
        assert not torch.isfinite(l.K.weight.grad).all(), fused
        scaler.step(opt)
        scaler.update()
        assert scaler.get_scale() < 40000.0, fused
        for p, q in zip(l.parameters(), before):
            assert torch.equal(p.detach(), q), fused


@pytest.mark.gpu
def test_graph_capture_sees_a_changed_K():
    """ParabolicBlock forward + backward under autocast, captured; K changed in place; the replay equals eager."""
    import cnn_with_pde_amd as P
    torch.manual_seed(21)
    blk = quiet(P.models.ParabolicBlock, 3, 32, num_steps=4, dt=0.5).cuda().train()
    blk.symmetric_layer.norm.track_running_stats = False          # replays must not move state the eager run reads
    blk.symmetric_layer.norm.running_mean = None
    blk.symmetric_layer.norm.running_var = None
    g = torch.Generator().manual_seed(21)
    Y = torch.randn(64, 3, 32, 32, generator=g).cuda()
    gy = torch.randn(64, 3, 32, 32, generator=g).cuda()
    params = list(blk.parameters())
    Ys = Y.clone().requires_grad_(True)

    def fn():
        with torch.autocast("cuda", dtype=torch.float16):
            out = blk(Ys)
        assert _fused_ran(out)
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
        blk.symmetric_layer.K.weight.add_(0.05 * torch.randn(3072, 3072, generator=g).cuda())
    graph.replay()
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in static]
    ref = [t.detach() for t in fn()]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))


@pytest.mark.gpu
def test_hybrid_model_trains_under_amp():
    """CIFAR10HybridPDEModel: 60 AdamW steps with GradScaler and fp16 autocast on a fixed batch, the fused fp16 path
    in every symmetric layer."""
    import cnn_with_pde_amd as P
    torch.manual_seed(0)
    model = quiet(P.CIFAR10HybridPDEModel).cuda().train()
    x = torch.randn(32, 3, 32, 32, device="cuda")
    target = torch.randint(0, 10, (32,), device="cuda")
    names = [n for n, _ in model.named_parameters() if ("parabolic" in n or "hamiltonian" in n)
             and ("K.weight" in n or "norm." in n)]
    assert len(names) == 9
    before = {n: p.detach().clone() for n, p in model.named_parameters() if n in names}
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=1e-4)
    scaler = torch.amp.GradScaler("cuda")
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    losses = []
    for i in range(60):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = model(x)
            loss = crit(out, target)
        if i == 0:
            assert _fused_ran(loss)
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss.detach()))
    assert all(l == l for l in losses), losses
    assert min(losses[-5:]) < 0.7 * losses[0], (losses[0], losses[-5:])
    for n, p in model.named_parameters():
        if n in names:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
            assert not torch.equal(p.detach(), before[n]), n
