"""float64 end to end: a float64 input or parameter runs every PDE layer in double (the pde_*_f64_* entry points), as the
reference's plain-torch layers do.  Gates: the reference's own float64 vectors and the float64 CPU oracle at 1e-11
(relative max-norm), torch.autograd.gradcheck against finite differences, dtype rules, models, determinism."""
import contextlib
import io

import pytest
import torch

import golden_util as G
from oracle import pde_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-11


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _check(layer, u, gy, y, ref, tol=TOL):
    """y and every gradient of the (already run backward) layer against (y_ref, gu_ref, {name: grad})."""
    y_ref, gu_ref, gp_ref = ref
    errs = {"y": G.rel_err(y.detach().cpu(), y_ref), "gu": G.rel_err(u.grad.cpu(), gu_ref)}
    for n, p in layer.named_parameters():
        if n in gp_ref and gp_ref[n] is not None:
            errs["g_" + n] = G.rel_err(p.grad.cpu(), gp_ref[n])
    bad = {k: v for k, v in errs.items() if not v <= tol}
    assert not bad, (bad, errs)


# ---- 1. the reference's own float64 vectors ------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.names(f64=True))
def test_f64_layer_matches_reference_vectors(name):
    import cnn_with_pde_amd as P
    g = G.Golden(name)
    # the vectors were made under a float64 default dtype (tools/make_golden.py): buffers such as the emotion layer's
    # coordinate grids are then float64 from the start, not float32 grids widened
    torch.set_default_dtype(torch.float64)
    try:
        layer = quiet(P.REFERENCE_CLASSES[(g.script, g.cls)], **g.ctor).double()
    finally:
        torch.set_default_dtype(torch.float32)
    missing = layer.load_state_dict({k: v.double() for k, v in g.params.items()}, strict=False)
    assert not missing.unexpected_keys and all(k in ("x", "y") for k in missing.missing_keys), missing
    layer = layer.cuda()
    u = g.u.double().cuda().requires_grad_(True)
    y = layer(u)
    assert y.dtype == torch.float64 and y.shape == g.y.shape
    y.backward(g.gy.double().cuda())
    torch.cuda.synchronize()
    errs = {"y": G.rel_err(y.detach().cpu(), g.y), "gu": G.rel_err(u.grad.cpu(), g.gu)}
    for n, p in layer.named_parameters():
        if g.grad_is_none[n]:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
            continue
        assert p.grad.dtype == torch.float64
        errs["g_" + n] = G.rel_err(p.grad.cpu(), g.grads[n])
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, (bad, errs)


# ---- 2. against the float64 oracle ---------------------------------------------------------------------------------
def _perturb(layer, gen, rel=0.15, slope=0.0):
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if n in ("alpha_base", "beta_base"):
                p.mul_(1 + rel * torch.randn(p.shape, generator=gen, dtype=p.dtype))
            elif n in ("alpha_time_coeff", "beta_time_coeff"):
                p.copy_(slope * torch.randn(p.shape, generator=gen, dtype=p.dtype))
            elif n in ("channel_mixing", "channel_coupling"):
                p.add_(0.05 * torch.randn(p.shape, generator=gen, dtype=p.dtype))


def _vs_oracle(layer, spec, B, seed=0, u=None, policy=None):
    gen = torch.Generator().manual_seed(seed)
    Cc, N = spec.channels, spec.size
    if u is None:
        u = torch.randn(B, Cc, N, N, generator=gen, dtype=torch.float64)
    gy = torch.randn(u.shape, generator=gen, dtype=torch.float64)
    params = {k: v.detach().clone() for k, v in layer.named_parameters()}
    ref = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec), u, params, gy)
    layer = layer.cuda()
    layer.zero_grad(set_to_none=True)
    if policy is not None:
        layer.checkpoint_policy = policy
    ud = u.cuda().requires_grad_(True)
    y = layer(ud)
    assert y.dtype == torch.float64
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    _check(layer, ud, gy, y, ref)
    return layer


def _make(kind, N, Cc=2, steps=2, seed=1):
    import cnn_with_pde_amd as P
    gen = torch.Generator().manual_seed(seed)
    if kind == "mnist":
        layer, spec = quiet(P.MnistDiffusionLayer, size=N, num_steps=steps), O.mnist_spec(size=N, num_steps=steps)
    elif kind == "cifar10":
        layer, spec = (quiet(P.EnhancedDiffusionLayer, size=N, channels=Cc, num_steps=steps),
                       O.cifar10_spec(size=N, channels=Cc, num_steps=steps))
    elif kind == "cifar2":
        layer, spec = (quiet(P.LearnableDiffusionLayer, size=N, channels=Cc, num_steps=steps),
                       O.cifar2_spec(size=N, channels=Cc, num_steps=steps))
    else:
        layer, spec = (quiet(P.SvhnDiffusionLayer, size=N, channels=Cc, num_steps=steps),
                       O.svhn_spec(size=N, channels=Cc, num_steps=steps))
    layer = layer.double()
    _perturb(layer, gen, slope=0.5)
    return layer, spec


@pytest.mark.parametrize("N", [2, 3, 6, 8, 12, 28, 30, 32, 36, 64, 100, 128])
@pytest.mark.parametrize("kind", ["mnist", "cifar10", "cifar2"])
def test_f64_layers_vs_oracle_any_n(kind, N):
    layer, spec = _make(kind, N)
    _vs_oracle(layer, spec, B=2)


@pytest.mark.parametrize("Cc,N,B", [(4, 16, 3), (128, 8, 2)])
def test_f64_svhn_coupling_and_skip_vs_oracle(Cc, N, B):
    layer, spec = _make("svhn", N, Cc=Cc)
    with torch.no_grad():
        layer.skip_weight.fill_(0.3)
    _vs_oracle(layer, spec, B=B)


@pytest.mark.parametrize("policy", ["auto", "lagged", 0, "all", "mixed"])
@pytest.mark.parametrize("kind", ["mnist", "cifar10"])
def test_f64_checkpoint_policies(kind, policy):
    layer, spec = _make(kind, 12, steps=3)
    with torch.no_grad():                                    # fashion-like coefficients: rebuilt states amplify rounding
        layer.alpha_base.mul_(200.0)
        layer.beta_base.mul_(200.0)
    per_step = kind == "cifar10"                             # with a channel operator masks are step-local
    S = 3 if per_step else 9
    if policy == "all":
        policy = (1 << (S - 1)) - 1
    elif policy == "mixed":
        policy = 0b01 if per_step else 0b10100101
    _vs_oracle(layer, spec, B=3, policy=policy)
    if policy == "lagged":                                   # second call: the plan from the first call's coefficients
        _vs_oracle(layer.cpu(), spec, B=3, seed=5, policy=policy)


def test_f64_empty_batch_and_noncontiguous_input():
    layer, spec = _make("cifar10", 8)
    layer = layer.cuda()
    e = torch.empty(0, 2, 8, 8, dtype=torch.float64, device="cuda", requires_grad=True)
    y = layer(e)
    assert y.dtype == torch.float64 and y.shape == e.shape
    y.sum().backward()
    gen = torch.Generator().manual_seed(3)
    base = torch.randn(2, 8, 8, 4, generator=gen, dtype=torch.float64)
    u = base.permute(0, 3, 1, 2)[:, 1:3]                     # (2, 2, 8, 8), not contiguous
    assert not u.is_contiguous()
    _vs_oracle(layer.cpu(), spec, B=2, u=u)


# ---- 3. gradcheck against finite differences -----------------------------------------------------------------------
def _gradcheck_layers():
    import cnn_with_pde_amd as P
    return {
        "mnist": (lambda: P.MnistDiffusionLayer(size=6, num_steps=2), (2, 1, 6, 6)),
        "fashion": (lambda: P.FashionDiffusionLayer(size=6, num_steps=2), (2, 1, 6, 6)),
        "svhn": (lambda: P.SvhnDiffusionLayer(size=6, channels=2, num_steps=2), (2, 2, 6, 6)),
        "cifar10": (lambda: P.EnhancedDiffusionLayer(size=7, channels=3, num_steps=2), (2, 3, 7, 7)),
        "cifar2": (lambda: P.LearnableDiffusionLayer(size=6, channels=2, num_steps=2), (2, 2, 6, 6)),
        "tiny": (lambda: P.ImprovedDiffusionLayer(size=8, channels=2, num_steps=2), (2, 2, 8, 8)),
        "emotion": (lambda: P.PDELayer(Nx=8, Ny=8, T=0.002, dt=0.001), (2, 1, 8, 8)),
    }


@pytest.mark.parametrize("kind", ["mnist", "fashion", "svhn", "cifar10", "cifar2", "tiny", "emotion"])
def test_f64_gradcheck(kind):
    make, shape = _gradcheck_layers()[kind]
    gen = torch.Generator().manual_seed(11)
    layer = quiet(make).double()
    with torch.no_grad():                                    # generic parameters, away from the clamp kinks
        for n, p in layer.named_parameters():
            if n in ("alpha_time_coeff", "beta_time_coeff"):
                p.copy_(0.3 * torch.randn(p.shape, generator=gen, dtype=p.dtype))
            elif n in ("channel_mixing", "channel_coupling"):
                p.add_(0.1 * torch.randn(p.shape, generator=gen, dtype=p.dtype))
            elif n in ("alpha_base", "beta_base") and p.dim() >= 2:
                p.mul_(1 + 0.1 * torch.randn(p.shape, generator=gen, dtype=p.dtype))
    layer = layer.cuda()
    u = torch.randn(shape, generator=gen, dtype=torch.float64).cuda().requires_grad_(True)
    params = [p for n, p in layer.named_parameters() if not (kind == "tiny" and n == "beta_base")]   # unused there
    assert torch.autograd.gradcheck(lambda x, *ps: layer(x), (u, *params))


# ---- 4. mixed dtypes, autocast -------------------------------------------------------------------------------------
def test_f64_mixed_dtypes():
    layer, spec = _make("cifar10", 12)
    gen = torch.Generator().manual_seed(4)
    u32 = torch.randn(2, 2, 12, 12, generator=gen)
    gy = torch.randn(2, 2, 12, 12, generator=gen, dtype=torch.float64)
    # float32 input into a float64 layer
    params = {k: v.detach().clone() for k, v in layer.named_parameters()}
    ref = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec), u32.double(), params, gy)
    d = layer.cuda()
    ud = u32.cuda().requires_grad_(True)
    y = d(ud)
    assert y.dtype == torch.float64
    y.backward(gy.cuda())
    assert ud.grad.dtype == torch.float32 and all(p.grad.dtype == torch.float64 for p in d.parameters())
    errs = [G.rel_err(y.detach().cpu(), ref[0])] + [G.rel_err(p.grad.cpu(), ref[2][n]) for n, p in d.named_parameters()]
    assert max(errs) <= TOL, errs
    assert G.rel_err(ud.grad.cpu(), ref[1]) <= 1e-7                    # the float64 gradient rounded to float32
    # float64 input into a float32 layer
    l32 = layer.float().cpu()
    l32.zero_grad(set_to_none=True)
    params = {k: v.detach().double() for k, v in l32.named_parameters()}
    u64 = u32.double()
    ref = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec), u64, params, gy)
    d = l32.cuda()
    ud = u64.cuda().requires_grad_(True)
    y = d(ud)
    assert y.dtype == torch.float64
    y.backward(gy.cuda())
    assert ud.grad.dtype == torch.float64 and all(p.grad.dtype == torch.float32 for p in d.parameters())
    assert G.rel_err(y.detach().cpu(), ref[0]) <= TOL and G.rel_err(ud.grad.cpu(), ref[1]) <= TOL
    for n, p in d.named_parameters():
        assert G.rel_err(p.grad.cpu(), ref[2][n]) <= 1e-7, n


@pytest.mark.parametrize("kind", ["mnist", "svhn"])
def test_f64_inside_fp16_autocast(kind):
    layer, _ = _make(kind, 8)
    layer = layer.cuda()
    u = torch.randn(2, layer.alpha_base.shape[0] if layer.alpha_base.dim() == 3 else 1, 8, 8, dtype=torch.float64,
                    device="cuda", requires_grad=True)
    with torch.autocast("cuda", torch.float16):
        y = layer(u)
    assert y.dtype == torch.float64
    y.sum().backward()
    assert u.grad.dtype == torch.float64


# ---- 5. models -----------------------------------------------------------------------------------------------------
def _models():
    import cnn_with_pde_amd as P
    return {
        "mnist": (P.MnistPDEClassifier, (4, 1, 28, 28)),
        "fashion": (P.FashionPDEClassifier, (4, 1, 28, 28)),
        "svhn": (P.SvhnPDEClassifier, (4, 3, 32, 32)),
        "cifar10_noconv": (P.CIFAR10PDENoConv, (4, 3, 32, 32)),
        "cifar10_hybrid": (P.CIFAR10HybridPDEModel, (4, 3, 32, 32)),
        "tiny": (P.TinyImageNetClassifier, (4, 3, 64, 64)),
        "emotion": (P.EmotionDiffusionClassifier, (4, 1, 48, 48)),
    }


@pytest.mark.parametrize("name", ["mnist", "fashion", "svhn", "cifar10_noconv", "cifar10_hybrid", "tiny", "emotion"])
def test_f64_models_train_step(name):
    cls, shape = _models()[name]
    torch.manual_seed(0)
    model = quiet(cls).double().cuda().train()
    x = torch.randn(shape, dtype=torch.float64, device="cuda")
    out = model(x)
    logits = out[0] if isinstance(out, (tuple, list)) else out
    assert logits.dtype == torch.float64
    logits.logsumexp(dim=1).sum().backward()
    for n, p in model.named_parameters():
        if p.grad is not None:
            assert p.grad.dtype == torch.float64 and bool(torch.isfinite(p.grad).all()), n


@pytest.mark.parametrize("name", [n for n in G.names(directory=G.MODEL_DIR) if n.startswith("model_cifar10_")])
def test_f64_models_match_reference_vectors(name):
    import cnn_with_pde_amd as P
    g = G.Golden(name, G.MODEL_DIR)
    model = quiet(P.REFERENCE_CLASSES[(g.script, g.cls)], **g.ctor).double()
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in g.params.items()}
    sd.update({k: (v.double() if v.is_floating_point() else v) for k, v in g.bufin.items()})
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys, missing
    model = model.cuda().train(name.endswith("_train"))
    u = g.u.double().cuda().requires_grad_(True)
    out = model(u)
    y = out[0] if isinstance(out, (tuple, list)) else out
    assert y.dtype == torch.float64
    y.backward(g.gy.double().cuda())
    torch.cuda.synchronize()
    gmax = max(float(v.abs().max()) for v in g.grads.values())

    def rel(a, b):
        return float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-2 * gmax)
    errs = {"y": G.rel_err(y.detach().cpu(), g.y), "gu": G.rel_err(u.grad.cpu(), g.gu)}
    for n, p in model.named_parameters():
        if g.grad_is_none[n]:
            continue
        errs["g_" + n] = rel(p.grad.cpu(), g.grads[n])
    tol = 2e-4 if name == "model_cifar10_noconv_train" else 1e-5          # as tests/test_gpu_models.py holds float32
    bad = {k: v for k, v in errs.items() if not v <= (max(tol, 1e-4) if k == "g_combine_weights" else tol)}
    assert not bad, (bad, errs)


# ---- 6. determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mnist", "svhn", "cifar10", "tiny", "emotion"])
def test_f64_bitwise_repeatable(kind):
    make, shape = _gradcheck_layers()[kind]
    layer = quiet(make).double().cuda()
    gen = torch.Generator().manual_seed(2)
    u0 = torch.randn((16,) + shape[1:], generator=gen, dtype=torch.float64).cuda()
    gy = torch.randn(u0.shape, generator=gen, dtype=torch.float64).cuda()
    runs = []
    for _ in range(2):
        layer.zero_grad(set_to_none=True)
        u = u0.clone().requires_grad_(True)
        y = layer(u)
        y.backward(gy)
        torch.cuda.synchronize()
        runs.append([y.detach().clone(), u.grad.clone()] + [p.grad.clone() for p in layer.parameters() if p.grad is not None])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
