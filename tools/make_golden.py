#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE layer classes (build
container only; needs /root/reference).  TEST INFRASTRUCTURE.

Each fixture is data only: the layer's constructor arguments, its parameters,
a seeded input ``u``, an upstream gradient ``gy``, and what the reference
returned: ``y``, ``gu`` and one gradient per parameter.  Nothing of the
reference's source is stored.

    python tools/make_golden.py            # rewrite every fixture
    python tools/make_golden.py rect       # only tests/golden/rect/ (the layer classes on rectangular planes)
"""
import json
import os
import sys

# MKL's reproducible mode, as tests/conftest.py runs the oracle (the products' rounding then does not depend on the CPU);
# set before torch loads MKL.  The thread count is pinned in main().
os.environ["MKL_CBWR"] = "COMPATIBLE"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")


def _run(layer, u, gy):
    u = u.clone().requires_grad_(True)
    y = layer(u)
    names = [n for n, _ in layer.named_parameters()]
    ps = [p for _, p in layer.named_parameters()]
    grads = torch.autograd.grad(y, [u] + ps, gy, allow_unused=True)
    out = {"y": y.detach(), "gu": grads[0]}
    for n, g in zip(names, grads[1:]):
        out["grad_" + n] = torch.zeros(()) if g is None else g
        out["gradnone_" + n] = torch.tensor(g is None)
    return out


def _save(name, script, cls, ctor, layer, u, gy, dtype, extra_meta=None):
    bufin = {"bufin_" + n: b.detach().clone() for n, b in layer.named_buffers()} if getattr(layer, "keep_buffers", False) else {}
    res = _run(layer, u, gy)
    blob = {"u": u, "gy": gy}
    blob.update(bufin)
    if bufin:                                            # what one training-mode forward left in the buffers
        blob.update({"bufout_" + n: b.detach().clone() for n, b in layer.named_buffers()})
    for n, p in layer.named_parameters():
        blob["param_" + n] = p.detach()
    blob.update(res)
    arrays = {k: v.detach().cpu().numpy() for k, v in blob.items()}
    meta = {"script": script, "cls": cls, "ctor": ctor, "dtype": str(dtype).replace("torch.", "")}
    meta.update(extra_meta or {})
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name:40s} {os.path.getsize(path) / 1024:8.1f} KiB  |y|max={float(res['y'].abs().max()):.4g}")


def _perturb(layer, g, rel=0.1, slope=0.0, dtype=torch.float32):
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if n in ("alpha_base", "beta_base"):
                p.mul_(1 + rel * torch.randn(p.shape, generator=g, dtype=dtype))
            elif n in ("alpha_time_coeff", "beta_time_coeff"):
                p.copy_(slope * torch.randn(p.shape, generator=g, dtype=dtype))


def make(name, script, cls, ctor, B, seed, dtype=torch.float32, tweak=None, u_fn=None):
    mod = ref_loader.load(script)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)  # constructors call torch.randn (cifar10.py:44, SVHN.py:26-27)
    # fp64 fixtures: run the reference under a float64 default dtype, because its
    # smoothing kernel is built with torch.ones(...) at the default dtype
    # (mnist_test.py:144) and cannot follow layer.double().
    torch.set_default_dtype(dtype)
    try:
        _make(name, script, cls, ctor, B, g, dtype, tweak, u_fn, mod)
    finally:
        torch.set_default_dtype(torch.float32)


def _make(name, script, cls, ctor, B, g, dtype, tweak, u_fn, mod):
    with ref_loader.quiet():
        layer = getattr(mod, cls)(**ctor)
    if tweak is not None:
        tweak(layer, g)
    if hasattr(layer, "channels"):
        C = layer.channels
    else:
        C = 1
    N = ctor.get("size", ctor.get("Nx", getattr(layer, "size", getattr(layer, "Nx", None))))
    u = torch.randn(B, C, N, N, generator=g, dtype=dtype)
    if u_fn is not None:
        u = u_fn(u)
    gy = torch.randn(B, C, N, N, generator=g, dtype=dtype)
    _save(name, script, cls, ctor, layer, u, gy, dtype)


def make_rect(name, script, cls, ctor, hw, B, seed, rel=0.2, slope=0.4):
    """A K1 class of the reference on a rectangular plane ``hw`` = (H, W): its constructors fix size x size, its sweeps
    read B, C, H, W from the input (mnist_test.py:45,72,105; cifar10.py:67,76,126,152), so the four coefficient
    parameters are replaced by (H, W) / (C, H, W) tensors — the constructor's own initial value, perturbed — and the
    layer is run as it is.  Written to tests/golden/rect/ (apart from the square fixtures, whose tests construct the
    product's layers from ``ctor`` alone); ``plane`` in the meta says what the parameters' plane is."""
    mod = ref_loader.load(script)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    with ref_loader.quiet():
        layer = getattr(mod, cls)(**ctor)
    C = getattr(layer, "channels", 1)
    with torch.no_grad():
        for n in ("alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff"):
            old = getattr(layer, n)
            shape = tuple(old.shape[:-2]) + tuple(hw)
            if n.endswith("_base"):
                new = float(old.flatten()[0]) * (1 + rel * torch.randn(shape, generator=g))
            else:
                new = slope * torch.randn(shape, generator=g)
            setattr(layer, n, torch.nn.Parameter(new))
        if hasattr(layer, "channel_mixing"):
            layer.channel_mixing.copy_(torch.eye(C) + 0.1 * torch.randn(C, C, generator=g))
    u = torch.randn(B, C, *hw, generator=g)
    gy = torch.randn(B, C, *hw, generator=g)
    os.makedirs(os.path.join(OUT, "rect"), exist_ok=True)
    with ref_loader.quiet():
        _save(os.path.join("rect", name), script, cls, ctor, layer, u, gy, torch.float32, extra_meta={"plane": list(hw)})


def rect():
    torch.set_num_threads(4)            # tests/golden_util.py GOLDEN_THREADS
    make_rect("mnist_20x36", "mnist_test", "DiffusionLayer", {"size": 20, "dt": 0.01, "dx": 1.0, "dy": 1.3, "num_steps": 3},
              (20, 36), 3, 81)
    make_rect("cifar10_c3_24x40", "cifar10", "EnhancedDiffusionLayer",
              {"size": 24, "channels": 3, "dt": 0.02, "num_steps": 3}, (24, 40), 2, 82, slope=0.5)


def make_model(name, script, cls, ctor, shape, seed, tweak=None, out_index=0, eval_mode=True, buffers=False):
    """A fixture of one of the reference's MODELS around the layers (tests/golden_models): same format, the output is
    element ``out_index`` of what the module returns.  eval(): dropout off, batch norm on its running statistics."""
    mod = ref_loader.load(script)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    with ref_loader.quiet():
        model = getattr(mod, cls)(**ctor)
    if eval_mode:
        model.eval()
    if tweak is not None:
        tweak(model, g)
    u = torch.randn(*shape, generator=g)

    def fwd(x):
        y = model(x)
        return y[out_index] if isinstance(y, (tuple, list)) else y
    y0 = fwd(u)
    gy = torch.randn(y0.shape, generator=g)

    class W(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.m = model

        def forward(self, x):
            return fwd(x)

        def named_parameters(self, *a, **k):
            return model.named_parameters(*a, **k)

        def named_buffers(self, *a, **k):
            return model.named_buffers(*a, **k)
    W.keep_buffers = buffers
    global OUT
    keep, OUT = OUT, os.path.join(os.path.dirname(HERE), "tests", "golden_models")
    os.makedirs(OUT, exist_ok=True)
    try:
        _save(name, script, cls, ctor, W(), u, gy, torch.float32)
    finally:
        OUT = keep


def models():
    def live(m, g):
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("alpha_base") or n.endswith("beta_base"):
                    p.mul_(1 + 0.2 * torch.randn(p.shape, generator=g))
                elif n.endswith("time_coeff"):
                    p.copy_(0.3 * torch.randn(p.shape, generator=g))
                elif n.endswith("channel_mixing"):
                    p.copy_(torch.eye(p.shape[0]) + 0.1 * torch.randn(p.shape, generator=g))
                elif n.endswith("combine_weights"):
                    p.copy_(torch.tensor([0.2, 0.5, -0.1]))
    # cifar10.MultiScaleExtractor: three PDE layers on one input + attention gates + softmax combination
    make_model("model_cifar10_multiscale", "cifar10", "MultiScaleExtractor", {"input_size": 32, "channels": 3},
               (3, 3, 32, 32), 81, tweak=live)
    make_model("model_cifar10_multiscale_default", "cifar10", "MultiScaleExtractor", {"input_size": 32, "channels": 3},
               (2, 3, 32, 32), 82)

    # cifar_2version.HybridPDEExtractor at 8x8 (its dense K matrices are (C*H*W)^2: 192^2 here, 3072^2 at 32x32):
    # two Lie-split diffusion layers + Parabolic + Hamiltonian blocks + softmax combination + BatchNorm2d (eval)
    def live2(m, g):
        live(m, g)
        with torch.no_grad():
            m.combination_weights.copy_(torch.tensor([0.3, -0.2, 0.1, 0.4]))
    make_model("model_cifar2_hybrid_8", "cifar_2version", "HybridPDEExtractor", {"input_size": 8, "channels": 3},
               (4, 3, 8, 8), 83, tweak=live2)

    # the whole cifar10.CIFAR10PDENoConv (cifar10.py:318-361): extractor + BatchNorm2d + 4x4 average / max pooling + classifier,
    # in training mode (batch statistics; dropout rate 0 through the constructor so that the pass is deterministic) and in eval
    # mode, BatchNorm parameters and running statistics away from their initial values
    def noconv(m, g):
        live(m, g)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n == "feature_bn.weight":
                    p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g))
                elif n == "feature_bn.bias":
                    p.copy_(0.2 * torch.randn(p.shape, generator=g))
            for n, b in m.named_buffers():
                if n.endswith("running_mean"):
                    b.copy_(0.1 * torch.randn(b.shape, generator=g))
                elif n.endswith("running_var"):
                    b.copy_(0.5 + torch.rand(b.shape, generator=g))
    make_model("model_cifar10_noconv_train", "cifar10", "CIFAR10PDENoConv", {"dropout_rate": 0.0}, (6, 3, 32, 32), 84,
               tweak=noconv, eval_mode=False, buffers=True)
    make_model("model_cifar10_noconv_eval", "cifar10", "CIFAR10PDENoConv", {}, (3, 3, 32, 32), 85, tweak=noconv, buffers=True)

    # the Ruthotto-Haber blocks alone (cifar_2version.py:190-258) at 8x8 (K is 192^2), training mode (batch statistics,
    # running statistics updated) and eval mode (running statistics), BatchNorm affine parameters and running
    # statistics away from their initial values
    def rh(m, g):
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("norm.weight"):
                    p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g))
                elif n.endswith("norm.bias"):
                    p.copy_(0.2 * torch.randn(p.shape, generator=g))
                elif n.endswith("K.weight"):
                    p.copy_(torch.eye(p.shape[0]) + 0.05 * torch.randn(p.shape, generator=g))
            for n, b in m.named_buffers():
                if n.endswith("running_mean"):
                    b.copy_(0.3 * torch.randn(b.shape, generator=g))
                elif n.endswith("running_var"):
                    b.copy_(0.5 + torch.rand(b.shape, generator=g))
    for mode, ev in (("train", False), ("eval", True)):
        make_model(f"model_rh_symmetric_8_{mode}", "cifar_2version", "SymmetricLayer", {"channels": 3, "spatial_size": 8},
                   (12, 3, 8, 8), 91, tweak=rh, eval_mode=ev, buffers=True)
        make_model(f"model_rh_symmetric_tanh_8_{mode}", "cifar_2version", "SymmetricLayer",
                   {"channels": 3, "spatial_size": 8, "activation": "tanh"}, (7, 3, 8, 8), 92, tweak=rh, eval_mode=ev, buffers=True)
        make_model(f"model_rh_parabolic_8_{mode}", "cifar_2version", "ParabolicBlock",
                   {"channels": 3, "spatial_size": 8, "num_steps": 4, "dt": 0.5}, (12, 3, 8, 8), 93, tweak=rh, eval_mode=ev, buffers=True)
        make_model(f"model_rh_hamiltonian_8_{mode}", "cifar_2version", "HamiltonianBlock",
                   {"channels": 3, "spatial_size": 8, "num_steps": 3, "dt": 0.8}, (12, 3, 8, 8), 94, tweak=rh, eval_mode=ev, buffers=True)
    # one application at the reference's own size (3 x 32 x 32: K is 3072^2, 37.7 MB — too large to store): K is rebuilt from
    # its seed by the test (eye + 0.01 randn, torch's CPU generator), its gradient is held by two projections
    big_symmetric()


def big_symmetric():
    mod = ref_loader.load("cifar_2version")
    g = torch.Generator().manual_seed(95)
    with ref_loader.quiet():
        layer = mod.SymmetricLayer(3, 32)
    D = layer.feature_dim
    with torch.no_grad():
        layer.K.weight.copy_(torch.eye(D) + 0.01 * torch.randn(D, D, generator=g))
        layer.norm.weight.copy_(1 + 0.3 * torch.randn(D, generator=g))
        layer.norm.bias.copy_(0.2 * torch.randn(D, generator=g))
    u = torch.randn(16, 3, 32, 32, generator=g).requires_grad_(True)
    gy = torch.randn(16, 3, 32, 32, generator=g)
    v1 = torch.randn(D, generator=g)
    v2 = torch.randn(D, generator=g)
    layer.train()
    y = layer(u)
    gu, gK, gw, gb = torch.autograd.grad(y, [u, layer.K.weight, layer.norm.weight, layer.norm.bias], gy)
    arrays = {"u": u.detach(), "gy": gy, "y": y.detach(), "gu": gu, "grad_norm.weight": gw, "grad_norm.bias": gb,
              "param_norm.weight": layer.norm.weight.detach(), "param_norm.bias": layer.norm.bias.detach(),
              "v1": v1, "v2": v2, "gK_v1": gK @ v1, "v2_gK": v2 @ gK, "gK_absmax": gK.abs().max(),
              "bufout_norm.running_mean": layer.norm.running_mean.clone(), "bufout_norm.running_var": layer.norm.running_var.clone()}
    arrays = {k: v.detach().cpu().numpy() for k, v in arrays.items()}
    meta = {"script": "cifar_2version", "cls": "SymmetricLayer", "ctor": {"channels": 3, "spatial_size": 32}, "dtype": "float32",
            "K": "eye(3072) + 0.01 * randn(3072, 3072, generator=manual_seed(95)) — the FIRST draw of the generator"}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(os.path.dirname(HERE), "tests", "golden_models", "model_rh_symmetric_32_train.npz")
    np.savez_compressed(path, **arrays)
    print(f"{'model_rh_symmetric_32_train':40s} {os.path.getsize(path) / 1024:8.1f} KiB")


def main():
    torch.set_num_threads(4)            # tests/golden_util.py GOLDEN_THREADS
    os.makedirs(OUT, exist_ok=True)
    f32, f64 = torch.float32, torch.float64
    models()

    # ---- mnist_test.DiffusionLayer ------------------------------------------------
    make("mnist_default", "mnist_test", "DiffusionLayer", {}, 3, 11)
    make("mnist_default_f64", "mnist_test", "DiffusionLayer", {}, 2, 11, f64)
    make("mnist_trained", "mnist_test", "DiffusionLayer", {}, 2, 12,
         tweak=lambda L, g: _perturb(L, g, 0.1, 0.1))
    make("mnist_dxdy_slopes", "mnist_test", "DiffusionLayer",
         {"size": 12, "dt": 0.02, "dx": 0.5, "dy": 2.0, "num_steps": 3}, 3, 13,
         tweak=lambda L, g: _perturb(L, g, 0.3, 20.0))

    def clamp_const(L, g):
        # some entries permanently below eps: clamp active at every sweep, mask constant in time
        _perturb(L, g, 0.2, 0.0)
        with torch.no_grad():
            L.alpha_base[2:5, 3:9] = -0.5
            L.beta_base[6:8, :] = -1.0
    make("mnist_clamp_const", "mnist_test", "DiffusionLayer",
         {"size": 12, "dt": 0.05, "num_steps": 2}, 2, 14, tweak=clamp_const)

    def clamp_cross(L, g):
        # base + slope*t crosses eps inside the time window: mask varies from sweep to sweep
        _perturb(L, g, 0.2, 0.0)
        with torch.no_grad():
            L.alpha_base[1:6, 2:7] = 0.02
            L.alpha_time_coeff[1:6, 2:7] = -0.5
            L.beta_base[4:9, 0:5] = -0.03
            L.beta_time_coeff[4:9, 0:5] = 0.6
    make("mnist_clamp_cross", "mnist_test", "DiffusionLayer",
         {"size": 12, "dt": 0.05, "num_steps": 3}, 2, 15, tweak=clamp_cross)
    make("mnist_clamp_cross_f64", "mnist_test", "DiffusionLayer",
         {"size": 12, "dt": 0.05, "num_steps": 3}, 2, 15, f64, tweak=clamp_cross)

    # ---- fashion_mnist.DiffusionLayer ----------------------------------------------
    make("fashion_default", "fashion_mnist", "DiffusionLayer", {}, 2, 21)
    make("fashion_default_f64", "fashion_mnist", "DiffusionLayer", {}, 2, 21, f64)
    make("fashion_trained", "fashion_mnist", "DiffusionLayer", {}, 2, 22,
         tweak=lambda L, g: _perturb(L, g, 0.2, 0.5))

    # ---- SVHN.DiffusionLayer -----------------------------------------------------------
    make("svhn_default", "SVHN", "DiffusionLayer", {"size": 32, "channels": 3}, 2, 31)

    def svhn_live(L, g):
        _perturb(L, g, 0.2, 0.0)
        with torch.no_grad():
            C = L.channels
            L.channel_coupling.copy_(torch.eye(C) + 0.05 * torch.randn(C, C, generator=g))
            L.skip_weight.fill_(0.3)
    make("svhn_live", "SVHN", "DiffusionLayer", {"size": 16, "channels": 3, "dt": 0.05, "num_steps": 4},
         2, 32, tweak=svhn_live)
    make("svhn_live_c5", "SVHN", "DiffusionLayer", {"size": 8, "channels": 5, "dt": 0.2, "num_steps": 2},
         3, 33, tweak=svhn_live)

    def svhn_identity(L, g):
        _perturb(L, g, 0.2, 0.0)
        with torch.no_grad():
            L.channel_coupling.copy_(torch.eye(L.channels))
            L.skip_weight.fill_(-40.0)
    make("svhn_identity_c4", "SVHN", "DiffusionLayer", {"size": 28, "channels": 4, "dt": 0.3, "num_steps": 4},
         2, 34, tweak=svhn_identity)

    # ---- cifar10.EnhancedDiffusionLayer -------------------------------------------------
    make("cifar10_default", "cifar10", "EnhancedDiffusionLayer", {"size": 32, "channels": 3}, 2, 41)
    make("cifar10_default_f64", "cifar10", "EnhancedDiffusionLayer", {"size": 32, "channels": 3}, 2, 41, f64)
    for i, (dt, steps, dx) in enumerate([(0.001, 5, 1.0), (0.002, 8, 2.0), (0.005, 4, 1.5)]):
        make(f"cifar10_scale{i + 1}", "cifar10", "EnhancedDiffusionLayer",
             {"size": 16, "channels": 3, "dt": dt, "num_steps": steps, "dx": dx, "dy": dx}, 2, 42 + i,
             tweak=lambda L, g: _perturb(L, g, 0.1, 0.1))

    def clampmax(L, g):
        with torch.no_grad():
            L.alpha_base.copy_(9.5 + 1.0 * torch.randn(L.alpha_base.shape, generator=g))
            L.beta_base.copy_(9.8 + 0.5 * torch.randn(L.beta_base.shape, generator=g))
    make("cifar10_clampmax", "cifar10", "EnhancedDiffusionLayer",
         {"size": 12, "channels": 3, "dt": 0.02, "num_steps": 3}, 2, 46, tweak=clampmax)
    make("cifar10_c8", "cifar10", "EnhancedDiffusionLayer",
         {"size": 16, "channels": 8, "dt": 0.01, "num_steps": 3}, 2, 47,
         tweak=lambda L, g: _perturb(L, g, 0.1, 1.0))

    def mix_identity(L, g):
        _perturb(L, g, 0.1, 0.1)
        with torch.no_grad():
            L.channel_mixing.copy_(torch.eye(L.channels))
    make("cifar10_c16_mixI", "cifar10", "EnhancedDiffusionLayer",
         {"size": 32, "channels": 16, "num_steps": 10}, 1, 48, tweak=mix_identity)

    # ---- cifar_2version.LearnableDiffusionLayer -----------------------------------------
    make("cifar2_default", "cifar_2version", "LearnableDiffusionLayer", {"size": 32, "channels": 3}, 2, 51)
    make("cifar2_trained", "cifar_2version", "LearnableDiffusionLayer",
         {"size": 16, "channels": 3, "dt": 0.05, "num_steps": 4}, 2, 52,
         tweak=lambda L, g: _perturb(L, g, 0.2, 2.0))
    make("cifar2_trained_f64", "cifar_2version", "LearnableDiffusionLayer",
         {"size": 16, "channels": 3, "dt": 0.05, "num_steps": 4}, 2, 52, f64,
         tweak=lambda L, g: _perturb(L, g, 0.2, 2.0, f64))

    # ---- tiny_imagenet.ImprovedDiffusionLayer -------------------------------------------
    make("tiny_default", "tiny_imagenet", "ImprovedDiffusionLayer", {"size": 64, "channels": 3}, 2, 61)

    def tiny_tw(L, g):
        with torch.no_grad():
            C = L.channels
            L.alpha_base.copy_(0.08 + 0.08 * torch.randn(C, generator=g))   # some above 0.15, some below 1e-6
            L.channel_scaling.copy_(1 + 0.2 * torch.randn(C, generator=g))
    make("tiny_trained_c6", "tiny_imagenet", "ImprovedDiffusionLayer", {"size": 16, "channels": 6}, 3, 62,
         tweak=tiny_tw)
    make("tiny_steps3", "tiny_imagenet", "ImprovedDiffusionLayer",
         {"size": 20, "channels": 4, "dt": 0.5, "num_steps": 3}, 2, 63, tweak=tiny_tw)
    make("tiny_steps3_f64", "tiny_imagenet", "ImprovedDiffusionLayer",
         {"size": 20, "channels": 4, "dt": 0.5, "num_steps": 3}, 2, 63, f64,
         tweak=lambda L, g: (tiny_tw(L, g)))

    # ---- emotion_recognition.PDELayer ---------------------------------------------------
    def emo_tame(L, g):
        with torch.no_grad():
            for n, v in dict(alpha_w1=0.05, alpha_w2=0.02, alpha_w3=-0.01,
                             beta_w1=0.04, beta_w2=0.015, beta_w3=0.01).items():
                getattr(L, n).fill_(v)
    make("emotion_tame", "emotion_recognition", "PDELayer", {"Nx": 48, "Ny": 48}, 2, 71, tweak=emo_tame)
    make("emotion_tame_f64", "emotion_recognition", "PDELayer", {"Nx": 48, "Ny": 48}, 2, 71, f64, tweak=emo_tame)
    make("emotion_tame_24", "emotion_recognition", "PDELayer", {"Nx": 24, "Ny": 24, "T": 0.005}, 3, 72,
         tweak=emo_tame)
    # default parameters are beyond the explicit stability limit:
    # keep the input smooth so the fixture stays finite and meaningful.
    smooth = lambda u: torch.nn.functional.avg_pool2d(
        torch.nn.functional.pad(u, (4, 4, 4, 4), mode="reflect"), 9, stride=1)
    make("emotion_default_smooth", "emotion_recognition", "PDELayer", {}, 2, 73, u_fn=smooth)

    rect()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "models":
        models()
    elif len(sys.argv) > 1 and sys.argv[1] == "rect":
        rect()
    else:
        main()
