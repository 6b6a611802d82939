"""Full-size layer calls held to the fp64 oracle by superposition (tests/superpose_util.py): the batch is a set of integer
combinations of K exact basis samples, so the oracle, which cannot run at 512 x 64 x 32 x 32, only sees the basis — and
the production path is compared with a reference at the batch sizes where its workgroups walk many chunks (the HO
forward's record ring, twin sweeps and counters carried across chunk boundaries; the assembly backward's per-chunk plane
bases and the chunk-to-chunk summation by parts of its time-weighted sums), where the properties of test_gpu_fullsize.py
(linearity, adjoint identity, additivity) cannot see an operator that is consistently wrong.

    case                 layer / shape                                            chunks per workgroup (fwd / bwd)
    headline             bench.build_layer(64, 32, 10), B = 512, 513, 2048;      2-9 / 8-33 (513: a one-plane chunk)
                         policy "auto" and "lagged" (second call)
    time dependence      the same, slopes x 20, B = 1000                          4 / 15-16
    moving clamp masks   512 x 64, two channels' masks move (assembly + masked HIP body in one call)     2 / 8
    over 2^31 bytes      headline, B = 8200 (2.15 GB per fp32 tensor)             32-33 / 128-129
    cfg2 .. cfg5         the BASELINE configurations at their full batch

plus oracle-size runs with fully random inputs in a child interpreter whose workgroups each walk every chunk of their
channel (PDE_G_FWD=1 PDE_G_BWD=1, the tuning knobs groups_per_channel reads).

Bounds: 1e-5 for fp32 (the SVHN skip-weight gradient, a cancelling scalar, may use the 2e-5 floor of test_gpu_fuzz.py),
3e-2 for cfg4's bf16 tensors against the unrounded oracle (as test_gpu_configs.py::cfg4)."""
import contextlib
import copy
import ctypes
import io
import os
import subprocess
import sys

import pytest
import torch

import golden_util as G
import superpose_util as S
from oracle import pde_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5

_bases = {}        # case -> superpose_util.Basis (several batch sizes reuse one)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _bench_layer(C, N, steps, mixing):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return quiet(bench.build_layer, C, N, steps, torch.device("cuda"), 0, mixing=mixing)


def _plain_spec(N, C, dt, steps):
    """The cifar10 layer without a channel operator (EnhancedDiffusionLayer(..., channel_mixing_enabled=False))."""
    return O.AdiSpec(N, C, dt, 1.0, 1.0, steps, "strang", False, 10.0, "none", False)


def _basis(key, layer, fn, dtype, seed, C, N):
    if key not in _bases:
        E, F = S.basis(dtype, C, N, seed)
        params = {n: p.detach().cpu() for n, p in layer.named_parameters()}
        _bases[key] = S.Basis(fn, params, E, F)
    return _bases[key]


def _superposed(layer, basis, B, dtype, calls=1):
    """The layer on the composed batch (``calls`` times, the last one checked); its errors against the reconstruction."""
    W, V = S.weights(dtype, B, seed=1), S.weights(dtype, B, seed=2)
    u = S.compose(basis.E, W, dtype, "cuda").requires_grad_(True)
    gy = S.compose(basis.F, V, dtype, "cuda")
    for _ in range(calls):
        for p in layer.parameters():
            p.grad = None
        u.grad = None
        y = layer(u)
        assert y.dtype == dtype and y.shape == u.shape
        y.backward(gy)
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in layer.named_parameters() if p.grad is not None}
    y, gu = y.detach(), u.grad
    del u, gy
    errs = S.errors(basis, W, V, y, gu, grads)
    del y, gu, grads
    torch.cuda.empty_cache()
    return errs


def _check(tag, errs, tol=TOL, loose=()):
    print(f"superposed {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v <= (2e-5 if k in loose else tol)}
    assert not bad, (tag, bad, errs)


def _kernels(layer, B):
    """(forward kernel, backward kernel) that a call of the plain layer on B samples takes: 3 = HO forward, 1 = the
    assembly backward.  The backward query assumes no checkpoints; that the plan has none is asserted here too."""
    import test_gpu_asm_bwd as T
    import cnn_with_pde_amd._lib as L
    lib = L.load()
    d = T._desc(B, layer.channels, layer.size, layer.num_steps, layer.dt)
    if layer.checkpoint_policy != 0:
        assert copy.deepcopy(layer).freeze_checkpoint_plan() == 0          # (the lagged budget: the stricter one)
    return lib.pde_adi_forward_kernel(ctypes.byref(d)), lib.pde_adi_backward_kernel(ctypes.byref(d), 0)


# ---- the headline layer ------------------------------------------------------------------------------------------
def _headline():
    layer = _bench_layer(64, 32, 10, False)
    spec = _plain_spec(32, 64, 0.001, 10)
    return layer, _basis("headline", layer, lambda a, p: O.adi_forward(a, p, spec), torch.float32, 101, 64, 32)


@pytest.mark.parametrize("policy", ["auto", "lagged"])
@pytest.mark.parametrize("B", [512, 513, 2048])
def test_headline_vs_oracle(B, policy):
    """At C = 64 the HO forward runs ceil(512/64) = 8 workgroups per channel over 32-plane chunks (2 to 8 chunks each at
    B = 512 and 2048) and the assembly backward 4 over 16-plane chunks (8 to 32 each); B = 513 ends every channel on a
    one-plane chunk in both.  "lagged": the second call runs on the plan the first one left."""
    layer, basis = _headline()
    layer.checkpoint_policy = policy
    assert _kernels(layer, B) == (3, 1)
    _check(f"headline B={B} {policy}", _superposed(layer, basis, B, torch.float32, calls=2 if policy == "lagged" else 1))


def test_headline_strong_time_dependence_vs_oracle():
    """Slopes x 20 (2.0 randn, as test_gpu_asm_bwd.CASES[4]): every time-weighted sum of the assembly backward matters,
    and at B = 1000 each backward workgroup adds up the parts of 15 or 16 chunks (4 forward chunks per workgroup)."""
    layer = _bench_layer(64, 32, 10, False)
    with torch.no_grad():
        layer.alpha_time_coeff.mul_(20.0)
        layer.beta_time_coeff.mul_(20.0)
    spec = _plain_spec(32, 64, 0.001, 10)
    basis = _basis("slopes", layer, lambda a, p: O.adi_forward(a, p, spec), torch.float32, 102, 64, 32)
    assert _kernels(layer, 1000) == (3, 1)
    _check("slopes x20 B=1000", _superposed(layer, basis, 1000, torch.float32))


def test_moving_clamp_masks_over_many_chunks_vs_oracle():
    """test_gpu_asm_bwd.test_channels_with_moving_clamp_masks_share_the_call at 512 x 64: channels 1 and 3 have
    coefficients that cross the clamp floor inside the time window, so the masked HIP body owns them while the assembly
    kernel runs the other 62, in one call, over 8 backward chunks per workgroup (2 forward).  No checkpoints (as there),
    so that the assembly kernel is what runs."""
    import cnn_with_pde_amd as P
    g = torch.Generator().manual_seed(77)
    N, C, B, steps, dt = 32, 64, 512, 3, 0.05
    layer = quiet(P.EnhancedDiffusionLayer, N, C, dt=dt, num_steps=steps, channel_mixing_enabled=False)
    with torch.no_grad():
        for k in ("alpha_base", "beta_base"):
            getattr(layer, k).mul_(1 + 0.1 * torch.randn(C, N, N, generator=g))
        for k in ("alpha_time_coeff", "beta_time_coeff"):
            getattr(layer, k).copy_(0.2 * torch.randn(C, N, N, generator=g))
        for c in (1, 3):
            layer.alpha_base[c, ::3, ::2] = 0.02
            layer.alpha_time_coeff[c, ::3, ::2] = -0.3
            layer.beta_base[c, 1::4, :] = 0.01
            layer.beta_time_coeff[c, 1::4, :] = -0.2
    layer = layer.cuda()
    layer.checkpoint_policy = 0
    spec = _plain_spec(N, C, dt, steps)
    basis = _basis("clamp", layer, lambda a, p: O.adi_forward(a, p, spec), torch.float32, 103, C, N)
    assert _kernels(layer, B) == (3, 1)
    _check("moving clamp masks B=512", _superposed(layer, basis, B, torch.float32))


def test_headline_tensors_over_2_31_bytes_vs_oracle():
    """B = 8200: each fp32 tensor of the call holds 8200 * 64 * 4096 bytes = 2.15 GB, so plane offsets pass 2^31 in every
    kernel of the forward and the backward."""
    layer, basis = _headline()
    B = 8200
    assert B * 64 * 32 * 32 * 4 > 2 ** 31
    assert _kernels(layer, B) == (3, 1)
    _check(f"headline B={B}", _superposed(layer, basis, B, torch.float32))


# ---- the BASELINE configurations at full batch ---------------------------------------------------------------------
def test_cfg2_with_channel_mixing_full_batch_vs_oracle():
    """EnhancedDiffusionLayer(32, 64, num_steps=10) with mixing before every step, 512 x 64 x 32 x 32: the one-launch
    wide forward, the per-step backward and the MFMA mixing backward."""
    layer = _bench_layer(64, 32, 10, True)
    g = torch.Generator().manual_seed(2064)
    with torch.no_grad():
        layer.channel_mixing.copy_((torch.eye(64) + 0.02 * torch.randn(64, 64, generator=g)).cuda())
    spec = O.cifar10_spec(32, 64, num_steps=10)
    basis = _basis("cfg2", layer, lambda a, p: O.adi_forward(a, p, spec), torch.float32, 104, 64, 32)
    _check("cfg2 B=512", _superposed(layer, basis, 512, torch.float32))


def test_cfg3_fashion_full_batch_vs_oracle():
    """FashionDiffusionLayer() on (4096, 1, 28, 28), coefficients as in test_gpu_fullsize (0.27 / 0.54 per sweep): the
    checkpointed backward over 4096 planes."""
    import cnn_with_pde_amd as P
    layer = quiet(P.FashionDiffusionLayer).cuda()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        layer.alpha_base.mul_((1 + 0.1 * torch.randn(layer.alpha_base.shape, generator=g)).cuda())
        layer.beta_time_coeff.copy_((0.2 * torch.randn(layer.beta_time_coeff.shape, generator=g)).cuda())
    spec = O.fashion_spec(28, 0.3, 1.0, 4)
    basis = _basis("cfg3", layer, lambda a, p: O.adi_forward(a, p, spec), torch.float32, 105, 1, 28)
    _check("cfg3 B=4096", _superposed(layer, basis, 4096, torch.float32))


def test_cfg3_at_32_channels_full_batch_vs_oracle():
    """SvhnDiffusionLayer(28, 32, dt=0.3, num_steps=4) on (512, 32, 28, 28), coupling and skip as in test_gpu_fullsize:
    the coupling after every step and the skip blend."""
    import cnn_with_pde_amd as P
    torch.manual_seed(6)                                   # the constructor's own draws (time coefficients)
    layer = quiet(P.SvhnDiffusionLayer, 28, 32, dt=0.3, num_steps=4)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        layer.alpha_base.fill_(1.8); layer.beta_base.fill_(1.8)
        layer.channel_coupling.copy_(torch.eye(32) + 0.05 * torch.randn(32, 32, generator=g))
        layer.skip_weight.fill_(0.3)
    layer = layer.cuda()
    spec = O.svhn_spec(28, 32, dt=0.3, num_steps=4)
    basis = _basis("cfg3_32", layer, lambda a, p: O.adi_forward(a, p, spec), torch.float32, 106, 32, 28)
    _check("cfg3 at 32 channels B=512", _superposed(layer, basis, 512, torch.float32), loose=("g_skip_weight",))


def test_cfg4_bf16_full_batch_vs_oracle():
    """SvhnDiffusionLayer(32, 128, num_steps=20) on bf16 tensors, (512, 128, 32, 32), parameters and coupling as in
    test_gpu_configs.py::cfg4: 60 sweeps, the bf16 operator backward; against the unrounded oracle (the layer rounds its
    state to bf16 41 times) at that test's 3e-2."""
    import cnn_with_pde_amd as P
    torch.manual_seed(7)
    g = torch.Generator().manual_seed(4128)
    C, N, steps = 128, 32, 20
    layer = P.SvhnDiffusionLayer(N, C, num_steps=steps)
    with torch.no_grad():
        layer.alpha_base.mul_(1 + 0.2 * torch.randn(C, N, N, generator=g))
        layer.beta_base.mul_(1 + 0.2 * torch.randn(C, N, N, generator=g))
        layer.alpha_time_coeff.copy_(0.5 * torch.randn(C, N, N, generator=g))
        layer.beta_time_coeff.copy_(0.5 * torch.randn(C, N, N, generator=g))
        layer.channel_coupling.copy_(torch.eye(C) + 0.05 / 4.0 * torch.randn(C, C, generator=g))
        layer.skip_weight.fill_(0.1)
    layer = layer.cuda()
    spec = O.svhn_spec(N, C, num_steps=steps)
    basis = _basis("cfg4", layer, lambda a, p: O.adi_forward(a, p, spec), torch.bfloat16, 107, C, N)
    _check("cfg4 bf16 B=512", _superposed(layer, basis, 512, torch.bfloat16), tol=3e-2)


def test_cfg5_tiny_imagenet_full_per_gpu_batch_vs_oracle():
    """ImprovedDiffusionLayer(64, 64) on (256, 64, 64, 64), coefficients as in test_gpu_fullsize: the explicit
    wave-per-plane kernels at the per-GPU batch."""
    import cnn_with_pde_amd as P
    layer = P.ImprovedDiffusionLayer(64, 64)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        layer.alpha_base.copy_(0.2 * torch.rand(64, generator=g))
        layer.channel_scaling.copy_(1 + 0.2 * torch.randn(64, generator=g))
    layer = layer.cuda()
    basis = _basis("cfg5", layer, lambda a, p: O.tiny_forward(a, p, dt=layer.dt, num_steps=layer.num_steps),
                   torch.float32, 108, 64, 64)
    _check("cfg5 B=256", _superposed(layer, basis, 256, torch.float32))


# ---- every workgroup walks every chunk of its channel, on fully random inputs --------------------------------------
CHILD = r"""
import sys, ctypes, torch
sys.path[:0] = [%(root)r, %(tests)r]
import cnn_with_pde_amd._lib as L
import test_gpu_asm_bwd as T
import test_gpu_fullsize_oracle as M
out = {}
for ci in range(len(T.CASES)):
    spec, params, u, gy, steps, dt = T._inputs(ci)
    out[ci] = T._run_gpu(params, u, gy, steps, dt)
layer = M._bench_layer(8, 32, 10, False)
g = torch.Generator().manual_seed(4008)
u = torch.randn(40, 8, 32, 32, generator=g)
gy = torch.randn(40, 8, 32, 32, generator=g)
ud = u.cuda().requires_grad_(True)
y = layer(ud)
y.backward(gy.cuda())
torch.cuda.synchronize()
out["headline"] = (y.detach().cpu(), ud.grad.cpu(), {n: getattr(layer, n).grad.cpu() for n in T.NAMES})
out["inputs"] = (u, gy, {n: getattr(layer, n).detach().cpu() for n in T.NAMES})
lib = L.load()
out["kernels"] = [(lib.pde_adi_forward_kernel(ctypes.byref(T._desc(B, C, 32, st, dt))),
                   lib.pde_adi_backward_kernel(ctypes.byref(T._desc(B, C, 32, st, dt)), 0))
                  for B, C, st, dt, _, _ in T.CASES if st > 1] + [M._kernels(layer, 40)]
torch.save(out, %(path)r)
"""


def test_one_group_per_channel_walks_every_chunk_vs_oracle(tmp_path):
    """PDE_G_FWD=1 PDE_G_BWD=1: one workgroup per channel, so every workgroup walks all the chunks of its channel — up to
    4 forward and 7 backward chunks on test_gpu_asm_bwd.CASES, 2 and 3 on the headline layer at 40 x 8 — with inputs that
    have no structure, against the oracle directly."""
    import test_gpu_asm_bwd as T
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in ("PDE_FWD_SCHED", "PDE_ASM_FWD", "PDE_ASM_BWD")}
    env.update(PDE_G_FWD="1", PDE_G_BWD="1")
    path = str(tmp_path / "g1.pt")
    code = CHILD % {"root": ROOT, "tests": here, "path": path}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    res = torch.load(path, weights_only=True)
    assert all(k == (3, 1) for k in res["kernels"]), res["kernels"]
    for ci in range(len(T.CASES)):
        spec, params, u, gy, steps, dt = T._inputs(ci)
        y_ref, gu_ref, gp_ref = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec), u, params, gy)
        y, gu, gp = res[ci]
        errs = {"y": G.rel_err(y, y_ref), "gu": G.rel_err(gu, gu_ref)}
        errs.update({"g_" + k: G.rel_err(gp[k], gp_ref[k]) for k in T.NAMES})
        _check(f"G=1 CASES[{ci}]", errs)
    u, gy, params = res["inputs"]
    spec = _plain_spec(32, 8, 0.001, 10)
    y_ref, gu_ref, gp_ref = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec), u, params, gy)
    y, gu, gp = res["headline"]
    errs = {"y": G.rel_err(y, y_ref), "gu": G.rel_err(gu, gu_ref)}
    errs.update({"g_" + k: G.rel_err(gp[k], gp_ref[k]) for k in T.NAMES})
    _check("G=1 headline 40 x 8", errs)
