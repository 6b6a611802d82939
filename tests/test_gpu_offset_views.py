"""Offset views through the public surface: tensors that begin where their storage offset puts them.

``.contiguous()`` does nothing for a contiguous view at a storage offset, and such views are ordinary: a batch slice
``big[1:]`` (a 6 x 6 bf16 sample is 72 bytes, a 7 x 7 fp16 one 98), parameters that are consecutive slices of one flat
buffer (flattened or sharded parameter storage: ``alpha_base`` then sits one element behind an aligned address), an
upstream gradient that is a stride-0 expand (``y.sum().backward()``) or itself an offset view, a permuted input, running
statistics cut from a flat buffer.  The library asks 16 bytes of tensors, coefficient planes and matrices
(include/pdecnn.h, "Alignment") and refuses less; the wrappers — ``functional._aligned`` on the ctypes path,
``aligned()`` in csrc/host_ext.cpp on the native one — copy what is below that and pass everything else through untouched.

Every call is made once on such views and once on fresh clones of the same values, on both host paths: output, input
gradient, every parameter gradient (read back through the flat buffer's ``.grad``) and the running statistics in the
caller's own view after the call are bitwise equal.  One implicit layer is also held to the fp64 oracle at the tolerance
of ``smoke()``, so that "equal" does not mean "equally wrong".  Shapes are the smallest that reach each kernel family."""
import contextlib
import io

import pytest
import torch

pytestmark = pytest.mark.gpu


def _gen(*key):
    return torch.Generator().manual_seed(20251 + sum(ord(c) for c in repr(key)))


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), (what, float((a.double() - b.double()).abs().max()))


@contextlib.contextmanager
def _host_path(native):
    from cnn_with_pde_amd import _lib as L
    ext = L.host_ext()
    assert ext is not None
    if not native:
        L._host = False
    try:
        yield
    finally:
        L._host = ext


# ---- arrangements: the same values, held differently ---------------------------------------------------------------
class Held:
    """``tensors``: what the call is handed; ``leaves``: the tensors that own the storage (gradients arrive there);
    ``grad_of(i)``: the gradient of tensor i, cut from its leaf's ``.grad``."""

    def __init__(self):
        self.tensors, self.leaves, self._cut = [], [], []

    def add(self, tensor, leaf, cut):
        self.tensors.append(tensor)
        if not any(leaf is l for l in self.leaves):
            self.leaves.append(leaf)
        self._cut.append((leaf, cut))

    def grad_of(self, i):
        leaf, cut = self._cut[i]
        return None if leaf.grad is None else cut(leaf.grad)


def hold(values, how):
    """values: [input, parameters ...] (CPU).  how: "clone" fresh allocations; "flat" the input one element into a buffer of
    its own, the parameters consecutive slices of ONE flat buffer behind a one-element lead; "batch" the input as big[1:];
    "permuted" the input a non-contiguous transpose of its storage, parameters as in "flat"."""
    h = Held()
    u, params = values[0], values[1:]

    def leaf(t):
        return t.clone().cuda().requires_grad_(t.is_floating_point())

    if how == "clone":
        for t in values:
            l = leaf(t)
            h.add(l, l, lambda g: g)
        return h
    n = u.numel()
    if how in ("flat",):
        fu = leaf(torch.cat([torch.zeros(1, dtype=u.dtype), u.flatten()]))
        h.add(fu[1:1 + n].view(u.shape), fu, lambda g, n=n, s=u.shape: g[1:1 + n].view(s))
    elif how == "batch":
        big = leaf(torch.cat([torch.zeros_like(u[:1]), u]))
        h.add(big[1:], big, lambda g: g[1:])
    elif how == "permuted":
        base = leaf(u.transpose(-1, -2).contiguous())
        h.add(base.transpose(-1, -2), base, lambda g: g.transpose(-1, -2))
    if how == "batch":
        for t in params:
            l = leaf(t)
            h.add(l, l, lambda g: g)
        return h
    by_dtype = {}
    for t in params:
        by_dtype.setdefault(t.dtype, []).append(t)
    flats = {dt: leaf(torch.cat([torch.zeros(1, dtype=dt)] + [t.flatten() for t in ts])) for dt, ts in by_dtype.items()}
    at = {dt: 1 for dt in flats}
    for t in params:
        f, a, m = flats[t.dtype], at[t.dtype], t.numel()
        h.add(f[a:a + m].view(t.shape), f, lambda g, a=a, m=m, s=t.shape: g[a:a + m].view(s))
        at[t.dtype] += m
    return h


def run(fn, values, gy, how, grad="given"):
    """fn(*tensors) -> output; backward with ``gy`` (as an offset view for every arrangement but "clone", or through
    ``sum()`` when grad == "sum": a stride-0 expand); returns [output, gradient of every floating tensor]."""
    h = hold(values, how)
    out = fn(*h.tensors)
    first = out[0] if isinstance(out, (tuple, list)) else out
    if grad == "sum":
        first.sum().backward()
    else:
        g = gy.to(first.dtype)
        if how != "clone":
            fg = torch.cat([torch.zeros(1, dtype=g.dtype), g.flatten()]).cuda()
            g = fg[1:].view(g.shape)
            assert g.data_ptr() % 16 != 0
        else:
            g = g.cuda()
        first.backward(g)
    torch.cuda.synchronize()
    res = [first.detach().clone()]
    for i, t in enumerate(values):
        if t.is_floating_point():
            g = h.grad_of(i)
            assert g is not None, f"no gradient for tensor {i}"
            res.append(g.detach().clone().contiguous())
    if how == "batch":                           # the sample in front of the slice took no part
        assert not bool(h.leaves[0].grad[0].any())
    return res


#: max-norm relative error allowed against the fp64 reference: the GPU gates' 1e-5 for fp32 tensors (DESIGN.md section 5,
#: ``golden_util.rel_err``), 1e-11 on the float64 route
ORACLE_TOL = {torch.float32: 1e-5, torch.float64: 1e-11}


def rel_err(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def against_oracle(got, oracle, values, gy, tol, what):
    """``got`` = [output, gradient of every floating tensor] of a run on offset views; ``oracle(*values)``: the same
    operation in plain fp64 torch on the CPU, differentiated by autograd.  Every figure is printed before it is held."""
    v64 = [t.detach().clone().double().requires_grad_(True) if t.is_floating_point() else t for t in values]
    out = oracle(*v64)
    leaves = [t for t in v64 if t.is_floating_point()]
    grads = torch.autograd.grad(out, leaves, gy.double().reshape(out.shape))
    errs = [rel_err(got[0], out.detach())] + [rel_err(g, r) for g, r in zip(got[1:], grads)]
    print(what, "vs fp64:", " ".join(f"{e:.2e}" for e in errs), f"(limit {tol:g})")
    assert len(got) == 1 + len(grads) and max(errs) < tol, (what, errs)


def check(fn, values, gy, arrangements=("flat", "batch", "permuted"), oracle=None):
    if oracle is not None:                       # the offset-view run itself against fp64, so that equal is not equally wrong
        with _host_path(True):
            against_oracle(run(fn, values, gy, arrangements[0]), oracle, values, gy, ORACLE_TOL[values[0].dtype],
                           f"{arrangements[0]} views")
    for native in (True, False):
        with _host_path(native):
            ref = run(fn, values, gy, "clone")
            ref_sum = run(fn, values, gy, "clone", grad="sum")
            for how in arrangements:
                got = run(fn, values, gy, how)
                assert len(got) == len(ref)
                for i, (a, b) in enumerate(zip(ref, got)):
                    _same(a, b, (how, "native" if native else "ctypes", i))
            got = run(fn, values, gy, arrangements[0], grad="sum")
            for i, (a, b) in enumerate(zip(ref_sum, got)):
                _same(a, b, ("sum", "native" if native else "ctypes", i))
    return ref


# ---- the implicit layers -------------------------------------------------------------------------------------------
def _adi_values(g, B, Cc, H, W, dtype, pdtype=torch.float32):
    u = torch.randn(B, Cc, H, W, generator=g).to(dtype)
    ps = [(1 + 0.15 * torch.randn(Cc, H, W, generator=g)).to(pdtype) for _ in range(2)]
    ps += [(0.5 * torch.randn(Cc, H, W, generator=g)).to(pdtype) for _ in range(2)]
    return [u] + ps, torch.randn(B, Cc, H, W, generator=g)


ADI = [("fused-n8", 8, 8, torch.float32), ("fused-n8", 8, 8, torch.bfloat16), ("fused-n12", 12, 12, torch.float16),
       ("fused-n12", 12, 12, torch.float32), ("any-n6", 6, 6, torch.bfloat16), ("any-n7", 7, 7, torch.float16),
       ("any-n7", 7, 7, torch.float32), ("rect-6x10", 6, 10, torch.float32), ("rect-6x10", 6, 10, torch.bfloat16),
       ("f64-n6", 6, 6, torch.float64), ("f64-n8", 8, 8, torch.float64)]


@pytest.mark.parametrize("tag,H,W,dtype", ADI, ids=[f"{t}-{str(d).split('.')[1]}" for t, _, _, d in ADI])
def test_implicit_layer_on_offset_views(tag, H, W, dtype):
    import cnn_with_pde_amd as P
    f64 = dtype == torch.float64
    pd = torch.float64 if f64 else (torch.float16 if dtype == torch.float16 else torch.float32)
    values, gy = _adi_values(_gen(tag, dtype), 3, 2, H, W, dtype, pd)
    sweeps = [s for st in P.adi_schedule(0.02, 1.0, 1.0, 2) for s in st]

    def fn(u, *ps):
        return P.adi_diffuse(u, *ps, sweeps, clamp_max=10.0, checkpoints=0b10)

    from oracle import pde_oracle as O
    spec = O.AdiSpec(H, 2, 0.02, 1.0, 1.0, 2, "strang", False, 10.0, "none", False)

    def ref(u, ab, bb, asl, bsl):
        return O.adi_forward(u, dict(alpha_base=ab, beta_base=bb, alpha_time_coeff=asl, beta_time_coeff=bsl), spec)

    # a transpose of a rectangle's storage is still that rectangle as the call sees it: every arrangement applies
    check(fn, values, gy, oracle=ref if dtype in ORACLE_TOL else None)


def test_the_trajectory_of_an_implicit_layer_on_offset_views():
    import cnn_with_pde_amd as P
    values, _ = _adi_values(_gen("traj"), 3, 2, 8, 8, torch.float32)
    sweeps = [s for st in P.adi_schedule(0.02, 1.0, 1.0, 2) for s in st]
    gy = torch.randn(3, 3, 2, 8, 8, generator=_gen("traj-g"))

    def fn(u, *ps):
        return P.adi_diffuse_states(u, *ps, sweeps, [0, 3, 5], clamp_max=10.0, checkpoints=0b10)

    check(fn, values, gy, arrangements=("flat", "batch"))


@pytest.mark.parametrize("which,Cc,N", [("small", 3, 16), ("mixed", 32, 8)])
def test_layers_with_a_channel_operator_on_offset_views(which, Cc, N):
    import cnn_with_pde_amd as P
    g = _gen(which)
    values, gy = _adi_values(g, 3, Cc, N, N, torch.float32)
    values.append(torch.eye(Cc) + 0.2 / Cc ** 0.5 * torch.randn(Cc, Cc, generator=g))
    steps = P.adi_schedule(0.02, 1.0, 1.0, 2)
    f = P.adi_diffuse_small if which == "small" else P.adi_diffuse_mixed

    def fn(u, ab, bb, asl, bsl, M):
        return f(u, ab, bb, asl, bsl, M, steps, "pre", clamp_max=10.0, checkpoints=0)

    from oracle import pde_oracle as O
    spec = O.AdiSpec(N, Cc, 0.02, 1.0, 1.0, 2, "strang", False, 10.0, "pre", False)

    def ref(u, ab, bb, asl, bsl, M):
        return O.adi_forward(u, dict(alpha_base=ab, beta_base=bb, alpha_time_coeff=asl, beta_time_coeff=bsl, channel_mixing=M),
                             spec)

    check(fn, values, gy, oracle=ref)


# ---- explicit and Jacobi layers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(8, 6), (8, 8)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_explicit_layer_on_offset_views(H, W, dtype):
    import cnn_with_pde_amd as P
    g = _gen("explicit", H, W, dtype)
    pd = torch.float64 if dtype == torch.float64 else torch.float32
    values = [torch.randn(3, 2, H, W, generator=g).to(dtype), (0.05 + 0.1 * torch.rand(2, generator=g)).to(pd),
              (1 + 0.1 * torch.randn(2, generator=g)).to(pd)]
    gy = torch.randn(3, 2, H, W, generator=g)
    from oracle import pde_oracle as O
    check(lambda u, a, s: P.explicit5_step(u, a, s, num_steps=3), values, gy,
          arrangements=("flat", "batch") + (("permuted",) if H == W else ()),
          oracle=(lambda u, a, s: O.tiny_forward(u, dict(alpha_base=a, channel_scaling=s), 0.01, 3, 1e-6, 0.15, 0.1))
          if dtype in ORACLE_TOL else None)


@pytest.mark.parametrize("H,W", [(8, 8), (65, 8)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_jacobi_layer_on_offset_views(H, W, dtype):
    import cnn_with_pde_amd as P
    g = _gen("jacobi", H, W, dtype)
    values = [torch.randn(3, H, W, generator=g).to(dtype), 0.05 + 0.15 * torch.rand(H, generator=g),
              0.05 + 0.15 * torch.rand(W, generator=g)]
    gy = torch.randn(3, H, W, generator=g)
    from oracle import pde_oracle as O
    check(lambda u, a, b: P.jacobi_diffuse(u, a, b, 12), values, gy, arrangements=("flat", "batch"),
          oracle=(lambda u, a, b: O.jacobi_forward(u, a, b, 12)) if dtype in ORACLE_TOL else None)


# ---- side kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_skip_blend_on_offset_views(dtype):
    from cnn_with_pde_amd import functional as F
    g = _gen("blend", dtype)
    pd = torch.float64 if dtype == torch.float64 else torch.float32
    values = [torch.randn(3, 85, generator=g).to(dtype), torch.randn(3, 85, generator=g).to(dtype), torch.tensor(0.4).to(pd)]
    check(lambda u0, u, w: F.skip_blend(u0, u, w), values, torch.randn(3, 85, generator=g), arrangements=("flat", "batch"),
          oracle=(lambda u0, u, w: torch.sigmoid(w) * u0 + (1 - torch.sigmoid(w)) * u) if dtype in ORACLE_TOL else None)


def test_channel_mix_and_gate_on_offset_views():
    import cnn_with_pde_amd as P
    g = _gen("mix")
    values = [torch.randn(3, 33, 7, 7, generator=g), torch.randn(33, 33, generator=g) / 6]
    check(lambda u, M: P.channel_mix(u, M), values, torch.randn(3, 33, 7, 7, generator=g), arrangements=("flat", "batch"),
          oracle=lambda u, M: torch.einsum("ij,bjhw->bihw", M, u))
    g = _gen("gate")
    ys = [torch.randn(3, 2, 6, 6, generator=g) for _ in range(2)]
    values = [ys[0], ys[1], torch.rand(3, 2, generator=g), torch.rand(3, 2, generator=g), torch.softmax(torch.randn(2, generator=g), 0)]
    check(lambda y0, y1, g0, g1, w: P.gate_combine([y0, y1], [g0, g1], w), values, torch.randn(3, 2, 6, 6, generator=g),
          arrangements=("flat", "batch"),
          oracle=lambda y0, y1, g0, g1, w: w[0] * g0[:, :, None, None] * y0 + w[1] * g1[:, :, None, None] * y1)


# ---- running statistics in the caller's own view -------------------------------------------------------------------------
def _bn_in_a_flat_buffer(bn_cls, D, g, flat):
    bn = bn_cls(D).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(D, generator=g))
        bn.bias.copy_(0.2 * torch.randn(D, generator=g))
    rm0, rv0 = 0.1 * torch.randn(D, generator=g), 1 + 0.1 * torch.rand(D, generator=g)
    if flat:
        buf = torch.zeros(1 + 2 * D, device="cuda")
        bn.running_mean, bn.running_var = buf[1:1 + D], buf[1 + D:1 + 2 * D]
        assert bn.running_mean.data_ptr() % 16 == 4
    else:
        buf = None
    with torch.no_grad():
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    return bn, buf


@pytest.mark.parametrize("amp", [None, torch.float16, torch.bfloat16])
def test_symmetric_layer_updates_running_statistics_in_a_sliced_buffer(amp):
    from cnn_with_pde_amd import functional as F
    B, D = 5, 64
    for native in (True, False):
        with _host_path(native):
            res = []
            for flat in (False, True):
                g = _gen("sym", amp)
                X = torch.randn(B, D, generator=g)
                K = torch.randn(D, D, generator=g) / D ** 0.5
                gy = torch.randn(B, D, generator=g)
                bn, buf = _bn_in_a_flat_buffer(torch.nn.BatchNorm1d, D, g, flat)
                h = hold([X, K], "flat" if flat else "clone")
                Xv, Kv = h.tensors
                # under fp16 / bf16 autocast the models call the layer with K16 = r(K), made once per region (models.py)
                with (torch.autocast("cuda", dtype=amp) if amp is not None else contextlib.nullcontext()):
                    K16 = None if amp is None else F.sym_k16(Kv, amp)
                    y = F.sym_layer(Xv, Kv, bn, "relu", base=Xv, scale=-1.0, K16=K16)
                y.backward(gy.cuda())
                torch.cuda.synchronize()
                if flat:                         # the update landed in the caller's buffer, and only inside the two slices
                    assert buf[0] == 0 and torch.equal(buf[1:1 + D], bn.running_mean)
                res.append([y.detach().clone(), h.grad_of(0).clone(), h.grad_of(1).clone(), bn.weight.grad.clone(),
                            bn.bias.grad.clone(), bn.running_mean.clone(), bn.running_var.clone()])
            for i, (a, b) in enumerate(zip(*res)):
                _same(a, b, (amp, native, i))
            assert not torch.equal(res[1][5], torch.zeros(D, device="cuda"))
            if amp is None and native:           # the run on views against plain fp64 torch (test_gpu_rh.py's 1e-5)
                g = _gen("sym", amp)
                X, K, gy = (torch.randn(B, D, generator=g).double().requires_grad_(True),
                            (torch.randn(D, D, generator=g) / D ** 0.5).double().requires_grad_(True),
                            torch.randn(B, D, generator=g).double())
                w = (1 + 0.2 * torch.randn(D, generator=g)).float().double().requires_grad_(True)
                b_ = (0.2 * torch.randn(D, generator=g)).float().double().requires_grad_(True)
                rm, rv = (0.1 * torch.randn(D, generator=g)).float().double(), (1 + 0.1 * torch.rand(D, generator=g)).float().double()
                Hh = torch.relu(torch.nn.functional.batch_norm(X @ K.t(), rm, rv, w, b_, True, 0.1, 1e-5))
                y = X - Hh @ K
                refs = [y.detach()] + list(torch.autograd.grad(y, [X, K, w, b_], gy)) + [rm, rv]
                errs = [rel_err(a, r) for a, r in zip(res[1], refs)]
                print("symmetric layer on views vs fp64:", " ".join(f"{e:.2e}" for e in errs))
                assert max(errs) < 1e-5, errs


def test_bn_pool_tail_updates_running_statistics_in_a_sliced_buffer():
    from cnn_with_pde_amd import functional as F
    res = []
    for flat in (False, True):
        g = _gen("tail")
        x = torch.randn(3, 5, 12, 12, generator=g)
        gy = torch.randn(3, 10, 4, 4, generator=g)
        bn, buf = _bn_in_a_flat_buffer(torch.nn.BatchNorm2d, 5, g, flat)
        before = bn.running_mean.clone()
        h = hold([x], "flat" if flat else "clone")
        assert F.bn_pool_supported(h.tensors[0], bn)
        y = F.bn_pool(h.tensors[0], bn)
        y.backward(gy.cuda())
        torch.cuda.synchronize()
        assert not torch.equal(bn.running_mean, before), "the running mean was not updated"
        if flat:
            assert buf[0] == 0 and torch.equal(buf[1:6], bn.running_mean) and torch.equal(buf[6:11], bn.running_var)
        res.append([y.detach().clone(), h.grad_of(0).clone(), bn.weight.grad.clone(), bn.bias.grad.clone(),
                    bn.running_mean.clone(), bn.running_var.clone()])
    for i, (a, b) in enumerate(zip(*res)):
        _same(a, b, ("tail", i))
    g = _gen("tail")                             # the run on views against plain fp64 torch (the GPU gates' 1e-5)
    x = torch.randn(3, 5, 12, 12, generator=g).double().requires_grad_(True)
    gy = torch.randn(3, 10, 4, 4, generator=g).double()
    w = (1 + 0.2 * torch.randn(5, generator=g)).float().double().requires_grad_(True)
    b_ = (0.2 * torch.randn(5, generator=g)).float().double().requires_grad_(True)
    rm, rv = (0.1 * torch.randn(5, generator=g)).float().double(), (1 + 0.1 * torch.rand(5, generator=g)).float().double()
    z = torch.nn.functional.batch_norm(x, rm, rv, w, b_, True, 0.1, 1e-5)
    y = torch.cat([torch.nn.functional.adaptive_avg_pool2d(z, 4), torch.nn.functional.adaptive_max_pool2d(z, 4)], 1)
    refs = [y.detach()] + list(torch.autograd.grad(y, [x, w, b_], gy)) + [rm, rv]
    errs = [rel_err(a, r) for a, r in zip(res[1], refs)]
    print("BatchNorm-pool tail on views vs fp64:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < 1e-5, errs


# ---- modules, the oracle, a captured graph, and the aligned path ---------------------------------------------------------
def _enhanced(N, Cc, steps, g):
    import cnn_with_pde_amd as P
    with contextlib.redirect_stdout(io.StringIO()):
        layer = P.EnhancedDiffusionLayer(N, Cc, dt=0.01, num_steps=steps).cuda()
    with torch.no_grad():
        layer.alpha_base.mul_(1 + 0.2 * torch.randn(layer.alpha_base.shape, generator=g).cuda())
        layer.beta_time_coeff.copy_((2.0 * torch.randn(layer.beta_base.shape, generator=g)).cuda())
    return layer


@pytest.mark.parametrize("kind,H,W", [("pde", 8, 8), ("pde", 65, 8), ("improved", 8, 6), ("improved", 8, 8)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_explicit_modules_on_offset_views(kind, H, W, dtype):
    """``PDELayer`` (one-workgroup and tiled planes) and ``ImprovedDiffusionLayer`` (W % 4 != 0 and float4 rows) through the
    modules' own parameter handling: the input as ``big[1:]`` / one element into a flat buffer / a permuted view, the
    parameters as the module's own or as consecutive slices of ONE flat buffer behind a one-element lead
    (``torch.func.functional_call``), the gradient as an offset view or a stride-0 expand (``sum().backward()``).  Output,
    input gradient and every parameter gradient (read back through the flat buffer's ``.grad``) are bitwise those of the
    run on clones.  Under ``.half()`` the parameters are fp16 too (the float16 route)."""
    import cnn_with_pde_amd as P
    g = _gen(kind, H, W, dtype)
    if kind == "pde":
        layer, Cc = P.PDELayer(Nx=W, Ny=H, T=0.012, dt=0.001), 1
    else:
        layer, Cc = P.ImprovedDiffusionLayer(size=H, channels=2, num_steps=3), 2
    layer = layer.cuda().to(dtype)
    names = [k for k, _ in layer.named_parameters()]
    u, gy = torch.randn(3, Cc, H, W, generator=g).to(dtype), torch.randn(3, Cc, H, W, generator=g).to(dtype)

    def one(inp, flat_params, grad):
        layer.zero_grad()
        h = hold([u], inp)
        x = h.tensors[0]
        if flat_params:
            vals = [p.detach().reshape(-1) for p in layer.parameters()]
            flat = torch.cat([torch.zeros(1, dtype=dtype, device="cuda")] + vals).requires_grad_(True)
            views, at = {}, 1
            for k, p in layer.named_parameters():
                views[k] = flat[at:at + p.numel()].view(p.shape)
                at += p.numel()
            y = torch.func.functional_call(layer, views, (x,))
        else:
            y = layer(x)
        if grad == "sum":
            y.sum().backward()
        else:
            gv = torch.cat([torch.zeros(1, dtype=dtype), gy.flatten()]).cuda()[1:].view(gy.shape) if inp != "clone" else gy.cuda()
            y.backward(gv)
        torch.cuda.synchronize()
        res = [y.detach().clone(), h.grad_of(0).detach().clone().contiguous()]
        at = 1
        for k, p in layer.named_parameters():
            gp = flat.grad[at:at + p.numel()].view(p.shape) if flat_params else p.grad
            at += p.numel()
            if flat_params and p.grad is not None:
                raise AssertionError("the module's own parameter took a gradient")
            res.append(None if gp is None else gp.detach().clone())
        return res

    for grad in ("given", "sum"):
        ref = one("clone", False, grad)
        used = [i for i, r in enumerate(ref) if r is not None and (i < 2 or bool(r.any()) or names[i - 2] != "beta_base")]
        assert len(used) >= 4
        for inp, flat_params in (("batch", False), ("flat", True)) + ((("permuted", True),) if H == W else ()):
            got = one(inp, flat_params, grad)
            for i in used:
                b = got[i] if got[i] is not None else torch.zeros_like(ref[i])
                _same(ref[i], b, (kind, H, W, grad, inp, flat_params, i))


def test_a_module_on_a_batch_slice_agrees_with_the_fp64_oracle():
    """The layer of ``smoke()`` on ``big[1:]`` with the gradient as an offset view: bitwise the run on clones, and within
    smoke()'s 1e-5 of the CPU fp64 oracle (oracle/pde_oracle.py) — output, input gradient and every parameter gradient."""
    from oracle import pde_oracle as O
    g = _gen("oracle")
    B, Cc, N, steps = 3, 3, 16, 2
    layer = _enhanced(N, Cc, steps, g)
    u, gy = torch.randn(B, Cc, N, N, generator=g), torch.randn(B, Cc, N, N, generator=g)
    outs = []
    for view in (False, True):
        layer.zero_grad()
        big = torch.cat([torch.zeros_like(u[:1]), u]).cuda().requires_grad_(True)
        x = big[1:] if view else big[1:].clone()
        gv = torch.cat([torch.zeros(1), gy.flatten()]).cuda()[1:].view(gy.shape) if view else gy.cuda()
        y = layer(x)
        y.backward(gv)
        torch.cuda.synchronize()
        outs.append([y.detach().clone(), big.grad[1:].clone()] + [p.grad.clone() for p in layer.parameters()])
    for i, (a, b) in enumerate(zip(*outs)):
        _same(a, b, ("module", i))
    spec = O.cifar10_spec(N, Cc, dt=0.01, num_steps=steps)
    params = {k: v.detach().cpu() for k, v in layer.named_parameters()}
    y_ref, gu_ref, gp_ref = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec), u, params, gy)

    def rel(a, b):
        return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max())

    errs = {"y": rel(outs[1][0], y_ref), "gu": rel(outs[1][1], gu_ref)}
    for (k, _), gp in zip(layer.named_parameters(), outs[1][2:]):
        errs["g_" + k] = rel(gp, gp_ref[k])
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < 1e-5, errs


def test_a_captured_step_whose_static_input_is_an_offset_view_replays_like_eager():
    """The realignment copy is part of the captured region: after the view's contents change, a replay equals eager."""
    from cnn_with_pde_amd import graphs as G
    g = _gen("graph")
    layer = _enhanced(16, 3, 2, g)
    G.freeze_checkpoint_plans(layer)
    n = 3 * 3 * 16 * 16
    flat = torch.zeros(n + 1, device="cuda")
    flat[1:] = torch.randn(n, generator=g).cuda()
    x = flat[1:].view(3, 3, 16, 16).requires_grad_(False)
    assert x.data_ptr() % 16 == 4
    xs = x.detach().requires_grad_(True)                     # the same storage: a leaf that is an offset view
    params = list(layer.parameters())

    def fn():
        y = layer(xs)
        return (y,) + torch.autograd.grad(y.square().sum(), [xs] + params)

    step = G.GraphedStep(fn)
    flat[1:] = torch.randn(n, generator=g).cuda()            # new contents, same address
    got = [o.clone() for o in step()]
    torch.cuda.synchronize()
    want = fn()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(want, got)):
        _same(a.detach(), b, ("graph", i))


def test_the_aligned_path_hands_the_callers_own_tensors_to_the_library(monkeypatch):
    """A fused layer on ordinary tensors: every address the ctypes path passes for the input and the coefficients is the
    caller's own (no copy), and a forward + backward costs the launches it cost before — pde_timing_* counts the sweep
    launches of a call: one per pass."""
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import functional as F
    values, gy = _adi_values(_gen("aligned"), 3, 2, 8, 8, torch.float32)
    h = hold(values, "clone")
    sweeps = [s for st in P.adi_schedule(0.02, 1.0, 1.0, 2) for s in st]
    seen = []
    real = F._ptr

    def spy(t):
        if t is not None:
            seen.append(t.data_ptr())
        return real(t)

    copies = []
    real_aligned = F._aligned

    def spy_aligned(t, *a):
        r = real_aligned(t, *a)
        if t is not None and r is not t:
            copies.append(tuple(t.shape))
        return r

    monkeypatch.setattr(F, "_ptr", spy)
    monkeypatch.setattr(F, "_aligned", spy_aligned)
    with _host_path(False):
        F.timing_enable(True)
        try:
            y = P.adi_diffuse(*h.tensors, sweeps, clamp_max=10.0, checkpoints=0)
            y.backward(gy.cuda())
            torch.cuda.synchronize()
            _, fwd_n, _, bwd_n = F.timing_read()
        finally:
            F.timing_enable(False)
    print('timing counters of one forward + backward:', fwd_n, bwd_n)
    assert not copies, copies
    for t in h.tensors:
        assert t.data_ptr() in seen
    assert (fwd_n, bwd_n) == (1, 1), (fwd_n, bwd_n)
    # and the helper itself: the caller's object
    for t in h.tensors:
        assert real_aligned(t.detach().contiguous()).data_ptr() == t.data_ptr()
    monkeypatch.undo()

    # both host paths, the native one too (no Python to spy on): the caching allocator's count of allocations.  A forward +
    # backward on the caller's aligned tensors makes N of them; the same call with ONLY the input one element into a flat
    # buffer makes exactly one more — the realignment copy — so none of the N is a copy of an aligned tensor
    def allocations(tensors):
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        y = P.adi_diffuse(*tensors, sweeps, clamp_max=10.0, checkpoints=0)
        (gu,) = torch.autograd.grad(y, tensors[0], gyd)
        torch.cuda.synchronize()
        return torch.cuda.memory_stats()["allocation.all.allocated"] - before

    gyd = gy.cuda()
    off = hold(values, "flat").tensors[:1] + h.tensors[1:]       # the input off 16 bytes, the coefficients the caller's own
    assert off[0].data_ptr() % 16 == 4
    for native in (True, False):
        with _host_path(native):
            allocations(h.tensors)                               # (warm: descriptors, pinned slots)
            n_aligned, n_off = allocations(h.tensors), allocations(off)
            print("allocations of one forward + backward, native" if native else "ctypes", n_aligned, n_off)
            assert n_off == n_aligned + 1, (native, n_aligned, n_off)
