"""The implicit sweeps on bf16 / fp16 tensors are the fp32 route rounded once: a whole-schedule call reads its 16-bit
tensors once, computes in fp32 and rounds to nearest even once on every tensor it writes (include/pdecnn.h,
pde_adi_forward_states).  tests/io16_cases.py has the gates, the case table and the fp64 reference;
tests/test_io16_cases.py shows on the CPU that the gates see a truncating store, one ulp and a misplaced element.

The calls go through the C ABI as functional._AdiFn makes them (``run_states``): *_forward_states and *_backward_states
with the case's emission mask, once with the 16-bit descriptor and once with the fp32 descriptor on the widened values.
The fp32 backward is handed the widened 16-bit ``y``: the backward rebuilds its states from the ``y`` it is given, so that
is the only reference which sees what the 16-bit kernel sees, and the parameter gradients are held to it at 2e-6 (the
bound between two kernels of one arithmetic, test_gpu_asm_bwd.py) instead of 2e-2 against an oracle.

Every figure is printed before it is asserted (lines that begin with ``io16``)."""
import ctypes as C
import os

import pytest
import torch

import io16_cases as K
import test_gpu_f16 as T16
from oracle import pde_oracle as O
from test_gpu_double_backward import mirror  # noqa: F401  (a fixture)
from test_gpu_parity import TOL, quiet

pytestmark = pytest.mark.gpu

ALL = [(c["name"], d) for c in K.TABLE for d in K.DTYPES]
TOL_PGRAD = 2e-6
NAN = float("nan")


def _io(dtype):
    from cnn_with_pde_amd import _lib as L
    return {torch.float32: L.PDE_IO_F32, torch.bfloat16: L.PDE_IO_BF16, torch.float16: L.PDE_IO_F16}[dtype]


def _desc(case, dtype):
    from cnn_with_pde_amd import _lib as L
    from cnn_with_pde_amd import functional as F_
    cls = L.PdeAdiRectDesc if case["family"] == "rect" else L.PdeAdiDesc
    return F_._fill_desc(cls, case["B"], case["C"], case["H"], case["W"], _io(dtype), K.sweeps_of(case), case["smooth3"],
                         case["clamp_max"], case["eps"])


def run_states(case, dtype, inp, y_bwd=None, emit="case", input_only=False):
    """One *_forward_states + *_backward_states of ``case`` on cuda:0 with tensors of ``dtype`` (rect_util.run_entry with an
    I/O type, an emission mask and a ``y`` to hand the backward).  ``inp``: fp32 CPU tensors (io16_cases.inputs).  ``emit``
    None is the plain call (NULL mask, no states).  Outputs are filled with NaN first.  ``input_only`` adds ``gu_input``,
    the gu of *_backward_input_states on the same arguments."""
    from cnn_with_pde_amd import _lib as L
    from cnn_with_pde_amd import functional as F_
    lib = L.load()
    pre = "pde_adi_rect_" if case["family"] == "rect" else "pde_adi_"
    d = _desc(case, dtype)
    emit = case["emit"] if emit == "case" else emit
    vp, st = F_._ptr, F_._stream()
    u, gy = inp["u"].to(dtype).cuda(), inp["gy"].to(dtype).cuda()
    p = [inp[k].cuda().contiguous() for k in K.PARAMS]
    y, gu = torch.full_like(u, NAN), torch.full_like(u, NAN)
    gp = [torch.full_like(t, NAN) for t in p]
    if emit is None:
        states = gst = mask = None
    else:
        gst = inp["gstates"].to(dtype).cuda()
        states = torch.full_like(gst, NAN)
        mask = F_._mask128(sum(1 << s for s in emit))
    nck = bin(case["ckpt"]).count("1")
    nf = getattr(lib, pre + "forward_workspace_bytes")(C.byref(d))
    nb = getattr(lib, pre + "backward_workspace_bytes")(C.byref(d), nck)
    assert nf > 0 and nb > 0, (nf, nb)
    fws, bws = F_._workspace(nf, "cuda"), F_._workspace(nb, "cuda")
    L.check(getattr(lib, pre + "forward_states")(C.byref(d), vp(u), vp(y), vp(states), mask, *[vp(t) for t in p], None, None,
                                                 None, vp(fws), fws.numel(), st), pre + "forward_states")
    yb = y if y_bwd is None else y_bwd.to(dtype).cuda()
    L.check(getattr(lib, pre + "backward_states")(C.byref(d), vp(gy), vp(gst), mask, vp(yb), vp(u if nck else None),
                                                  F_._mask128(case["ckpt"]), vp(gu), *[vp(t) for t in p],
                                                  *[vp(t) for t in gp], vp(fws), vp(bws), bws.numel(), st),
            pre + "backward_states")
    out = {"y": y, "states": states, "gu": gu, "gp": gp}
    if input_only:
        gi = torch.full_like(u, NAN)
        ni = getattr(lib, pre + "backward_input_workspace_bytes")(C.byref(d))
        assert ni > 0
        iws = F_._workspace(ni, "cuda")
        L.check(getattr(lib, pre + "backward_input_states")(C.byref(d), vp(gy), vp(gst), mask, vp(gi), *[vp(t) for t in p],
                                                            vp(fws), vp(iws), iws.numel(), st), pre + "backward_input_states")
        out["gu_input"] = gi
    torch.cuda.synchronize()
    return out


def _gates(tag, got, f32, ref64, tau_rel, equal):
    """The three gates on one tensor; the figures are printed first.  ``got``: the 16-bit call's tensor; ``f32``: the fp32
    route's; ``ref64``: the fp64 reference."""
    dt = got.dtype
    got, f32, ref64 = got.cpu(), f32.cpu(), ref64.double().cpu().reshape(got.shape)
    tau = tau_rel * float(ref64.abs().max())
    err32 = float((f32.double() - ref64).abs().max())
    want = f32.to(dt)
    u, nd = K.ulps(got, want), K.n_diff(got, want)
    ok, worst = K.bracket_ok(got, ref64, tau)
    print(f"io16 {tag}: ulps {u} n_diff {nd}/{got.numel()} fp32_err/tau {err32 / tau:.3f} bracket {'ok' if ok else worst}")
    assert err32 <= tau, (tag, "the fp32 route misses the bound the bracket rests on", err32, tau)
    assert u <= 1, (tag, u, nd)                                               # gate 1
    if equal:
        assert nd == 0 and torch.equal(got, want), (tag, nd)                  # gate 2
    assert ok, (tag, worst)                                                   # gate 3
    return u, nd


@pytest.mark.parametrize("name,dname", ALL)
def test_16_bit_call_is_the_fp32_call_rounded_once(name, dname):
    from cnn_with_pde_amd import _lib as L
    case, dt, inp = K.BY_NAME[name], K.DTYPES[dname], K.inputs(name, dname)
    ref = K.reference(name, dname)
    if case["family"] != "rect":                           # which kernels the plain call of this descriptor runs
        lib, nck = L.load(), bin(case["ckpt"]).count("1")
        for t in (torch.float32, dt):
            d = _desc(case, t)
            kern = lib.pde_adi_forward_kernel(C.byref(d)), lib.pde_adi_backward_kernel(C.byref(d), nck)
            assert kern == K.expected_kernels(case, t == torch.float32, os.environ), (t, kern)
    r16 = run_states(case, dt, inp)
    r32 = run_states(case, torch.float32, inp, y_bwd=r16["y"].float())
    for r, t in ((r16, dt), (r32, torch.float32)):
        assert r["y"].dtype == r["gu"].dtype == r["states"].dtype == t and all(g.dtype == torch.float32 for g in r["gp"])
    equal = case["family"] != "fused"                      # the any-size templates: the tangent pass holds equality there
    tag, tr = f"{name} {dname}", K.tau_rel(case)
    # (a) forward: every emitted state, then y
    for i, s in enumerate(case["emit"]):
        _gates(f"{tag} state[{s}]", r16["states"][i], r32["states"][i], ref["states"][i], tr, equal)
    _gates(f"{tag} y", r16["y"], r32["y"], ref["states"][-1], tr, equal)
    # (b) the input gradient
    _gates(f"{tag} gu", r16["gu"], r32["gu"], ref["gu"], tr, equal)
    # (c) the fp32 parameter gradients against the fp32 backward fed the same y
    worst = 0.0
    for k, a, b in zip(K.PARAMS, r16["gp"], r32["gp"]):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), k
        den = float(b.abs().max())
        assert den > 0, k
        rel = float((a - b).abs().max()) / den
        print(f"io16 {tag} g_{k}: rel {rel:.3e} bitwise {torch.equal(a, b)} n_diff {K.n_diff(a, b)}/{a.numel()}")
        worst = max(worst, rel)
    assert worst <= TOL_PGRAD, (tag, worst)


@pytest.mark.parametrize("dname", list(K.DTYPES))
@pytest.mark.parametrize("name", ["fused12-strang-5x3-cifar", "anysize30", "rect5x9"])
def test_backward_input_is_bitwise_the_full_backward(name, dname):
    r = run_states(K.BY_NAME[name], K.DTYPES[dname], K.inputs(name, dname), input_only=True)
    assert torch.equal(r["gu_input"], r["gu"]), K.n_diff(r["gu_input"], r["gu"])


# ---- (d) the same results through the modules -----------------------------------------------------------------------------
def _set(layer, inp, squeeze):
    with torch.no_grad():
        for k, n in zip(K.PARAMS, ("alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff")):
            getattr(layer, n).copy_(inp[k][0] if squeeze else inp[k])
    layer.checkpoint_policy = 0
    return layer


def _through(layer, u, gy):
    layer.zero_grad(set_to_none=True)
    x = u.clone().requires_grad_(True)
    y = layer(x)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), x.grad, [getattr(layer, n).grad for n in ("alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff")]


def test_bf16_input_into_an_fp32_layer_is_the_c_abi(mirror):  # noqa: F811
    import cnn_with_pde_amd as P
    name = "fused20-strang-5x3-cifar"
    case, inp = K.BY_NAME[name], K.inputs(name, "bf16")
    ly = quiet(P.EnhancedDiffusionLayer, case["H"], case["C"], dt=K.DT, dx=K.DX, dy=K.DY, num_steps=case["steps"],
               channel_mixing_enabled=False)
    ly = _set(ly, inp, False).cuda()
    y, gu, gp = _through(ly, inp["u"].bfloat16().cuda(), inp["gy"].bfloat16().cuda())
    r = run_states(case, torch.bfloat16, inp, emit=None)
    assert y.dtype == gu.dtype == torch.bfloat16
    assert torch.equal(y, r["y"]) and torch.equal(gu, r["gu"])
    for k, a, b in zip(K.PARAMS, gp, r["gp"]):
        assert a.dtype == torch.float32 and torch.equal(a, b), k
    ref = K.reference(name, "bf16", False)["states"][-1]
    ok, worst = K.bracket_ok(y, ref, K.tau_rel(case) * float(ref.abs().max()))
    assert ok, worst


def test_half_layer_is_the_c_abi_and_rounds_its_parameter_gradients_once(mirror):  # noqa: F811
    import cnn_with_pde_amd as P
    name = "fused28-strang-37x1-mnist"
    case = K.BY_NAME[name]
    inp = dict(K.inputs(name, "f16"))
    for k in K.PARAMS:                                     # a half() model holds fp16 parameters: make them exact
        inp[k] = K.exact(inp[k], torch.float16)
    ly = quiet(P.MnistDiffusionLayer, case["H"], K.DT, K.DX, K.DY, case["steps"])
    ly = _set(ly, inp, True).half().cuda()
    assert all(torch.equal(getattr(ly, n).float().cpu(), inp[k][0]) for k, n in
               zip(K.PARAMS, ("alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff")))
    y, gu, gp = _through(ly, inp["u"].half().cuda(), inp["gy"].half().cuda())
    r = run_states(case, torch.float16, inp, emit=None)
    assert y.dtype == gu.dtype == torch.float16
    assert torch.equal(y, r["y"]) and torch.equal(gu, r["gu"])
    for k, a, b in zip(K.PARAMS, gp, r["gp"]):
        assert a.dtype == torch.float16 and torch.equal(a, b.half().reshape(a.shape)), k       # the fp32 sums, rounded once


# ---- (e) the one-launch C <= 4 layers under no_grad: a plain 16-bit call that keeps no states rounds once ------------------
def _operator_layer(kind):
    import cnn_with_pde_amd as P
    gen = torch.Generator().manual_seed(16 + len(kind))
    if kind == "svhn":
        ly, spec = quiet(P.SvhnDiffusionLayer, 16, 3, num_steps=2), O.svhn_spec(16, 3, num_steps=2)
    else:
        ly, spec = quiet(P.EnhancedDiffusionLayer, 16, 3, num_steps=2), O.cifar10_spec(16, 3, num_steps=2)
    T16._perturb(ly, gen)                                  # bases, slopes, an operator that keeps the state's size
    if kind == "svhn":
        with torch.no_grad():
            ly.skip_weight.fill_(0.3)
    return T16._half_exact(ly), spec, gen


@pytest.mark.parametrize("dname", list(K.DTYPES))
@pytest.mark.parametrize("kind", ["svhn", "enhanced"])
def test_one_launch_layers_under_no_grad_round_once(kind, dname):
    dt = K.DTYPES[dname]
    l32, spec, gen = _operator_layer(kind)
    u = K.exact(torch.randn(5, 3, 16, 16, generator=gen), dt)
    params = {k: v.detach().double() for k, v in l32.named_parameters()}
    with torch.no_grad():
        ref = O.adi_forward(u.double(), params, spec)
        l32 = l32.cuda()
        y32 = l32(u.cuda())
        if dt == torch.float16:                            # the float16 route: every parameter fp16 (they are fp16-exact)
            l16 = quiet(lambda: _operator_layer(kind)[0]).half().cuda()
            l16.load_state_dict(l32.state_dict())
        else:
            l16 = l32                                      # bf16 tensors through the fp32 layer
        y = l16(u.to(dt).cuda())
        torch.cuda.synchronize()
    assert y.dtype == dt and y32.dtype == torch.float32
    _gates(f"{kind} no_grad {dname} y", y, y32, ref, TOL, False)
    # the dtype rule beside it: in training mode the same layer keeps its states in the 16-bit type and goes
    # on from them, one rounding per step, so that forward is another tensor (and no single-rounding route)
    y_train = l16(u.to(dt).cuda().requires_grad_(True)).detach()
    nd = K.n_diff(y_train, y)
    print(f"io16 {kind} {dname}: training-mode forward differs from the no_grad forward in {nd}/{y.numel()} elements")
    assert nd > 0
