"""The shared-input layer group (pde_adi_multi_forward / pde_adi_multi_backward through P.diffuse_shared_input) in both
launch arrangements — side by side (B < 1024) and one after the other (B >= 1024) — against the fp64 references of
tests/shared_input_cases.py: every output and every gradient of every case of its table, the three tensor types, and the
bitwise properties that follow from the kernel's code (csrc/pde_adi_small.h).  DESIGN §5 has the table and the figures."""
import contextlib
import functools
import io

import pytest
import torch

import golden_util as G
import shared_input_cases as S

pytestmark = pytest.mark.gpu

ALL = [c.name for c in S.CASES]
F32 = [c.name for c in S.F32_CASES]
IO16 = [c.name for c in S.IO16_CASES]
CTYPES_PATH = ["par-n32-c4-l4", "seq-n16-c3-l3-1024"]       # one case of each arrangement also through _AdiMultiFn

#: (case, result) -> (bound, measured on the MI355X, the fp32 oracle's own distance from fp64): results that miss the
#: limit of ``S.limits`` and are pinned with the bound they meet, as tests/test_gpu_fuzz.py PINNED does.  None needed.
PINNED = {}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _layers(case, inp):
    import cnn_with_pde_amd as P
    cls = P.EnhancedDiffusionLayer if case.kind == "cifar10" else P.LearnableDiffusionLayer
    out = []
    for ly, p in zip(case.layers, inp.params):
        m = quiet(cls, case.N, case.C, dt=ly.dt, num_steps=ly.steps, dx=ly.dx, dy=ly.dx)
        with torch.no_grad():
            for k, v in p.items():
                getattr(m, k).copy_(v.float())
        m.checkpoint_policy = ly.ckpt
        out.append((m.half() if case.io == "f16" else m).cuda())
    return out


def _tiled(case, t, dtype):
    return None if t is None else t.to(dtype)[case.index()].cuda()


def _run(case, inp, layers, path="native", only=None):
    """One forward and one backward of the group on the tiled batch; every result on the CPU, keyed like
    ``S.Reference.flat``.  ``only``: gys / gs reach these layers only (and nothing arrives at `out`)."""
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import functional as F_
    iot = S.IO_DTYPE[case.io]
    pt = torch.float16 if case.io == "f16" else torch.float32
    for m in layers:
        for p in m.parameters():
            p.grad = None
    x = _tiled(case, inp.u, iot).requires_grad_(True)
    w = inp.w.to(pt).cuda().requires_grad_(True) if inp.w is not None else None
    if path == "native":
        out, ys, sums = P.diffuse_shared_input(layers, x, w, plane_sums=True)
        node = ys[0].grad_fn
        assert type(node).__name__ == "CppFunction" and "MultiFn" in node.name(), "not the fused native host path"
    else:
        specs = tuple((F_._as_schedule(m._schedule()), bool(m._smooth3), m._clamp_max, float(m.stability_eps)) for m in layers)
        flat = [t for m in layers for t in (m.alpha_base, m.beta_base, m.alpha_time_coeff, m.beta_time_coeff, m.channel_mixing)]
        ck = "auto" if case.layers[0].ckpt == "auto" else tuple(int(ly.ckpt) for ly in case.layers)
        res = F_._AdiMultiFn.apply(x, w, specs, True, ck, *flat)
        out, ys, sums = res[0], list(res[1:1 + case.L]), list(res[1 + case.L:])
        assert type(ys[0].grad_fn).__name__ == "_AdiMultiFnBackward", "not the fused ctypes path"
    assert out is None or out.dtype == iot
    assert all(y.dtype == iot for y in ys)
    heads, grads = [], []
    if only is None and inp.gy is not None:
        heads.append(out)
        grads.append(_tiled(case, inp.gy, iot))
    for i in range(case.L):
        if only is not None and i not in only:
            continue
        if inp.gys[i] is not None:
            heads.append(ys[i])
            grads.append(_tiled(case, inp.gys[i], iot))
        if inp.gs[i] is not None:
            heads.append(sums[i])
            grads.append(_tiled(case, inp.gs[i], sums[i].dtype))
    torch.autograd.backward(heads, grads)
    torch.cuda.synchronize()
    got = {"gu": x.grad}
    for i in range(case.L):
        got[f"y{i}"], got[f"s{i}"] = ys[i].detach(), sums[i].detach()
        for k, p in layers[i].named_parameters():
            got[f"g{i}.{k}"] = p.grad
    if w is not None:
        got["out"] = out.detach()
        got["g_weight"] = w.grad
    return {k: v.cpu() for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def results(name, path="native"):
    """The group's results on a case, computed once per process and shared (never modified)."""
    case = S.BY_NAME[name]
    inp, _ = S.cached(name)
    return _run(case, inp, _layers(case, inp), path)


def _per_sample(case, key):
    return key == "gu" or key == "out" or key[0] in "ys"


def _arrangement(case):
    """The row's arrangement, from the kernel's own rule (csrc/pde_adi.hip multi_parallel: L > 1 and B < 1024)."""
    side_by_side = case.L > 1 and case.B < 1024
    assert side_by_side == (case.arrangement == "par")
    assert (case.L > 1 and case.B >= 1024) == (case.arrangement == "seq")
    if case.arrangement == "par":
        assert case.B * case.L <= 1023 * 4


def _check(case, got, ref, limits, what, keys=None):
    _arrangement(case)
    idx = case.index()
    flat = ref.flat()
    assert set(flat) == set(got), set(flat) ^ set(got)
    if keys is not None:
        flat = {k: flat[k] for k in keys}
    errs = {}
    for k, r in flat.items():
        r = r[idx] if _per_sample(case, k) else r
        errs[k] = G.rel_err(got[k].reshape(r.shape), r)
    print(what, case.name, {k: f"{v:.2e}" for k, v in errs.items()})
    lim = {k: PINNED.get((case.name, k), (limits[k],))[0] for k in errs}
    bad = {k: (v, lim[k]) for k, v in errs.items() if not v <= lim[k]}
    assert not bad, bad
    return errs


# ---- a. against fp64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F32)
def test_fp32_group_against_fp64(name):
    """y_i, s_i, out, gu, the four coefficient gradients and gM of every layer, and g_weight: rel_err <= 1e-5 against the
    fp64 oracle; results of at most four entries (gM at C <= 2, g_weight) within max(2e-5, 4 * min(oracle32, 1e-4)),
    oracle32 the fp32 oracle's own distance from fp64 on the case (tests/test_gpu_fuzz.py::check_case)."""
    case = S.BY_NAME[name]
    _check(case, results(name), S.cached(name)[1], S.limits(case), "fp64")


@pytest.mark.parametrize("name", CTYPES_PATH)
def test_fp32_group_against_fp64_through_the_ctypes_path(name):
    case = S.BY_NAME[name]
    got = results(name, "ctypes")
    _check(case, got, S.cached(name)[1], S.limits(case), "fp64/ctypes")
    for k, v in results(name).items():                   # the two host paths make the same call
        assert torch.equal(v, got[k]), k


# ---- b. layers that received no gradient -----------------------------------------------------------------------------
def test_layer_without_incoming_gradient():
    """seq-n28-c2-l2-lie-2049 with gys / gs for layer 1 only: layer 0 walks its samples with a zero adjoint — its
    parameter gradients are exactly 0 — and gu is layer 1's alone."""
    case = S.BY_NAME["seq-n28-c2-l2-lie-2049"]
    _arrangement(case)
    inp, _ = S.cached(case.name)
    got = _run(case, inp, _layers(case, inp), only=(1,))
    ref = S.reference(case, inp, only_layers=(1,))
    for k, v in got.items():
        if k.startswith("g0."):
            assert float(v.abs().max()) == 0.0, k
    assert float(ref.gu.abs().max()) > 0
    assert G.rel_err(got["gu"], ref.gu[case.index()]) <= S.TOL
    for k, v in ref.gp[1].items():
        lim = S.limits(case)[f"g1.{k}"]
        assert G.rel_err(got[f"g1.{k}"], v) <= lim, k


# ---- c. bitwise -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_group_outputs_equal_the_one_layer_calls_bitwise(name):
    """The per-layer arithmetic does not depend on L or on the arrangement: y_i is ``layers[i](x)`` (the one-launch
    kernel with L = 1, states kept as in the group), s_i the plane sum of the one-layer group."""
    import cnn_with_pde_amd as P
    case = S.BY_NAME[name]
    _arrangement(case)
    inp, _ = S.cached(name)
    got = results(name)
    layers = _layers(case, inp)
    x = _tiled(case, inp.u, S.IO_DTYPE[case.io]).requires_grad_(True)
    for i, m in enumerate(layers):
        assert m.small_channel_kernels
        y = m(x)
        assert torch.equal(y.detach().cpu(), got[f"y{i}"]), i
        _, _, s = P.diffuse_shared_input([m], x, plane_sums=True)
        assert torch.equal(s[0].detach().cpu(), got[f"s{i}"]), i


@pytest.mark.parametrize("name", ALL)
def test_periodic_batch_gives_periodic_results_bitwise(name):
    """x[b] = x[b mod P]: y_i, s_i, out and gu of sample b equal those of sample b mod P — a workgroup's first, second
    and third trips, and the layer boundaries behind each, against one another."""
    case = S.BY_NAME[name]
    _arrangement(case)
    got = results(name)
    idx = case.index()
    for k, v in got.items():
        if _per_sample(case, k):
            assert v.shape[0] == case.B
            assert torch.equal(v, v[:case.P][idx]), k


@pytest.mark.parametrize("name", ALL)
def test_two_calls_in_a_row_are_bitwise_equal(name):
    case = S.BY_NAME[name]
    inp, _ = S.cached(name)
    again = _run(case, inp, _layers(case, inp))
    for k, v in results(name).items():
        assert v.dtype == again[k].dtype and torch.equal(v, again[k]), k


# ---- d. out against its definition ------------------------------------------------------------------------------------
EPS = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TINY = {"f32": 0.0, "bf16": 0.0, "f16": 2.0 ** -25}


@pytest.mark.parametrize("name", [c.name for c in S.CASES if c.weights])
def test_out_is_the_weighted_sum_of_the_groups_own_outputs(name):
    """|out - S| <= (L+1) eps A + (L+1) tiny elementwise, S = sum_i w_i y_i in fp64 from the group's own y_i (tied to
    the reference above), A = sum_i |w_i y_i|, eps the unit roundoff of the tensor type (2^-24, 2^-8, 2^-11), tiny half
    the spacing of fp16's subnormals (absolute error of a rounding below 2^-14).

    Side by side: layer i's workgroup stores t_i = r(w_i y_i), one rounding to the tensor type (error <= eps |w_i y_i|);
    the combining launch adds the slabs in layer order in fp32 (L-1 roundings of 2^-24 |partial sum| <= 2^-24 A each) and
    rounds the sum to the tensor type once (<= eps (A + the errors before)): in all <= (2 eps + (L-1) 2^-24) A (1 + eps)
    for 16-bit tensors and <= L eps A (1 + eps)^L for fp32.
    One after the other: out_0 = r(w_0 y_0), out_i = r(fma(w_i, y_i, out_{i-1})) with out_{i-1} re-read from the
    workgroup's own store in the tensor type: L roundings, each <= eps |partial sum| <= eps A (1 + eps)^i, in all
    <= ((1 + eps)^L - 1) A = L eps A (1 + O(L eps)); with eps = 2^-8 and L = 4 that is 4.02 eps A.
    A single layer: out = r(w_0 y_0), one rounding.  (L+1) eps A covers all three."""
    case = S.BY_NAME[name]
    _arrangement(case)
    inp, _ = S.cached(name)
    got = results(name)
    pt = torch.float16 if case.io == "f16" else torch.float32
    w = inp.w.to(pt).double()                             # what the kernel reads: the weights widened to fp32
    terms = [w[i] * got[f"y{i}"].double() for i in range(case.L)]
    Ssum, A = sum(terms), sum(t.abs() for t in terms)
    bound = (case.L + 1) * EPS[case.io] * A + (case.L + 1) * TINY[case.io]
    diff = (got["out"].double() - Ssum).abs()
    worst = float((diff / (EPS[case.io] * A + TINY[case.io])).max())
    print("out", name, f"worst |out - S| = {worst:.3f} (eps A + tiny), allowed {case.L + 1}")
    assert bool((diff <= bound).all()), worst


# ---- e. 16-bit tensors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IO16)
def test_16_bit_group_against_the_state_cast_reference(name):
    """bf16 / fp16 tensors against the fp64 oracle that rounds its state where this kernel does (the sweep output of every
    step, shared_input_cases.kernel_cast): the limits of the one-layer tests for the same quantities — 2e-2 for bf16
    (tests/test_gpu_small.py), 2e-3 for fp16 (tests/test_gpu_f16.py TOL_CAST, TOL_PGRAD).  g_weight has no one-layer limit:
    four times the fp32 rounding oracle's distance from the fp64 one (at most 1.7e-4, bf16-par) is below the one-layer
    limit, which therefore holds it too (tests/test_shared_input_cases.py).

    gu, the coefficient gradients and gM are also held, at the same limits, to the reference with the rounding points of
    oracle.pde_oracle.adi_forward's state_cast (behind every operator too, adjoints rounded), which the one-layer limits were
    made with; g_weight is not: those extra roundings alone move the two-entry sum of f16-seq by 4.1e-3."""
    case = S.BY_NAME[name]
    got = results(name)
    inp, _ = S.cached(name)
    keys = ["gu"] + [f"g{i}.{k}" for i in range(case.L) for k in inp.params[i]]
    _check(case, got, S.reference(case, inp, points="oracle"), S.limits(case), "state_cast/oracle points", keys)
    pdt = torch.float16 if case.io == "f16" else torch.float32
    for k, v in got.items():
        want = S.IO_DTYPE[case.io] if _per_sample(case, k) and k[0] != "s" else pdt
        assert v.dtype == want, (k, v.dtype)
    _check(case, got, S.cached(name)[1], S.limits(case), "state_cast")
