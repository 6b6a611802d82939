"""The coefficient stage of the implicit (ADI) layers — adi_factor_kernel / adi_flags_kernel / adi_kmax_kernel /
adi_pgrad_kernel of csrc/pde_adi.hip and gen_factor / gen_bwd_kernel of csrc/pde_adi_gen.hip — held to fp64 at its clamp
and smoothing edges, through every backward body that consumes the pass-through mask and the per-channel flag: the two
halves of the HIP backward's grid (A), the assembly backward with its masked-only launch (B), the per-step launches of a
layer with a channel operator (C), the one-launch C <= 4 kernel (D), the any-size kernel (E), the emitting variant (F), and
the one-launch wide forward at C = 32 / 64, which reads its own lane-major copy of the records, with the per-step backward
behind it — without checkpoints and with a step-local mask, which first recomputes the operator outputs in place (G).

Cases, scenarios S1-S8 and the fp64 reference: tests/adi_edge_cases.py (checked on the CPU by tests/test_adi_edge_cases.py,
which also shows that a wrong comparison operator, a mask taken from the wrong sweep or time, or a wrong end weight of the
transposed smoothing moves a designated element by at least ten tolerances).  Every test asserts the path it claims before
it compares.  Tolerances: 1e-5 (golden_util.rel_err), 2e-5 for the 66-sweep schedule, 1e-12 for float64 tensors; blocked
elements are exactly 0.0."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import adi_edge_cases as E
import golden_util as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
IO = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
TOL16 = {"bf16": 2e-2, "f16": 2e-3}      # test_gpu_fuzz.py::test_random_bf16_case_vs_oracle; test_gpu_f16.py TOL_CAST / TOL_PGRAD
FWD_KERNEL_B = 3                         # family B's forward: the hand-over schedule of the HIP kernel (pde_adi_forward_kernel)


def _sweeps(case):
    from cnn_with_pde_amd import functional as F
    return tuple(F.Sweep(a, d, (case.dx if a == 0 else case.dy) ** 2, t) for a, d, t in case.sweeps)


def _steps(case):
    sw, sps = _sweeps(case), {"strang": 3, "lie": 2}[case.sched]
    return [list(sw[k:k + sps]) for k in range(0, len(sw), sps)]


def _desc(case, B=None):
    import cnn_with_pde_amd._lib as L
    from cnn_with_pde_amd import functional as F
    io = {"f32": L.PDE_IO_F32, "bf16": L.PDE_IO_BF16, "f16": L.PDE_IO_F16}[case.io]
    return F._build_desc(B or case.B, case.C, case.N, io, _sweeps(case), case.smooth3, case.clamp_max, E.EPS)


def _nck(case, p):
    from cnn_with_pde_amd import functional as F
    bits = case.ckpt_bits()
    if bits == "auto":
        bits = F.plan_checkpoints(E.kappa_reference(case, p))
    return bin(bits).count("1")


def assert_path(case, p, ud):
    """The kernels the case claims are the ones the library will run."""
    import cnn_with_pde_amd._lib as L
    from cnn_with_pde_amd import functional as F
    lib = L.load()
    H, W = case.shape
    if case.W:
        assert lib.pde_adi_rect_supported(H, W)
        return
    path = lib.pde_adi_line_length_path(case.N)
    if case.io == "f64":
        assert F._is_f64(ud)                       # the any-size kernels instantiated for double, at every line length
        return
    d = _desc(case)
    fwd, bwd = lib.pde_adi_forward_kernel(ctypes.byref(d)), lib.pde_adi_backward_kernel(ctypes.byref(d), _nck(case, p))
    if case.family == "E":
        assert (path, fwd, bwd) == (2, 2, 2)
        return
    assert path == 1
    if case.family == "G":                                           # the one-launch wide forward (pde_adi_wide.h)
        assert lib.pde_adi_mixed_one_launch(ctypes.byref(d), {"strang": 3, "lie": 2}[case.sched]) == 1
        assert not F.adi_small_supported(ud, _steps(case), case.smooth3, case.clamp_max, E.EPS)
        assert (_nck(case, p) > 0) == case.name.endswith("-ckpt")    # the twin reaches the backward's recompute branch
        return
    if case.family == "B":
        assert fwd == FWD_KERNEL_B
        assert bwd == (0 if case.name.endswith("-ckpt") else 1)     # 1: assembly kernel, then the masked-only launch
        return
    assert (fwd, bwd) == (0, 0)
    small = F.adi_small_supported(ud, _steps(case), case.smooth3, case.clamp_max, E.EPS) if case.mix != "none" else None
    if case.family == "C":
        assert not small and case.C not in (32, 64)                  # neither one-launch family: per-step launches
    if case.family == "D":
        assert small


def run(case):
    """The case through the public function of its family; returns (y, gu, {name: grad}) on the CPU."""
    from cnn_with_pde_amd import functional as F
    (u, p, gy), _ = E.cached(case)
    dt = IO[case.io]
    pdt = dt if case.io in ("f16", "f64") else torch.float32
    ud = u.to(dt).cuda().requires_grad_(True)
    ps = {k: p[k].to(pdt).cuda().requires_grad_(True) for k in p}
    assert_path(case, p, ud)
    kw = dict(smooth3=case.smooth3, clamp_max=case.clamp_max, eps=E.EPS, checkpoints=case.ckpt_bits())
    four = [ps[k] for k in E.NAMES]
    if case.family in ("C", "G"):
        y = F.adi_diffuse_mixed(ud, *four, ps["M"], _steps(case), case.mix, **kw)
    elif case.family == "D":
        y = F.adi_diffuse_small(ud, *four, ps["M"], _steps(case), case.mix, **kw)
    elif case.family == "F":
        y = F.adi_diffuse_states(ud, *four, _sweeps(case), list(case.emit), **kw)
    else:
        y = F.adi_diffuse(ud, *four, _sweeps(case), **kw)
    assert y.dtype == dt
    y.backward(gy.to(dt).cuda())
    torch.cuda.synchronize()
    return y.detach().cpu(), ud.grad.cpu(), {k: v.grad.cpu() for k, v in ps.items()}


def check(case, got):
    """Assertions 1-3 of the module docstring's families; returns the per-tensor errors."""
    _, (y_ref, gu_ref, gp_ref) = E.cached(case)
    y, gu, gp = got
    tol = TOL16.get(case.io, case.tol)
    errs = {"y": G.rel_err(y, y_ref), "gu": G.rel_err(gu, gu_ref)}
    errs.update({k: G.rel_err(gp[k], gp_ref[k]) for k in gp_ref})
    print(case.name, {k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v <= tol}
    assert not bad, (bad, errs)
    has_y = any(a == 1 for a, _, _ in case.sweeps)
    for q in E.placements(case):
        for k in (q.axis + "_base", q.axis + "_time_coeff"):
            g, r = gp[k].double()[q.c, q.i, q.j], gp_ref[k][q.c, q.i, q.j]
            if q.scen in E.ZERO:
                assert float(g) == 0.0, (q, k, float(g))                 # exactly: the mask multiplies, nothing leaks
            if case.io not in TOL16:
                assert abs(float(g - r)) <= tol * float(gp_ref[k].abs().max()), (q, k, float(g), float(r))
    if not has_y:
        assert not gp["beta_base"].any() and not gp["beta_time_coeff"].any()
    if case.smooth3 and case.io not in TOL16:
        # line ends of the channel that is NOT flagged: the epilogue's transposed smoothing with doubled end weights,
        # and — with exactly one flagged channel beside it — that this channel was computed by exactly one body
        for ax, (c, m) in E.line_ends(case).items():
            for k in (ax + "_base", ax + "_time_coeff"):
                d = (gp[k].double()[c] - gp_ref[k][c])[m].abs().max()
                assert float(d) <= tol * float(gp_ref[k].abs().max()), (ax, k, float(d))
    return errs


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_case_vs_fp64(name):
    case = E.BY_NAME[name]
    check(case, run(case))


def test_checkpointed_twin_shares_inputs_and_reference():
    """Family B's cases with one checkpoint bit leave the assembly kernel for the HIP one on the SAME inputs."""
    for c in E.CASES:
        if c.name.endswith("-ckpt"):
            twin = E.BY_NAME[c.name[:-5]]
            (u0, p0, gy0), _ = E.cached(twin)
            (u1, p1, gy1), _ = E.cached(c)
            assert torch.equal(u0, u1) and torch.equal(gy0, gy1) and all(torch.equal(p0[k], p1[k]) for k in p0)


@pytest.mark.parametrize("name", ["A-n8-c3-strang", "B-n32-c3-2steps"])
def test_bitwise_repeatable(name):
    case = E.BY_NAME[name]
    a = run(case)
    torch.empty(1 << 22, device="cuda").normal_()                       # unrelated work in between
    torch.mm(torch.ones(256, 256, device="cuda"), torch.ones(256, 256, device="cuda"))
    b = run(case)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


# ---- the per-sweep coefficient maxima on the fused sizes ---------------------------------------------------------------
@pytest.mark.parametrize("case,where", E.kappa_cases(), ids=[c.name for c, _ in E.kappa_cases()])
def test_kappa_max_on_fused_sizes(case, where):
    """adi_kmax_kernel (kappa_max_async) and the factor kernel's partials reduced by adi_flags_kernel (the forward's own
    values, through the mapped host buffer or the copy): the same float, and the fp64 value — exactly without smoothing
    (dyadic inputs), to 1e-6 with it (a spike at a line end: the replicate weight decides)."""
    import cnn_with_pde_amd._lib as L
    from cnn_with_pde_amd import functional as F
    assert L.load().pde_adi_line_length_path(case.N) == 1
    u, p, gy = E.make_inputs(case)
    q = E.place_kappa_peak(case, p, where)
    want = E.kappa_reference(case, q)
    ps = [q[k].float().cuda().requires_grad_(True) for k in E.NAMES]
    kw = dict(smooth3=case.smooth3, clamp_max=case.clamp_max, eps=E.EPS)
    ud = u.float().cuda()
    km = F.kappa_max_async(ud, *ps, _sweeps(case), **kw)
    km.event.synchronize()
    alone = km.host.tolist()[:len(want)]
    sink = []
    F.adi_diffuse(ud, *ps, _sweeps(case), checkpoints="auto", kmax_sink=sink, **kw)
    assert len(sink) == 1
    fused = sink[0].wait()[:len(want)]
    print(case.name, alone, want)
    assert alone == fused, (alone, fused)
    if case.smooth3:
        assert max(abs(a - b) / b for a, b in zip(alone, want)) < 1e-6, (alone, want)
    else:
        assert alone == [float(torch.tensor(v, dtype=torch.float32)) for v in want], (alone, want)
    if where == "clamped" and not case.smooth3:
        for (axis, delta, t), v in zip(case.sweeps, alone):
            assert v == case.clamp_max * delta / (case.dx if axis == 0 else case.dy) ** 2


def test_kappa_max_through_the_copy_path():
    """The same kappa tests with the maxima reaching the host through a device buffer and a copy (PDE_KMAX_MAPPED is read
    once per process: a child interpreter, as tests/test_gpu_env_paths.py does)."""
    env = dict(os.environ, PDE_KMAX_MAPPED="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_adi_edges.py", "-k", "test_kappa_max_on_fused_sizes"],
                       cwd=os.path.dirname(HERE), env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-1500:] + (r.stderr or "")[-500:]
    assert r.returncode == 0, tail
    assert f"{len(E.kappa_cases())} passed" in r.stdout and "failed" not in r.stdout, tail
