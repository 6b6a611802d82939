"""The one-launch wide forward (csrc/pde_adi_wide.h, adi_wide_fwd_kernel: fp32, C = 32 / 64, N = 28 / 32) held to fp64
STAGE BY STAGE, through the C ABI: ``pde_adi_mixed_forward`` is called by ctypes exactly as
``functional._AdiMixedFn.forward`` calls it, with ``states`` and ``y`` NaN-filled, and every state it stores is compared
with the float64 stage reference of tests/wide_cases.py started from the device's own previous stored state.

What is held, per case of C x N x {Strang, Lie} x mode {1, 2} (K = 3, B = 3: the four instantiations per N, both modes):

* ownership of slots: mode 1 writes slots 2k+1 and y, mode 2 slots 2k and y; every other slot is still all NaN;
* the mix stage (mode 2): y against fp64 M states[2(K-1)] — whole tensor 5e-7, per channel 2e-6, the project's standing
  bars for three-piece products (tests/test_gpu_parity.py::test_channel_mix_three_piece_products).  The CPU file
  tests/test_wide_cases.py shows every plausible mistake of the product at least 4 of these bars away;
* the step stages: at most 4 x the distance of the fp32 oracle from the same fp64 reference, computed here for that stage
  and case (the 4 x oracle32 window of tests/test_gpu_fuzz.py);
* one workgroup, several samples (B = 2100 on 2048 workgroups): samples b and b + 2048 bitwise equal to the same call on
  them alone, and their mix stage against fp64."""
import ctypes as C

import pytest
import torch

import wide_cases as W

pytestmark = pytest.mark.gpu


def forward(case, u, p, B=None):
    """``pde_adi_mixed_forward`` as ``_AdiMixedFn.forward`` calls it (no kappa outputs); returns (states, y) on the CPU,
    both NaN-filled before the call."""
    from cnn_with_pde_amd import _lib as L
    from cnn_with_pde_amd import functional as F
    lib = L.load()
    B = B or u.shape[0]
    steps = F.adi_schedule(W.DT, 1.0, 1.0, case.K, case.split)
    sweeps = tuple(s for st in steps for s in st)
    assert [(s.axis, s.delta, s.t) for s in sweeps] == list(case.sweeps)
    d = F._make_desc(B, case.C, case.N, L.PDE_IO_F32, sweeps, case.smooth3, case.clamp_max, W.EPS)
    assert lib.pde_adi_mixed_one_launch(C.byref(d), case.sps) == 1
    ud = u.cuda().contiguous()
    par = [p[k].cuda().contiguous() for k in ("alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff")]
    Md = p["M"].cuda().contiguous()
    sws = F._workspace(lib.pde_adi_steps_workspace_bytes(C.byref(d), case.sps), ud.device)
    states = torch.full((2 * case.K - 1,) + tuple(ud.shape), float("nan"), device=ud.device)
    y = torch.full_like(ud, float("nan"))
    L.check(lib.pde_adi_mixed_forward(C.byref(d), case.sps, case.mode, F._ptr(ud), F._ptr(states), F._ptr(y), F._ptr(Md),
                                      *[F._ptr(t) for t in par], F._ptr(None), F._ptr(None), C.c_void_p(0),
                                      F._ptr(sws), sws.numel(), F._stream()), "pde_adi_mixed_forward")
    torch.cuda.synchronize()
    return states.cpu(), y.cpu()


def stored_slots(case):
    """Slot index of the state step k stores; the last one of mode 1 is y."""
    return [2 * k + 1 if case.mode == 1 else 2 * k for k in range(case.K)]


def check_ownership(case, states, y):
    own = [s for s in stored_slots(case) if s < 2 * case.K - 1]
    for s in range(2 * case.K - 1):
        if s in own:
            assert bool(torch.isfinite(states[s]).all()), f"slot {s} not written everywhere"
        else:
            assert bool(torch.isnan(states[s]).all()), f"slot {s} is not this kernel's to write"
    assert bool(torch.isfinite(y).all())


def check_mix_stage(name, last_state, y, M):
    """y = M (last stored state), from the device's own state: the project's bars for a three-piece product."""
    ref = W.mix(last_state, M)
    whole, per = W.rel_err(y, ref), W.rel_err_channel(y, ref)
    print(f"{name} mix stage: whole {whole:.2e} (bar {W.BAR:.0e}), per channel {per:.2e} (bar {W.BAR_CHANNEL:.0e})")
    assert whole <= W.BAR, whole              # test_gpu_parity.py::test_channel_mix_three_piece_products
    assert per <= W.BAR_CHANNEL, per          # the same test's per-channel bar


def check_step_stages(case, u, p, states, y):
    got = [y if s == 2 * case.K - 1 else states[s] for s in stored_slots(case)]
    prev, bad = u, []
    for k in range(case.K):
        ref = W.step_stage(prev, k, case, p)
        d32 = W.rel_err(W.step_stage(prev, k, case, p, torch.float32), ref)
        dgpu = W.rel_err(got[k], ref)
        print(f"{case.name} step {k}: gpu {dgpu:.2e}, oracle32 {d32:.2e}, ratio {dgpu / d32:.2f}")
        if not dgpu <= W.ORACLE32_FACTOR * d32:           # 4 x oracle32 (tests/test_gpu_fuzz.py)
            bad.append((k, dgpu, d32))
        prev = got[k]                                     # the next stage starts from the device's own state
    assert not bad, bad


@pytest.mark.parametrize("name", [c.name for c in W.CASES])
def test_stages_vs_fp64(name):
    case = W.BY_NAME[name]
    u, p = W.cached(case)
    states, y = forward(case, u, p)
    check_ownership(case, states, y)
    if case.mode == 2:
        check_mix_stage(case.name, states[2 * (case.K - 1)], y, p["M"])
    check_step_stages(case, u, p, states, y)


def test_one_workgroup_several_samples():
    """2100 samples on 2048 workgroups: workgroups 0..51 walk samples b and b + 2048 with the LDS (operator fragments,
    exchange image, the waves' private images inside it) the first sample left.  Both samples of each such workgroup
    equal, bit for bit, the same call on those 104 samples alone (one sample per workgroup), and their stages hold the
    bars of the other cases."""
    case = W.MANY
    u, p = W.cached(case)
    assert case.B > W.GRID and case.B - W.GRID == W.MANY_HEAD and case.K == 1 and case.mode == 2
    idx = torch.cat([torch.arange(W.MANY_HEAD), torch.arange(W.GRID, case.B)])
    states, y = forward(case, u, p)
    check_ownership(case, states, y)
    s_all, y_all = states[0][idx].clone(), y[idx].clone()
    del states, y
    us = u[idx].contiguous()
    s_sub, y_sub = forward(case, us, p)
    assert torch.equal(s_sub[0], s_all) and torch.equal(y_sub, y_all)
    check_mix_stage(case.name + "-many", s_all, y_all, p["M"])
    check_step_stages(case, us, p, s_all.unsqueeze(0), y_all)
