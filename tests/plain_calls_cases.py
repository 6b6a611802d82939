"""The cases of tests/golden/plain_calls/parent.npz (tools/record_plain_calls.py, tests/test_gpu_plain_calls.py): the
smallest shapes that reach every dispatch the autograd nodes of functional.py choose between — square / rectangle,
fused / any-size kernels, fp32 / bf16 / fp16 / float64, every checkpoint policy, the Jacobi workspace path and the step
counts a trajectory call does not take — each through the public functions only, as a plain call and (unless ``traj`` is
None) as a trajectory call selecting two steps.  Inputs and cotangents come from one seeded CPU generator per case."""
import torch

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64


def _adi(name, shape, dtype=F32, pdtypes=(F32,) * 4, ck="auto", sink=False, traj=True, flat=False):
    return dict(name=name, family="adi", shape=shape, dtype=dtype, pdtypes=pdtypes, ck=ck, sink=sink, flat=flat,
                traj=(2, 5) if traj else None, grad=True, backward=True)


def _ex(name, shape, dtype=F32, steps=3, traj=True, grad=True):
    return dict(name=name, family="explicit5", shape=shape, dtype=dtype, pdtypes=(F64 if dtype == F64 else F32,) * 2,
                steps=steps, traj=(1, 3) if traj else None, grad=grad, backward=grad)


def _jac(name, shape, nt, dtype=F32, traj=None, backward=True):
    pd = dtype if dtype in (F16, F64) else F32
    return dict(name=name, family="jacobi", shape=shape, dtype=dtype, pdtypes=(pd, pd), steps=nt, traj=traj, grad=True,
                backward=backward)


CASES = [
    # implicit sweeps: two Strang steps = 6 sweeps; a trajectory call emits the state after each step
    _adi("adi_fused_auto", (3, 2, 8, 8)),
    _adi("adi_fused_ck0", (3, 2, 8, 8), ck=0),
    _adi("adi_fused_ck101", (3, 2, 8, 8), ck=0b101),
    _adi("adi_fused_auto_sink", (3, 2, 8, 8), sink=True),
    _adi("adi_asm_backward", (2, 8, 32, 32), sink=True, traj=False),     # the sink keeps the call on the ctypes node
    _adi("adi_anysize", (3, 2, 10, 10)),
    _adi("adi_anysize_bf16", (3, 2, 10, 10), dtype=BF16),
    _adi("adi_rect", (2, 2, 6, 10)),
    _adi("adi_f64_input", (2, 2, 8, 8), dtype=F64),
    _adi("adi_f64_param", (2, 2, 8, 8), pdtypes=(F64, F32, F32, F32)),
    _adi("adi_rect_f64", (2, 2, 6, 10), dtype=F64, pdtypes=(F64,) * 4),
    _adi("adi_f16", (2, 1, 8, 8), dtype=F16, pdtypes=(F16,) * 4),
    _adi("adi_f16_widened", (2, 1, 8, 8), dtype=F16),
    _adi("adi_flat_param", (2, 1, 8, 8), flat=True),                      # (N, N) parameters at C = 1
    # explicit 5-point, 3 steps
    _ex("ex_wave", (2, 2, 16, 16)),
    _ex("ex_wave_bf16", (2, 2, 16, 16), dtype=BF16),
    _ex("ex_col", (2, 2, 5, 7)),
    _ex("ex_vec4", (2, 2, 8, 8)),
    _ex("ex_f64", (2, 2, 5, 7), dtype=F64),
    _ex("ex_wave_no_grad", (2, 2, 16, 16), grad=False),
    _ex("ex_130_steps", (1, 1, 16, 16), steps=130, traj=False),
    # Jacobi
    _jac("jac", (2, 8, 8), 3, traj=(1, 3)),
    _jac("jac_f16", (2, 8, 8), 3, dtype=F16, traj=(1, 3)),
    _jac("jac_f64", (2, 8, 8), 3, dtype=F64, traj=(1, 3)),
    _jac("jac_tiled_ws", (1, 70, 66), 12, traj=(5, 12)),                  # more steps than one tiled launch takes
    _jac("jac_nt0", (1, 8, 8), 0, backward=False),
    _jac("jac_130_steps", (1, 8, 8), 130),
]


def _inputs(case, g):
    """(u, parameters) on the CPU, in the case's types."""
    shape = case["shape"]
    u = torch.randn(*shape, generator=g).to(case["dtype"])
    if case["family"] == "adi":
        Cc, H, W = shape[1:]
        ps = (Cc, H, W) if not case["flat"] else (H, W)
        raw = [0.2 * (1 + 0.5 * torch.rand(ps, generator=g)), 0.2 * (1 + 0.5 * torch.rand(ps, generator=g)),
               0.5 * torch.randn(ps, generator=g), 0.5 * torch.randn(ps, generator=g)]
    elif case["family"] == "explicit5":
        Cc = shape[1]
        raw = [0.05 * (1 + 0.5 * torch.rand(Cc, generator=g)), 1 + 0.1 * torch.randn(Cc, generator=g)]
    else:
        H, W = shape[1:]
        raw = [0.05 + 0.1 * torch.rand(H, generator=g), 0.05 + 0.1 * torch.rand(W, generator=g)]
    return u, [p.to(dt) for p, dt in zip(raw, case["pdtypes"])]


def _call(F_, case, u, params, traj):
    if case["family"] == "adi":
        sweeps = tuple(s for st in F_.adi_schedule(0.5, 1.0, 1.0, 2, "strang") for s in st)
        sink = [] if case["sink"] else None
        if traj:
            y = F_.adi_diffuse_states(u, *params, sweeps, case["traj"], checkpoints=case["ck"], kmax_sink=sink)
        else:
            y = F_.adi_diffuse(u, *params, sweeps, checkpoints=case["ck"], kmax_sink=sink)
        if sink is not None and u.requires_grad:
            assert len(sink) == 1, "the call did not hand out its coefficient maxima"
        return y
    if case["family"] == "explicit5":
        if traj:
            return F_.explicit5_states(u, *params, steps=case["traj"])
        return F_.explicit5_step(u, *params, num_steps=case["steps"])
    if traj:
        return F_.jacobi_diffuse_states(u, *params, case["traj"])
    return F_.jacobi_diffuse(u, *params, case["steps"])


def run_case(F_, case, traj, dev="cuda"):
    """One call of ``case`` (``traj``: its trajectory twin) through the functions of ``F_``.  Returns
    ({name: CPU tensor} of the output, the input gradient and every parameter gradient; the output on the device)."""
    g = torch.Generator().manual_seed(1000 + [c["name"] for c in CASES].index(case["name"]))
    u, params = _inputs(case, g)
    u = u.to(dev).requires_grad_(case["grad"])
    params = [p.to(dev).requires_grad_(case["grad"]) for p in params]
    with torch.enable_grad() if case["grad"] else torch.no_grad():
        y = _call(F_, case, u, params, traj)
    res = {"y": y.detach().cpu()}
    if case["backward"]:
        gy = torch.randn(*y.shape, generator=g).to(y.dtype).to(dev)
        y.backward(gy)
        res["gu"] = u.grad.cpu()
        for i, p in enumerate(params):
            res[f"g{i}"] = p.grad.cpu()
    torch.cuda.synchronize()
    return res, y


def variants():
    """(case, traj) of every recorded call."""
    for case in CASES:
        yield case, False
        if case["traj"] is not None:
            yield case, True


def key(case, traj, name, t):
    """The fixture's key of one result: the tensor's dtype is part of it, so a changed dtype is a missing key."""
    return f"{case['name']}|{'traj' if traj else 'plain'}|{name}|{str(t.dtype).replace('torch.', '')}"


def to_numpy(t):
    """16-bit tensors are stored widened to fp32 (exact); ``torch.equal`` on the widened values is equality of the bits up
    to the sign of zero and NaN payloads, as it is on the tensors themselves."""
    return (t.float() if t.dtype in (BF16, F16) else t).numpy()
