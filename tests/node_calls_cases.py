"""The cases of tests/golden/node_calls/*.npz (tools/record_node_calls.py, tests/test_gpu_node_calls.py): the smallest
shapes at which each decision of the host glue around the implicit layers can still go wrong — which C entry point a node
calls, what it keeps, whether it asks for coefficient maxima, how it plans checkpoints, how it casts cotangents and shapes
gradients — each through the public functions only.  Every case runs three ways (``WAYS``): everything requires a gradient,
only the input does (frozen parameters), and forward only under ``no_grad``; and through both mirrors of the glue, the
native nodes of csrc/host_ext.cpp and the ctypes nodes of functional.py (``_lib._host = False``).  Inputs and cotangents come
from one seeded CPU generator per case."""
import contextlib
import hashlib
import io

import numpy as np
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
WAYS = ("trainable", "frozen", "no_grad")
SMALL = (3, 3, 16, 16)


def _small(name, mode, dtype=F32, ck="auto", skip=False, shape=SMALL, split="strang", sink=False):
    # a sink keeps the call on the ctypes node in both mirrors
    return dict(name=name, family="small", shape=shape, dtype=dtype, mode=mode, ck=ck, skip=skip, split=split, sink=sink,
                steps=2, native=not sink)


def _states(name, mode, emit, dtype=F32):
    # the C <= 4 trajectory has no native node: always the ctypes path
    return dict(name=name, family="small_states", shape=SMALL, dtype=dtype, mode=mode, emit=emit, ck="auto", steps=3,
                split="strang", native=False)


def _mixed(name, shape, dtype=F32, ck="auto", mode="pre", file="parent"):
    return dict(name=name, family="mixed", shape=shape, dtype=dtype, mode=mode, ck=ck, steps=2, split="strang", native=True,
                file=file)


def _multi(name, nl, weights, sums, ck, dtype=F32, skip_y=None):
    return dict(name=name, family="multi", shape=SMALL, dtype=dtype, nl=nl, weights=weights, sums=sums, ck=ck, skip_y=skip_y,
                native=True)


def _adi(name, shape):
    return dict(name=name, family="adi", shape=shape, dtype=F32, ck="auto", steps=2, split="strang", native=True)


#: (dt, dx, num_steps) of the layers of a shared-input group: different schedules, all Strang
MULTI_SCHEDULES = ((0.5, 1.0, 2), (0.3, 2.0, 3), (0.4, 1.5, 2))

CASES = [
    # C <= 4, the whole time loop in one launch per pass (adi_diffuse_small): two Strang steps on (3, 3, 16, 16)
    _small("small_pre_f32_auto", "pre"),
    _small("small_post_bf16_ck0", "post", dtype=BF16, ck=0),
    _small("small_post_skip_f16_ck01", "post", dtype=F16, ck=0b01, skip=True),
    _small("small_post_skip_f32_auto", "post", skip=True),
    _small("small_lie_n28_c4", "pre", shape=(1, 4, 28, 28), split="lie"),
    _small("small_pre_f32_sink", "pre", sink=True),
    # its trajectory (adi_diffuse_small_states): three steps, the states after steps 0 and 2, or the empty mask
    _states("states_pre_f32_e02", "pre", (0, 2)),
    _states("states_post_bf16_e02", "post", (0, 2), dtype=BF16),
    _states("states_pre_bf16_empty", "pre", (), dtype=BF16),
    _states("states_post_f32_empty", "post", ()),
    # a channel operator between the steps at C > 4 (adi_diffuse_mixed): the per-step pieces at C = 5 ...
    _mixed("mixed_c5_auto", (2, 5, 8, 8)),
    _mixed("mixed_c5_bf16_ck01", (2, 5, 8, 8), dtype=BF16, ck=0b01, mode="post"),
    # ... and the one-launch wide forward.  pde_adi_mixed_one_launch takes C = 32 / 64 fp32 at N = 28 / 32 only (it
    # refuses (2, 32, 16, 16)): (1, 32, 28, 28) is the smallest shape it accepts.  A file of its own: the (32, 28, 28)
    # parameter gradients alone are 400 kB
    _mixed("mixed_wide_auto", (1, 32, 28, 28), file="parent_wide"),
    # several layers on one input (adi_diffuse_multi)
    _multi("multi2_w_auto", 2, True, False, "auto"),
    _multi("multi3_sums_masks_skip_y1", 3, False, True, (0, 0b01, 0b10), skip_y=1),
    _multi("multi2_w_sums_bf16_ck01", 2, True, True, 0b01, dtype=BF16),
    # the plain sweeps through the native node (tests/plain_calls_cases.py keeps the ctypes ones)
    _adi("adi_fused", (3, 2, 8, 8)),
    _adi("adi_anysize", (3, 2, 10, 10)),
    # a layers.py layer under the "lagged" policy, two consecutive forward + backward calls
    dict(name="lagged_fashion", family="lagged", shape=(3, 1, 16, 16), dtype=F32, native=True),
    # the float16 route of a group: every coefficient view is an fp32 copy that only the node keeps alive until the launch
    _multi("multi2_w_f16_auto", 2, True, False, "auto", dtype=F16),
]
for _c in CASES:
    _c.setdefault("file", "parent")
FILES = sorted({c["file"] for c in CASES})


def _coeffs(g, Cc, N, dtype):
    """Coefficients large enough that the "auto" plan of a Strang step sets a checkpoint (1 + 4 * 1.5 * 0.5 per sweep)."""
    ps = (Cc, N, N)
    raw = [1 + 0.5 * torch.rand(ps, generator=g), 1 + 0.5 * torch.rand(ps, generator=g),
           0.5 * torch.randn(ps, generator=g), 0.5 * torch.randn(ps, generator=g)]
    return [p.to(dtype) for p in raw]


def _operator(g, Cc, dtype):
    return (torch.eye(Cc) + 0.1 * torch.randn(Cc, Cc, generator=g)).to(dtype)


def _run_lagged(P, case, way, native, g, dev):
    with contextlib.redirect_stdout(io.StringIO()):
        l = P.FashionDiffusionLayer(size=16, num_steps=2)
    with torch.no_grad():
        for p in (l.alpha_base, l.beta_base):
            p.mul_(1 + 0.2 * torch.rand(p.shape, generator=g))
        for p in (l.alpha_time_coeff, l.beta_time_coeff):
            p.copy_(0.5 * torch.randn(p.shape, generator=g))
    l = l.to(dev).requires_grad_(way == "trainable")
    l.checkpoint_policy = "lagged"
    x = torch.randn(*case["shape"], generator=g).to(dev)
    gy = torch.randn(*case["shape"], generator=g).to(dev)
    res = {}
    for call in range(2):
        for p in l.parameters():
            p.grad = None
        xx = x.clone().requires_grad_(way != "no_grad")
        with torch.no_grad() if way == "no_grad" else torch.enable_grad():
            y = l(xx)
        res[f"y{call}"] = y.detach().cpu()
        if way != "no_grad":
            assert (type(y.grad_fn).__name__ == "CppFunction") == native
            y.backward(gy)
            res[f"gu{call}"] = xx.grad.cpu()
            if way == "trainable":
                for i, p in enumerate(l.parameters()):
                    res[f"g{i}_{call}"] = p.grad.cpu()
    return res


def run_case(P, case, way, native, dev="cuda"):
    """One call of ``case`` run the ``way`` of WAYS through the package ``P``; ``native`` says which mirror ``_lib._host``
    selects at the moment (the caller switches it), and the node that served the call is held to it.  Returns
    {name: CPU tensor}: every output, the input gradient and every parameter / operator / skip-weight / weight gradient."""
    F_ = P.functional
    g = torch.Generator().manual_seed(2000 + [c["name"] for c in CASES].index(case["name"]))
    if case["family"] == "lagged":
        res = _run_lagged(P, case, way, native, g, dev)
        torch.cuda.synchronize()
        return res
    B, Cc, N, _ = case["shape"]
    dt = case["dtype"]
    pdt = F16 if dt == F16 else F32                        # the float16 route needs every parameter in fp16
    train = way == "trainable"
    u = torch.randn(*case["shape"], generator=g).to(dt).to(dev).requires_grad_(way != "no_grad")
    named = {}                                             # parameters whose gradient is recorded

    def par(name, t):
        named[name] = t.to(dev).requires_grad_(train)
        return named[name]

    outs, sink = {}, None
    with torch.no_grad() if way == "no_grad" else torch.enable_grad():
        if case["family"] == "multi":
            layers = []
            for i in range(case["nl"]):
                sdt, sdx, sk = MULTI_SCHEDULES[i]
                co = [par(f"l{i}g{j}", p) for j, p in enumerate(_coeffs(g, Cc, N, pdt))]
                layers.append(dict(alpha_base=co[0], beta_base=co[1], alpha_time_coeff=co[2], beta_time_coeff=co[3],
                                   M=par(f"l{i}gM", _operator(g, Cc, pdt)), steps=F_.adi_schedule(sdt, sdx, sdx, sk)))
            w = par("gw", torch.tensor([0.2, 0.5, 0.3][:case["nl"]]).to(pdt)) if case["weights"] else None
            r = F_.adi_diffuse_multi(u, layers, weights=w, plane_sums=case["sums"], checkpoints=case["ck"])
            node = r[1][0].grad_fn
            if w is not None:                              # without weights ``out`` is not meaningful
                outs["out"] = r[0]
            for i, y in enumerate(r[1]):
                outs[f"y{i}"] = y
            if case["sums"]:
                for i, s in enumerate(r[2]):
                    outs[f"s{i}"] = s
            lossless = {f"y{case['skip_y']}", f"s{case['skip_y']}"} if case["skip_y"] is not None else set()
        else:
            co = [par(f"g{j}", p) for j, p in enumerate(_coeffs(g, Cc, N, pdt))]
            steps = F_.adi_schedule(0.5, 1.0, 1.0, case["steps"], case["split"])
            if case["family"] == "adi":
                y = F_.adi_diffuse(u, *co, tuple(s for st in steps for s in st), checkpoints=case["ck"])
            else:
                M = par("gM", _operator(g, Cc, pdt))
                if case["family"] == "mixed":
                    y = F_.adi_diffuse_mixed(u, *co, M, steps, case["mode"], checkpoints=case["ck"])
                elif case["family"] == "small_states":
                    y = F_.adi_diffuse_small_states(u, *co, M, steps, case["mode"], case["emit"], checkpoints=case["ck"])
                else:
                    sink = [] if case["sink"] else None
                    sw = par("gskip", torch.tensor(0.9).to(pdt)) if case["skip"] else None
                    y = F_.adi_diffuse_small(u, *co, M, steps, case["mode"], skip_weight=sw, checkpoints=case["ck"],
                                             kmax_sink=sink)
            node, outs["y"], lossless = y.grad_fn, y, set()
    res = {k: v.detach().cpu() for k, v in outs.items()}
    if sink is not None:                                   # the maxima reach the sink whenever a backward may follow
        assert len(sink) == (0 if way == "no_grad" else 1), "the call did not hand out its coefficient maxima"
        if sink:
            res["kmax"] = torch.tensor(sink[0].wait(), dtype=F32)
    if way != "no_grad":
        assert (type(node).__name__ == "CppFunction") == (native and case["native"]), type(node).__name__
        if case["family"] == "small" and not case["native"]:
            assert type(node).__name__ == "_AdiSmallFnBackward"
        heads = [v for k, v in outs.items() if k not in lossless]
        torch.autograd.backward(heads, [torch.randn(*v.shape, generator=g).to(v.dtype).to(dev) for v in heads])
        res["gu"] = u.grad.cpu()
        if train:
            for k, p in named.items():
                res[k] = p.grad.cpu()
    torch.cuda.synchronize()
    return res


def both_mirrors(P, case, way):
    """(what the native nodes give, what the ctypes nodes give) for one case and way."""
    L = P._lib
    ext = L.host_ext()
    assert ext is not None
    a = run_case(P, case, way, True)
    L._host = False
    try:
        b = run_case(P, case, way, False)
    finally:
        L._host = ext
    return a, b


def variants():
    for case in CASES:
        for way in WAYS:
            yield case, way


def key(case, way, name, t):
    """The fixture's key of one result: the tensor's dtype is part of it, so a changed dtype is a missing key."""
    return f"{case['name']}|{way}|{name}|{str(t.dtype).replace('torch.', '')}"


def to_numpy(t):
    """16-bit tensors are stored as their bits."""
    return (t.view(torch.int16) if t.dtype in (BF16, F16) else t).contiguous().numpy()


# The frozen route's input gradient is bitwise the full backward's, and most outputs are the same tensor in all three ways:
# a fixture file stores every distinct array once ("blob_<digest>") and an "index" of "key=digest" lines.
def pack(results):
    """{key: array} -> the arrays of one .npz file."""
    out, index = {}, []
    for k, a in sorted(results.items()):
        h = hashlib.sha1(str((a.dtype, a.shape)).encode() + a.tobytes()).hexdigest()[:16]
        out["blob_" + h] = a
        index.append(f"{k}={h}")
    out["index"] = np.array(index)
    return out


def unpack(z):
    """The inverse of ``pack`` on an opened .npz file."""
    blobs = {}
    res = {}
    for line in z["index"].tolist():
        k, h = line.rsplit("=", 1)
        if h not in blobs:
            blobs[h] = z["blob_" + h]
        res[k] = blobs[h]
    return res
