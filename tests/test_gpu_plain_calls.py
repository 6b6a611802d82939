"""A plain call is its family's trajectory call with no emission mask, served by the same autograd node
(functional._AdiFn, _Explicit5Fn, _JacobiFn).  tests/golden/plain_calls/parent.npz holds what the public functions
returned — output, input gradient, every parameter gradient — for the cases of tests/plain_calls_cases.py at the commit
before the nodes were folded (tools/record_plain_calls.py).  The library's sources are the same and its kernels use no
float atomics (test_gpu_determinism.py), so the results are equal bit for bit: a mismatch is a change of behaviour."""
import functools
import os

import numpy as np
import pytest
import torch

import plain_calls_cases as PC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plain_calls", "parent.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_exactly_the_cases():
    from cnn_with_pde_amd import functional as F_  # noqa: F401
    want = {(c["name"], "traj" if t else "plain") for c, t in PC.variants()}
    have = {tuple(k.split("|")[:2]) for k in _golden()}
    assert have == want


@pytest.mark.parametrize("case,traj", list(PC.variants()),
                         ids=[c["name"] + ("-traj" if t else "-plain") for c, t in PC.variants()])
def test_results_are_those_of_the_parent_commit_bit_for_bit(case, traj):
    from cnn_with_pde_amd import functional as F_
    res, _ = PC.run_case(F_, case, traj)
    gold = _golden()
    prefix = f"{case['name']}|{'traj' if traj else 'plain'}|"
    assert {PC.key(case, traj, n, t) for n, t in res.items()} == {k for k in gold if k.startswith(prefix)}
    for n, t in res.items():
        ref = torch.from_numpy(gold[PC.key(case, traj, n, t)])
        got = torch.from_numpy(PC.to_numpy(t))
        assert got.shape == ref.shape, n
        assert torch.equal(got, ref), (n, float((got.double() - ref.double()).abs().max()))


def test_jacobi_of_no_steps_returns_the_input():
    from cnn_with_pde_amd import functional as F_
    case = next(c for c in PC.CASES if c["name"] == "jac_nt0")
    res, _ = PC.run_case(F_, case, False)
    u, _ = PC._inputs(case, torch.Generator().manual_seed(1000 + PC.CASES.index(case)))
    assert torch.equal(res["y"], u)


@pytest.mark.parametrize("name,node", [("adi_fused_auto_sink", "_AdiFnBackward"), ("jac", "_JacobiFnBackward")])
def test_a_plain_call_returns_a_tensor_of_its_own(name, node):
    """The plain call's output is no slice of a (1, ...) trajectory buffer, and one node class serves both calls."""
    from cnn_with_pde_amd import functional as F_
    case = next(c for c in PC.CASES if c["name"] == name)
    _, y = PC.run_case(F_, case, False)
    assert tuple(y.shape) == tuple(case["shape"]) and y._base is None
    assert y.untyped_storage().nbytes() == y.numel() * y.element_size()
    assert type(y.grad_fn).__name__ == node
    _, t = PC.run_case(F_, case, True)
    assert tuple(t.shape) == (2,) + tuple(case["shape"])
    assert type(t.grad_fn).__name__ == node
