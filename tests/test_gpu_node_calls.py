"""The host glue of the implicit-layer autograd nodes exists twice — the ctypes nodes of functional.py and the native nodes
of csrc/host_ext.cpp — and each mirror builds its nodes from one shared core.  tests/golden/node_calls/ holds what the public
functions returned — every output, the input gradient, every parameter / operator / skip-weight / weight gradient — for the
cases of tests/node_calls_cases.py at the commit before that core was factored out (tools/record_node_calls.py), where both
mirrors agreed bit for bit.  The library's sources are the same and its kernels use no float atomics
(test_gpu_determinism.py), so both mirrors still give those bits: a mismatch is a change of behaviour."""
import functools
import os

import numpy as np
import pytest
import torch

import node_calls_cases as NC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_calls")


@functools.lru_cache(maxsize=None)
def _golden():
    res = {}
    for f in NC.FILES:
        with np.load(os.path.join(GOLDEN, f + ".npz")) as z:
            res.update(NC.unpack(z))
    return res


def test_fixture_holds_exactly_the_cases():
    want = {(c["name"], w) for c, w in NC.variants()}
    have = {tuple(k.split("|")[:2]) for k in _golden()}
    assert have == want
    assert sorted(os.listdir(GOLDEN)) == [f + ".npz" for f in NC.FILES]


@pytest.mark.parametrize("case,way", list(NC.variants()), ids=[f"{c['name']}-{w}" for c, w in NC.variants()])
def test_both_mirrors_give_the_results_of_the_parent_commit_bit_for_bit(case, way):
    import cnn_with_pde_amd as P
    from cnn_with_pde_amd import _lib, functional  # noqa: F401
    gold = _golden()
    prefix = f"{case['name']}|{way}|"
    for mirror, res in zip(("native", "ctypes"), NC.both_mirrors(P, case, way)):
        assert {NC.key(case, way, n, t) for n, t in res.items()} == {k for k in gold if k.startswith(prefix)}, mirror
        for n, t in res.items():
            ref = torch.from_numpy(gold[NC.key(case, way, n, t)])
            got = torch.from_numpy(NC.to_numpy(t))
            assert got.shape == ref.shape, (mirror, n)
            assert torch.equal(got, ref), (mirror, n)
