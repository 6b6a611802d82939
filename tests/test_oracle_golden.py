"""Pin the CPU oracle (oracle/pde_oracle.py) against vectors produced by the
reference's own layer classes (tests/golden, made by tools/make_golden.py).

K1 in fp32 must agree BITWISE (same op order as the reference); everything else
within a few ulp.  These run on CPU (-m "not gpu"), with MKL in its reproducible mode
(tests/conftest.py) and the thread count the vectors were made with, so on any x86 host."""
import pytest
import torch

import golden_util as G
from oracle import pde_oracle as O


@pytest.mark.parametrize("name", G.names())
def test_oracle_matches_reference_vectors(name):
    g = G.Golden(name)
    fn = g.oracle_fn()
    threads = torch.get_num_threads()
    torch.set_num_threads(G.GOLDEN_THREADS)        # as the vectors were made (golden_util)
    try:
        y, gu, grads = O.value_and_grads(fn, g.u, g.params, g.gy)
    finally:
        torch.set_num_threads(threads)
    k1_f32 = g.family() == "adi" and g.dtype == torch.float32
    tol = 0.0 if k1_f32 else (1e-12 if g.dtype == torch.float64 else 2e-6)
    if name == "emotion_default_smooth":
        # default PDELayer parameters exceed the explicit stability limit:
        # values reach 1e5 and the scalar parameter gradients are sums with heavy cancellation.
        tol = 1e-4
    assert y.dtype == g.dtype
    assert G.rel_err(y, g.y) <= tol, ("y", G.rel_err(y, g.y))
    assert G.rel_err(gu, g.gu) <= tol, ("gu", G.rel_err(gu, g.gu))
    for n, ref in g.grads.items():
        if g.grad_is_none[n]:
            # tiny_imagenet beta_base is unused by the live forward
            assert grads[n] is None or float(grads[n].abs().max()) == 0.0
            continue
        e = G.rel_err(grads[n], ref)
        # a scalar parameter's gradient is one long reduction whose summation order autograd does not pin
        assert e <= (max(tol, 1e-6) if ref.numel() == 1 else tol), (n, e)
