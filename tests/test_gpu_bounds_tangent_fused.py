"""The fused tangent-linear pass held to its buffers, through the C ABI: every case of tests/bounds_tangent_fused_cases.py
through the runner of tests/test_gpu_bounds.py — inside a ``guard_util.Arena`` (1 MiB of 0xFF on both sides of every buffer,
outputs pre-filled with 0xFF, workspaces of exactly the queried size and 0xFF-filled) against ordinary tensors — and once more
inside the skewed arena of tests/test_gpu_alignment.py, where every buffer begins on exactly the 16 bytes the header asks of
its pointer and on nothing larger.

Beyond what the runner asserts — guards intact, no output element left 0xFF, finite, bitwise the plain run — the y of the
tangent call is bitwise the y of the fused forward (``bounds_tangent_fused_cases.twins``)."""
import pytest
import torch

import bounds_cases as BC
import bounds_tangent_fused_cases as BF
import test_gpu_alignment as GA
import test_gpu_bounds as TB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def library():
    return BC.lib(), BF.header_functions()


def _twins_equal(case, ctx):
    for mine, full in BF.twins(case):
        a, b = ctx.t[mine], ctx.t[full]
        same = TB._bits(a) == TB._bits(b)
        assert bool(same.all()), f"{case.id}: {int((~same).sum())} of {a.numel()} elements of {mine} differ from {full}"
    assert bool(torch.isfinite(ctx.t["dy"].double()).all()), case.id


@pytest.mark.parametrize("case", BF.CASES, ids=[c.id for c in BF.CASES])
def test_tangent_fused_bounds(case, library):
    lib, hdr = library
    try:
        print(TB.check_case(case, lib, hdr))
        for ctx in (TB.ArenaCtx(), TB.PlainCtx()):
            calls = TB._run(case, ctx, lib, hdr)
            assert calls[-1][0] in BF.NEW_FUNCTIONS
            _twins_equal(case, ctx)
            if isinstance(ctx, TB.ArenaCtx):
                ctx.arena.check()
    except RuntimeError as e:
        if not TB._is_fault(e):
            raise
        pytest.exit(f"GPU fault in {case.id}: {e}", returncode=3)


@pytest.mark.parametrize("case", BF.CASES, ids=[c.id for c in BF.CASES])
def test_minimal_alignment(case, library):
    lib, hdr = library
    try:
        print(TB.check_case(case, lib, hdr, guarded_ctx=GA.MinAlignCtx))
        ctx = GA.MinAlignCtx()
        TB._run(case, ctx, lib, hdr)
        for name in ctx.roles:
            a = ctx.aligns[name]
            assert a == 16 and ctx.ptr(name) % (2 * a) == a, (case.id, name, a, hex(ctx.ptr(name)))
        _twins_equal(case, ctx)
        ctx.arena.check()
    except RuntimeError as e:
        if not TB._is_fault(e):
            raise
        pytest.exit(f"GPU fault in {case.id} at its minimal alignment: {e}", returncode=3)


def test_the_cases_call_the_new_entry_point():
    called = {fn for c in BF.CASES for fn, _ in c.build(BC.SpecCtx())[0]}
    assert set(BF.NEW_FUNCTIONS) <= called, set(BF.NEW_FUNCTIONS) - called
