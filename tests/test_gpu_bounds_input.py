"""The backward for the input alone held to its buffers: every *_backward_input[_states] entry point once on ordinary
tensors and once inside a ``guard_util.Arena`` (1 MiB of 0xFF on both sides of every buffer, outputs pre-filled with
0xFF, workspaces of exactly the queried size and 0xFF-filled), through the runner of tests/test_gpu_bounds.py.

A case (tests/bounds_input_cases.py) is a case of the ``adi`` family of tests/bounds_cases.py — the forward, the full
backward — and then the input backward on the same gy / gstates / mask, with an output (``gu_input``) and a workspace of its own.  The
smallest fused length, the any-size kernel at 128 x 128 (where the any-size kernels change their LDS decisions) and the
smallest rectangle, each with and without the forward's workspace and with and without an emission mask, in every
sub-family.  Beyond what the runner asserts — guards intact, no output element left 0xFF, finite, bitwise the plain
run — ``gu_input`` must be bitwise the full backward's ``gu`` in both runs."""
import pytest
import torch

import bounds_cases as BC
import bounds_input_cases as BI
import test_gpu_bounds as TB

BI.register()
pytestmark = pytest.mark.gpu

CASES = BI.TABLE_CASES + BI.MATRIX_CASES


@pytest.fixture(scope="module")
def library():
    return BC.lib(), BC.header_functions()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_input_backward_bounds(case, library):
    lib, hdr = library
    fam = BC._adi_fam(case.p)
    try:
        print(TB.check_case(case, lib, hdr))
        for ctx in (TB.ArenaCtx(), TB.PlainCtx()):
            calls = TB._run(case, ctx, lib, hdr)
            assert calls[-1][0] == fam + "backward_input" + ("_states" if case.p.get("emit") else "")
            assert calls[-1][1]["fwd_workspace"] == ("fws" if case.p.get("reuse", True) else None)
            a, b = ctx.t["gu_input"], ctx.t["gu"]
            assert bool(torch.isfinite(a.double()).all())
            assert torch.equal(TB._bits(a), TB._bits(b)), f"{case.id}: gu of the input backward differs from the full backward's"
            if isinstance(ctx, TB.ArenaCtx):
                ctx.arena.check()
    except RuntimeError as e:
        if not TB._is_fault(e):
            raise
        pytest.exit(f"GPU fault in {case.id}: {e}", returncode=3)


def test_the_cases_call_every_new_entry_point():
    called = {fn for c in CASES for fn, _ in c.build(BC.SpecCtx())[0]}
    assert set(BI.NEW_FUNCTIONS) <= called, set(BI.NEW_FUNCTIONS) - called
