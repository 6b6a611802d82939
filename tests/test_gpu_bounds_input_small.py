"""The one-launch layers' input backward held to its buffers: every case of tests/bounds_input_small_cases.py through the
runner of tests/test_gpu_bounds.py — once inside a ``guard_util.Arena`` (1 MiB of 0xFF on both sides of every buffer,
outputs pre-filled with 0xFF, workspaces of exactly the queried size and 0xFF-filled) and once on ordinary tensors.

Beyond what the runner asserts — guards intact, no output element left 0xFF, finite, bitwise the plain run:
  * ``gu_input`` is bitwise the full backward's ``gu``, and ``y_input`` (pde_adi_small_forward_input) bitwise the ``y`` of the
    forward that kept its states;
  * a one-layer call touches no scratch: ``iws`` still holds the 0xFF it was filled with;
  * the shared-input call leaves the fields it does not read (coefficient gradients, gM, g_weight) as they were, and its
    ``gu`` is bitwise the ``gu`` of pde_adi_multi_backward, called on the side with buffers of its own."""
import ctypes as C

import pytest
import torch

import bounds_cases as BC
import bounds_input_small_cases as BS
import test_gpu_bounds as TB

pytestmark = pytest.mark.gpu

CASES = BS.TABLE_CASES + BS.MATRIX_CASES


@pytest.fixture(scope="module")
def library():
    return BC.lib(), BS.header_functions()


def _full_multi_gu(case, ctx, lib):
    """gu of pde_adi_multi_backward on the case's group: the same struct with outputs and a workspace of its own."""
    from cnn_with_pde_amd import _lib as L
    nl = ctx.values["num_layers"]
    src = ctx.values["layers"]
    arr = (L.PdeSmallLayer * nl)()
    keep = []
    zero = (C.c_uint64 * 2)(0, 0)
    for i in range(nl):
        C.memmove(C.byref(arr[i]), C.byref(src[i]), C.sizeof(L.PdeSmallLayer))
        d = src[i].desc.contents
        shape = tuple(ctx.t[f"alpha_base_{i}"].shape)
        outs = [torch.empty(shape, device="cuda") for _ in range(4)] + [torch.empty_like(ctx.t[f"M_{i}"]), torch.empty(1, device="cuda")]
        ws = torch.empty(lib.pde_adi_small_backward_workspace_bytes(C.byref(d), 3, 0), dtype=torch.uint8, device="cuda")
        a = arr[i]
        a.g_alpha_base, a.g_beta_base, a.g_alpha_slope, a.g_beta_slope, a.gM, a.g_weight = (t.data_ptr() for t in outs)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        a.ckpt_mask = zero
        keep.append((outs, ws))
    gu = torch.empty_like(ctx.t["gu"])
    rc = lib.pde_adi_multi_backward(nl, arr, C.c_void_p(ctx.ptr("gy")), C.c_void_p(ctx.ptr("u")), C.c_void_p(gu.data_ptr()),
                                    ctx.stream())
    assert rc == 0, rc
    TB._sync()
    return gu


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_input_backward_bounds(case, library):
    lib, hdr = library
    try:
        print(TB.check_case(case, lib, hdr))
        for ctx in (TB.ArenaCtx(), TB.PlainCtx()):
            calls = TB._run(case, ctx, lib, hdr)
            assert bool(torch.isfinite(ctx.t["gu"].double()).all())
            if case.family == "small":
                assert calls[-1][0] == "pde_adi_small_backward_input" + ("_states" if case.p.get("emit") else "")
                a, b = ctx.t["gu_input"], ctx.t["gu"]
                assert torch.equal(TB._bits(a), TB._bits(b)), f"{case.id}: gu of the input backward differs from the full backward's"
                if not case.p.get("emit"):
                    assert torch.equal(TB._bits(ctx.t["y_input"]), TB._bits(ctx.t["y"])), f"{case.id}: y of forward_input differs"
                if isinstance(ctx, TB.ArenaCtx):
                    assert bool((ctx.t["iws"] == 0xFF).all()), f"{case.id}: a one-layer call wrote to its workspace"
            else:
                assert calls[-1][0] == "pde_adi_multi_backward_input"
                want = _full_multi_gu(case, ctx, lib)
                assert torch.equal(TB._bits(ctx.t["gu"]), TB._bits(want)), f"{case.id}: gu differs from pde_adi_multi_backward's"
                # the fields the call does not read: rebuilt from the case's generator, they hold what they were given
                ref = TB.PlainCtx()
                case.build(ref)
                for i in range(ctx.values["num_layers"]):
                    for k in BS.UNTOUCHED:
                        assert torch.equal(TB._bits(ctx.t[f"{k}_{i}"]), TB._bits(ref.t[f"{k}_{i}"])), (case.id, k, i)
            if isinstance(ctx, TB.ArenaCtx):
                ctx.arena.check()
    except RuntimeError as e:
        if not TB._is_fault(e):
            raise
        pytest.exit(f"GPU fault in {case.id}: {e}", returncode=3)


def test_the_cases_call_every_new_entry_point():
    called = {fn for c in CASES for fn, _ in c.build(BC.SpecCtx())[0]}
    assert set(BS.NEW_FUNCTIONS) <= called, set(BS.NEW_FUNCTIONS) - called
