"""pde_channel_mix_path / pde_channel_mix_splits (include/pdecnn.h) over a grid of (C, HW, tensor type, PDE_MIX_* switch)
against the dispatch table written out here by hand.  The query is host code: no GPU is needed, and since the entry
points dispatch on the same function, this pins which kernel family every call takes.  The switches are read with getenv
on every call, so setting them in this process selects the path."""
import ctypes as C
import itertools

import pytest

F32, BF16, F64, F16 = 0, 1, 2, 3
SCALAR, MFMA_F32, MFMA_16, SPLIT3, FUSED = 0, 1, 2, 3, 4
SWITCHES = ("PDE_MIX_NO_BF16_MFMA", "PDE_MIX_NO_SPLIT", "PDE_MIX_UNFUSED")


def expected(Cc, HW, io, backward, on):
    sixteen = io in (BF16, F16) and Cc in (64, 128) and HW % 64 == 0 and "PDE_MIX_NO_BF16_MFMA" not in on
    mfma = Cc % 32 == 0 and Cc <= 128 and HW % 4 == 0
    if sixteen:
        return MFMA_16
    if not backward:
        return MFMA_F32 if mfma else SCALAR
    if io == F32 and Cc in (32, 64, 96) and HW % 4 == 0 and HW >= 4 and "PDE_MIX_NO_SPLIT" not in on:
        return SPLIT3
    if Cc in (32, 64, 96, 128) and HW % 4 == 0 and "PDE_MIX_UNFUSED" not in on:
        return FUSED
    return MFMA_F32 if mfma else SCALAR


@pytest.mark.parametrize("on", [c for r in range(4) for c in itertools.combinations(SWITCHES, r)], ids=lambda c: "+".join(c) or "default")
def test_path_query_matches_the_dispatch_table(on, monkeypatch):
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s in on:
        monkeypatch.setenv(s, "1")
    seen = set()
    for Cc, HW, io, bwd in itertools.product((1, 2, 7, 31, 32, 33, 64, 96, 128, 160, 192), (1, 3, 4, 36, 49, 64, 100, 128, 196, 784, 1024, 4096),
                                             (F32, BF16, F16), (0, 1)):
        for B in (1, 5):
            got = lib.pde_channel_mix_path(B, Cc, HW, io, bwd)
            assert got == expected(Cc, HW, io, bwd, on), (B, Cc, HW, io, bwd, on, got)
            seen.add((bwd, got))
            chunks = C.c_int64(-1)
            walkers = lib.pde_channel_mix_splits(B, Cc, HW, io, bwd, C.byref(chunks))
            assert walkers >= 1 and chunks.value >= 1
            assert lib.pde_channel_mix_splits(B, Cc, HW, io, bwd, None) == walkers
            if bwd:
                assert chunks.value == B * ((HW + 63) // 64) and walkers <= chunks.value
                # the workspace holds one partial matrix per walker, whatever the path
                assert lib.pde_channel_mix_backward_workspace_bytes(B, Cc, HW) >= walkers * Cc * Cc * 4
    assert (0, SPLIT3) not in seen and (0, FUSED) not in seen
    if not on:
        assert seen == {(0, SCALAR), (0, MFMA_F32), (0, MFMA_16), (1, SCALAR), (1, MFMA_16), (1, SPLIT3), (1, FUSED)}
    if set(on) == {"PDE_MIX_NO_SPLIT", "PDE_MIX_UNFUSED"}:
        assert (1, MFMA_F32) in seen and (1, FUSED) not in seen and (1, SPLIT3) not in seen


def test_path_query_refuses_what_the_entry_points_refuse():
    from cnn_with_pde_amd import _lib as L
    lib = L.load()
    for bwd in (0, 1):
        for args in ((0, 64, 64, F32), (5, 0, 64, F32), (5, 64, 0, F32), (-1, 64, 64, F32), (5, 64, 64, F64), (5, 64, 64, 7),
                     (5, 64, 64, -1)):
            assert lib.pde_channel_mix_path(*args, bwd) == -1, args
            chunks = C.c_int64(-7)
            assert lib.pde_channel_mix_splits(*args, bwd, C.byref(chunks)) == -1 and chunks.value == -7, args
    assert (L.PDE_MIX_PATH_SCALAR, L.PDE_MIX_PATH_MFMA_F32, L.PDE_MIX_PATH_MFMA_16, L.PDE_MIX_PATH_SPLIT3,
            L.PDE_MIX_PATH_FUSED) == (SCALAR, MFMA_F32, MFMA_16, SPLIT3, FUSED)
