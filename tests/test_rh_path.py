"""pde_sym_layer_path / pde_sym_layer_dk_path / pde_sym_layer_workspace_bytes (include/pdecnn.h) over a grid of
(B, D, workspace, PDE_RH_* switch) against the dispatch table written out here by hand.  The query is host code: no GPU is
needed, and since pde_sym_layer_forward and _backward dispatch on the same function, this pins which kernels every call
takes.  The switches are read with getenv on every call, so setting them in this process selects the path."""
import ctypes as C

import pytest

STRIP32, STRIP16, ROW_BLOCKS = 0, 1, 2
DK_SPLIT3, DK_MFMA_F32 = 0, 1
SWITCHES = ("PDE_RH_NO_STRIP32", "PDE_RH_SPLIT", "PDE_RH_NO_SPLIT")
BATCHES = (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 255, 256, 257, 385, 1030)
WIDTHS = (64, 128, 192, 256, 320, 384, 448, 512, 576, 640, 768, 1024, 1536, 2048, 3072, 4096, 4608, 8192)


def expected(B, D, has_workspace, env):
    """(family, split, waves, row_blocks)"""
    if B > 128:
        return ROW_BLOCKS, 0, 8, -(-B // 128)
    if not has_workspace or "PDE_RH_NO_STRIP32" in env:
        return STRIP16, 0, 8, 1
    start = 8
    forced = env.get("PDE_RH_SPLIT")
    if forced is not None and forced.isdigit() and int(forced) in (2, 4, 8, 16):
        start = int(forced)
    cap = 2048 if B <= 64 else 1024
    S = 0
    for s in (16, 8, 4, 2):
        if s <= start and D % (64 * s) == 0 and (D // 32) * s <= cap:
            S = s
            break
    if S >= 2:
        return STRIP32, S, 2 if B <= 64 else 4, 1
    return STRIP16, 0, 8, 1


def _query(lib, B, D, ws):
    s, w, r = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    fam = lib.pde_sym_layer_path(B, D, ws, C.byref(s), C.byref(w), C.byref(r))
    return fam, s.value, w.value, r.value


@pytest.fixture
def lib_env(monkeypatch):
    from cnn_with_pde_amd import _lib as L
    lib = L.load()

    def go(env):
        for s in SWITCHES:
            monkeypatch.delenv(s, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return lib
    return go


ENVS = [{}, {"PDE_RH_NO_STRIP32": "1"}, {"PDE_RH_SPLIT": "2"}, {"PDE_RH_SPLIT": "4"}, {"PDE_RH_SPLIT": "16"},
        {"PDE_RH_SPLIT": "3"}, {"PDE_RH_SPLIT": "12"}, {"PDE_RH_SPLIT": "32"}, {"PDE_RH_SPLIT": "1"}, {"PDE_RH_SPLIT": "x"},
        {"PDE_RH_NO_SPLIT": "1"}, {"PDE_RH_NO_SPLIT": "1", "PDE_RH_SPLIT": "4"}, {"PDE_RH_NO_STRIP32": "1", "PDE_RH_SPLIT": "16"}]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: "+".join(f"{k[7:]}={v}" for k, v in e.items()) or "default")
def test_path_query_matches_the_dispatch_table(env, lib_env):
    lib = lib_env(env)
    seen = set()
    for B in BATCHES:
        for D in WIDTHS:
            for ws in (0, 1):
                want = expected(B, D, ws, env)
                assert _query(lib, B, D, ws) == want, (B, D, ws, env)
                assert lib.pde_sym_layer_path(B, D, ws, None, None, None) == want[0]
                seen.add(want[:3])
            assert lib.pde_sym_layer_dk_path(B, D) == (DK_MFMA_F32 if "PDE_RH_NO_SPLIT" in env else DK_SPLIT3)
            # the workspace is what the path WITH a workspace needs: one tile of waves x 1024 floats per (strip, slice)
            _, S, waves, _ = expected(B, D, 1, env)
            assert lib.pde_sym_layer_workspace_bytes(B, D) == (D // 32) * S * waves * 1024 * 4, (B, D, env)
            assert lib.pde_sym_layer_supported(B, D) == 1
    if "PDE_RH_NO_STRIP32" in env:
        assert {f for f, _, _ in seen} == {STRIP16, ROW_BLOCKS}
    elif "PDE_RH_SPLIT" not in env:
        assert seen == {(ROW_BLOCKS, 0, 8), (STRIP16, 0, 8)} | {(STRIP32, s, w) for s in (2, 4, 8) for w in (2, 4)}


def test_default_splits_by_width(lib_env):
    lib = lib_env({})
    table = {64: 0, 128: 2, 192: 0, 256: 4, 320: 0, 384: 2, 512: 8, 640: 2, 768: 4, 1024: 8, 3072: 8}
    for D, S in table.items():
        for B, waves in ((1, 2), (64, 2), (65, 4), (128, 4)):
            want = (STRIP32, S, waves, 1) if S else (STRIP16, 0, 8, 1)
            assert _query(lib, B, D, 1) == want, (B, D)
            assert _query(lib, B, D, 0) == (STRIP16, 0, 8, 1), (B, D)
    # the workgroup cap: (4608 / 32) * 8 = 1152 strips x slices, allowed with two waves (2048), halved with four (1024)
    assert _query(lib, 64, 4608, 1) == (STRIP32, 8, 2, 1)
    assert _query(lib, 65, 4608, 1) == (STRIP32, 4, 4, 1)
    assert _query(lib, 129, 4608, 1) == (ROW_BLOCKS, 0, 8, 2) and _query(lib, 129, 4608, 0) == (ROW_BLOCKS, 0, 8, 2)
    assert lib.pde_sym_layer_workspace_bytes(129, 4608) == 0


def test_forced_splits(lib_env):
    lib = lib_env({"PDE_RH_SPLIT": "16"})
    assert _query(lib, 33, 1024, 1) == (STRIP32, 16, 2, 1) and _query(lib, 128, 1024, 1) == (STRIP32, 16, 4, 1)
    assert _query(lib, 33, 512, 1) == (STRIP32, 8, 2, 1)               # 512 % (64 * 16) != 0: halved
    assert lib.pde_sym_layer_workspace_bytes(128, 1024) == 32 * 16 * 4 * 1024 * 4
    lib = lib_env({"PDE_RH_SPLIT": "2"})
    assert _query(lib, 33, 512, 1) == (STRIP32, 2, 2, 1) and _query(lib, 128, 3072, 1) == (STRIP32, 2, 4, 1)
    lib = lib_env({"PDE_RH_SPLIT": "4"})
    assert _query(lib, 33, 512, 1) == (STRIP32, 4, 2, 1) and _query(lib, 33, 128, 1) == (STRIP32, 2, 2, 1)
    for junk in ("3", "6", "12", "32", "0", "-4", "abc", ""):           # no power of two in 2..16: ignored
        lib = lib_env({"PDE_RH_SPLIT": junk})
        assert _query(lib, 33, 512, 1) == (STRIP32, 8, 2, 1), junk


def test_path_query_refuses_what_the_entry_points_refuse(lib_env):
    from cnn_with_pde_amd import _lib as L
    lib = lib_env({})
    for B, D in ((0, 128), (-1, 128), (8, 0), (8, 32), (8, 96), (8, 100), (8, -64), (0, 0)):
        for ws in (0, 1):
            assert _query(lib, B, D, ws) == (-1, -7, -7, -7), (B, D)
        assert lib.pde_sym_layer_dk_path(B, D) == -1
        assert lib.pde_sym_layer_workspace_bytes(B, D) == 0 and lib.pde_sym_layer_supported(B, D) == 0
    assert (L.PDE_RH_PATH_STRIP32, L.PDE_RH_PATH_STRIP16, L.PDE_RH_PATH_ROW_BLOCKS) == (STRIP32, STRIP16, ROW_BLOCKS)
    assert (L.PDE_RH_DK_SPLIT3, L.PDE_RH_DK_MFMA_F32) == (DK_SPLIT3, DK_MFMA_F32)
