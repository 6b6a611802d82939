"""Bounds cases of the backward for the input alone (the *_backward_input[_states] entry points), as an extension of the
case table of tests/bounds_cases.py kept in a file of its own.

A case is a case of that table's ``adi`` family — the forward, the full backward and the per-sweep maxima, built by
``bounds_cases.build_adi`` unchanged — followed by the input backward on the same gy / gstates / mask with an output
(``gu_input``) and a workspace (``iws``) of its own.  ``fwd_workspace`` is the forward's workspace, or NULL where
``reuse`` is False (the call then factorises into ``iws``).

``register()`` appends ``TABLE_CASES`` to ``bounds_cases.CASES`` (once per interpreter): tests/test_bounds_cases.py holds
that every entry point of the header that writes device memory has a case in that table, and checks every case of it
(bindings, roles, element counts, masks, sizes).  tests/test_bounds_input_cases.py and tests/test_gpu_bounds_input.py
register at import, i.e. while pytest collects the suite.  A session that collects tests/test_bounds_cases.py WITHOUT
either of them sees the table without these cases and reports the new entry points as uncovered."""
import ctypes as C

import bounds_cases as BC


class InputCase(BC.Case):
    """An ``adi`` case with the input backward behind its calls (``p["input"]`` is set for every one of them)."""

    def build(self, ctx):
        p = dict(self.p)
        calls, expect = BC.build_adi(ctx, p)
        lib = BC.lib()
        d = ctx.values["d"]
        fam = BC._adi_fam(p)
        shape = (p["B"], p["C"], p["H"], p["W"])
        ctx.out("gu_input", shape, BC.IO[p["io"]][1])
        ni = ctx.ws("iws", getattr(lib, fam + "backward_input_workspace_bytes")(C.byref(d)))
        assert ni > 0, ni
        calls = list(calls)
        calls.append((fam + "backward_input" + ("_states" if p.get("emit") else ""),
                      {"gu": "gu_input", "fwd_workspace": "fws" if p.get("reuse", True) else None, "workspace": "iws",
                       "workspace_bytes": ni}))
        expect = list(expect)
        if "input_kernel" in p:
            expect.append(("pde_adi_backward_input_kernel", (C.byref(d),), p["input_kernel"]))
        return calls, expect


def _case(**p):
    H, W = p["H"], p["W"]
    size = f"n{H}" if H == W and not p.get("rect") else f"{H}x{W}"
    cid = (f"adi-input-{size}-b{p['B']}c{p['C']}-{p['io']}-{BC._sched_id(p['steps'], p.get('split', 'strang'))}"
           f"-{'fws' if p.get('reuse', True) else 'nofws'}-em{p.get('emit', 0):x}")
    return InputCase(cid, "adi", dict(p, input=True))


def _table_cases():
    """The smallest fused length, a batch one chunk of 32 planes cannot hold at N = 32, the any-size kernel where the
    planes are largest, a rectangle, float64: every new entry point of every sub-family at least once."""
    out = []
    for io in BC.IO3:
        out.append(_case(B=3, C=5, H=8, W=8, io=io, steps=2, input_kernel=0))
        out.append(_case(B=3, C=5, H=8, W=8, io=io, steps=2, emit=BC._all_but_last(6), input_kernel=0))
    out.append(_case(B=3, C=5, H=8, W=8, io="f32", steps=1, reuse=False, input_kernel=0))
    out.append(_case(B=37, C=5, H=32, W=32, io="f32", steps=2, input_kernel=0))
    out.append(_case(B=37, C=5, H=32, W=32, io="bf16", steps=2, split="lie", emit=BC._all_but_last(4), input_kernel=0))
    out.append(_case(B=3, C=2, H=128, W=128, io="f32", steps=1, input_kernel=2))
    out.append(_case(B=3, C=2, H=128, W=128, io="f16", steps=2, reuse=False, emit=BC._all_but_last(6), input_kernel=2))
    out.append(_case(B=3, C=2, H=5, W=9, io="f32", steps=1, rect=True))
    out.append(_case(B=3, C=2, H=5, W=9, io="f32", steps=2, rect=True, reuse=False, emit=BC._all_but_last(6)))
    out.append(_case(B=3, C=2, H=128, W=128, io="f64", steps=1))
    out.append(_case(B=3, C=2, H=5, W=5, io="f64", steps=2, reuse=False, emit=BC._all_but_last(6)))
    out.append(_case(B=3, C=2, H=5, W=9, io="f64", steps=1, rect=True, reuse=False))
    out.append(_case(B=3, C=2, H=5, W=9, io="f64", steps=2, rect=True, emit=BC._all_but_last(6)))
    return out


def _matrix_cases():
    """tests/test_gpu_bounds_input.py: smallest fused, any-size 128 x 128 and rectangle cases of every sub-family, each with
    and without the forward's workspace and with and without a mask."""
    out = []
    shapes = [(dict(H=8, W=8, C=5), ("f32", "bf16", "f16", "f64")),
              (dict(H=128, W=128, C=2), ("f32", "f16", "f64")),
              (dict(H=5, W=9, C=2, rect=True), ("f32", "bf16", "f64"))]
    for hw, ios in shapes:
        for io in ios:
            for reuse in (True, False):
                for emit in (0, BC._bits(0), BC._all_but_last(6)):
                    if emit == BC._bits(0) and io != "f32":
                        continue
                    out.append(_case(B=3, io=io, steps=2, reuse=reuse, emit=emit, **hw))
    return out


TABLE_CASES = _table_cases()
MATRIX_CASES = [c for c in _matrix_cases() if c.id not in {t.id for t in TABLE_CASES}]
NEW_FUNCTIONS = sorted(f + s for f in ("pde_adi_", "pde_adi_rect_", "pde_adi_f64_", "pde_adi_rect_f64_")
                       for s in ("backward_input", "backward_input_states"))


def register():
    """Append TABLE_CASES to the table of tests/bounds_cases.py, once."""
    have = {c.id for c in BC.CASES}
    for c in TABLE_CASES:
        if c.id not in have:
            BC.CASES.append(c)
            BC.BY_ID[c.id] = c
