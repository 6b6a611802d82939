"""Static guard of the look-ahead schedule of the assembly backward (MODE D, `8d`, gen_adi_bwd_asm.py; CPU only): it is
MODE C's floating-point stream with the step top's round trips issued one step ahead, so the default variant must keep
`8c`'s arithmetic instruction for instruction, `8c` must stay built in to be compared against, and — when the default is
`8d` — no scalar load may stand between the step's top and its first sweep."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cnn-with-pde_amd", "csrc")
sys.path.insert(0, CSRC)
import gen_adi_bwd_asm as G  # noqa: E402

BASE = "8c"
FP = r"v_(fma|fmac|mul|add|sub)_f32"


def _default_spec():
    src = open(os.path.join(CSRC, "pde_adi_asm.hip")).read()
    m = re.search(r'std::string w = want \? want : "([0-9a-z]+)";', src)
    assert m, "default variant not found in pde_adi_asm.hip"
    return m.group(1)


def _asmw():
    return re.search(r"^ASMW \?= (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()


def _step_loop(spec):
    """the instructions of the static time-step loop, `L_step:` to its back-edge, as token lists"""
    text, _ = G.gen(*G.parse_spec(spec))
    lines = text.split("\n")
    out = []
    for ln in lines[lines.index("L_step:") + 1:]:
        t = ln.split(";")[0].split()
        if t:
            out.append(t)
        if t[:2] == ["s_cbranch_scc1", "L_step"]:
            return out
    raise AssertionError("no back-edge")


def _fp_ops(spec):
    return [" ".join(t) for t in _step_loop(spec) if re.match(FP, t[0])]


def test_8c_stays_built_in():
    asmw = _asmw()
    assert BASE in asmw and "8b" in asmw and "12" in asmw and _default_spec() in asmw


def test_parse_spec_knows_the_letter_d():
    assert G.parse_spec("8d") == (8, 0, "D")
    assert G.parse_spec("8da4096") == (8, 4096, "D")
    assert G.parse_spec("8c") == (8, 0, "C") and G.parse_spec("8b") == (8, 0, "B") and G.parse_spec("12") == (12, 0, "A")


def test_default_keeps_the_arithmetic_of_8c():
    a, b = _fp_ops(_default_spec()), _fp_ops(BASE)
    assert len(b) > 700
    assert a == b


def test_8d_keeps_the_arithmetic_of_8c():
    assert _fp_ops("8d") == _fp_ops(BASE)


def test_no_scalar_load_at_the_top_of_the_default_8d():
    spec = _default_spec()
    if not spec.startswith("8d"):
        assert spec == BASE                  # the look-ahead schedule did not become the default: nothing to hold it to
        spec = "8d"                          # (the selectable variant is still held to it)
    loop = _step_loop(spec)
    first_fp = next(i for i, t in enumerate(loop) if re.match(FP, t[0]))
    top = [t[0] for t in loop[:first_fp]]
    assert top and not [op for op in top if op.startswith("s_load")], top
    # and the loop still loads the increments once per step, further down
    assert sum(t[0].startswith("s_load") for t in loop) == 1


def test_every_built_variant_generates():
    """gen() runs its own checks while it emits (Emit.assert_idle at the step top and before the plane stores, the
    outstanding-load accounting behind every counted s_waitcnt, the look-ahead hook's empty-queue assertion)"""
    for spec in _asmw():
        text, info = G.gen(*G.parse_spec(spec))
        assert info["name"] == "adi_bwd_asm_n32_w" + spec
        c = G.step_loop_counts(text)
        assert c["swap"] == 10 and c["total"] < 1200, (spec, c)
