"""Static guard of the assembly backward's time step (CPU only): generate the default variant and the round-4 one
(gen_adi_bwd_asm.py) and count the instructions of the time-step loop, `L_step:` to its back-edge.  The default schedule
must keep the previous one's vector arithmetic (give or take the address / counter moves it dropped or moved out of line)
and carry at most 80 scalar instructions per step, against 196 before."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cnn-with-pde_amd", "csrc")
sys.path.insert(0, CSRC)
import gen_adi_bwd_asm as G  # noqa: E402

PREVIOUS = "8b"


def _default_spec():
    src = open(os.path.join(CSRC, "pde_adi_asm.hip")).read()
    m = re.search(r'std::string w = want \? want : "([0-9a-z]+)";', src)
    assert m, "default variant not found in pde_adi_asm.hip"
    return m.group(1)


def _counts(spec):
    text, _ = G.gen(*G.parse_spec(spec))
    return text, G.step_loop_counts(text)


def test_the_default_is_built_into_the_library():
    asmw = re.search(r"^ASMW \?= (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert _default_spec() in asmw and PREVIOUS in asmw


def test_previous_schedule_is_the_round4_one():
    _, c = _counts(PREVIOUS)
    assert (c["valu"], c["salu"], c["lds"], c["vmem"], c["total"]) == (791, 196, 123, 22, 1167), c


def test_default_step_is_leaner():
    spec = _default_spec()
    assert spec != PREVIOUS
    _, old = _counts(PREVIOUS)
    _, new = _counts(spec)
    assert new["salu"] <= 80, new
    assert new["total"] < old["total"], (new, old)
    assert new["swap"] == old["swap"] == 10
    # the arithmetic is unchanged: only v_mov / address / v_subrev moves (out of line or per chunk) may differ
    assert old["valu"] - 8 <= new["valu"] <= old["valu"], (new, old)


def test_same_arithmetic_stream():
    """the floating-point instructions of the step, in order, are the same in both schedules (the time-weighted
    update's adjusting v_subrev_f32 left the loop in MODE C: it runs out of line, once per chunk)"""
    def fp_ops(s):
        text, _ = _counts(s)
        lines = text.split("\n")
        i0 = lines.index("L_step:")
        out = []
        for ln in lines[i0:]:
            t = ln.split(";")[0].split()
            if t and re.match(r"v_(fma|fmac|mul|add|sub)_f32", t[0]):
                out.append(" ".join(t))
            if t[:2] == ["s_cbranch_scc1", "L_step"]:
                break
        return out
    assert fp_ops(_default_spec()) == fp_ops(PREVIOUS)


def test_lane_exchanges_have_their_wait_states():
    """in straight-line order, no v_permlane32_swap_b32 reads a register a VALU wrote within two wait states, and no
    VALU reads a swap result within two (the branches that skip code only add instructions in between)"""
    text, _ = _counts(_default_spec())
    hist = []                                   # (written registers, was a swap) per issued instruction
    for ln in text.split("\n"):
        t = ln.split(";")[0].replace(",", " ").split()
        if not t or t[0].endswith(":") or t[0].startswith("."):
            continue
        op = t[0]
        if op == "s_nop":
            hist += [(set(), False)] * (int(t[1]) + 1)
            continue
        regs = [r for r in t[1:] if re.fullmatch(r"-?v\d+", r)]
        regs = [r.lstrip("-") for r in regs]
        swap = op.startswith("v_permlane32_swap")
        for d, (w, was_swap) in enumerate(reversed(hist[-2:])):
            reads = set(regs) if swap else set(regs[1:])
            if w & reads:
                assert not (swap or was_swap), (ln, d)
        writes = set(regs[:2]) if swap else ({regs[0]} if op.startswith("v_") and regs else set())
        hist.append((writes, swap))
