"""Every C entry point at exactly the alignment include/pdecnn.h asks of its pointers, and no more.

Every GPU test before this one handed the library buffers that begin on 256 bytes or more (fresh allocations, the arena of
tests/guard_util.py).  Here every case of tests/bounds_cases.py runs once more inside a SKEWED arena: each buffer begins on
the alignment the header's "Alignment" section asks of the pointer it is bound to and on nothing larger — address = 16
(mod 32) for tensors, coefficient planes and every workspace, 4 (mod 8) for the fp32 scalars and per-channel vectors,
2 (mod 4) / 8 (mod 16) for 16-bit / double tensors of the element-wise calls, 8 (mod 16) for 16-bit tensors of the explicit
layer on float4 rows.  That is a legitimate call by the contract; nothing below the documented alignment is ever launched
(tests/test_alignment_refusal.py holds the refusals, without a device).

The assertions are those of tests/test_gpu_bounds.py (``check_case``): every return code 0, every guard byte intact, no
element of an overwritten output left all-ones, results finite and BITWISE equal to the run on ordinary tensors — so a
kernel that reads a neighbour's bytes through a wider access than its pointer allows, or a workspace whose carve-up only
works from a 256-byte base, shows as a difference.  Kernels behind an environment switch run in one child interpreter per
switch value (this file run as a script), as there.  After a fault of the device nothing more is started on it."""
import json
import os
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bounds_cases as BC  # noqa: E402
import bounds_input_cases  # noqa: E402
import test_gpu_bounds as TB  # noqa: E402

bounds_input_cases.register()                    # the *_backward_input cases belong to the table (see that file)
pytestmark = pytest.mark.gpu
IN_PROCESS = [c for c in BC.CASES if c.switch is None]


class MinAlignCtx(TB.ArenaCtx):
    skew = True


def test_the_skewed_context_places_every_buffer_at_its_documented_minimum():
    """On the device: one case with tensors, fp32 scalars and workspaces — each buffer a multiple of its alignment and of
    nothing larger, whatever the caching allocator returned."""
    case = next(c for c in BC.CASES if c.family == "small" and c.p.get("skip"))
    ctx = MinAlignCtx()
    case.build(ctx)
    seen = set()
    for name in ctx.roles:
        a = ctx.aligns[name]
        assert ctx.ptr(name) % (2 * a) == a, (name, a, hex(ctx.ptr(name)))
        seen.add(a)
    assert seen == {4, 16} and ctx.aligns["skip_weight"] == 4 and ctx.aligns["u"] == 16 and ctx.aligns["sws"] == 16


@pytest.mark.parametrize("case", IN_PROCESS, ids=[c.id for c in IN_PROCESS])
def test_minimal_alignment(case, library):
    try:
        print(TB.check_case(case, *library, guarded_ctx=MinAlignCtx))
    except RuntimeError as e:
        if not TB._is_fault(e):
            raise
        pytest.exit(f"GPU fault in {case.id} at its minimal alignment: {e}", returncode=3)


@pytest.fixture(scope="module")
def library():
    return BC.lib(), BC.header_functions()


@pytest.mark.parametrize("switch", BC.SWITCHES)
def test_minimal_alignment_behind_a_switch(switch, tmp_path):
    import subprocess
    name, _, value = switch.partition("=")
    want = [c.id for c in BC.CASES if c.switch == switch]
    assert want
    report = str(tmp_path / "report.json")
    keep = {k: v for k, v in os.environ.items() if k not in {s.partition("=")[0] for s in BC.SWITCHES}}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), switch, report], env=dict(keep, **{name: value}),
                           capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired as e:       # a hang: the next child must not start on this device
        pytest.exit(f"the child {switch} ran into its time limit: {str(e.stderr)[-1500:]}", returncode=3)
    if r.returncode == 3:
        pytest.exit(f"GPU fault in the child {switch}: {r.stderr[-1500:]}", returncode=3)
    assert r.returncode == 0, (switch, r.stdout[-1500:], r.stderr[-3000:])
    print(r.stdout)
    rep = json.load(open(report))
    assert sorted(rep) == sorted(want)
    bad = {k: v for k, v in rep.items() if v != "ok"}
    assert not bad, bad


def _main(switch, report):
    lib, hdr = BC.lib(), BC.header_functions()
    rep = {}
    try:
        for c in BC.CASES:
            if c.switch == switch:
                t0 = time.time()
                try:
                    print(TB.check_case(c, lib, hdr, guarded_ctx=MinAlignCtx), f"[{time.time() - t0:.2f} s]")
                    rep[c.id] = "ok"
                except Exception as e:  # noqa: BLE001  (the parent names the case from the report)
                    if TB._is_fault(e):
                        raise TB.GpuFault(str(e)) from e
                    rep[c.id] = f"{type(e).__name__}: {e}"[:600]
    except TB.GpuFault as e:
        print(f"GPU fault: {e}", file=sys.stderr)
        return 3
    json.dump(rep, open(report, "w"))
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv[1], sys.argv[2]))
