"""Every pointer of the explicit and Jacobi layers' input backward below its alignment is refused on the host, as
include/pdecnn.h says: the sweep of tests/test_alignment_refusal.py (``sweep_case`` / ``FakeCtx``, imported from there)
replayed over the cases of tests/bounds_input_explicit_cases.py in a child interpreter that sees no device.  Every device
pointer of every new entry point is advanced by one element (a workspace by 4 bytes); the answer must be PDE_E_BADARG, for
a workspace PDE_E_WORKSPACE, and every call with its pointers in order must get past validation.

The entry points are declared in include/pdecnn_explicit_input.h; the sweep is handed the parse of both headers
(``bounds_input_explicit_cases.header_functions()``).  The cases are not in the table of tests/bounds_cases.py, so the
existing sweep does not replay them: this file does."""
import json
import os
import subprocess
import sys

import bounds_cases as BC
import bounds_input_explicit_cases as BE
import test_alignment_refusal as TA


def _child(report):
    import torch
    assert not torch.cuda.is_available(), "the sweep must not see a device"
    lib, hdr = BC.lib(), BE.header_functions()
    json.dump({c.id: TA.sweep_case(c, lib, hdr) for c in BE.CASES}, open(report, "w"))
    return 0


def test_every_pointer_of_the_new_entry_points_below_its_alignment_is_refused(tmp_path):
    report = str(tmp_path / "report.json")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), report], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rep = json.load(open(report))
    assert sorted(rep) == sorted(c.id for c in BE.CASES)
    base = [(cid, row[0], row[4]) for cid, rows in rep.items() for row in rows if row[1] is None]
    stuck = [b for b in base if b[2] in TA.HOST_REFUSALS]
    assert not stuck, f"{len(stuck)} calls do not get past validation with every pointer in order: {stuck[:12]}"
    rows = [(cid,) + tuple(row) for cid, rows in rep.items() for row in rows if row[1] is not None]
    wrong = [r for r in rows if r[5] != r[6]]
    assert not wrong, f"{len(wrong)} misaligned pointers were not refused as the header says (case, function, parameter, " \
                      f"buffer, advance, answer, expected): {wrong[:12]}"
    # no pointer skipped: every device pointer parameter of every new function
    hdr = BE.header_functions()
    exercised = {}
    for _, fn, pname, *_ in rows:
        exercised.setdefault(fn, set()).add(pname)
    for fn in BE.NEW_FUNCTIONS:
        want = {p for p, is_ptr, _ in hdr[fn] if is_ptr and p not in TA.HOST_POINTERS}
        if fn.startswith("pde_jacobi_f64_"):
            assert "workspace" not in want
        assert want <= exercised[fn], (fn, want - exercised[fn])
    n = sum(1 for r in rows if r[1] in BE.NEW_FUNCTIONS)
    print(f"{n} replays of the new entry points, {len(rows)} in all")
    assert n > 200


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1]))
