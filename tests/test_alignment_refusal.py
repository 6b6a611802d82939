"""Every entry point refuses a pointer below the alignment include/pdecnn.h asks of it, on the host, before anything touches
the runtime (the "Alignment" section of the header; the table is tests/bounds_cases.py).

For every call of every case of the table, and for every non-NULL device pointer the call is handed — directly, inside a
``PdeSmallLayer`` or inside an array of pointers — the call is replayed through the real library with that ONE pointer
advanced: by one element of its type where the requirement exceeds the element, otherwise by one byte (elements wider than a
byte), a workspace by 4 bytes.  The answer must be PDE_E_BADARG, for a workspace PDE_E_WORKSPACE.  Addresses are made up
(a context that hands out well-separated 4 KiB-aligned numbers), workspaces have the sizes really queried; nothing is
allocated.  Every call is also made once with all its pointers in order: it must get PAST validation (any answer but the
host-side refusals), or its replays would be refused for some other reason and prove nothing.

The replays run in one child interpreter that sees no device (this file run as a script): a refusal that is missing would
otherwise launch a kernel on made-up addresses on a machine that has a GPU; without a device such a launch fails and the
call answers PDE_E_LAUNCH, which the parent reports as the missing refusal it is — and which is what the call with all its
pointers in order answers.

No pointer may be skipped: per function the parent counts the pointer parameters the sweep exercised against
``header_functions()`` and fails on a shortfall."""
import ctypes as C
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bounds_cases as BC  # noqa: E402
import bounds_input_cases  # noqa: E402

bounds_input_cases.register()                    # the *_backward_input cases belong to the table (see that file)
#: the table, and the input backward's own matrix: only there does every sub-family get the forward's workspace handed over
CASES = list(BC.CASES) + list(bounds_input_cases.MATRIX_CASES)

BADARG, WORKSPACE = -1, -5
#: what validation on the host answers (pdecnn.h: BADARG, UNSUPPORTED_N, TOO_MANY_SWEEPS, WORKSPACE); PDE_E_LAUNCH is not among them
HOST_REFUSALS = (-1, -2, -3, -5)

#: pointer parameters that are no device buffers, and why the sweep does not advance them
HOST_POINTERS = {
    "d": "the launch descriptor, host memory",
    "layers": "an array of PdeSmallLayer in host memory (the device pointers inside it are advanced one by one)",
    "ckpt_mask": "two host words", "emit_mask": "two host words",
    "stream": "a hipStream_t", "kappa_event": "a hipEvent_t, NULL in every case",
    "kappa_max_host": "pinned host memory, NULL in every case (its check shares the line of kappa_max)",
}
#: families whose calls take device pointers inside a struct (PdeSmallLayer) or inside host arrays of pointers
EMBEDDED = ("multi", "gate")
#: buffers of the shared-input cases that are not named after the PdeSmallLayer field they are stored in
FIELD_OF = {"sws": "steps_workspace", "bws": "workspace", "weights": "weight_ptr"}


class FakeCtx(BC.SpecCtx):
    """Hands out addresses nothing lives at; ``bump`` moves one buffer."""

    def __init__(self, bump=None):
        super().__init__()
        self.bump = dict(bump or {})
        self.addr = {}

    def _alloc(self, name, role, shape, dtype, fill):
        self.addr[name] = (1 << 40) + (len(self.addr) << 32)
        return None

    def ptr(self, name, byte_offset=0):
        return self.addr[name] + self.bump.get(name, 0) + byte_offset


def _step(ctx, buf):
    """(bytes to advance the buffer by, the code the call must answer) — None where no advance leaves the requirement."""
    item = torch.empty((), dtype=ctx.dtypes[buf]).element_size()
    if ctx.dtypes[buf] == torch.uint8 and ctx.roles[buf] in ("ws", "carry"):
        return 4, WORKSPACE
    if ctx.aligns[buf] > item:
        return item, BADARG
    return (1, BADARG) if item > 1 else None


def sweep_case(case, lib, hdr):
    """[(function, parameter, buffer, advance, answer, expected)] for every pointer of every call of the case."""
    rows = []
    ctx = FakeCtx()
    calls, _ = case.build(ctx)
    embedded = case.family in EMBEDDED
    direct = set()
    for fn, amap in calls:
        # the call as the case makes it: past every host-side check (no device: its first launch then fails)
        rows.append((fn, None, None, 0, getattr(lib, fn)(*BC.call_args(ctx, hdr[fn], amap)), None))
        for pname, buf, _ in BC.bound_buffers(ctx, hdr[fn], amap):
            direct.add(buf)
            step = _step(ctx, buf)
            assert step is not None, (case.id, fn, pname, buf)
            ctx.bump = {buf: step[0]}
            rc = getattr(lib, fn)(*BC.call_args(ctx, hdr[fn], amap))
            ctx.bump = {}
            rows.append((fn, pname, buf, step[0], rc, step[1]))
    if embedded:                                             # the pointers were stored when the case was built: build again
        for buf in ctx.roles:
            if buf in direct:
                continue
            step = _step(ctx, buf)
            assert step is not None, (case.id, buf)
            moved = FakeCtx({buf: step[0]})
            mcalls, _ = case.build(moved)
            field = FIELD_OF.get(BC.param_of(buf), BC.param_of(buf)) if case.family == "multi" else BC.param_of(buf)
            for fn, amap in mcalls:
                # a shared-input call checks the whole struct, the other pass's pointers too; a gate call the arrays it takes
                if case.family == "gate" and field not in {n for n, _, _ in hdr[fn]}:
                    continue
                rc = getattr(lib, fn)(*BC.call_args(moved, hdr[fn], amap))
                rows.append((fn, field, buf, step[0], rc, step[1]))
    return rows


def _child(report):
    assert not torch.cuda.is_available(), "the sweep must not see a device"
    lib, hdr = BC.lib(), BC.header_functions()
    out = {}
    for c in CASES:
        out[c.id] = sweep_case(c, lib, hdr)
    json.dump(out, open(report, "w"))
    return 0


def test_every_pointer_below_its_alignment_is_refused(tmp_path):
    report = str(tmp_path / "report.json")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), report], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rep = json.load(open(report))
    assert sorted(rep) == sorted(c.id for c in CASES)
    base = [(cid, row[0], row[4]) for cid, rows in rep.items() for row in rows if row[1] is None]
    stuck = [b for b in base if b[2] in HOST_REFUSALS]
    assert len(base) > 1500 and not stuck, f"{len(stuck)} calls do not get past validation with every pointer in order: {stuck[:12]}"
    rep = {cid: [row for row in rows if row[1] is not None] for cid, rows in rep.items()}
    wrong = [(cid,) + tuple(row) for cid, rows in rep.items() for row in rows if row[4] != row[5]]
    assert not wrong, f"{len(wrong)} misaligned pointers were not refused as the header says (case, function, parameter, " \
                      f"buffer, advance, answer, expected): {wrong[:12]}"
    # the count: every pointer parameter of every function the table calls was advanced at least once, is host memory, or
    # travels inside the struct / arrays whose entries were
    hdr = BC.header_functions()
    exercised = {}
    for rows in rep.values():
        for fn, pname, *_ in rows:
            exercised.setdefault(fn, set()).add(pname)
    from cnn_with_pde_amd import _lib
    fields = {f for f, t in _lib.PdeSmallLayer._fields_ if t is C.c_void_p}          # its device pointers
    total = short = 0
    for fn in sorted(exercised):
        for pname, is_ptr, _ in hdr[fn]:
            if not is_ptr or pname in HOST_POINTERS:
                continue
            total += 1
            if pname not in exercised[fn]:
                short += 1
                print(f"not exercised: {pname} of {fn}")
        if fn.startswith("pde_adi_multi_"):
            # NULL in the shared-input cases (mode 1 has no skip blend; the pinned mirror is NULL in every case): the one-layer
            # calls pde_adi_small_* hand skip_weight / g_skip_weight over as parameters, and those are counted above
            missing = fields - {"kappa_max_host", "skip_weight", "g_skip_weight"} - exercised[fn]
            total += len(fields) - 3
            short += len(missing)
            assert not missing, (fn, missing)
    n = sum(len(rows) for rows in rep.values())
    print(f"{n} replays over {len(exercised)} functions; {total} device-pointer parameters, {short} never advanced")
    assert short == 0 and len(exercised) >= len(BC.writing_functions()) - len(BC.EXCLUDED)
    assert n > 5000


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1]))
