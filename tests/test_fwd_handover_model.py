"""The host-side model of the forward's hand-over protocol (tools/fwd_handover_model.py): for every set of round trips the
kernel issues ahead of their use, eight waves stepped through jobs of 1-3 chunks in arbitrary interleavings never stall,
never wait for progress through a record they have not passed themselves, never overwrite a ring slot a wave may still
read, and always find a complete record where they read one.  The kernel's spin has no bound, so this is what stands
between a mistake in the order and a hung device.  Planted mistakes show that the checks see one.  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fwd_handover_model as M  # noqa: E402


@pytest.mark.parametrize("ahead", M.CANDIDATES)
def test_every_interleaving_runs_to_the_end(ahead):
    for chunks in (1, 2, 3):
        for steps, pair_x in ((2, 1), (3, 0)):
            assert M.waits_only_for_earlier_records(chunks, steps, pair_x, ahead)
            runs, moves, polls, met = M.check(chunks, steps, pair_x, ahead, seeds=2)
            assert runs == 2 + 2 * M.WAVES + 1 and moves > 0
            assert (met > 0) == bool(ahead & M.POLL and polls)


def test_the_masks_are_the_kernel_instantiations():
    # PDE_FWD_AHEAD_LIST of csrc/pde_adi_launch.h
    src = open(os.path.join(os.path.dirname(M.__file__), "..", "cnn-with-pde_amd", "csrc", "pde_adi_launch.h")).read()
    line = [ln for ln in src.splitlines() if ln.startswith("#define PDE_FWD_AHEAD_LIST")][0]
    built = sorted(int(x.split(")")[0]) for x in line.split("PDE_CASE(")[1:])
    assert built == sorted(M.MASKS)


@pytest.mark.parametrize("mistake", M.MISTAKES)
def test_a_planted_mistake_is_seen(mistake):
    with pytest.raises(M.Violation):
        for ahead in (0, M.ROWS | M.POLL | M.HEAD | M.CHUNK):
            M.check(3, 3, 0, ahead, seeds=3, mistake=mistake)
