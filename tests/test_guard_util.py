"""tests/guard_util.py on CPU tensors: the arena reports an overwrite in the right buffer and on the right side, passes when
nothing was touched, counts exactly the elements that were never stored, and puts the tail guard at a tensor's exact end."""
import pytest
import torch

import guard_util as GU

DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64]


def _arena():
    a = GU.Arena("cpu")
    x = a.tensor((3, 5), torch.float32, fill=torch.arange(15.0), name="x")
    y = a.tensor((7,), torch.float16, name="y")
    w = a.raw(300, name="ws")
    return a, x, y, w


def _rec(a, name):
    return next(r for r in a.bufs if r.name == name)


def test_untouched_arena_passes():
    a, x, y, w = _arena()
    a.check()
    assert a.damage() == []
    x.mul_(2.0)                                    # writing the tensors themselves is what they are for
    y.zero_()
    w.zero_()
    a.check()
    assert torch.equal(x.flatten(), 2 * torch.arange(15.0))


def test_layout_alignment_and_guard_sizes():
    a, x, y, w = _arena()
    for t, name in ((x, "x"), (y, "y"), (w, "ws")):
        r = _rec(a, name)
        assert t.is_contiguous() and t.data_ptr() % 256 == 0 and a.ptr(t) == t.data_ptr()
        assert r.off >= GU.GUARD and r.buf.numel() - (r.off + r.nbytes) >= GU.GUARD
        assert r.nbytes == t.numel() * t.element_size() == a.nbytes(t)
    assert GU.GUARD > 32 * 32 * 32 * 4 and GU.GUARD > 128 * 128 * 8      # one pass of planes of any kernel
    assert a.guarded_bytes() >= 6 * GU.GUARD
    # the poison is a NaN in every floating type
    for dt in DTYPES:
        assert bool(torch.isnan(a.tensor((4,), dt)).all())


@pytest.mark.parametrize("where", ["before", "after", "tail_end"])
def test_planted_overwrite_is_reported_in_the_right_buffer_and_side(where):
    a, x, y, w = _arena()
    r = _rec(a, "y")
    pos = {"before": r.off - 1, "after": r.off + r.nbytes, "tail_end": r.buf.numel() - 1}[where]
    r.buf[pos] = 0
    side = "head" if where == "before" else "tail"
    want = {"before": -1, "after": 0, "tail_end": r.buf.numel() - 1 - (r.off + r.nbytes)}[where]
    assert a.damage() == [("y", side, want, want, 1)]
    with pytest.raises(GU.GuardError) as e:
        a.check()
    msg = str(e.value)
    assert msg.startswith("y: " + side) and f"{want:+d}" in msg and "x:" not in msg and "ws:" not in msg


def test_first_and_last_changed_offsets_of_a_run():
    a, x, y, w = _arena()
    r = _rec(a, "ws")
    end = r.off + r.nbytes
    r.buf[end + 4:end + 1028] = 1
    assert a.damage() == [("ws", "tail", 4, 1027, 1024)]


def test_tail_guard_starts_at_the_exact_end_of_an_odd_sized_tensor():
    a = GU.Arena("cpu")
    t = a.tensor((37, 3), torch.bfloat16, fill=torch.zeros(37, 3))           # 222 bytes: no multiple of 256, nor of 16
    r = a.bufs[0]
    assert r.nbytes == 222 and r.nbytes % 16 != 0
    flat = r.buf
    assert int(flat[r.off + 221]) == 0 and int(flat[r.off + 222]) == GU.POISON
    a.check()
    flat[r.off + 222] = 7                                                    # a store one element too far
    assert a.damage() == [(r.name, "tail", 0, 0, 1)]
    ws = a.raw(1001)
    assert ws.numel() == 1001 and a.bufs[1].buf[a.bufs[1].off + 1001:].numel() >= GU.GUARD
    empty = a.raw(0)
    assert empty.numel() == 0 and a.ptr(empty) % 256 == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_unwritten_counts_exactly_the_elements_not_stored(dtype):
    a = GU.Arena("cpu")
    t = a.tensor((5, 9), dtype)
    assert a.unwritten(t) == 45
    t[:, :4] = 1.5
    assert a.unwritten(t) == 25
    t[4, 8] = float("nan")                       # an ordinary NaN is a stored value, not the poison
    assert a.unwritten(t) == 24
    t.view(-1)[:] = 0
    assert a.unwritten(t) == 0
    full = a.tensor((6,), dtype, fill=torch.ones(6))
    assert a.unwritten(full) == 0
    a.check()


def test_unwritten_on_integer_outputs():
    a = GU.Arena("cpu")
    t = a.tensor((2, 3), torch.int32)
    assert a.unwritten(t) == 6
    t[0] = 0
    assert a.unwritten(t) == 3
