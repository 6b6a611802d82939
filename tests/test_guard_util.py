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


@pytest.mark.parametrize("align", [2, 4, 8, 16, 256])
def test_a_skewed_arena_places_buffers_at_exactly_their_alignment(align):
    """address = align (mod 2 * align): a multiple of the alignment asked for and of nothing larger — 16 mod 32 for a
    tensor of the C ABI, 4 mod 8 for one of its fp32 scalars — for odd sizes and for the empty buffer too."""
    a = GU.Arena(skew=True)
    for nbytes in (0, 1, 24, 1001):
        v = a.raw(nbytes, align=align)
        assert a.ptr(v) % (2 * align) == align and v.numel() == nbytes
        if nbytes:
            assert v.data_ptr() == a.ptr(v)
    for dtype in (torch.float16, torch.float32, torch.float64, torch.int32):
        item = torch.empty((), dtype=dtype).element_size()
        if align < item:
            with pytest.raises(ValueError):
                a.tensor((3, 5), dtype, align=align)
            continue
        t = a.tensor((3, 5), dtype, fill=torch.arange(15).reshape(3, 5), align=align)
        assert t.data_ptr() % (2 * align) == align and t.is_contiguous() and t.dtype == dtype
        assert torch.equal(t, torch.arange(15).reshape(3, 5).to(dtype)) and a.unwritten(t) == 0
    a.check()
    with pytest.raises(ValueError):
        a.raw(8, align=24)


def test_an_arena_without_skew_keeps_its_default_and_honours_a_smaller_alignment():
    a = GU.Arena()
    assert a.ptr(a.raw(40)) % GU.ALIGN == 0                          # what every test before the skew relied on
    assert a.tensor((7,), torch.float32, align=16).data_ptr() % 16 == 0


def test_the_guards_of_a_skewed_buffer_start_at_its_exact_first_and_last_byte():
    """The placement moves the view, never the guards' edges: a byte just before the first element and a byte just behind
    the last one of an odd-sized tensor are both reported at offsets -1 and 0."""
    a = GU.Arena(skew=True)
    t = a.tensor((37, 3), torch.bfloat16, fill=torch.zeros(37, 3), name="t", align=16)
    s = a.tensor((1,), torch.float32, fill=torch.zeros(1), name="s", align=4)
    assert t.data_ptr() % 32 == 16 and s.data_ptr() % 8 == 4
    a.check()
    r = a.bufs[0]
    assert r.nbytes == 37 * 3 * 2 and r.buf.data_ptr() + r.off == t.data_ptr()
    end = r.off + r.nbytes
    r.buf[r.off - 1] = 0
    r.buf[end] = 0
    assert a.damage() == [("t", "head", -1, -1, 1), ("t", "tail", 0, 0, 1)]
    r.buf[r.off - 1] = GU.POISON
    r.buf[end] = GU.POISON
    t[0, 0] = 1.0                                                    # the first and the last element are inside, not guard
    t[-1, -1] = 1.0
    a.check()
    q = a.bufs[1]
    q.buf[q.off + 4] = 0
    assert a.damage() == [("s", "tail", 0, 0, 1)]
    assert r.off >= GU.GUARD and r.buf.numel() - end >= GU.GUARD     # 1 MiB on both sides still
