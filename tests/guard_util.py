"""Guard bands and poison for the buffers of a C ABI call.

An ``Arena`` hands out tensors that are views into private ``uint8`` buffers: 1 MiB of guard in front of the view, 1 MiB
behind it (starting at the view's exact last byte + 1, no rounding), the view's base 256-byte aligned by default — far
more than include/pdecnn.h asks of any pointer.  With ``skew=True`` a buffer sits at EXACTLY the alignment asked for and
no more: its address is a multiple of ``align`` but not of ``2 * align`` (address = align mod 2 align: 16 mod 32 for a
tensor, 4 mod 8 for an fp32 scalar), which is how tests/test_gpu_alignment.py runs every entry point at the documented
minimum.  The guards begin at the view's exact first and last byte either way.  The whole buffer is filled with 0xFF before an
input's values are copied in: all-ones is a NaN in fp16, bf16, fp32 and fp64 (and -1 as an integer), so one pattern is both
the canary around a buffer and the poison inside an output or a workspace.

  * a write past either end of a buffer changes a guard byte: ``check()`` finds it and says where;
  * an output element the call never stored is still all-ones: ``unwritten()`` counts them;
  * scratch or partial sums read before the call wrote them are NaN and surface in the results.

The 1 MiB is a condition, not a measurement: it exceeds one pass of planes of any kernel of the library (32 planes of
32 x 32 fp32 are 128 KiB, one 128 x 128 double plane is 128 KiB), so a stray pass lands inside the guard."""
import torch

GUARD = 1 << 20
ALIGN = 256
POISON = 0xFF

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class GuardError(AssertionError):
    pass


class _Buf:
    __slots__ = ("name", "buf", "off", "nbytes")

    def __init__(self, name, buf, off, nbytes):
        self.name, self.buf, self.off, self.nbytes = name, buf, off, nbytes


class Arena:
    def __init__(self, device="cpu", skew=False):
        """``skew``: place every buffer at exactly its ``align`` (see above) instead of at least at it."""
        self.device = torch.device(device)
        self.skew = bool(skew)
        self.bufs = []
        self._by_view = {}

    # ---- handing out --------------------------------------------------------------------------------------------------
    def raw(self, nbytes, name=None, align=ALIGN):
        """A uint8 view of exactly ``nbytes`` bytes (0 allowed), 0xFF-filled, guards on both sides, its base a multiple of
        ``align`` (a power of two) — and, in a skewed arena, an odd multiple of it."""
        nbytes, align = int(nbytes), int(align)
        if nbytes < 0:
            raise ValueError("negative size")
        if align < 1 or align & (align - 1):
            raise ValueError("the alignment must be a power of two")
        span = 2 * align if self.skew else align
        buf = torch.full((GUARD + span - 1 + nbytes + GUARD,), POISON, dtype=torch.uint8, device=self.device)
        off = GUARD + (-(buf.data_ptr() + GUARD)) % span
        if self.skew:
            off += align                                         # a multiple of 2 * align, plus align: never more aligned
        rec = _Buf(name or f"buffer{len(self.bufs)}", buf, off, nbytes)
        self.bufs.append(rec)
        view = buf[off:off + nbytes]
        self._by_view[id(view)] = (rec, view)
        return view

    def tensor(self, shape, dtype, fill=None, name=None, align=ALIGN):
        """A contiguous tensor of ``shape`` / ``dtype`` inside the arena; ``fill`` (an input's values) is copied in,
        otherwise every element stays all-ones.  ``align``: as in ``raw``, at least the element's size."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = 1
        for s in shape:
            n *= s
        item = torch.empty((), dtype=dtype).element_size()
        if int(align) % item:
            raise ValueError("a tensor cannot begin between two of its elements' boundaries")
        raw = self.raw(n * item, name, align)
        rec = self._by_view.pop(id(raw))[0]
        t = raw.view(dtype).view(shape) if n else torch.empty(shape, dtype=dtype, device=self.device)
        self._by_view[id(t)] = (rec, t)
        if fill is not None:
            t.copy_(torch.as_tensor(fill).reshape(shape).to(dtype))
        return t

    def ptr(self, t):
        """The address of a tensor of this arena (defined for an empty one too: where its guard begins)."""
        rec = self._by_view[id(t)][0]
        return rec.buf.data_ptr() + rec.off

    def nbytes(self, t):
        return self._by_view[id(t)][0].nbytes

    def guarded_bytes(self):
        return sum(r.buf.numel() - r.nbytes for r in self.bufs)

    # ---- looking afterwards -------------------------------------------------------------------------------------------
    def damage(self):
        """[(buffer name, "head" | "tail", first, last, count)] for every guard that changed.  Offsets are in bytes from
        the tensor's edge: head -1 is the byte just before the tensor, tail 0 the byte just behind its last one."""
        found = []
        for r in self.bufs:
            end = r.off + r.nbytes
            for side, seg, origin in (("head", r.buf[:r.off], r.off), ("tail", r.buf[end:], 0)):
                if bool((seg == POISON).all()):
                    continue
                idx = (seg != POISON).nonzero().flatten()
                found.append((r.name, side, int(idx[0]) - origin, int(idx[-1]) - origin, int(idx.numel())))
        return found

    def check(self):
        bad = self.damage()
        if bad:
            raise GuardError("; ".join(
                f"{name}: {side} guard overwritten, {n} bytes changed, first at offset {a:+d} and last at {b:+d} "
                f"from the tensor's {'first byte' if side == 'head' else 'end'}" for name, side, a, b, n in bad))

    @staticmethod
    def unwritten(t):
        """How many elements of ``t`` are still the all-ones pattern."""
        if t.numel() == 0:
            return 0
        return int((t.contiguous().view(_INT_VIEW[t.element_size()]) == (POISON if t.element_size() == 1 else -1)).sum())
