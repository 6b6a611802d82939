"""functional._aligned on CPU tensors: what the wrappers do to every read-only tensor before its address goes to the library
(include/pdecnn.h, "Alignment").  An aligned tensor comes back as the same object — no copy, no launch on the common path —
and a contiguous view at a storage offset, which ``.contiguous()`` leaves where it is, comes back aligned with equal values."""
import pytest
import torch


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64])
def test_aligned_passes_an_aligned_tensor_through_and_copies_an_offset_view(dtype):
    from cnn_with_pde_amd import functional as F
    assert F.ALIGN == 16 and F._aligned(None) is None
    t = torch.arange(4 * 6 * 6, dtype=torch.float32).reshape(4, 6, 6).to(dtype)
    assert t.data_ptr() % F.ALIGN == 0
    assert F._aligned(t) is t
    assert F._aligned(t.detach()).data_ptr() == t.data_ptr()
    flat = torch.zeros(t.numel() + 1, dtype=dtype)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.contiguous() is view and view.data_ptr() % F.ALIGN != 0
    got = F._aligned(view.contiguous())
    assert got is not view and got.data_ptr() % F.ALIGN == 0 and got.is_contiguous()
    assert got.dtype == dtype and got.shape == t.shape and torch.equal(got, t)
    assert torch.equal(flat[1:], t.flatten()) and flat[0] == 0                   # the caller's buffer is left alone
    # a batch slice: 6 x 6 bf16 / fp16 samples are 72 bytes, fp32 ones 144, doubles 288 — u[1:] begins there
    s = t[1:]
    want_same = (36 * t.element_size()) % F.ALIGN == 0
    assert (F._aligned(s.contiguous()) is s) == want_same
    assert F._aligned(s.contiguous()).data_ptr() % F.ALIGN == 0 and torch.equal(F._aligned(s.contiguous()), t[1:])
