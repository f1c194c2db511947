"""Guarded device buffers and the error collector shared by the operator-level GPU tests (test_text_ops_gpu.py,
test_gemm_ops_gpu.py, test_attn_ops_gpu.py)."""
import numpy as np
import torch

from _text_refs import measure

SENTINEL = 12345.0


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Guarded:
    """A device buffer: NaN-filled live region of `shape` between two guard blocks of >= `guard` sentinel elements."""

    def __init__(self, shape, dtype, guard):
        self.n = int(np.prod(shape))
        self.g = max(64, (int(guard) + 63) // 64 * 64)          # multiples of 64 elements keep the live region 16-byte aligned
        self.buf = torch.full((2 * self.g + self.n,), SENTINEL, dtype=dtype, device="cuda")
        self.live = self.buf[self.g:self.g + self.n].view(shape)
        self.live.fill_(float("nan"))
        self.guard_bits = _bits(torch.full((self.g,), SENTINEL, dtype=dtype))

    @property
    def ptr(self):
        return self.live.data_ptr()

    def check(self, tag, written=None):
        """Guards untouched bit for bit, no NaN in the live region (or in its first `written` elements).  Returns a CPU copy."""
        raw = _bits(self.buf).cpu()
        assert torch.equal(raw[:self.g], self.guard_bits), f"{tag}: front guard written"
        assert torch.equal(raw[self.g + self.n:], self.guard_bits), f"{tag}: back guard written"
        out = self.live.cpu()
        chk = out.reshape(-1)[:written] if written is not None else out
        nan = int(torch.isnan(chk.float()).sum())
        assert nan == 0, f"{tag}: {nan} elements NaN / not written"
        return out


class Acc:
    """Collects (error, bound) pairs of one test; `add` asserts, `flush` reports the largest error and fraction of its bound."""

    def __init__(self, tag):
        self.tag, self.worst = tag, {}

    def add(self, name, err, bound, case):
        err, bound = float(err), float(bound)
        e, f = self.worst.get(name, (0.0, 0.0))
        self.worst[name] = (max(e, err), max(f, err / bound if bound > 0 else float(err > 0)))
        if not (np.isfinite(err) and err <= bound):
            print(f"[measured] {self.tag}/{name} {case}: error {err:.3e} bound {bound:.3e}")
        assert np.isfinite(err) and err <= bound, (self.tag, name, case, err, bound)

    def flush(self):
        for name, (e, f) in self.worst.items():
            measure(f"{self.tag}/{name}/max_abs_err", e)
            measure(f"{self.tag}/{name}/max_fraction_of_bound", f)


def check_written(tag, out, init_bits, mask):
    """The written-region rule of Guarded2D.check on host tensors: every element of `mask` holds no NaN any more, every other
    element still holds its initial bits (`init_bits`: NaN where a write was expected, the sentinel elsewhere)."""
    bits = _bits(out)
    keep = ~mask
    bad = int((bits[keep] != init_bits[keep]).sum())
    assert bad == 0, f"{tag}: {bad} elements outside the written region changed (pad columns / skipped rows / columns past N)"
    nan = int(torch.isnan(out[mask].float()).sum())
    assert nan == 0, f"{tag}: {nan} elements NaN / not written"


class Guarded2D(Guarded):
    """A [rows, ld] matrix whose first `cols` columns are live (NaN before the launch); the pad columns ld - cols hold the
    sentinel like the guards and must keep it.  `check` takes the (rows, cols) mask of the elements the launch has to write
    (default: all of them): those hold no NaN afterwards, every other element still holds its initial bits."""

    def __init__(self, rows, cols, ld, dtype, guard=None):
        assert ld >= cols
        super().__init__((rows, ld), dtype, guard if guard is not None else 4 * ld)
        self.rows, self.cols, self.ld = rows, cols, ld
        self.live[:, cols:] = SENTINEL
        self.init_bits = _bits(self.live).cpu().clone()

    def check(self, tag, written=None):
        out = super().check(tag, written=0)                       # guards only
        mask = torch.zeros(self.rows, self.ld, dtype=torch.bool)
        mask[:, :self.cols] = True if written is None else written.cpu()
        check_written(tag, out, self.init_bits, mask)
        return out[:, :self.cols]

    def untouched(self, tag):
        """Nothing at all was written (a refused launch)."""
        super().check(tag, written=0)
        assert torch.equal(_bits(self.live).cpu(), self.init_bits), f"{tag}: a refused launch wrote to its output"


def nan_after(values, dtype=None, pad=64):
    """`values` copied to the device with `pad` NaN elements right behind the last one: a read past the end shows."""
    flat = values.reshape(-1)
    dtype = dtype or values.dtype
    buf = torch.full((flat.numel() + pad,), float("nan"), dtype=dtype, device="cuda")
    buf[:flat.numel()] = flat.to(dtype)
    return buf[:flat.numel()].view(values.shape), buf


def padded(mat, ld, dtype=None):
    """[rows, cols] -> device [rows, ld] view of the first `cols` columns; the pad columns and 64 elements behind the last row
    hold NaN.  Returns (view, backing buffer): keep the buffer alive, pass view.data_ptr() and ld."""
    rows, cols = mat.shape
    dtype = dtype or mat.dtype
    buf = torch.full((rows * ld + 64,), float("nan"), dtype=dtype, device="cuda")
    full = buf[:rows * ld].view(rows, ld)
    full[:, :cols] = mat.to(dtype)
    return full[:, :cols], buf
