"""Operands inside larger buffers, for the layout tests of the row kernels (test_hip_row_op_edges.py, test_hip_instnorm_forms.py): inputs sit
in NaN-filled buffers (a read outside the view poisons the result), outputs in sentinel-filled buffers whose every byte outside the view must
survive."""
import ctypes as C

import torch

DEV = "cuda"
SENT = 1536.0          # exact in bf16


def _nvec(dtype):
    return 16 // torch.empty(0, dtype=dtype).element_size()


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Slot:
    """a channels-last view of `shape` = (..., C) inside a larger buffer.  layout: "contig" (the buffer is the view), "slice" (16-byte aligned
    channel slice of wider rows, ld % N == 0), "off8" (slice that starts 8 bytes into a 16-byte unit, ld % N == 0), "ldodd" (aligned base,
    ld % N != 0), "off4" / "off2" (slice that starts 4 / 2 bytes into a 16-byte unit, ld % N == 0; "off2": two-byte types only).  The
    non-contiguous layouts have 16 leading and one trailing slab of rows around the view (16 keeps the base aligned)."""

    def __init__(self, shape, dtype, layout, fill):
        n = _nvec(dtype)
        c = shape[-1]
        cp = -(-c // n) * n
        self.layout = layout
        if layout == "contig":
            self.buf = torch.full(shape, fill, dtype=dtype, device=DEV)
            self.view = self.buf
            self.index = None
            return
        off, ld = {"slice": (n, cp + 3 * n), "off8": (n // 2, cp + 2 * n), "ldodd": (0, cp + n + 1), "off4": (n // 4, cp + 2 * n),
                   "off2": (n // 8, cp + 2 * n)}[layout]
        assert off > 0 or layout == "ldodd", (layout, dtype)
        pre = 16
        self.buf = torch.full((pre + shape[0] + 1,) + tuple(shape[1:-1]) + (ld,), fill, dtype=dtype, device=DEV)
        self.index = (slice(pre, pre + shape[0]),) + (slice(None),) * (len(shape) - 2) + (slice(off, off + c),)
        self.view = self.buf[self.index]
        es = self.buf.element_size()
        assert self.buf.data_ptr() % 16 == 0
        assert (self.view.data_ptr() % 16 == 0) == (layout not in ("off8", "off4", "off2")) and (ld % n == 0) == (layout != "ldodd") and ld * es >= c * es


def place_in(values, layout):
    """an input operand: `values` copied into a view of the given layout, NaN all around it"""
    s = Slot(tuple(values.shape), values.dtype, layout, float("nan"))
    s.view.copy_(values)
    return s.view


def place_out(shape, dtype, layout):
    return Slot(tuple(shape), dtype, layout, SENT)


def assert_untouched(slot, what):
    """every element of the buffer outside the view still holds the sentinel, bit for bit"""
    if slot.index is None:
        return
    keep = torch.ones(slot.buf.shape, dtype=torch.bool, device=DEV)
    keep[slot.index] = False
    want = int(_bits(torch.tensor([SENT], dtype=slot.buf.dtype))[0])
    bad = (_bits(slot.buf) != want) & keep
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} element(s) outside the output view were written, first at {tuple(bad.nonzero()[0].tolist())}"


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
