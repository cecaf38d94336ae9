"""Guarded arenas for the footprint tests: a tensor view whose every neighbouring byte is a known sentinel.

``guarded(shape, dtype, device, ld=...)`` returns ``(view, handle)``.  The view has the logical shape and a row stride of
``ld`` elements (leading dimensions are flattened into rows, ``ld`` elements apart); it lies inside ONE larger allocation
whose other bytes -- a red zone in front, one behind, and the columns ``shape[-1] .. ld`` of every row -- hold the
sentinel.  A kernel that stores outside its documented output changes a sentinel byte, which ``handle.assert_untouched()``
finds and reports as (row, column) relative to the view; a kernel whose result depends on padding it was told to ignore
gives different bits under two different sentinels (``PATTERNS``).

The sentinel is a 16-bit word repeated over the allocation.  Both patterns are NaN read as bf16, NaN read as fp32 (the
word twice) and a recognisable non-zero value read as uint8 / int32 / int64.
"""
import contextlib
import math

import torch

PATTERNS = (0x7FC1, 0xFFA5)        # bf16 NaN; doubled (0x7FC17FC1, 0xFFA5FFA5): fp32 NaN; bytes C1 7F / A5 FF
RED_ZONE = 1 << 20                 # bytes on each side, every arena
GEMM_RED_ZONE = 4 << 20            # GEMM operands and outputs: more than a 256-row band at the widest ld the tests use
ALIGN = 256                        # bytes; what the caching allocator gives a fresh tensor, so no entry point sees less


def _pattern_bytes(fill, nbytes, device, phase=0):
    """nbytes of the repeated little-endian 16-bit word ``fill``, starting at byte ``phase`` of the word"""
    lo, hi = fill & 0xFF, (fill >> 8) & 0xFF
    assert lo and hi, "both sentinel bytes must be non-zero"
    pair = torch.tensor([lo, hi] if phase % 2 == 0 else [hi, lo], dtype=torch.uint8, device=device)
    return pair.repeat((nbytes + 1) // 2)[:nbytes]


class Arena:
    """One allocation: [front red zone | rows of ld elements, shape[-1] of them logical | back red zone]."""

    def __init__(self, shape, dtype, device, ld, front, back, fill, misalign, align):
        self.shape = tuple(int(s) for s in shape)
        assert len(self.shape) >= 1 and all(s > 0 for s in self.shape)
        self.dtype, self.fill = dtype, fill
        self.item = torch.empty((), dtype=dtype).element_size()
        self.cols = self.shape[-1]
        self.rows = int(math.prod(self.shape[:-1]))
        self.ld = self.cols if ld is None else int(ld)
        assert self.ld >= self.cols
        assert align % self.item == 0 and align % 2 == 0
        front = -(-int(front) // align) * align
        # the view starts `front` bytes into an aligned base, plus `misalign` elements (the 4-byte-aligned paths)
        span = ((self.rows - 1) * self.ld + self.cols) * self.item
        total = front + misalign * self.item + span + int(back)
        total += total % 2
        raw = torch.empty(total + align, dtype=torch.uint8, device=device)
        skew = (-raw.data_ptr()) % align
        self.bytes = raw[skew:skew + total]
        self.bytes.copy_(_pattern_bytes(fill, total, device))
        self.start = front + misalign * self.item            # byte offset of the view inside self.bytes
        self.span = span
        assert self.start % self.item == 0
        self.view = self._strided(self.bytes)
        assert (self.view.data_ptr() - misalign * self.item) % align == 0

    def _strided(self, byte_tensor):
        """the logical view laid over a byte tensor of the arena's size"""
        n = (self.rows - 1) * self.ld + self.cols
        flat = byte_tensor[self.start:self.start + n * self.item].view(self.dtype)
        strides, s = [], self.ld
        for dim in reversed(self.shape[:-1]):
            strides.insert(0, s)
            s *= dim
        return flat.as_strided(self.shape, strides + [1])

    @property
    def ptr(self):
        return self.view.data_ptr()

    def logical(self):
        """the logical elements (the strided view itself; clone it to keep a copy)"""
        return self.view

    def fill_logical_(self, value):
        self.view.fill_(value)
        return self

    def _sentinel_mask(self):
        """True for every byte of the allocation that is no logical element"""
        mask = torch.ones_like(self.bytes)
        mask[self.start:self.start + self.span].as_strided((self.rows, self.cols * self.item), (self.ld * self.item, 1)).zero_()
        return mask.bool()

    def where(self, byte_offset):
        """(row, column) of a byte of the allocation relative to the view; rows < 0 lie in the front zone, columns >=
        shape[-1] in the padding, rows >= the row count in the back zone"""
        rel = int(byte_offset) - self.start
        row_bytes = self.ld * self.item
        row = rel // row_bytes
        return row, (rel - row * row_bytes) // self.item

    def changed_sentinel_bytes(self):
        """byte offsets (into the allocation, ascending) of the sentinel bytes that no longer hold the pattern"""
        expect = _pattern_bytes(self.fill, self.bytes.numel(), self.bytes.device)
        bad = (self.bytes != expect) & self._sentinel_mask()
        return torch.nonzero(bad).flatten()

    def assert_untouched(self, name="arena"):
        idx = self.changed_sentinel_bytes()
        if idx.numel():
            first, last = int(idx[0]), int(idx[-1])
            raise AssertionError(
                f"{name}: {idx.numel()} sentinel byte(s) changed around a view of shape {self.shape}, ld {self.ld}: first at "
                f"(row {self.where(first)[0]}, column {self.where(first)[1]}), last at (row {self.where(last)[0]}, column "
                f"{self.where(last)[1]}); byte offsets {first - self.start} .. {last - self.start} from the view's first element")

    def snapshot(self):
        return self.bytes.clone()

    def assert_same(self, snap, name="arena"):
        """every byte of the allocation, logical elements included, is what ``snap`` recorded"""
        idx = torch.nonzero(self.bytes != snap).flatten()
        if idx.numel():
            first, last = int(idx[0]), int(idx[-1])
            raise AssertionError(f"{name}: {idx.numel()} byte(s) of an input changed: first at (row, column) {self.where(first)}, "
                                 f"last at {self.where(last)}")


def guarded(shape, dtype, device, ld=None, front=None, back=None, fill=PATTERNS[0], misalign=0, gemm=False, align=ALIGN):
    """(view, handle): a strided view of ``shape`` with row stride ``ld`` inside a sentinel-filled allocation.  The logical
    elements start as sentinel too (NaN for the float types); ``handle.fill_logical_`` overwrites them."""
    zone = GEMM_RED_ZONE if gemm else RED_ZONE
    front = zone if front is None else front
    back = zone if back is None else back
    a = Arena(shape, dtype, device, ld, front, back, fill, misalign, align)
    return a.view, a


def guarded_like(t, device, ld=None, **kw):
    """a guarded copy of the (CPU) tensor ``t``: the input form, padding poisoned"""
    view, h = guarded(t.shape, t.dtype, device, ld=ld, **kw)
    view.copy_(t)
    return view, h


def _bits(t):
    return t.detach().contiguous().view(torch.uint8)


@contextlib.contextmanager
def unchanged(*tensors):
    """asserts on exit that every tensor (or Arena: then its whole allocation) is bitwise what it was on entry"""
    snaps = [t.snapshot() if isinstance(t, Arena) else _bits(t).clone() for t in tensors]
    yield
    for i, (t, s) in enumerate(zip(tensors, snaps)):
        if isinstance(t, Arena):
            t.assert_same(s, f"input {i}")
        else:
            assert torch.equal(_bits(t), s), f"input {i} (shape {tuple(t.shape)}) was modified"
