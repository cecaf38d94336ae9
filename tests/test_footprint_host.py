"""The guarded arenas of tests/_footprint.py on CPU tensors: a changed byte in the padding columns, the front zone or the
back zone is found and located; an untouched arena passes; the sentinels are NaN in fp32 and bf16; views are aligned."""
import re

import pytest
import torch

import _footprint as F

CPU = torch.device("cpu")


@pytest.mark.parametrize("fill", F.PATTERNS)
def test_sentinel_is_nan_in_fp32_and_bf16_and_nonzero_as_integers(fill):
    for dtype in (torch.float32, torch.bfloat16):
        view, h = F.guarded((5, 7), dtype, CPU, ld=12, fill=fill)
        assert bool(torch.isnan(view).all())                                  # the logical elements start as sentinel
        pad = torch.as_strided(view, (5, 12), (12, 1))[:, 7:]
        assert bool(torch.isnan(pad).all())
        zone = h.bytes[:h.start].view(dtype)
        assert bool(torch.isnan(zone).all()) and zone.numel() * h.item >= F.RED_ZONE
    lo, hi = fill & 0xFF, fill >> 8
    _, h = F.guarded((3,), torch.uint8, CPU, fill=fill)
    assert set(h.bytes.tolist()) == {lo, hi} and lo and hi
    v32, _ = F.guarded((3,), torch.int32, CPU, fill=fill)
    v64, _ = F.guarded((3,), torch.int64, CPU, fill=fill)
    word = fill | fill << 16
    assert [x & 0xFFFFFFFF for x in v32.tolist()] == [word] * 3
    assert [x & 0xFFFFFFFFFFFFFFFF for x in v64.tolist()] == [word | word << 32] * 3
    assert F.PATTERNS[0] != F.PATTERNS[1]


def test_an_untouched_arena_passes_and_logical_writes_are_free():
    view, h = F.guarded((2, 3, 42), torch.float32, CPU, ld=46)
    assert view.shape == (2, 3, 42) and view.stride() == (138, 46, 1)
    h.assert_untouched()
    h.fill_logical_(float("nan"))
    h.assert_untouched()
    view.copy_(torch.arange(2 * 3 * 42, dtype=torch.float32).view(2, 3, 42))
    h.assert_untouched()
    assert torch.equal(h.logical().reshape(-1), torch.arange(252, dtype=torch.float32))
    assert h.logical().data_ptr() == view.data_ptr()


def _poke(h, row, col, byte=0):
    """flip one byte of the element at (row, col) relative to the view"""
    off = h.start + (row * h.ld + col) * h.item + byte
    h.bytes[off] ^= 0x10
    return off


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8, torch.int64])
@pytest.mark.parametrize("row,col,what", [(3, 42, "first pad column"), (3, 45, "last pad column"), (0, 42, "pad of row 0"),
                                          (-1, 45, "front zone, the byte before the view"), (-700, 3, "deep in the front zone"),
                                          (4, 42, "back zone, right behind the last logical element"), (5, 0, "back zone, next row"),
                                          (900, 7, "deep in the back zone")])
def test_one_changed_sentinel_byte_raises_and_is_located(dtype, row, col, what):
    view, h = F.guarded((5, 42), dtype, CPU, ld=46)
    _poke(h, row, col, byte=h.item - 1)
    with pytest.raises(AssertionError) as e:
        h.assert_untouched("out")
    msg = str(e.value)
    assert msg.startswith("out: 1 sentinel byte(s) changed"), msg
    assert len(re.findall(rf"\(row {row}, column {col}\)", msg)) == 2, (what, msg)      # first == last


def test_first_last_and_count_are_reported():
    view, h = F.guarded((5, 42), torch.float32, CPU, ld=46)
    view.fill_(1.0)
    h.bytes[0] ^= 1                                     # the very first byte of the front zone
    _poke(h, 2, 43)
    h.bytes[-1] ^= 1                                    # the very last byte of the back zone
    with pytest.raises(AssertionError) as e:
        h.assert_untouched()
    msg = str(e.value)
    assert "3 sentinel byte(s)" in msg
    first, last = h.where(0), h.where(h.bytes.numel() - 1)
    assert first[0] < 0 and last[0] >= 5
    assert f"first at (row {first[0]}, column {first[1]})" in msg and f"last at (row {last[0]}, column {last[1]})" in msg


def test_every_sentinel_byte_is_watched_and_no_logical_byte_is():
    """exhaustive on a small arena: flipping any single byte raises exactly when it is not a logical element"""
    view, h = F.guarded((3, 5), torch.bfloat16, CPU, ld=8, front=64, back=64, align=64)
    logical = set()
    for r in range(3):
        for c in range(5):
            for b in range(2):
                logical.add(h.start + (r * 8 + c) * 2 + b)
    assert h.bytes.numel() >= 64 + (2 * 8 + 5) * 2 + 64
    for off in range(h.bytes.numel()):
        h.bytes[off] ^= 0x55
        if off in logical:
            h.assert_untouched()
        else:
            with pytest.raises(AssertionError):
                h.assert_untouched()
        h.bytes[off] ^= 0x55
    h.assert_untouched()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.uint8])
def test_views_are_aligned_and_misalign_shifts_by_elements(dtype):
    item = torch.empty((), dtype=dtype).element_size()
    v, h = F.guarded((4, 10), dtype, CPU, ld=16)
    assert v.data_ptr() % F.ALIGN == 0 and h.ptr == v.data_ptr()
    assert h.start >= F.RED_ZONE and h.bytes.numel() - h.start - h.span >= F.RED_ZONE
    v1, h1 = F.guarded((4, 10), dtype, CPU, ld=16, misalign=1)
    assert v1.data_ptr() % F.ALIGN == item
    assert h1.start >= F.RED_ZONE and h1.bytes.numel() - h1.start - h1.span >= F.RED_ZONE
    vg, hg = F.guarded((4, 10), dtype, CPU, ld=16, gemm=True)
    assert hg.start >= F.GEMM_RED_ZONE and hg.bytes.numel() - hg.start - hg.span >= F.GEMM_RED_ZONE
    # more than a 256-row band at the widest leading dimension the GEMM cases use (2048 + 16 bf16, 768 + 8 fp32)
    assert F.GEMM_RED_ZONE > 256 * (2048 + 16) * 2 and F.GEMM_RED_ZONE > 256 * (768 + 8) * 4
    h1.assert_untouched()
    # the sentinel stays NaN for a misaligned fp32 view's padding (the pattern has a period of two bytes)
    if dtype == torch.float32:
        assert bool(torch.isnan(torch.as_strided(v1, (4, 16), (16, 1))[:, 10:]).all())


def test_unchanged_context_manager():
    t = torch.randn(7, 3)
    t[0, 0] = float("nan")                              # bitwise: a NaN that stays is no change
    view, h = F.guarded_like(torch.randn(4, 5), CPU, ld=9)
    with F.unchanged(t, h, view):
        pass
    with pytest.raises(AssertionError, match="input 0"):
        with F.unchanged(t, h):
            t[3, 1] += 1.0
    with pytest.raises(AssertionError, match="input 1"):
        with F.unchanged(t, h):
            view[2, 2] = 0.5
    with pytest.raises(AssertionError, match="input 1"):
        with F.unchanged(t, h):
            _poke(h, 1, 7)                              # padding of an input counts too
