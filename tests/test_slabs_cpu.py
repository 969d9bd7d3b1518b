"""The slab helper of the kernel memory-contract tests (tests/helpers/slabs.py) on CPU tensors: every defect the GPU file
relies on it to report is planted here by hand and must be reported — a stray store one element past a row end, one row
past the last row and in the front guard, a logical element left unwritten — and a hardware NaN must not pass for the
sentinel."""

import pytest
import torch

from helpers import slabs as S

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
ROWS, COLS, GAP = 37, 40, 24


def _written(dtype, batch=1):
    """an output slab after a well-behaved kernel: sentinel everywhere, then every logical element written"""
    s = S.Slab.matrix(ROWS, COLS, dtype, gap=GAP, batch=batch)
    s.fill_all(S.SENTINEL[dtype])
    g = torch.Generator().manual_seed(1)
    s.fill_logical(torch.randn(*s.shape, generator=g))
    return s


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_guards_and_gap(dtype):
    s = S.Slab.matrix(ROWS, COLS, dtype, gap=GAP)
    ld = COLS + GAP
    assert s.view.shape == (ROWS, COLS) and s.view.stride() == (ld, 1) and ld % 8 == 0 and ld - COLS >= 8
    assert s.offset >= 64 * ld and s.buf.numel() - (s.offset + ROWS * ld) >= 256 * ld
    assert int(s.mask.sum()) == ROWS * COLS
    assert s.view.data_ptr() == s.buf.data_ptr() + s.byte_offset
    b = S.Slab.matrix(ROWS, COLS, dtype, gap=GAP, batch=3)
    assert b.view.shape == (3, ROWS, COLS) and b.view.stride() == ((ROWS + 256) * ld, ld, 1)   # guard rows between batches
    assert not bool(b.mask[b.offset + ROWS * ld: b.offset + b.strides[0]].any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_clean_slab_passes(dtype):
    s = _written(dtype)
    assert s.outside_intact(S.SENTINEL[dtype]) and s.logical_has_no_sentinel(S.SENTINEL[dtype])
    snap = s.snapshot()
    assert s.unchanged(snap) and torch.equal(s.logical_bits(), _written(dtype).logical_bits())


@pytest.mark.parametrize("dtype", DTYPES)
def test_stray_write_one_past_row_end_is_reported(dtype):
    s = _written(dtype)
    s.buf[s.offset + 5 * s.ld + COLS] = 1.0
    with pytest.raises(AssertionError, match=rf"\(row 5, col {COLS}\)"):
        s.outside_intact(S.SENTINEL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("batch", [1, 3])
def test_stray_write_one_row_past_the_last_is_reported(dtype, batch):
    s = _written(dtype, batch)
    s.buf[s.offset + ROWS * s.ld + 3] = 0.0          # (0.0: all bits clear, the easiest stray value to overlook)
    with pytest.raises(AssertionError, match=rf"\(row {ROWS}, col 3\)"):
        s.outside_intact(S.SENTINEL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
def test_stray_write_in_the_front_guard_is_reported(dtype):
    s = _written(dtype)
    s.buf[s.offset - s.ld + 7] = float("nan")        # a hardware NaN one row in front: not the sentinel's bits
    with pytest.raises(AssertionError, match=r"\(row -1, col 7\)"):
        s.outside_intact(S.SENTINEL[dtype])
    s = _written(dtype)
    s.buf[0] = 2.0                                   # the very first guard element
    with pytest.raises(AssertionError, match=r"\(row -64, col 0\)"):
        s.outside_intact(S.SENTINEL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
def test_unwritten_logical_element_is_found(dtype):
    s = _written(dtype)
    s.bits[s.offset + 11 * s.ld + 39] = S._signed(S.SENTINEL[dtype], s.nbits)
    with pytest.raises(AssertionError, match=r"never written.*\(row 11, col 39\)"):
        s.logical_has_no_sentinel(S.SENTINEL[dtype])
    assert s.outside_intact(S.SENTINEL[dtype])       # (the guards are fine: the two checks are independent)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hardware_nan_is_not_the_sentinel(dtype):
    """NaNs as arithmetic produces them (0/0, inf - inf, either sign, the conversion of an f32 NaN) in the logical region
    count as WRITTEN; and the sentinel and the input poison are NaNs themselves, with different bits"""
    s = _written(dtype)
    z = torch.zeros(4)
    inf = torch.full((1,), float("inf"))
    hw = torch.cat([z[:1] / z[:1], -(z[:1] / z[:1]), inf - inf, inf * 0, torch.tensor([float("nan")])]).to(dtype)
    s.view[2, :5] = hw
    assert bool(torch.isnan(s.view[2, :5]).all())
    assert s.logical_has_no_sentinel(S.SENTINEL[dtype])
    for pattern in (S.SENTINEL[dtype], S.QNAN[dtype]):
        t = torch.zeros(1, dtype=dtype)
        t.view(S._INT[t.element_size()]).fill_(S._signed(pattern, 8 * t.element_size()))
        assert bool(torch.isnan(t).all())
    assert S.SENTINEL[dtype] != S.QNAN[dtype]
    hw_bits = {int(v) & ((1 << s.nbits) - 1) for v in hw.view(S._INT[hw.element_size()])}
    assert S.SENTINEL[dtype] not in hw_bits


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_slabs_of_one_case_have_identical_offsets(dtype):
    a, b = S.Slab.matrix(ROWS, COLS, dtype, gap=GAP, batch=2), S.Slab.matrix(ROWS, COLS, dtype, gap=GAP, batch=2)
    assert a.layout() == b.layout() and torch.equal(a.mask, b.mask)
    assert a.view.data_ptr() - a.buf.data_ptr() == b.view.data_ptr() - b.buf.data_ptr() == a.byte_offset
    assert a.byte_offset % 16 == 0                   # (ld % 8 == 0 in 16-bit elements: rows start on 16-byte chunks)
    i, j = (S.Slab.image(3, 3, 9, 21, torch.float32) for _ in range(2))
    assert i.layout() == j.layout()


def test_image_slab_is_a_strided_window():
    s = S.Slab.image(2, 3, 9, 21, torch.float32)
    v = s.view
    assert v.shape == (2, 3, 9, 21) and v.stride() == (4 * 11 * 24, 11 * 24, 24, 1)
    s.fill_all(S.QNAN[torch.float32])
    s.fill_logical(torch.ones(2, 3, 9, 21))
    assert float(v.sum()) == 2 * 3 * 9 * 21 and int(torch.isnan(s.buf).sum()) == s.buf.numel() - v.numel()
    s.buf[s.offset + 21] = 0.0                        # one pixel to the right of the first row of the window
    with pytest.raises(AssertionError, match=r"\(row 0, col 21\)"):
        s.outside_intact(S.QNAN[torch.float32])


def test_int64_slot_sums_guards_and_inputs():
    s = S.Slab.matrix(2 * 8 * 32, 4, torch.int64, gap=0)      # gn_sums [Bn][slots][G][4]: contiguous, guards front and back
    s.fill_all(S.INT_PATTERN)
    s.fill_logical(0)
    assert int(s.view.abs().sum()) == 0 and s.outside_intact(S.INT_PATTERN)
    s.buf[s.offset + s.view.numel()] += 1                     # an atomic add one word past the end
    with pytest.raises(AssertionError, match=r"\(row 512, col 0\)"):
        s.outside_intact(S.INT_PATTERN)
    x = S.Slab.matrix(ROWS, COLS, torch.float16, gap=GAP)
    x.fill_outside(S.QNAN[torch.float16])
    snap = x.snapshot()
    x.view[3, 4] = 1.0
    with pytest.raises(AssertionError, match=r"input was written.*\(row 3, col 4\)"):
        x.unchanged(snap)
    a = x.logical_bits()
    x.view[3, 4] = 2.0
    with pytest.raises(AssertionError, match=r"\(row 3, col 4\)"):
        S.first_difference(a, x.logical_bits(), x, "run B vs run A")
