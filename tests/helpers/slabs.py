"""Guarded operand slabs for the kernel memory-contract tests (tests/test_kernel_contracts_gpu.py).

A Slab is ONE flat buffer that holds a logical operand of the C ABI as a strided view — `[rows, cols]` with row stride
`ld > cols`, optionally batched, or an arbitrary `[B, C, H, W]` view — surrounded by guard elements: at least FRONT_ROWS rows
in front of the first logical row, at least BACK_ROWS rows behind the last one (and behind every batch matrix), and the
`ld - cols` gap after every row.  It remembers which elements are logical (a boolean mask) so that a test can

  - poison everything a kernel has no business reading (`fill_outside`) and see whether the result changes,
  - prefill everything a kernel has to write with a sentinel (`fill_all`) and see whether an element was left out
    (`logical_has_no_sentinel`) or a store strayed (`outside_intact`),
  - compare two runs bit for bit (`logical_bits`, `snapshot` / `unchanged`).

Patterns are RAW BITS (Python ints), written and compared through the integer view of the buffer (`int16` / `int32` /
`int64` by element size): NaN == NaN is false and -0.0 == 0.0 is true for floats, neither is wanted here.  The layout is a
pure function of the constructor arguments: two slabs of one case have identical element offsets, so alignment never
differs between runs."""
import torch

FRONT_ROWS = 64    # guard rows in front of the logical rows
BACK_ROWS = 256    # guard rows behind them: the tallest GEMM tile's BM

_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

# quiet NaNs of the operand formats: what a poisoned INPUT surrounding holds
QNAN = {torch.float16: 0x7E00, torch.bfloat16: 0x7FC0, torch.float32: 0x7FC00000}
# NaNs whose payload differs from the canonical NaN the hardware produces (0x7E00 / 0x7FC0 / 0x7FC00000, either sign): what
# an OUTPUT holds before the launch, so that "the kernel wrote NaN here" and "the kernel never wrote here" differ in bits
SENTINEL = {torch.float16: 0x7E5A, torch.bfloat16: 0x7FDA, torch.float32: 0x7FC5A5A5}
# guards of the 64-bit fixed-point GroupNorm slot sums (integers: there is no NaN to use)
INT_PATTERN = 0x5A5AA5A55A5AA5A5


def _signed(pattern, bits):
    """the Python int `pattern` (raw bits) as the signed integer of that width torch wants"""
    pattern &= (1 << bits) - 1
    return pattern - (1 << bits) if pattern >> (bits - 1) else pattern


class Slab:
    def __init__(self, numel, shape, strides, offset, dtype, device="cpu"):
        """a flat `numel`-element buffer whose logical operand is the view (shape, strides, offset), all in elements;
        use `Slab.matrix` / `Slab.image` unless the layout is special"""
        self.dtype, self.shape, self.strides, self.offset = dtype, tuple(shape), tuple(strides), int(offset)
        last = self.offset + sum((n - 1) * s for n, s in zip(self.shape, self.strides))
        assert 0 <= self.offset and last < numel, "the logical view leaves the slab"
        self.buf = torch.zeros(numel, dtype=dtype, device=device)
        self.bits = self.buf.view(_INT[self.buf.element_size()])
        self.nbits = 8 * self.buf.element_size()
        self.mask = torch.zeros(numel, dtype=torch.bool, device=device)
        self.mask.as_strided(self.shape, self.strides, self.offset).fill_(True)
        assert int(self.mask.sum()) == self.view.numel(), "the logical view overlaps itself"
        self.ld = self.strides[-2] if len(self.strides) >= 2 else self.shape[-1]   # what (row, col) reports are relative to

    # ---------------------------------------------------------------------------------------- layouts
    @classmethod
    def matrix(cls, rows, cols, dtype, gap=8, batch=1, device="cpu", front=FRONT_ROWS, back=BACK_ROWS):
        """`[rows, cols]` (batch == 1) or `[batch, rows, cols]` with row stride ld = cols + gap; `gap` is a multiple of 8 (the
        ABI's ld % 8 rule holds when cols % 8 == 0), >= 8 for an operand that has an ld, 0 for one the ABI takes contiguous
        (vectors, lse, slot sums: guards in front and behind only).  Every batch matrix is followed by `back` guard rows of
        its own, so the space between two batches is guard."""
        assert gap % 8 == 0 and gap >= 0 and front >= FRONT_ROWS and back >= BACK_ROWS
        ld = cols + gap
        bstride = (rows + back) * ld
        numel = front * ld + batch * bstride
        if batch == 1:
            return cls(numel, (rows, cols), (ld, 1), front * ld, dtype, device)
        return cls(numel, (batch, rows, cols), (bstride, ld, 1), front * ld, dtype, device)

    @classmethod
    def image(cls, Bn, Cc, H, W, dtype, device="cpu", pad_c=1, pad_y=(1, 1), pad_x=(2, 1)):
        """a `[Bn, Cc, H, W]` window of a planar `[Bn, Cc + pad_c, H + pad_y, W + pad_x]` image (channel, row and batch
        strides all differ from the dense ones), as vneti_conv3x3_in / vneti_im2col3x3_small take it, with FRONT_ROWS /
        BACK_ROWS image rows of guard around the whole"""
        Wp, Hp, Cp = W + sum(pad_x), H + sum(pad_y), Cc + pad_c
        strides = (Cp * Hp * Wp, Hp * Wp, Wp, 1)
        offset = FRONT_ROWS * Wp + pad_y[0] * Wp + pad_x[0]
        numel = (FRONT_ROWS + BACK_ROWS) * Wp + Bn * strides[0]
        return cls(numel, (Bn, Cc, H, W), strides, offset, dtype, device)

    # ---------------------------------------------------------------------------------------- access
    @property
    def view(self):
        """the logical operand: what is handed to the kernel"""
        return self.buf.as_strided(self.shape, self.strides, self.offset)

    @property
    def byte_offset(self):
        return self.offset * self.buf.element_size()

    def layout(self):
        """everything that fixes the operand's address relative to the buffer (equal for two slabs of one case)"""
        return (self.buf.numel(), self.shape, self.strides, self.byte_offset)

    # ---------------------------------------------------------------------------------------- filling
    def fill_all(self, pattern):
        self.bits.fill_(_signed(pattern, self.nbits))

    def fill_outside(self, pattern):
        self.bits.masked_fill_(~self.mask, _signed(pattern, self.nbits))

    def fill_logical(self, values):
        """`values`: a tensor of the logical shape (copied, converted to the slab's dtype) or a raw bit pattern"""
        if isinstance(values, torch.Tensor):
            self.view.copy_(values.reshape(self.shape))
        else:
            self.bits.masked_fill_(self.mask, _signed(values, self.nbits))

    # ---------------------------------------------------------------------------------------- checks
    def _where(self, flat_index):
        rel = int(flat_index) - self.offset
        return rel // self.ld, rel % self.ld

    def outside_intact(self, pattern, what="slab"):
        """every element that is not logical still holds `pattern`, bit for bit; raises naming the first offending
        (row, col) relative to the view (row < 0: the front guard; col >= cols: the ld gap) otherwise"""
        bad = ((self.bits != _signed(pattern, self.nbits)) & ~self.mask).nonzero()
        if bad.numel():
            i = int(bad[0])
            row, col = self._where(i)
            raise AssertionError(f"{what}: stray store outside the logical extents: {bad.shape[0]} element(s), the first at "
                                 f"(row {row}, col {col}) of the view (flat element {i}), bits "
                                 f"{int(self.bits[i]) & ((1 << self.nbits) - 1):#x}, guard pattern {pattern:#x}")
        return True

    def logical_has_no_sentinel(self, pattern, what="slab"):
        """no logical element still holds the prefill `pattern`: the kernel wrote every element it owns"""
        bad = ((self.bits == _signed(pattern, self.nbits)) & self.mask).nonzero()
        if bad.numel():
            i = int(bad[0])
            row, col = self._where(i)
            raise AssertionError(f"{what}: {bad.shape[0]} logical element(s) never written (still the sentinel {pattern:#x}), "
                                 f"the first at (row {row}, col {col}) of the view")
        return True

    def logical_bits(self):
        """the logical elements' raw bits in memory order (1-D integer tensor, a copy): `torch.equal` of two of them is
        bit-for-bit equality of two runs"""
        return self.bits[self.mask].clone()

    def snapshot(self):
        """the whole slab's raw bits, guards included"""
        return self.bits.clone()

    def unchanged(self, snap, what="slab"):
        """the whole slab is bit-identical to `snap`: the kernel wrote nothing into it"""
        bad = (self.bits != snap).nonzero()
        if bad.numel():
            row, col = self._where(int(bad[0]))
            raise AssertionError(f"{what}: an input was written: {bad.shape[0]} element(s) changed, the first at "
                                 f"(row {row}, col {col}) of the view")
        return True


def first_difference(a_bits, b_bits, slab, what):
    """raises naming the first logical element (row, col of the view) at which two `logical_bits()` of `slab` differ"""
    if torch.equal(a_bits, b_bits):
        return True
    k = int((a_bits != b_bits).nonzero()[0])
    flat = int(slab.mask.nonzero()[k])
    row, col = slab._where(flat)
    n = int((a_bits != b_bits).sum())
    m = (1 << slab.nbits) - 1
    raise AssertionError(f"{what}: {n} logical element(s) differ, the first at (row {row}, col {col}) of the view: "
                         f"{int(a_bits[k]) & m:#x} vs {int(b_bits[k]) & m:#x}")
