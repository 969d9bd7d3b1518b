"""The geometry table of the convolution edge tests, and the data they run on.  Nothing here touches a GPU or a kernel.

A ROW is (family, Bn, H, W): the forward convolution's input.  `conv_dict(row, mode, Ci)` derives the descriptor of the
implicit GEMM exactly as tests/test_kernels_gpu.py (test_conv3x3_fwd, test_conv3x3_dgrad) builds its own: mode 1 gathers
from the (H, W) input to the (Ho, Wo) of torch's formula for the family; mode 2 (the input gradient) gathers from that
(Ho, Wo) grid back to (H, W).  What each row reaches ("Convolutions at their edges"):

    s1      (3,1,1) (3,1,7) (3,5,1)          every pixel is a border pixel; a one-row and a one-column image
            (37,3,3)                         M = 333: one 256-row tile spans 28 images, every image seam inside a tile
            (2,9,13) (2,9,12)                odd sizes; the 12 x 9 level of the 768 x 576 evaluation
            (1,16,24) (1,24,16)              tile 18 must fall back to 17: one dimension is off its 16-pixel grid
            (2,16,16) (1,16,48) (1,48,16)    tile 18 on its grid: one tile, a row of tiles, a column of tiles
    s2p1    (3,1,1) (3,2,2) (2,3,3) (2,9,13) (2,18,24)    odd stride-2 inputs; outputs 1x1, 1x1, 2x2, 5x7, 9x12
    s2vae   (3,2,2) (3,3,3) (2,9,13)         pad (0,1,0,1): outputs 1x1, 1x1, 4x6; the last row / column only partly read
    ups     (3,1,1) (3,1,7) (3,5,1) (2,9,12) fused 2x upsample from odd low-resolution grids (mode 1 only)
    valid   (3,3,3) (2,9,13)                 stride 1, pad 0, Ho = H - 2: Hi != Ho with stride 1 (mode 1 only)
    padtl   (2,9,13) -> 9 x 11               pad_t = 1, pad_l = 0: the two pads are separate fields (mode 1 only)

Wide placement (`place_in`, `place_out`): the NHWC input is a column slice of a wider buffer (ldx = Ci + 8 or Ci + 72),
the output a column slice too (ldc = N + 8, one more row below); the neighbours hold the finite value 1024, which a wrong
stride would read and a stray store would replace.

`normal_data`: signed values, Gaussian in sign and mantissa, 2^-8 <= |x| <= 8 — a normal number in fp16 and in bf16 (and
so is 4 x it), so a bit-exact test does not depend on how the matrix units treat subnormal inputs.

`selector_weights`: output channel n = tap * Ci + ci has ONE non-zero weight, (1, 2, 4)[n % 3] at (ci, dy, dx): every
output element is one input element times a power of two, or zero padding — exact in the f32 accumulation, in split-K
partials and in the 16-bit store, so the launch's result must EQUAL the reference.

The mutants (`mutate`) state, on the explicit im2col matrix, the addressing errors the tests must be able to see."""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import torch

from helpers import gemm_ref as G

Row = namedtuple("Row", "family Bn H W")
PAD = 1024.0  # the value around every wide placement: finite, a normal number in both formats

_S1 = [(3, 1, 1), (3, 1, 7), (3, 5, 1), (37, 3, 3), (2, 9, 13), (2, 9, 12), (1, 16, 24), (1, 24, 16), (2, 16, 16), (1, 16, 48),
       (1, 48, 16)]
ROWS = ([Row("s1", *g) for g in _S1]
        + [Row("s2p1", *g) for g in [(3, 1, 1), (3, 2, 2), (2, 3, 3), (2, 9, 13), (2, 18, 24)]]
        + [Row("s2vae", *g) for g in [(3, 2, 2), (3, 3, 3), (2, 9, 13)]]
        + [Row("ups", *g) for g in [(3, 1, 1), (3, 1, 7), (3, 5, 1), (2, 9, 12)]]
        + [Row("valid", *g) for g in [(3, 3, 3), (2, 9, 13)]]
        + [Row("padtl", 2, 9, 13)])
MODES = {"s1": (1, 2), "s2p1": (1, 2), "s2vae": (1, 2), "ups": (1,), "valid": (1,), "padtl": (1,)}
CASES = [(r, m) for r in ROWS for m in MODES[r.family]]            # every (row, mode) of the table
GN_ROW = Row("s1", 11, 5, 13)  # gn_hw = 65, M = 715: a 256-row tile spans five images, the capacity of the fused GroupNorm sums
PARITY_CASES = CASES + [(GN_ROW, 1), (GN_ROW, 2)]                  # the Gaussian tests run the table and that row
EPILOGUE_ROWS = [Row("s1", 2, 9, 13), Row("s1", 2, 16, 16), GN_ROW]  # the rows that also run the engines' resnet epilogues


def row_id(row):
    return f"{row.family}-{row.Bn}x{row.H}x{row.W}"


def case_id(case):
    return f"{row_id(case[0])}-mode{case[1]}"


def family_geometry(row):
    """-> (Ho, Wo, stride, pad_t, pad_l, ups) of the forward convolution; Ho, Wo by torch's conv2d formula"""
    H, W = row.H, row.W
    if row.family == "s1":
        return H, W, 1, 1, 1, 0
    if row.family == "s2p1":       # F.conv2d(x, w, stride=2, padding=1)
        return (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1, 2, 1, 1, 0
    if row.family == "s2vae":      # F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2): AutoencoderKL's Downsample2D
        return (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1, 2, 0, 0, 0
    if row.family == "ups":        # F.conv2d(F.interpolate(x, scale_factor=2), w, padding=1)
        return 2 * H, 2 * W, 1, 1, 1, 1
    if row.family == "valid":      # F.conv2d(x, w)
        return H - 2, W - 2, 1, 0, 0, 0
    if row.family == "padtl":      # F.conv2d(F.pad(x, (0, 0, 1, 1)), w): rows padded, columns not
        return H, W - 2, 1, 1, 0, 0
    raise ValueError(row.family)


def torch_forward(row, x, w):
    """the family's forward convolution in torch's own operators (x NCHW, w [Co][Ci][3][3])"""
    import torch.nn.functional as F
    f = row.family
    if f == "s1":
        return F.conv2d(x, w, None, padding=1)
    if f == "s2p1":
        return F.conv2d(x, w, None, stride=2, padding=1)
    if f == "s2vae":
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, None, stride=2, padding=0)
    if f == "ups":
        return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, None, padding=1)
    if f == "valid":
        return F.conv2d(x, w, None)
    if f == "padtl":
        return F.conv2d(F.pad(x, (0, 0, 1, 1)), w, None)
    raise ValueError(f)


def conv_dict(row, mode, Ci, korder=0, ldx=None):
    """the `conv` dict of ops.gemm for the row: mode 1 the forward gather (Ci input channels), mode 2 the transposed gather
    of the input gradient (Ci = the channels of dy)"""
    Ho, Wo, stride, pt, pl, ups = family_geometry(row)
    assert mode in MODES[row.family]
    if mode == 1:
        d = dict(mode=1, Hi=row.H, Wi=row.W, Ci=Ci, Ho=Ho, Wo=Wo, stride=stride, pad_t=pt, pad_l=pl, ups=ups)
    else:
        d = dict(mode=2, Hi=Ho, Wi=Wo, Ci=Ci, Ho=row.H, Wo=row.W, stride=stride, pad_t=pt, pad_l=pl, ups=0)
    d.update(ldx=Ci if ldx is None else ldx, korder=korder)
    return d


def rows_M(row, mode):
    c = conv_dict(row, mode, 64)
    return row.Bn * c["Ho"] * c["Wo"]


def in_pixels(row, mode):
    c = conv_dict(row, mode, 64)
    return row.Bn * c["Hi"] * c["Wi"]


def halo_accepts(row, mode, korder):
    """where tile 18 runs as itself (include/vneti.h, tile_hint): stride 1, pad 1, chunk-major K, both dims on the 16 grid"""
    return row.family == "s1" and korder == 1 and row.H % 16 == 0 and row.W % 16 == 0


# ---------------------------------------------------------------------------------------------- placement
def place_in(rows, ldx):
    """[pixels][Ci] -> the same values as a column slice of a [pixels][ldx] buffer of PAD (16-byte aligned offset)"""
    npix, Ci = rows.shape
    assert ldx >= Ci and ldx % 8 == 0
    off = ((ldx - Ci) // 2) // 8 * 8
    buf = torch.full((npix, ldx), PAD, dtype=rows.dtype, device=rows.device)
    view = buf[:, off:off + Ci]
    view.copy_(rows)
    return view


def place_out(M, N, dtype, device="cpu"):
    """-> (buffer [M + 1][N + 8] of PAD, the [M][N] view the launch writes); ldc = N + 8 (N % 8 == 0)"""
    buf = torch.full((M + 1, N + 8), PAD, dtype=dtype, device=device)
    return buf, buf[:M, :N]


def untouched(buf, M, N):
    """the neighbours of the output still hold PAD"""
    return bool((buf[:M, N:] == PAD).all()) and bool((buf[M:] == PAD).all())


# ---------------------------------------------------------------------------------------------- data
def normal_data(shape, seed):
    """float64, signed, Gaussian in sign and mantissa, 2^-8 <= |x| <= 8: a normal number in fp16 and bf16 after rounding"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g, dtype=torch.float64)
    sign = torch.where(x < 0, -1.0, 1.0).double()
    return sign * x.abs().clamp(2.0 ** -8, 8.0)


def gauss(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


SCALES = (1.0, 2.0, 4.0)


@functools.lru_cache(maxsize=None)
def selector_weights(Ci, mode):
    """the torch-layout weight [Co][Ci][3][3] of the selector: mode 1 [9 * Ci][Ci][3][3] with w[n][ci][dy][dx] =
    SCALES[n % 3] for n = (dy * 3 + dx) * Ci + ci; mode 2 its mirror image [Ci][9 * Ci][3][3] (w[c][n][dy][dx], n = tap *
    Ci + c: packing.conv3x3_dgrad turns it into the [9 * Ci][9 * Ci] matrix of the transposed gather)"""
    n = torch.arange(9 * Ci)
    tap, c = n // Ci, n % Ci
    val = torch.tensor(SCALES, dtype=torch.float64)[n % 3]
    if mode == 1:
        w = torch.zeros(9 * Ci, Ci, 3, 3, dtype=torch.float64)
        w[n, c, tap // 3, tap % 3] = val
    else:
        w = torch.zeros(Ci, 9 * Ci, 3, 3, dtype=torch.float64)
        w[c, n, tap // 3, tap % 3] = val
    return w


def pack(w, mode, korder):
    from view_neti_amd import packing
    return (packing.conv3x3_fwd if mode == 1 else packing.conv3x3_dgrad)(w, cm=bool(korder))


@functools.lru_cache(maxsize=None)
def selector_packed(Ci, mode, korder):
    """float64 [9 * Ci][9 * Ci], packed with packing.conv3x3_fwd / conv3x3_dgrad for the K order"""
    return pack(selector_weights(Ci, mode), mode, korder)


def selector_plane(x_nhwc, conv, tap, ci):
    """what column tap * Ci + ci of a selector launch must hold, before its scale: the input plane `ci` shifted by the tap —
    written with slices of a zero-padded (mode 1) or zero-stuffed (mode 2) image, not with the reference's index gather.
    x_nhwc: [Bn][Hi][Wi][Ci] -> [Bn][Ho][Wo]"""
    dy, dx = tap // 3, tap % 3
    Ho, Wo, s, pt, pl = conv["Ho"], conv["Wo"], conv["stride"], conv["pad_t"], conv["pad_l"]
    p = x_nhwc[..., ci].double()
    Bn = p.shape[0]
    if conv["mode"] == 1:
        if conv.get("ups"):
            p = p.repeat_interleave(2, 1).repeat_interleave(2, 2)
        Hs, Ws = p.shape[1], p.shape[2]
        need_h, need_w = (Ho - 1) * s + 3, (Wo - 1) * s + 3
        z = torch.zeros(Bn, max(need_h, Hs + pt), max(need_w, Ws + pl), dtype=torch.float64)
        z[:, pt:pt + Hs, pl:pl + Ws] = p
        return z[:, dy:dy + (Ho - 1) * s + 1:s, dx:dx + (Wo - 1) * s + 1:s]
    # mode 2: out(oy, ox) = in((oy + pt - dy) / s, (ox + pl - dx) / s): the input zero-stuffed onto the stride grid, offset 2
    Hi, Wi = p.shape[1], p.shape[2]
    z = torch.zeros(Bn, max(Ho + pt + 2, (Hi - 1) * s + 3), max(Wo + pl + 2, (Wi - 1) * s + 3), dtype=torch.float64)
    z[:, 2:2 + (Hi - 1) * s + 1:s, 2:2 + (Wi - 1) * s + 1:s] = p
    y0, x0 = pt - dy + 2, pl - dx + 2
    return z[:, y0:y0 + Ho, x0:x0 + Wo]


# ---------------------------------------------------------------------------------------------- mutants
def _tap_source(conv, oy, ox, dy, dx):
    """-> (in range?, iy, ix) of one tap of one output pixel, (iy, ix) by floor division even where the tap is masked: the
    address a kernel that forgot the mask would form"""
    s, pt, pl = conv["stride"], conv["pad_t"], conv["pad_l"]
    if conv["mode"] == 1:
        iy, ix = oy * s + dy - pt, ox * s + dx - pl
        if conv.get("ups"):
            ok = 0 <= iy < 2 * conv["Hi"] and 0 <= ix < 2 * conv["Wi"]
            return ok, iy >> 1, ix >> 1
        return (0 <= iy < conv["Hi"] and 0 <= ix < conv["Wi"]), iy, ix
    ny, nx = oy + pt - dy, ox + pl - dx
    iy, ix = ny // s, nx // s
    ok = ny >= 0 and nx >= 0 and ny % s == 0 and nx % s == 0 and iy < conv["Hi"] and ix < conv["Wi"]
    return ok, iy, ix


def _kcols(conv, tap):
    """the columns of the im2col matrix that hold `tap`, in channel order"""
    Ci = conv["Ci"]
    c = torch.arange(Ci)
    if conv.get("korder"):
        return (c // 64) * (9 * 64) + tap * 64 + c % 64
    return tap * Ci + c


def mutate(kind, col, x_rows, conv, Bn):
    """-> a copy of the explicit im2col matrix `col` [M][9 * Ci] with one addressing error (None for "unwritten": that
    mutant acts on the output).  x_rows: the [pixels][Ci] float64 input rows.
      wrap:  one masked tap of one border pixel of the LAST image takes the pixel at the flat address the unmasked gather
             forms (the previous row's last pixel, the previous image's last row) instead of zero.  A valid convolution
             masks nothing: there the tap of the last image's last pixel reads one pixel further along in memory.
      seam:  the first output row of the last image takes, for the tap (0, 1), the LAST row of the image before it.
      swap:  two channels of one tap of one pixel change places."""
    Hi, Wi, Ho, Wo = conv["Hi"], conv["Wi"], conv["Ho"], conv["Wo"]
    npix = Bn * Hi * Wi
    col = col.clone()
    b = Bn - 1
    if kind == "wrap":
        for oy in range(Ho):
            for ox in range(Wo):
                for tap in range(9):
                    ok, iy, ix = _tap_source(conv, oy, ox, tap // 3, tap % 3)
                    flat = (b * Hi + iy) * Wi + ix
                    if not ok and 0 <= flat < npix:
                        col[(b * Ho + oy) * Wo + ox, _kcols(conv, tap)] = x_rows[flat]
                        return col
        m = (b * Ho + Ho - 1) * Wo + Wo - 1  # nothing is masked (valid): the centre tap of the last pixel, one pixel on
        ok, iy, ix = _tap_source(conv, Ho - 1, Wo - 1, 1, 1)
        col[m, _kcols(conv, 4)] = x_rows[(b * Hi + iy) * Wi + ix + 1]
        return col
    if kind == "seam":
        assert b > 0
        for ox in range(Wo):
            _, _, ix = _tap_source(conv, 0, ox, 0, 1)
            ix = min(max(ix, 0), Wi - 1)
            col[(b * Ho) * Wo + ox, _kcols(conv, 1)] = x_rows[((b - 1) * Hi + Hi - 1) * Wi + ix]
        return col
    if kind == "swap":
        # the centre-most tap that is in range at the last image's first pixel, and two channels whose values differ
        for tap in (4, 5, 7, 8, 0, 1, 2, 3, 6):
            ok, iy, ix = _tap_source(conv, 0, 0, tap // 3, tap % 3)
            if ok:
                break
        assert ok
        k = _kcols(conv, tap)
        m = (b * Ho) * Wo
        v = col[m, k]
        j = int((v != v[0]).nonzero()[0])
        col[m, k[0]], col[m, k[j]] = v[j].clone(), v[0].clone()
        return col
    raise ValueError(kind)


def im2col_of(x_rows, conv, M):
    return G.im2col(x_rows.contiguous(), dict(conv, ldx=conv["Ci"]), M)


# ---------------------------------------------------------------------------------------------- the parity launches
def parity_operands(case, Ci, Co, korder, dtype, epi, seed=0):
    """CPU operands of one Gaussian launch of the case, rounded to `dtype` (the 16-bit format under test; float64 keeps them
    exact).  epi: "bias+resid", "resnet" (bias + rowadd per image + resid + GroupNorm sums: Co / 8 groups, 4 slots) or
    "gate" (the SiLU-gradient gate of the GroupNorm-SiLU backward).  -> (A rows [pixels][Ci], packed B, conv, M, kwargs);
    the gn_sums buffer is the caller's (it lives on the device)."""
    row, mode = case
    conv = conv_dict(row, mode, Ci, korder)
    M, npix = rows_M(row, mode), in_pixels(row, mode)
    a = gauss((npix, Ci), seed + 1).to(dtype)
    if mode == 1:
        w = gauss((Co, Ci, 3, 3), seed + 2, 1 / math.sqrt(9 * Ci)).to(dtype)
    else:  # dy has Ci channels, dx has Co: the forward weight is [Ci][Co][3][3]
        w = gauss((Ci, Co, 3, 3), seed + 2, 1 / math.sqrt(9 * Ci)).to(dtype)
    Bp = pack(w, mode, korder)
    kw = {}
    if epi in ("bias+resid", "resnet"):
        kw["bias"] = gauss((Co,), seed + 3).to(torch.float64 if dtype == torch.float64 else torch.float32)
        kw["resid"] = gauss((M, Co), seed + 4).to(dtype)
    if epi == "resnet":
        kw["rowadd"] = gauss((row.Bn, Co), seed + 5).to(dtype)
        kw["rows_per_group"] = conv["Ho"] * conv["Wo"]
    if epi == "gate":
        kw["gate"] = gauss((M, Co), seed + 6).to(dtype)
        kw["gate_act"] = 1
    return a, Bp, conv, M, kw
