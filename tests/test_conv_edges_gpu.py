"""The implicit-GEMM convolutions (csrc/gemm_conv.hip, csrc/gemm8.hip) and the two small kernels beside them at the image
geometries where an address or a mask goes wrong: every row of tests/helpers/conv_cases.py (its docstring says what each
reaches) against the float64 reference of the launch (tests/helpers/gemm_ref.py, pinned by tests/test_conv_edges_cpu.py).

  test_edges_conv_select*   a bit-exact address probe: selector weights on `normal_data`, so that every output element is
                            one input element times 1, 2 or 4, or zero padding; the result must EQUAL the reference for every
                            tile hint and split-K form.  A wrong channel of one tap of one pixel, which sits inside any
                            tolerance, fails it.
  test_edges_conv_parity*   Gaussian values through the engines' epilogues (bias + residual; the resnet epilogue with the
                            fused GroupNorm sums at their five-images-per-tile capacity; the SiLU-gradient gate of the input
                            gradient) at the bars the existing convolution tests use.
  test_edges_conv_small*    vneti_im2col3x3_small (bit for bit) and vneti_conv3x3_in at the same edges.

No bar is new: forward and transposed gather t16(2e-3) (test_conv3x3_fwd, test_conv3x3_dgrad); where tile 18 runs as itself
t16(4e-3) forward, t16(3e-3) with split-K and on the transposed gather (test_conv3x3_halo_tile, _split_k,
test_conv3x3_dgrad_halo_tile); the decoded GroupNorm sums 1e-4 against the float64 sums of the stored values.  The file is
precision-generic (tests/test_kernels_gpu.py's docstring); tests/test_kernels_bf16_gpu.py re-runs it against the bf16 build."""
from functools import partial

import pytest
import torch

from helpers import conv_cases as CC
from helpers import gemm_ref as G
from helpers.checks import DEV, DT, check, t16
from helpers.checks import ops as _ops

pytestmark = pytest.mark.gpu

HINTS = [0, 1, 3, 4, 5, 6, 7, 8, 9, 13, 15, 16, 17, 18, 101, 103]  # those of test_conv3x3_fwd
SPLITS = [1, 3, 0]                                                  # 3 and 0 (the heuristic) with a workspace
KORDERS = pytest.mark.parametrize("korder", [0, 1], ids=["tap-major", "chunk-major"])
ALL_CASES = pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)

_refs = {}  # references of the module, computed once per key and only read afterwards


def _cached(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def _workspace(M, N):
    return torch.empty(4 * M * N, dtype=torch.float32, device=DEV)  # (the heuristic lowers its split to what fits)


def _launch(a_dev, b_dev, conv, M, N, hint, split, ws, zero, **kw):
    """one launch into a fresh PAD-surrounded output -> the [M][N] result; asserts the surroundings"""
    buf, out = CC.place_out(M, N, DT, DEV)
    if zero:
        out.zero_()
    _ops().gemm(a_dev, b_dev, out, conv=conv, M=M, tile_hint=hint, split_k=split, workspace=ws if split != 1 else None, **kw)
    torch.cuda.synchronize()
    assert CC.untouched(buf, M, N), f"hint {hint} split {split}: the output's neighbouring columns / rows were written"
    return out


# ---------------------------------------------------------------------------------------------- the address probe
@KORDERS
@pytest.mark.parametrize("Ci", [64, 128])
@ALL_CASES
def test_edges_conv_select(case, Ci, korder):
    row, mode = case
    ldx = Ci + (72 if korder else 8)
    conv = CC.conv_dict(row, mode, Ci, korder, ldx)
    M, N = CC.rows_M(row, mode), 9 * Ci
    x = CC.normal_data((CC.in_pixels(row, mode), Ci), 7).to(DT)
    Bp = CC.selector_packed(Ci, mode, korder).to(DT)

    def reference():
        f = partial(_ops().gemm, CC.place_in(x, ldx), Bp, torch.zeros(M, N, dtype=DT), conv=conv, M=M)
        return G.reference(f).out.to(DT)

    ref = _cached(("select", case, Ci, korder), reference).to(DEV).float()
    a_dev, b_dev, ws = CC.place_in(x.to(DEV), ldx), Bp.to(DEV), _workspace(M, N)
    ran, wrong, outs = [], [], {}
    for hint in HINTS:
        for split in SPLITS:
            out = _launch(a_dev, b_dev, conv, M, N, hint, split, ws, zero=False)
            ran.append((hint, split))
            if not torch.equal(out.float(), ref):  # (as values: -0 equals +0)
                bad = (out.float() != ref).nonzero()
                wrong.append((hint, split, int(bad.shape[0]), [int(i) for i in bad[0]]))
            if hint in (17, 18) and split == 1:
                outs[hint] = out
    print(f"[select {CC.case_id(case)} Ci{Ci} korder{korder}] {len(ran)} (hint, split) pairs: {ran}")
    assert len(ran) == len(HINTS) * len(SPLITS)
    assert not wrong, f"(hint, split, wrong elements, first [m, n]): {wrong}"
    if CC.halo_accepts(row, mode, korder):
        assert torch.equal(outs[17].view(torch.int16), outs[18].view(torch.int16)), "tile 18 differs from tile 17 in its bits"


# ---------------------------------------------------------------------------------------------- parity
P_HINTS = [3, 7, 17, 18]
P_CI = 128


def _bar(case, korder, hint, split):
    row, mode = case
    if hint == 18 and CC.halo_accepts(row, mode, korder):
        return t16(4e-3) if (mode == 1 and split == 1) else t16(3e-3)
    return t16(2e-3)


def _parity_case(case, Co, korder, epi):
    """the operands on the device and the float64 reference of the launch (cached: the reference is the same for every
    hint and split)"""
    def make():
        a, Bp, conv, M, kw = CC.parity_operands(case, P_CI, Co, korder, DT, epi)
        f = partial(_ops().gemm, a, Bp, torch.zeros(M, Co, dtype=DT), conv=conv, M=M, **kw)
        return a, Bp, conv, M, kw, G.reference(f)
    return _cached(("parity", case, Co, korder, epi), make)


def _dev(kw):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}


@KORDERS
@pytest.mark.parametrize("case", CC.PARITY_CASES, ids=CC.case_id)
def test_edges_conv_parity_bias_resid(case, korder):
    row, mode = case
    Co = 72  # (an N tail in every tile)
    a, Bp, conv, M, kw, ref = _parity_case(case, Co, korder, "bias+resid")
    a_dev, b_dev, kwd, ws = a.to(DEV), Bp.to(DEV), _dev(kw), _workspace(M, Co)
    outs = {}
    for hint in P_HINTS:
        for split in (1, 3):
            out = _launch(a_dev, b_dev, conv, M, Co, hint, split, ws, zero=True, **kwd)
            check(f"parity {CC.case_id(case)} korder{korder} hint{hint} split{split}", out, ref.out, _bar(case, korder, hint, split))
            outs[hint, split] = out
    if CC.halo_accepts(row, mode, korder):
        assert torch.equal(outs[17, 1], outs[18, 1]), "tile 18 differs from tile 17"


@KORDERS
@pytest.mark.parametrize("Co", [128, 320])
@pytest.mark.parametrize("row", CC.EPILOGUE_ROWS, ids=CC.row_id)
def test_edges_conv_parity_resnet_epilogue(row, Co, korder):
    """bias + time-embedding row-add per image + residual + the fused GroupNorm sums of the stored values"""
    case = (row, 1)
    a, Bp, conv, M, kw, ref = _parity_case(case, Co, korder, "resnet")
    a_dev, b_dev, kwd = a.to(DEV), Bp.to(DEV), _dev(kw)
    hw, groups = row.H * row.W, Co // 8
    outs = {}
    for hint in P_HINTS:
        sums = torch.zeros(row.Bn, 4, groups, 4, dtype=torch.int64, device=DEV)
        out = _launch(a_dev, b_dev, conv, M, Co, hint, 1, None, zero=True, gn_sums=sums, gn_hw=hw, gn_groups=groups, gn_slots=4,
                      **kwd)
        name = f"parity resnet {CC.row_id(row)} Co{Co} korder{korder} hint{hint}"
        check(name, out, ref.out, _bar(case, korder, hint, 1))
        got = _ops().gn_sums_decode(sums.sum(1))
        stored = G.gn_sums(out.double().cpu(), hw, groups)
        check(name + " gn sum", got[..., 0].float(), stored[..., 0].float(), 1e-4)
        check(name + " gn sumsq", got[..., 1].float(), stored[..., 1].float(), 1e-4)
        outs[hint] = out
    if CC.halo_accepts(row, 1, korder):
        assert torch.equal(outs[17], outs[18]), "tile 18 differs from tile 17"


@KORDERS
@pytest.mark.parametrize("Co", [128, 320])
@pytest.mark.parametrize("row", CC.EPILOGUE_ROWS, ids=CC.row_id)
def test_edges_conv_parity_dgrad_silu_gate(row, Co, korder):
    """the input gradient with the activation-gradient gate of the GroupNorm-SiLU backward fused into its epilogue"""
    case = (row, 2)
    a, Bp, conv, M, kw, ref = _parity_case(case, Co, korder, "gate")
    a_dev, b_dev, kwd = a.to(DEV), Bp.to(DEV), _dev(kw)
    outs = {}
    for hint in P_HINTS:
        out = _launch(a_dev, b_dev, conv, M, Co, hint, 1, None, zero=True, **kwd)
        check(f"parity dgrad gate {CC.row_id(row)} Co{Co} korder{korder} hint{hint}", out, ref.out, _bar(case, korder, hint, 1))
        outs[hint] = out
    if CC.halo_accepts(row, 2, korder):
        assert torch.equal(outs[17], outs[18]), "tile 18 differs from tile 17"


# ---------------------------------------------------------------------------------------------- the small kernels
SMALL_ROWS = [r for r in CC.ROWS if r.family in ("s1", "s2p1", "s2vae") and r.Bn <= 3]


def _strided_image(Bn, Cc, H, W, f32, seed):
    """a view with differing batch, channel and row strides (as test_conv3x3_in_direct builds): CPU values, device view"""
    full = CC.gauss((Bn, Cc + 1, H + 2, W + 3), seed).to(torch.float32 if f32 else DT)
    return full[:, :Cc, 1:H + 1, 2:W + 2], full.to(DEV)[:, :Cc, 1:H + 1, 2:W + 2]


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "16bit"])
@pytest.mark.parametrize("row", SMALL_ROWS, ids=CC.row_id)
def test_edges_conv_small_im2col(row, f32):
    ops = _ops()
    Ho, Wo, stride, pt, pl, _ = CC.family_geometry(row)
    M = row.Bn * Ho * Wo
    for Cc in (1, 4, 7):
        x, xd = _strided_image(row.Bn, Cc, row.H, row.W, f32, 30 + Cc)
        col = torch.full((M + 1, 64), CC.PAD, dtype=DT, device=DEV)
        ops.im2col3x3_small(xd, col, row.Bn, Cc, row.H, row.W, Ho, Wo, stride, pt, pl, xd.stride())
        torch.cuda.synchronize()
        rows = x.permute(0, 2, 3, 1).reshape(-1, Cc).double().contiguous()
        ref = (G.im2col(rows, CC.conv_dict(row, 1, Cc), M) + 0.0).to(DT)  # (+ 0.0: the reference's masked taps are value * 0, so -0)
        assert torch.equal(col[:M, :9 * Cc].cpu().view(torch.int16), ref.view(torch.int16)), f"C = {Cc}: im2col is not bit-exact"
        assert bool((col[:M, 9 * Cc:] == 0).all()), f"C = {Cc}: the columns 9 * C .. 63 are not zero"
        assert bool((col[M:] == CC.PAD).all()), f"C = {Cc}: a row past the last was written"


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "16bit"])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1), (3, 3)])
def test_edges_conv_small_conv_in(H, W, f32):
    """(the kernel's GroupNorm sums need H * W % 256 == 0, so none of these images has them: that refusal is asserted)"""
    ops = _ops()
    from view_neti_amd import packing
    Bn, Co = 3, 128
    for Cc in (1, 3):
        x, xd = _strided_image(Bn, Cc, H, W, f32, 40 + Cc)
        w = CC.gauss((Co, Cc, 3, 3), 41, 0.3).to(DT)
        bias = CC.gauss((Co,), 42).float()
        M = Bn * H * W
        buf, out = CC.place_out(M, Co, DT, DEV)
        ops.conv3x3_in(xd, packing.conv_in_direct(w).to(DEV), bias.to(DEV), out, Bn, Cc, H, W, xd.stride())
        torch.cuda.synchronize()
        assert CC.untouched(buf, M, Co)
        rows = x.to(DT).permute(0, 2, 3, 1).reshape(-1, Cc).contiguous()
        conv = CC.conv_dict(CC.Row("s1", Bn, H, W), 1, Cc)
        want = G.im2col(rows, conv, M) @ packing.conv3x3_fwd(w, cm=False).double().t() + bias.double()
        check(f"conv_in {H}x{W} C{Cc} f32={f32}", out, want, t16(2e-3))
        sums = torch.zeros(Bn, 4, 16, 4, dtype=torch.int64, device=DEV)
        with pytest.raises(RuntimeError, match="gn_sums"):
            ops.conv3x3_in(xd, packing.conv_in_direct(w).to(DEV), bias.to(DEV), out, Bn, Cc, H, W, xd.stride(), gn_sums=sums,
                           gn_hw=H * W, gn_groups=16, gn_slots=4)
        assert int(sums.abs().sum()) == 0
