"""The pins under tests/test_conv_edges_gpu.py, WITHOUT any kernel (no GPU): for every row of the geometry table
(tests/helpers/conv_cases.py)

  * the float64 reference of the launch (tests/helpers/gemm_ref.py) is torch's own convolution, and for mode 2 autograd's
    input gradient, to <= 1e-12 — on wide placement, in both K orders (the bar of tests/test_gemm_ref_cpu.py, extended
    from its one 6 x 10 image);
  * the selector launch is what it claims: its float64 reference is exactly representable in fp16 and in bf16, and column
    tap * Ci + ci is the input plane ci shifted by the tap, times 1, 2 or 4;
  * the GPU file's two kinds of test see the addressing errors they are there for: a tap that wraps to the flat-memory
    neighbour, a first row that reads the previous image's last row and an unwritten last pixel fail `check` at the bf16
    bar on Gaussian data and fail equality on selector data; two swapped channels of one tap of one pixel fail the selector
    equality (whether `check` sees them on Gaussian data is printed, not asserted: on a third of the table's launches it
    does not, at either format's bar, which is why the bit-exact form exists);
  * the bars are not the failure: the float64 reference of every parity launch, rounded to the 16-bit format, passes the
    `check` the GPU file applies to the kernel."""
from functools import partial

import pytest
import torch

from helpers import conv_cases as CC
from helpers import gemm_ref as G
from helpers.checks import check, ops as _ops

TOL = 1e-12
FORMATS = [torch.float16, torch.bfloat16]
BAR = {torch.float16: 2e-3, torch.bfloat16: 8 * 2e-3}  # t16(2e-3) of either process: the tightest bar of the parity tests
KORDERS = pytest.mark.parametrize("korder", [0, 1], ids=["tap-major", "chunk-major"])
ALL_CASES = pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)


def close(name, got, ref):
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(ref.shape), (name, got.dtype, got.shape, ref.shape)
    err = ((got - ref).norm() / ref.norm()).item()
    worst = ((got - ref).abs().max() / ref.abs().max()).item()
    assert err <= TOL and worst <= TOL, f"{name}: rel {err:.2e}, max {worst:.2e}"


def _nhwc_rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def test_table_outputs_and_extents():
    """the outputs the families' formulas give, and the extents the GPU file promises"""
    out = {CC.row_id(r): CC.family_geometry(r)[:2] for r in CC.ROWS}
    assert out["s2p1-3x1x1"] == (1, 1) and out["s2p1-3x2x2"] == (1, 1) and out["s2p1-2x3x3"] == (2, 2)
    assert out["s2p1-2x9x13"] == (5, 7) and out["s2p1-2x18x24"] == (9, 12)
    assert out["s2vae-3x2x2"] == (1, 1) and out["s2vae-3x3x3"] == (1, 1) and out["s2vae-2x9x13"] == (4, 6)
    assert out["ups-3x1x1"] == (2, 2) and out["ups-2x9x12"] == (18, 24)
    assert out["valid-3x3x3"] == (1, 1) and out["valid-2x9x13"] == (7, 11) and out["padtl-2x9x13"] == (9, 11)
    assert len(CC.ROWS) == 26 and len(CC.CASES) == 45
    assert max(CC.rows_M(r, m) for r, m in CC.CASES) == 864          # the largest launch: M = 864, N = K = 9 * 128
    assert CC.rows_M(CC.Row("s1", 37, 3, 3), 1) == 333 and CC.rows_M(CC.GN_ROW, 1) == 715
    assert [CC.row_id(r) for r in CC.ROWS if CC.halo_accepts(r, 1, 1)] == ["s1-2x16x16", "s1-1x16x48", "s1-1x48x16"]


# ---------------------------------------------------------------------------------------------- the reference pin
@KORDERS
@ALL_CASES
def test_reference_is_torch_conv(case, korder):
    row, mode = case
    Cx, Cy = (128, 24) if mode == 1 else (8, 128)  # mode 2: dy has 128 channels (two chunks: the K orders differ)
    x = CC.gauss((row.Bn, Cx, row.H, row.W), 1).requires_grad_(mode == 2)
    w = CC.gauss((Cy, Cx, 3, 3), 2, 0.05)
    y = CC.torch_forward(row, x, w)
    Ho, Wo = CC.family_geometry(row)[:2]
    assert tuple(y.shape) == (row.Bn, Cy, Ho, Wo)
    if mode == 1:
        a, want, Ci, N = x.detach(), y, Cx, Cy
    else:
        dy = CC.gauss(tuple(y.shape), 3)
        y.backward(dy)
        a, want, Ci, N = dy, x.grad, Cy, Cx
    for ldx in (Ci + 8, Ci + 72):
        conv = CC.conv_dict(row, mode, Ci, korder, ldx)
        M = CC.rows_M(row, mode)
        buf, out = CC.place_out(M, N, torch.float64)
        f = partial(_ops().gemm, CC.place_in(_nhwc_rows(a), ldx), CC.pack(w, mode, korder), out, conv=conv, M=M)
        got = G.reference(f).out
        close(f"{CC.case_id(case)} ldx {ldx}", got, _nhwc_rows(want.detach()))
        g = G.geometry(f)
        assert (g.M, g.N, g.K) == (M, N, 9 * Ci) and g.out_strides[1] == N + 8 and CC.untouched(buf, M, N)


# ---------------------------------------------------------------------------------------------- the selector
def _selector_launch(case, Ci, korder, dt, ldx=None):
    row, mode = case
    conv = CC.conv_dict(row, mode, Ci, korder, ldx or Ci + 8)
    M = CC.rows_M(row, mode)
    x = CC.normal_data((CC.in_pixels(row, mode), Ci), 7).to(dt).double()
    _, out = CC.place_out(M, 9 * Ci, torch.float64)
    f = partial(_ops().gemm, CC.place_in(x, conv["ldx"]), CC.selector_packed(Ci, mode, korder), out, conv=conv, M=M)
    return f, x, conv, M


def test_normal_data_is_normal_in_both_formats():
    x = CC.normal_data((4096, 64), 7)
    assert x.abs().min() >= 2.0 ** -8 and x.abs().max() <= 8.0 and (x < 0).any() and (x > 0).any()
    for dt in FORMATS:
        v = x.to(dt)
        assert v.abs().min() >= 2.0 ** -8 and v.abs().max() <= 8.0
        assert torch.equal((4 * v.double()).to(dt).double(), 4 * v.double())  # the largest selector scale stays exact
        assert v.unique().numel() > 200                                        # a wrong address shows as a wrong value
    w = CC.selector_weights(64, 1)
    assert tuple(w.shape) == (576, 64, 3, 3) and int((w != 0).sum()) == 576 and set(w.unique().tolist()) == {0.0, 1.0, 2.0, 4.0}
    assert (w != 0).sum((1, 2, 3)).eq(1).all()
    w2 = CC.selector_weights(64, 2)
    assert tuple(w2.shape) == (64, 576, 3, 3) and (w2 != 0).sum((0, 2, 3)).eq(1).all()
    assert w[67, 3, 0, 1] == CC.SCALES[67 % 3] and w2[3, 67, 0, 1] == CC.SCALES[67 % 3]


@KORDERS
@ALL_CASES
def test_selector_reference_is_exact_and_selects(case, korder):
    row, mode = case
    Ci = 128
    for dt in FORMATS:
        f, x, conv, M = _selector_launch(case, Ci, korder, dt)
        ref = G.reference(f).out
        assert torch.equal(ref.to(dt).double(), ref), f"{dt}: the selector reference is not representable"
        img = x.view(row.Bn, conv["Hi"], conv["Wi"], Ci)
        got = ref.view(row.Bn, conv["Ho"], conv["Wo"], 9 * Ci)
        for n in range(0, 9 * Ci, 37):  # (37 is coprime to 3, 9 and 128: every tap, scale and chunk is visited)
            tap, ci = n // Ci, n % Ci
            assert torch.equal(got[..., n], CC.selector_plane(img, conv, tap, ci) * CC.SCALES[n % 3]), \
                f"{CC.case_id(case)} {dt}: column {n} is not plane {ci} shifted by tap {tap}"


# ---------------------------------------------------------------------------------------------- the mutation proofs
def _mutants(col, x_rows, conv, Bn, Bm, epilogue=None):
    """-> {name: float64 output of the mutated launch}; `epilogue` adds what the launch adds to col @ B^T"""
    epilogue = epilogue or (lambda t: t)
    base = epilogue(col @ Bm.t())
    outs = {}
    for kind in ("wrap", "seam"):
        if kind == "seam" and Bn == 1:
            continue  # (a row with one image has no seam)
        outs[kind] = epilogue(CC.mutate(kind, col, x_rows, conv, Bn) @ Bm.t())
    unwritten = base.clone()
    unwritten[-1] = 0.0  # the GPU tests hand the launch a zeroed (parity) or PAD-filled (selector) output
    outs["unwritten"] = unwritten
    return base, outs


@ALL_CASES
def test_mutants_fail_the_gaussian_check(case):
    """Ci = 64, Co = 24, at the bars of both formats: the three whole-tap / whole-pixel errors are seen by `check`; the
    single-channel swap is reported only"""
    row, mode = case
    Ci, Co = 64, 24
    for dt in FORMATS:
        a, Bp, conv, M, kw = CC.parity_operands(case, Ci, Co, 0, dt, "bias+resid")
        a, Bm = a.double(), Bp.double()
        epi = lambda t: t + kw["bias"].double() + kw["resid"].double()
        col = CC.im2col_of(a, conv, M)
        f = partial(_ops().gemm, a, Bm, torch.zeros(M, Co, dtype=torch.float64), conv=conv, M=M, bias=kw["bias"].double(),
                    resid=kw["resid"].double())
        ref = G.reference(f).out
        base, outs = _mutants(col, a, conv, row.Bn, Bm, epi)
        assert torch.allclose(base, ref, rtol=0, atol=1e-12)
        check(f"{CC.case_id(case)} {dt} unmutated", ref.to(dt), ref, BAR[dt])
        for name, bad in outs.items():
            with pytest.raises(AssertionError):
                check(f"{CC.case_id(case)} {dt} mutant {name}", bad.to(dt), ref, BAR[dt])
        swapped = epi(CC.mutate("swap", col, a, conv, row.Bn) @ Bm.t())
        try:
            check(f"{CC.case_id(case)} {dt} mutant swap", swapped.to(dt), ref, BAR[dt])
            print(f"[{CC.case_id(case)} {dt}] one swapped channel pair PASSES the Gaussian check")
        except AssertionError:
            print(f"[{CC.case_id(case)} {dt}] one swapped channel pair fails the Gaussian check")


@KORDERS
@ALL_CASES
def test_mutants_fail_the_selector_equality(case, korder):
    row, mode = case
    Ci = 128
    for dt in FORMATS:
        f, x, conv, M = _selector_launch(case, Ci, korder, dt)
        ref = G.reference(f).out.to(dt)
        Bm = CC.selector_packed(Ci, mode, korder)
        col = CC.im2col_of(x, conv, M)
        base, outs = _mutants(col, x, conv, row.Bn, Bm)
        assert torch.equal(base.to(dt).float(), ref.float())
        outs["swap"] = CC.mutate("swap", col, x, conv, row.Bn) @ Bm.t()
        outs["unwritten"][-1] = CC.PAD
        for name, bad in outs.items():
            assert not torch.equal(bad.to(dt).float(), ref.float()), f"{CC.case_id(case)} {dt}: mutant {name} equals the reference"


# ---------------------------------------------------------------------------------------------- the bars
def _rounded_reference_passes(case, Ci, Co, korder, dt, epi):
    a, Bp, conv, M, kw = CC.parity_operands(case, Ci, Co, korder, dt, epi)
    kw64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in kw.items()}
    f = partial(_ops().gemm, a.double(), Bp.double(), torch.zeros(M, Co, dtype=torch.float64), conv=conv, M=M, **kw64)
    ref = G.reference(f).out
    check(f"{CC.case_id(case)} {epi} Co{Co} {dt}: rounded reference", ref.to(dt), ref, BAR[dt])


@pytest.mark.parametrize("case", CC.PARITY_CASES, ids=CC.case_id)
def test_bars_hold_for_the_rounded_reference(case):
    """bias + resid at Ci = 128, Co = 72: what every row runs on the GPU"""
    for dt in FORMATS:
        _rounded_reference_passes(case, 128, 72, 1, dt, "bias+resid")


@pytest.mark.parametrize("Co", [128, 320])
@pytest.mark.parametrize("row", CC.EPILOGUE_ROWS, ids=CC.row_id)
def test_bars_hold_for_the_rounded_reference_epilogues(row, Co):
    for dt in FORMATS:
        _rounded_reference_passes((row, 1), 128, Co, 1, dt, "resnet")
        _rounded_reference_passes((row, 2), 128, Co, 1, dt, "gate")
