"""No GPU: proves that tests/test_attn_edges_gpu.py is FAIR (the kernels' algorithm, evaluated in float32 with 16-bit P, dS
and outputs, meets every bar the GPU file asserts with half of it to spare) and SHARP (a tail mask off by one, a moved
causal diagonal, an unwritten row, a rescale threshold that lets P overflow — each fails those same bars on the GPU
file's own data).  Everything under test is in tests/helpers/attn_ref.py; both float16 and bfloat16 are judged in this one
process, since nothing here loads the library.

Attainability: for every case of the GPU file and every output it asserts, `attn_model16` against `attn_ref64` is <= 0.5 of
the relative-Frobenius bar and <= 0.5 of the element-wise bound.  A condition: a bar that the correct algorithm cannot
meet would make the GPU file fail a correct kernel.  The `[model-margin]` lines it prints are the table of DESIGN.md
section 6.

Nk = 1: the true dQ and dK are exactly zero (one key: P = 1, O = V, delta = dP), `check` divides by their norm, so the GPU
file bounds them by 1e-4 in absolute value.  The model must stay <= 1e-5.  With every dot product rounded once it gives
exactly 0 — O equals V bit for bit — so what a kernel leaves is float32 summation order alone; evaluated with plain
float32 sums (one possible order) the model must stay <= 5e-5, half the GPU bound.  (Estimate: a float32 sum of D
products of unit Gaussians errs by about 2^-24 sqrt(D) times its partial sums' size sqrt(D), 1e-5 at D = 160, in dP and
in delta; dK adds Nq = 33 of these times q0 scale = 0.63: about 2e-5.)

Sharpness, at every head dim, in both formats:
  * a zero key admitted at Nk (`key <= Nk` for `key < Nk`; loads past the end return zeros) on `negative` data, at every
    non-causal ragged shape;
  * the causal diagonal moved by +1 and by -1 on `gauss` data, at every causal ragged shape ((1, 1) by -1 only: by +1 the
    key it would admit does not exist);
  * the last query row left unwritten (NaN in O, lse and dQ), at every ragged shape;
  * the rescale threshold at 16 nat instead of 8 on `staircase` data, float16 only.
What bfloat16 cannot see, and why.  (1) Threshold 16: bfloat16 has float32's exponent range, P = e^15 is an ordinary
number and its rounding is relative whatever the stale maximum; the bf16 model passes every bar and the test says so.  (2)
The phantom key on `gauss` data at any tested size: it moves every output by about 1 / Nk, and the bf16 bars are eight
times wider — `test_gauss_data_cannot_see_a_phantom_key` keeps that on record."""
import math

import pytest
import torch

from helpers import attn_ref as A

DTYPES = [torch.float16, torch.bfloat16]
_id = lambda d: str(d).replace("torch.", "") if isinstance(d, torch.dtype) else str(d)
NAN = float("nan")


def _model(kind, Bn, H, Nq, Nk, D, c, dtype, **switches):
    cs = A.case(kind, Bn, H, Nq, Nk, D, c, dtype)
    return cs, A.attn_model16(cs["q"], cs["k"], cs["v"], cs["do"], H, D, D ** -0.5, bool(c), dtype, **switches)


def _fails(group, kind, Bn, H, Nq, Nk, D, c, dtype, outs, ref):
    return A.failing_outputs(f"{_id(dtype)} {kind} D{D} {Nq}x{Nk} c{c}", group, kind, Nk, H, D, dtype, outs, ref)


# ------------------------------------------------------------------------------------------ fair
def test_case_lists():
    """the lists the two files share: every shape the issue names, each once; seeds differ between cases"""
    cases = A.all_cases()
    assert len(cases) == len(set(cases)) == 4 * (2 * 20 + 2 * 3) + 2 * 6 + 2 * 10 * 2
    keys = {(k, nq, nk, D, c) for _, k, _, _, nq, nk, D, c in cases}
    assert len({A.seed_of(*key) for key in keys}) == len(keys)
    for kind in A.KINDS:
        q, k, v, do = A.attn_data(kind, 2, 3, 5, 130, 40, torch.float16, 1)
        assert q.shape == do.shape == (2, 5, 120) and k.shape == v.shape == (2, 130, 120) and q.dtype == torch.float16
        s = (q.view(2, 5, 3, 40).double().transpose(1, 2) @ k.view(2, 130, 3, 40).double().transpose(1, 2).transpose(-1, -2)) * 40 ** -0.5
        tiles = [s[..., t * 64:(t + 1) * 64].mean().item() for t in range(3)]
        want = {"gauss": [0, 0, 0], "negative": [-6, -6, -6], "staircase": [0, 7.5, 15], "descend": [15, 7.5, 0]}[kind]
        assert all(abs(a - b) < 0.3 for a, b in zip(tiles, want)), (kind, tiles)


def test_margins_is_check():
    """`margins` restates helpers.checks.check: both ratios under 1 <=> check passes"""
    from helpers.checks import check
    ref = torch.randn(64, 64, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    for scale, col, passes in [(1e-4, None, True), (1.5e-3, None, False), (1e-4, 5, False)]:
        got = ref * (1 + scale)
        if col is not None:
            got[3, col] += 0.05  # one element: inside the norm, outside the element-wise bound
        r, e = A.margins(got, ref, 1e-3)
        assert (r < 1 and e <= 1) == passes
        if col is not None:
            assert r < 1 < e and A.margins(got, ref, 1e-3, skip_cols=[col])[1] <= 1
        if passes:
            check("margins", got, ref, 1e-3)
        else:
            with pytest.raises(AssertionError):
                check("margins", got, ref, 1e-3)
    assert math.isnan(A.margins(ref * NAN, ref, 1e-3)[1])


@pytest.mark.parametrize("group", ["ragged", "softmax", "qsplit", "small"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_model_meets_every_bar_with_half_to_spare(dtype, group):
    worst, over = {}, []
    for g, kind, Bn, H, Nq, Nk, D, c in A.all_cases():
        if g != group:
            continue
        cs, m = _model(kind, Bn, H, Nq, Nk, D, c, dtype)
        for name, tol, skip_cols, abs_bound in A.spec(group, kind, Nk, H, D, dtype):
            if abs_bound is not None:
                continue  # (test_model_nk1)
            r, e = A.margins(m[name], cs["ref"][name], tol, skip_cols)
            w = worst.get((kind, name), (0.0, 0.0))
            worst[(kind, name)] = (max(w[0], r), max(w[1], e))
            if not (r <= 0.5 and e <= 0.5):
                over.append(f"{kind} D{D} {Nq}x{Nk} c{c} {name}: rel/bar {r:.3f} elem/bound {e:.3f}")
    for (kind, name), (r, e) in sorted(worst.items()):
        print(f"[model-margin] {_id(dtype)} {group} {kind} {name}: rel/bar {r:.3f} elem/bound {e:.3f}")
    assert not over, "the model of the correct algorithm uses more than half of a bar:\n" + "\n".join(over)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_model_nk1(dtype):
    n = 0
    for g, kind, Bn, H, Nq, Nk, D, c in A.all_cases():
        if Nk != 1:
            continue
        for f32_order, bound in ((False, 1e-5), (True, 5e-5)):
            cs, m = _model(kind, Bn, H, Nq, Nk, D, c, dtype, f32_order=f32_order)
            assert float(cs["ref"]["dq"].abs().max()) < 1e-15 and float(cs["ref"]["dk"].abs().max()) < 1e-15
            worst = max(m["dq"].float().abs().max().item(), m["dk"].float().abs().max().item())
            print(f"[model-nk1] {_id(dtype)} {g} {kind} D{D} {Nq}x{Nk} c{c} f32_order={f32_order}: {worst:.2e}")
            assert worst <= bound
        n += 1
    assert n == 4 * 2 * 3 + 2 * 2  # ragged (1, 1), (33, 1), causal (1, 1) per D and kind; small N = 1


# ------------------------------------------------------------------------------------------ sharp
@pytest.mark.parametrize("D", A.HEAD_DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_sharp_phantom_key_on_negative_data(dtype, D):
    for Nq, Nk in A.RAGGED_NONCAUSAL:
        cs, m = _model("negative", A.BN, A.H_EDGE, Nq, Nk, D, 0, dtype, phantom_key=True)
        bad = _fails("ragged", "negative", A.BN, A.H_EDGE, Nq, Nk, D, 0, dtype, m, cs["ref"])
        assert bad, f"a zero key admitted at Nk passes every bar at {Nq}x{Nk} D{D} {_id(dtype)}"


@pytest.mark.parametrize("shift", [1, -1])
@pytest.mark.parametrize("D", A.HEAD_DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_sharp_causal_diagonal(dtype, D, shift):
    for Nq, Nk in A.RAGGED_CAUSAL:
        if shift == 1 and Nk == 1:
            continue
        cs, m = _model("gauss", A.BN, A.H_EDGE, Nq, Nk, D, 1, dtype, diag_shift=shift)
        bad = _fails("ragged", "gauss", A.BN, A.H_EDGE, Nq, Nk, D, 1, dtype, m, cs["ref"])
        assert bad, f"the causal diagonal moved by {shift} passes every bar at {Nq}x{Nk} D{D} {_id(dtype)}"


@pytest.mark.parametrize("D", A.HEAD_DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_sharp_unwritten_last_query_row(dtype, D):
    for Nq, Nk, c in A.RAGGED:
        cs, m = _model("gauss", A.BN, A.H_EDGE, Nq, Nk, D, c, dtype)
        assert not _fails("ragged", "gauss", A.BN, A.H_EDGE, Nq, Nk, D, c, dtype, m, cs["ref"])
        for name in ("o", "lse", "dq"):
            left = dict(m)
            left[name] = m[name].clone()
            if name == "lse":
                left[name][:, :, -1] = NAN
            else:
                left[name][:, -1, :] = NAN
            bad = _fails("ragged", "gauss", A.BN, A.H_EDGE, Nq, Nk, D, c, dtype, left, cs["ref"])
            assert len(bad) == 1, f"an unwritten last row of {name} at {Nq}x{Nk} c{c} D{D}: {bad}"


@pytest.mark.parametrize("D", A.HEAD_DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_sharp_rescale_threshold_16_on_the_staircase(dtype, D):
    """P <= e^8 fits float16; with the threshold at 16 the third tile's P = e^15 does not"""
    for Nq, Nk, c in A.SOFTMAX_SHAPES:
        cs, m = _model("staircase", A.BN, A.H_EDGE, Nq, Nk, D, c, dtype)
        assert bool(torch.isfinite(m["o"].float()).all())
        cs, m = _model("staircase", A.BN, A.H_EDGE, Nq, Nk, D, c, dtype, threshold=16.0)
        bad = _fails("softmax", "staircase", A.BN, A.H_EDGE, Nq, Nk, D, c, dtype, m, cs["ref"])
        if dtype == torch.float16:
            assert bad and not bool(torch.isfinite(m["o"].float()).all()), f"threshold 16 passes at {Nq}x{Nk} c{c} D{D}"
        else:
            assert not bad, "bfloat16 does not overflow: the module docstring says this mutation is invisible there"


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_staircase_reaches_the_stale_max_path(dtype):
    """the data does what its name says: under the real threshold P reaches e^7 and more against a stale maximum (so the
    8-nat path is exercised), and never e^8.7 (float16 has room: 65504 = e^11.09)"""
    for Nq, Nk, c in A.SOFTMAX_SHAPES:
        cs = A.case("staircase", A.BN, A.H_EDGE, Nq, Nk, 64, c, dtype)
        qh, kh = (A._heads(cs[n].float(), A.H_EDGE, 64) for n in ("q", "k"))
        s = (qh @ kh.transpose(-1, -2)) * 64 ** -0.5
        s = s.masked_fill(~A._mask(Nq, Nk, bool(c)), float("-inf"))
        m = s[..., :64].max(-1, keepdim=True).values
        over = (s[..., 64:128] - m).max().item()
        print(f"staircase {Nq}x{Nk} c{c}: second tile up to {over:.2f} nat over the first tile's maximum")
        assert 7.0 < over < 8.7


# ------------------------------------------------------------------------------------------ the existing data, documented
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_gauss_data_cannot_see_a_phantom_key(dtype):
    """THE REASON FOR THE `negative` KIND.  On unit-Gaussian data (what tests/test_kernels_gpu.py and the contract cases
    use) a zero key admitted at Nk = 520 has a share of about 1 / Nk of every softmax and moves O, lse, dQ, dK and dV by
    about that fraction: inside every bar, in both formats.  If the suite's bars are ever tightened so that this test
    fails, `gauss` data has become sharp enough and the `negative` kind can go."""
    Nq, Nk, D = 65, 520, 40
    cs, m = _model("gauss", A.BN, A.H_EDGE, Nq, Nk, D, 0, dtype, phantom_key=True)
    assert not _fails("ragged", "gauss", A.BN, A.H_EDGE, Nq, Nk, D, 0, dtype, m, cs["ref"])
    cs, m = _model("negative", A.BN, A.H_EDGE, Nq, Nk, D, 0, dtype, phantom_key=True)
    assert len(_fails("ragged", "negative", A.BN, A.H_EDGE, Nq, Nk, D, 0, dtype, m, cs["ref"])) >= 4
