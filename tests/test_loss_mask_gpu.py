"""The object-masked diffusion loss on the GPU: the three entries through the C ABI, the whole
step against the CPU oracle, and the engine / Coach behaviour around them.

References.  Kernels: the float64 restatement of tests/helpers/loss_mask_ref.py from the same uint8 masks and the same
16-bit-rounded predictions.  vneti_loss_weights_from_mask is f32 out of integers and f64: the f32 bar rule `check32`.
vneti_mse_loss_grad_weighted at the bars of test_kernel_mse_loss_grad_snr_against_float64 (loss_sum 1e-5 relative, dpred
t16(1e-3)); vneti_mse_loss_per_sample_weighted at the 1e-5 of test_mse_per_sample_matches_float64 (ten times the pairwise
summation bound at 16384 terms; the one more rounded product per pixel is 2^-24).  Whole step: the unchanged oracle's
prediction and target with the restatement's weights, at the bars of test_train_step_with_options_matches_oracle.
Everything the option must NOT change is compared for bit equality.  The kernel cases (test_kernel_*) also run against
libvneti_hip_bf16.so in a child process."""
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from helpers import coach_runs as rt
from helpers import loss_mask_ref as MR
from helpers import loss_options_ref as LR
from helpers import slabs as S
from helpers.bf16_child import run_bf16_child
from helpers.checks import DEV, DT, check, check32, rnd, t16, ops as _ops
from helpers.engines import FORMS, STATE, build_device_rng_engine as _build, build_train_engine as build_step
from helpers.engines import feed_device_rng, feed_six as _feed, run_steps, six_steps as _six_steps, snapshot

pytestmark = pytest.mark.gpu
F32 = torch.float32
AC = LR.scaled_linear_alphas_cumprod_f32()
GAMMA = 5.0
B, H, W = 2, 64, 64   # of the device-RNG engines (helpers.engines.build_device_rng_engine)
ROWS = 16
THR = 3


# ================================================================================================ kernel (a): the weights
def _weights(mask, f, bg, stride=1, Bn=1, b=0, misalign=0, thr=THR):
    """row b of a [Bn][hw] table prefilled with -7 from a (H, W) uint8 mask laid out with `stride` bytes per pixel (the
    other channels hold 255 where channel 0 holds 0 and the reverse) -> (row, the whole table)"""
    ops = _ops()
    Hh, Ww = mask.shape
    img = mask if stride == 1 else torch.stack([mask, 255 - mask, 255 - mask], dim=-1)
    flat = torch.zeros(img.numel() + 8, dtype=torch.uint8)
    flat[misalign:misalign + img.numel()] = img.reshape(-1)
    dev = flat.to(DEV)[misalign:misalign + img.numel()]
    q = torch.full((Bn, (Hh // f) * (Ww // f)), -7.0, dtype=F32, device=DEV)
    ws = torch.full((ops.loss_weights_from_mask_ws_ints(Hh, Ww, f),), -1, dtype=torch.int32, device=DEV)
    ops.loss_weights_from_mask(dev, Hh, Ww, stride, f, thr, bg, q, b, ws)
    torch.cuda.synchronize()
    return q[b].cpu(), q.cpu()


def _weights_ref32(mask, f, bg, thr=THR):
    """the restatement's formula evaluated in torch float32: the e32 of check32"""
    cnt = MR.cell_counts(mask, f, thr).reshape(-1).float()
    bg = torch.tensor(bg, dtype=F32)
    m = bg + (1 - bg) * (cnt / float(f * f))
    return m * (float(m.numel()) / m.sum())


@pytest.mark.parametrize("bg", [0.0, 0.25], ids=["bg0", "bg0.25"])
@pytest.mark.parametrize("stride", [1, 3], ids=["stride1", "stride3"])
@pytest.mark.parametrize("Hh,Ww", [(8, 8), (24, 40), (136, 248)], ids=["1cell", "3x5", "17x31"])
def test_kernel_loss_weights_against_float64(Hh, Ww, stride, bg):
    """one cell; 15 cells of one block; 527 cells = two 256-cell blocks and a tail of 15.  Per-pixel random masks with values
    on both sides of the threshold (2 | 3): almost every cell is partial"""
    mask = MR.random_mask(Hh, Ww, seed=Hh + Ww)
    if (Hh, Ww) == (8, 8) and bg == 0.0:
        assert 0 < int(MR.cell_counts(mask, 8).item()) < 64
    row, table = _weights(mask, 8, bg, stride)
    ref = MR.weights_from_mask(mask, 8, THR, bg)
    check32(f"loss_weights {Hh}x{Ww} stride{stride} bg{bg}", row, ref, _weights_ref32(mask, 8, bg))
    assert abs(row.double().mean().item() - 1.0) < 1e-6
    # the byte loop (a base that is not 8-byte aligned) and the 8-byte loads give the same row
    if stride == 1:
        assert torch.equal(row, _weights(mask, 8, bg, 1, misalign=1)[0])
    # another factor: 4 x 4 cells
    row4, _ = _weights(mask, 4, bg, stride)
    check32(f"loss_weights {Hh}x{Ww} f4", row4, MR.weights_from_mask(mask, 4, THR, bg), _weights_ref32(mask, 4, bg))


@pytest.mark.parametrize("stride", [1, 3], ids=["stride1", "stride3"])
def test_kernel_loss_weights_exact_properties(stride):
    Hh, Ww = 136, 248
    full, empty = torch.full((Hh, Ww), 255, dtype=torch.uint8), torch.zeros(Hh, Ww, dtype=torch.uint8)
    for bg in (0.0, 0.1, 0.25, 1.0):  # all foreground: exactly 1.0f whatever the background weight
        row, _ = _weights(full, 8, bg, stride)
        assert bool((row == 1.0).all()), f"bg {bg}: {row.min().item()!r} .. {row.max().item()!r}"
        at_thr, _ = _weights(torch.full((Hh, Ww), THR, dtype=torch.uint8), 8, bg, stride)
        assert bool((at_thr == 1.0).all())
    row, _ = _weights(empty, 8, 0.0, stride)
    assert bool((row == 0.0).all()) and bool(torch.isfinite(row).all()), "an empty mask with bg 0 is a row of exact zeros"
    below, _ = _weights(torch.full((Hh, Ww), THR - 1, dtype=torch.uint8), 8, 0.0, stride)
    assert bool((below == 0.0).all())
    uniform, _ = _weights(empty, 8, 0.25, stride)
    assert bool((uniform == 1.0).all())
    # a function of the mask alone: (Bn = 1, b = 0) and (Bn = 3, b = 2) bit for bit, and the other rows untouched
    mask = MR.random_mask(Hh, Ww, seed=5)
    alone, _ = _weights(mask, 8, 0.25, stride)
    last, table = _weights(mask, 8, 0.25, stride, Bn=3, b=2)
    assert torch.equal(alone, last) and bool((table[:2] == -7.0).all())
    assert not torch.equal(alone, _weights(mask, 8, 0.0, stride)[0])


def test_kernel_loss_weights_refuses_bad_arguments():
    from view_neti_amd import lib
    ops = _ops()
    m = torch.zeros(24 * 24 * 3, dtype=torch.uint8, device=DEV)
    q, ws = torch.zeros(1, 9, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    good = (m.data_ptr(), 24, 24, 1, 8, THR, 0.25, q.data_ptr(), ws.data_ptr(), ops.stream())
    lib.call("loss_weights_from_mask", *good)
    for i, v, word in ((1, 20, "multiples"), (2, 20, "multiples"), (3, 2, "pixel_stride"), (4, 0, "factor"), (4, 65, "factor"),
                       (5, 256, "threshold"), (5, -1, "threshold"), (6, -0.5, "background"), (6, 1.5, "background"),
                       (6, math.nan, "background"), (0, None, "null"), (7, None, "null"), (8, None, "null")):
        args = list(good)
        args[i] = v
        with pytest.raises(RuntimeError, match=word):
            lib.call("loss_weights_from_mask", *args)
    torch.cuda.synchronize()
    assert lib.query("loss_weights_from_mask_ws_ints", 20, 24, 8) < 0 and lib.query("loss_weights_from_mask_ws_ints", 24, 20, 8) < 0
    assert ops.loss_weights_from_mask_ws_ints(136, 248, 8) == 3 and ops.loss_weights_from_mask_ws_ints(8, 8, 8) == 1
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.loss_weights_from_mask(m, 20, 24, 1, 8, THR, 0.0, torch.zeros(1, 6, device=DEV), 0, ws)


# ================================================================================================ kernel (b): loss + gradient
def _mse_inputs(Bn, Lc, HW, ld):
    return rnd(Bn * HW, ld, seed=84), rnd(Bn, Lc, HW, seed=85, dtype=F32)


def _q(Bn, HW, zero_sample=None):
    """weights of the restatement's kind: >= 0, mean 1 per sample, exact zeros among them"""
    g = torch.Generator().manual_seed(86)
    q = torch.rand(Bn, HW, generator=g) * (torch.rand(Bn, HW, generator=g) < 0.7)
    q = (q / q.mean(dim=1, keepdim=True).clamp_min(1e-3)).float()
    if HW == 1:
        q = torch.full((Bn, 1), 1.5)
    if zero_sample is not None:
        q[zero_sample] = 0.0
    return q


def _mse_launch(entry, pbig, target, Bn, Lc, HW, scale, start, *extra, **kw):
    """one launch on strided 4-of-ld-column views; -> (dbig with 7.0 beyond the channels, loss_sum)"""
    ops = _ops()
    dbig = torch.full(tuple(pbig.shape), 7.0, dtype=DT, device=DEV)
    loss_sum = torch.tensor([start], dtype=F32, device=DEV)
    getattr(ops, entry)(pbig.to(DEV)[:, :Lc], target.to(DEV), dbig[:, :Lc], loss_sum, torch.tensor([scale], device=DEV),
                        *extra, **kw)
    torch.cuda.synchronize()
    return dbig, loss_sum


def _snr_kw(t, vpred):
    return dict(t=t.to(DEV), ac=AC.to(DEV), gamma=GAMMA, vpred=vpred)


@pytest.mark.parametrize("mode", ["plain", "snr-epsilon", "snr-v"])
@pytest.mark.parametrize("Bn,HW,t", [(3, 81, (0, 146, 147)), (1, 1, (40,))], ids=["four-blocks", "one-pixel"])
def test_kernel_mse_loss_grad_weighted_against_float64(Bn, HW, t, mode):
    """the shapes and bars of test_kernel_mse_loss_grad_snr_against_float64: N = 972 with 4 of 8 strided columns, and N = 4;
    loss scale 128, loss_sum starts at 3.25.  Sample 1 of the three has all-zero weights"""
    Lc, ld, scale, start = 4, 8, 128.0, 3.25
    pbig, target = _mse_inputs(Bn, Lc, HW, ld)
    q = _q(Bn, HW, zero_sample=1 if Bn > 1 else None)
    tt = torch.tensor(t, dtype=torch.int64)
    vpred = mode == "snr-v"
    kw = {} if mode == "plain" else _snr_kw(tt, vpred)
    dbig, loss_sum = _mse_launch("mse_loss_grad_weighted", pbig, target, Bn, Lc, HW, scale, start, q.to(DEV), Bn, Lc, HW, **kw)
    w = None if mode == "plain" else LR.min_snr_weight(AC, tt, GAMMA, vpred)
    pr = pbig[:, :Lc].double().view(Bn, HW, Lc).permute(0, 2, 1)   # (B, C, HW)
    loss, grad = MR.weighted_loss(pr, target, q, w)
    name = f"mse_weighted Bn{Bn} HW{HW} {mode}"
    check(f"{name} loss_sum", loss_sum, (start + loss * pr.numel()).reshape(1), 1e-5)
    if Bn * Lc * HW == 972:
        check(f"{name} loss (mean)", (loss_sum.cpu().double() - start) / (Bn * Lc * HW), loss.reshape(1), 1e-5)
    got = dbig[:, :Lc].view(Bn, HW, Lc)
    check(f"{name} dpred", got, (grad * scale).permute(0, 2, 1), t16(1e-3))
    assert bool((dbig[:, Lc:] == 7).all()), "columns beyond Lc were written"
    assert bool(torch.isfinite(got.float()).all()) and math.isfinite(loss_sum.item())
    if Bn > 1:
        assert bool((got[1] == 0).all()), "a sample whose weights are all zero has exact-zero dpred rows"
        assert bool((got[0] != 0).any()) and bool((got[2] != 0).any())
        zero_px = (q[0] == 0).nonzero().flatten()
        assert zero_px.numel() > 0 and bool((got[0][zero_px] == 0).all())
        plain, _ = _mse_launch("mse_loss_grad", pbig, target, Bn, Lc, HW, scale, start, Bn, Lc, HW)
        assert not torch.equal(plain, dbig)


@pytest.mark.parametrize("vpred", [False, True], ids=["epsilon", "v-prediction"])
@pytest.mark.parametrize("Bn,HW", [(3, 81), (1, 1)], ids=["four-blocks", "one-block"])
def test_kernel_mse_loss_grad_weighted_ones_is_the_existing_entry(Bn, HW, vpred):
    """q == 1.0f: dpred bit for bit that of vneti_mse_loss_grad (null pair) and of vneti_mse_loss_grad_snr (with it);
    loss_sum bit for bit where one block adds to it, at 1e-5 where four blocks add with float atomics in any order"""
    Lc, ld, scale, start = 4, 8, 128.0, 3.25
    pbig, target = _mse_inputs(Bn, Lc, HW, ld)
    ones = torch.ones(Bn, HW, device=DEV)
    t = torch.tensor([0, 146, 147][:Bn], dtype=torch.int64)
    pairs = [(_mse_launch("mse_loss_grad", pbig, target, Bn, Lc, HW, scale, start, Bn, Lc, HW),
              _mse_launch("mse_loss_grad_weighted", pbig, target, Bn, Lc, HW, scale, start, ones, Bn, Lc, HW)),
             (_mse_launch("mse_loss_grad_snr", pbig, target, Bn, Lc, HW, scale, start, Bn, Lc, HW, t.to(DEV), AC.to(DEV), GAMMA, vpred),
              _mse_launch("mse_loss_grad_weighted", pbig, target, Bn, Lc, HW, scale, start, ones, Bn, Lc, HW, **_snr_kw(t, vpred)))]
    for (d0, s0), (d1, s1) in pairs:
        assert torch.equal(d0, d1), "q == 1 changed dpred"
        if Bn * Lc * HW <= 256:
            assert torch.equal(s0, s1), (s0.item(), s1.item())
        else:
            check("mse_weighted q=1 loss_sum", s1, s0.double(), 1e-5)
    assert not torch.equal(pairs[0][0][0], pairs[1][0][0])


def test_kernel_mse_loss_grad_weighted_refuses_bad_arguments():
    pbig, target = _mse_inputs(1, 4, 1, 8)
    q = torch.ones(1, 1, device=DEV)
    t = torch.zeros(1, dtype=torch.int64, device=DEV)
    for gamma in (0.0, -1.0, math.nan):
        with pytest.raises(RuntimeError, match="gamma"):
            _mse_launch("mse_loss_grad_weighted", pbig, target, 1, 4, 1, 1.0, 0.0, q, 1, 4, 1, t=t, ac=AC.to(DEV), gamma=gamma)
    from view_neti_amd import lib
    ops = _ops()
    pd, td, dp, ls, sc = pbig.to(DEV), target.to(DEV), torch.zeros(1, 8, dtype=DT, device=DEV), torch.zeros(1, device=DEV), torch.ones(1, device=DEV)
    good = [pd.data_ptr(), 8, td.data_ptr(), dp.data_ptr(), 8, ls.data_ptr(), sc.data_ptr(), q.data_ptr(), 1, 4, 1, None, None,
            0.0, 0, ops.stream()]
    lib.call("mse_loss_grad_weighted", *good)
    for i, v, word in ((7, None, "null"), (11, t.data_ptr(), "pair"), (12, AC.to(DEV).data_ptr(), "pair"), (8, 0, "bad shape"),
                       (1, 3, "bad shape"), (4, 3, "bad shape"), (1, 1 << 40, "2 GiB")):
        args = list(good)
        args[i] = v
        with pytest.raises(RuntimeError, match=word):
            lib.call("mse_loss_grad_weighted", *args)
    torch.cuda.synchronize()


# ================================================================================================ kernel (c): per sample
def _ps_inputs(HW, Lc, ldp, Bn, seed=0):
    g = torch.Generator().manual_seed(1000 * HW + ldp + seed)
    wide = torch.randn((Bn * HW, ldp), generator=g).to(DT)
    target = torch.randn((Bn, Lc, HW), generator=g)
    return wide, target


def _ps_run(wide, target, q, Bn, Lc, HW):
    ops = _ops()
    wd, td = wide.to(DEV), target.to(DEV).contiguous()
    out = torch.full((Bn,), -1.0, device=DEV)
    ws = torch.full((ops.mse_loss_per_sample_ws_floats(Bn, HW),), float("nan"), device=DEV)
    if q is None:
        ops.mse_loss_per_sample(wd[:, :Lc], td, out, ws, Bn, Lc, HW)
    else:
        ops.mse_loss_per_sample_weighted(wd[:, :Lc], td, q.to(DEV).contiguous(), out, ws, Bn, Lc, HW)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("HW", [1, 81, 257])
def test_kernel_mse_per_sample_weighted_against_float64(HW):
    """one pixel; 81 pixels of one chunk; 257 = a full chunk and a tail of one.  4 of 8 strided columns, Bn = 3, sample 1
    with all-zero weights"""
    Lc, ldp, Bn = 4, 8, 3
    wide, target = _ps_inputs(HW, Lc, ldp, Bn)
    q = _q(Bn, HW, zero_sample=1)
    got = _ps_run(wide, target, q, Bn, Lc, HW)
    pr = wide[:, :Lc].double().view(Bn, HW, Lc).permute(0, 2, 1)
    ref = MR.per_sample(pr, target, q)
    rel = ((got.double() - ref).abs() / ref.clamp_min(1e-300))[[0, 2]].max().item()
    print(f"[mse_per_sample_weighted HW={HW}] got {got.tolist()} ref {ref.tolist()} max rel err {rel:.2e}")
    assert rel <= 1e-5 and got[1].item() == 0.0 and ref[1].item() == 0.0
    assert torch.equal(got, _ps_run(wide, target, q, Bn, Lc, HW)), "two calls must be bit-equal"
    # q == 1: the unweighted entry bit for bit
    assert torch.equal(_ps_run(wide, target, torch.ones(Bn, HW), Bn, Lc, HW), _ps_run(wide, target, None, Bn, Lc, HW))
    assert not torch.equal(got, _ps_run(wide, target, None, Bn, Lc, HW))
    # sample 2 of 3 alone, and as sample 4 of 5: bit for bit
    rows, tg, qq = wide[2 * HW:], target[2:], q[2:]
    alone = _ps_run(rows, tg, qq, 1, Lc, HW)
    fw, ft = _ps_inputs(HW, Lc, ldp, 5, seed=7)
    fq = _q(5, HW)
    fw[4 * HW:], ft[4], fq[4] = rows, tg[0], qq[0]
    last = _ps_run(fw, ft, fq, 5, Lc, HW)
    assert torch.equal(alone[0], got[2]) and torch.equal(last[4], got[2])


def test_bf16_library_runs_the_kernel_cases(tmp_path):
    """the test_kernel_* and test_contract_* cases against libvneti_hip_bf16.so, in a child pytest process with
    VNETI_PRECISION=bf16: no failure, no error, nothing skipped, as many cases as were collected"""
    from view_neti_amd import lib
    if lib.precision() == "bf16":
        return  # this IS the bf16 run
    run_bf16_child(os.path.join("tests", os.path.basename(__file__)), "test_kernel_ or test_contract_", 240, tmp_path, least=30)


# ================================================================================================ memory contracts
def _three_runs(ins, outs, scratch, call, verify):
    """the three runs of tests/test_kernel_contracts_gpu.py on guarded slabs: clean; poisoned surroundings, sentinel outputs
    and NaN / -1 scratch; replay.  ins: [(slab, values, poison bits)], outs: [slab], scratch: [tensor]"""
    def results():
        return [s.logical_bits() for s in outs]

    def contract(run, snaps):
        for s in outs:
            s.outside_intact(S.SENTINEL[s.dtype], f"{s.name} after run {run}")
            s.logical_has_no_sentinel(S.SENTINEL[s.dtype], f"{s.name} after run {run}")
        for (s, _, _), snap in zip(ins, snaps):
            s.unchanged(snap, f"{s.name} after run {run}")

    for s, v, _ in ins:
        s.fill_all(0)
        s.fill_logical(v)
    for s in outs:
        s.fill_all(0)
    for w in scratch:
        w.zero_()
    call()
    torch.cuda.synchronize()
    a = results()
    for s, _, poison in ins:
        s.fill_outside(poison)
    for s in outs:
        s.fill_all(S.SENTINEL[s.dtype])
    for w in scratch:
        w.fill_(float("nan") if w.dtype.is_floating_point else -1)
    snaps = [s.snapshot() for s, _, _ in ins]
    call()
    torch.cuda.synchronize()
    contract("B", snaps)
    b = results()
    verify()
    for s, x, y in zip(outs, a, b):
        S.first_difference(x, y, s, f"{s.name}: run B (poisoned) differs from run A (clean)")
    call()
    torch.cuda.synchronize()
    contract("C", snaps)
    for s, x, y in zip(outs, b, results()):
        S.first_difference(x, y, s, f"{s.name}: run C (replay) differs from run B")


def _slab(name, rows, cols, dtype, gap):
    s = S.Slab.matrix(rows, cols, dtype, gap=gap, device=DEV)
    s.name = name
    return s


@pytest.mark.parametrize("stride", [1, 3])
def test_contract_loss_weights_from_mask(stride):
    """the mask is one contiguous image in the middle of a slab whose surroundings are 255 (foreground): a read outside it
    would raise a count; the row is a one-row table in a guarded slab of its own, whose guards must keep the sentinel (that
    the other rows of a [3][hw] table stay untouched is test_kernel_loss_weights_exact_properties)"""
    ops = _ops()
    Hh, Ww, f, bg = 136, 248, 8, 0.25
    mask = MR.random_mask(Hh, Ww, seed=9)
    img = mask if stride == 1 else torch.stack([mask, 255 - mask, 255 - mask], dim=-1)
    ms = _slab("mask", Hh, Ww * stride, torch.uint8, 0)
    hw = (Hh // f) * (Ww // f)
    qs = _slab("q row", 1, hw, F32, 0)
    ws = torch.zeros(ops.loss_weights_from_mask_ws_ints(Hh, Ww, f), dtype=torch.int32, device=DEV)
    ref = MR.weights_from_mask(mask, f, THR, bg)
    _three_runs([(ms, img.reshape(Hh, -1), 0xFF)], [qs], [ws],
                lambda: ops.loss_weights_from_mask(ms.view.reshape(-1), Hh, Ww, stride, f, THR, bg, qs.view, 0, ws),
                lambda: check32(f"contract loss_weights stride{stride}", qs.view[0], ref, _weights_ref32(mask, f, bg)))


@pytest.mark.parametrize("snr", [False, True], ids=["plain", "snr"])
def test_contract_mse_loss_grad_weighted(snr):
    ops = _ops()
    Bn, Lc, HW, scale = 3, 4, 81, 128.0
    pbig, target = _mse_inputs(Bn, Lc, HW, 4)
    q = _q(Bn, HW, zero_sample=1)
    t = torch.tensor([0, 146, 147], dtype=torch.int64)
    ps, ts_, qs = _slab("pred", Bn * HW, Lc, DT, 8), _slab("target", Bn * Lc, HW, F32, 0), _slab("q", Bn, HW, F32, 0)
    ds = _slab("dpred", Bn * HW, Lc, DT, 16)
    ls = _slab("loss_sum", 1, 1, F32, 0)
    sc, tt, ac = torch.tensor([scale], device=DEV), t.to(DEV), AC.to(DEV)
    kw = dict(t=tt, ac=ac, gamma=GAMMA, vpred=False) if snr else {}
    w = LR.min_snr_weight(AC, t, GAMMA) if snr else None
    pr = pbig.double().view(Bn, HW, Lc).permute(0, 2, 1)
    loss, grad = MR.weighted_loss(pr, target, q, w)

    def call():
        ls.view.zero_()  # (the entry adds into loss_sum: the caller zeroes it, as the step does)
        ops.mse_loss_grad_weighted(ps.view, ts_.view.view(Bn, Lc, HW), ds.view, ls.view.view(-1), sc, qs.view, Bn, Lc, HW, **kw)

    def verify():
        check(f"contract mse_weighted snr={snr} dpred", ds.view.view(Bn, HW, Lc), (grad * scale).permute(0, 2, 1), t16(1e-3))
        check(f"contract mse_weighted snr={snr} loss_sum", ls.view.view(-1), (loss * pr.numel()).reshape(1), 1e-5)

    # loss_sum is summed over four blocks by float atomics in any order: not among the bit-compared outputs
    _three_runs([(ps, pbig, S.QNAN[DT]), (ts_, target.reshape(Bn * Lc, HW), S.QNAN[F32]), (qs, q, S.QNAN[F32])], [ds], [],
                call, verify)
    ls.outside_intact(0, "loss_sum")


def test_contract_mse_loss_per_sample_weighted():
    ops = _ops()
    Bn, Lc, HW = 3, 4, 257
    wide, target = _ps_inputs(HW, Lc, 4, Bn)
    q = _q(Bn, HW, zero_sample=1)
    ps, ts_, qs = _slab("pred", Bn * HW, Lc, DT, 8), _slab("target", Bn * Lc, HW, F32, 0), _slab("q", Bn, HW, F32, 0)
    os_ = _slab("out", 1, Bn, F32, 0)
    ws = torch.zeros(ops.mse_loss_per_sample_ws_floats(Bn, HW), device=DEV)
    ref = MR.per_sample(wide.double().view(Bn, HW, Lc).permute(0, 2, 1), target, q)

    def verify():
        got = os_.view.view(-1).cpu().double()
        assert got[1].item() == 0.0 and ((got - ref).abs() / ref.clamp_min(1e-300))[[0, 2]].max().item() <= 1e-5

    _three_runs([(ps, wide, S.QNAN[DT]), (ts_, target.reshape(Bn * Lc, HW), S.QNAN[F32]), (qs, q, S.QNAN[F32])], [os_], [ws],
                lambda: ops.mse_loss_per_sample_weighted(ps.view, ts_.view.view(Bn, Lc, HW), qs.view, os_.view.view(-1), ws,
                                                         Bn, Lc, HW), verify)


# ================================================================================================ whole step vs the CPU oracle
_ORACLE, _STEP_BUILDS = {}, {}
T_STEP = (40, 700)  # gamma = 5 clips the first (snr ~ 32) and not the second (snr ~ 0.09)


def _step_inputs(cfg, with_view, Hh, Ww):
    from view_neti_amd import synth
    Bn = 2
    ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
    return dict(ids=synth.input_ids(Bn, ph, cfg.clip.vocab_size, view_placeholder_id=phv if with_view else None),
                px=synth.pixel_values(Bn, Hh, Ww), t=torch.tensor(T_STEP, dtype=torch.int64),
                eps=synth.gaussian((Bn, 4, Hh // 8, Ww // 8), 3), noise=synth.gaussian((Bn, 4, Hh // 8, Ww // 8), 4),
                vparams=synth.gaussian((Bn, 12), 9).clamp(-1, 1) if with_view else None,
                masks=torch.stack([MR.blocky_mask(Hh, Ww, 8, 20 + b) for b in range(Bn)]))


def _oracle(cfg_name, with_view, Hh, Ww):
    """the oracle's forward, once per family and left unchanged -> dict(pred with its graph, target, parameter leaves)"""
    if cfg_name in _ORACLE:
        return _ORACLE[cfg_name]
    from oracle import sd_ref as R
    Bn = 2
    cfg, (uw, vw, cw), sd, w_enc, extra = _STEP_BUILDS[cfg_name]
    ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
    inp = _step_inputs(cfg, with_view, Hh, Ww)
    r16 = lambda d: {k: (v.half().float() if v.dim() >= 2 and "embedding" not in k else v) for k, v in d.items()}
    p_o = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    leaves, view = [p_o], None
    if with_view:
        p_v = {k: v.clone().requires_grad_(True) for k, v in extra["mapper_view"].items()}
        leaves.append(p_v)
        view = dict(p=p_v, w_enc=extra["w_enc_view"], norm_scale=0.35, placeholder=torch.full((Bn,), phv),
                    params=inp["vparams"], alpha=0.3, unconstrained=False)
    _, aux = R.train_step_loss(cfg, r16(uw), r16(vw), r16(cw), p_o, w_enc, 0.4, inp["px"], inp["ids"], torch.full((Bn,), ph),
                               inp["t"], inp["eps"], inp["noise"], alpha=0.2, view=view)
    vpred = cfg.ddpm.prediction_type == "v_prediction"
    target = R.get_velocity(R.alphas_cumprod(cfg.ddpm), aux["latents"], inp["noise"], inp["t"]) if vpred else inp["noise"]
    _ORACLE[cfg_name] = dict(pred=aux["pred"], target=target, leaves=leaves, vpred=vpred)
    return _ORACLE[cfg_name]


def _oracle_loss_and_grad(o, q, w):
    """sum_{b,c,p} w_b q_bp d^2 / N of the oracle's prediction and its mapper gradient (the graph is kept)"""
    from view_neti_amd.engine.text import flatten_mapper_state
    d2 = (o["pred"].float() - o["target"].float()) ** 2
    Bn, Cc, h, w_ = d2.shape
    wq = (q.float() * w.float().view(-1, 1)).view(Bn, 1, h, w_)
    loss = (wq * d2).sum() / d2.numel()
    flat = [v for p in o["leaves"] for v in p.values()]
    grads = torch.autograd.grad(loss, flat, retain_graph=True)
    out, i = [], 0
    for p in o["leaves"]:
        out.append(flatten_mapper_state({k: g for k, g in zip(p, grads[i:i + len(p)])}))
        i += len(p)
    return loss.item(), torch.cat(out)


def _bars(loss_gpu, g_gpu, loss_ref, g_ref):
    rel = abs(loss_gpu - loss_ref) / loss_ref
    cos = torch.nn.functional.cosine_similarity(g_gpu, g_ref, dim=0).item()
    gerr = ((g_gpu - g_ref).norm() / g_ref.norm()).item()
    return rel, cos, gerr


@pytest.mark.parametrize("snr_on,bg", [(False, 0.0), (False, 0.25), (True, 0.0)], ids=["bg0", "bg0.25", "bg0-snr"])
@pytest.mark.parametrize("cfg_name,with_view,Hh,Ww", [("tiny", False, 64, 64), ("tiny21", True, 64, 128)],
                         ids=["tiny-epsilon", "tiny21-v-view"])
def test_train_step_with_mask_matches_oracle(cfg_name, with_view, Hh, Ww, snr_on, bg):
    """B = 2, t = (40, 700), blocky random masks with one row of partial cells: masked loss within 1e-3 relative,
    mapper-gradient cosine > 0.999 and relative error < 5e-2 (the bars of test_train_step_with_options_matches_oracle) — and
    NOT within them of the plain objective"""
    Bn = 2
    cfg, eng, weights, sd, w_enc, extra = build_step(cfg_name, Bn, Hh, Ww, with_view=with_view, device_rng=False, lr=4e-3,
                                                     loss_mask=True, loss_mask_background=bg,
                                                     snr_gamma=GAMMA if snr_on else None)
    _STEP_BUILDS.setdefault(cfg_name, (cfg, weights, sd, w_enc, extra))
    inp = _step_inputs(cfg, with_view, Hh, Ww)
    ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
    assert bool((eng.loss_weights == 1.0).all()) and tuple(eng.loss_weights.shape) == (Bn, (Hh // 8) * (Ww // 8))
    eng.set_batch(inp["px"], inp["ids"], torch.full((Bn,), ph), torch.full((Bn,), phv) if with_view else None, inp["vparams"])
    eng.set_noise(inp["eps"], inp["noise"], inp["t"])
    eng.set_loss_masks(inp["masks"])
    q = torch.stack([MR.weights_from_mask(m, 8, THR, bg) for m in inp["masks"]])
    torch.cuda.synchronize()
    check32(f"engine loss_weights {cfg_name} bg{bg}", eng.loss_weights, q,
            torch.stack([_weights_ref32(m, 8, bg) for m in inp["masks"]]))
    eng.forward_backward()
    torch.cuda.synchronize()
    loss_gpu, g_gpu = eng.loss(), (eng.grads / eng.scaler[0]).float().cpu()
    o = _oracle(cfg_name, with_view, Hh, Ww)
    ones = torch.ones(Bn, dtype=torch.float64)
    w = LR.min_snr_weight(AC, inp["t"], GAMMA, o["vpred"]) if snr_on else ones
    rel, cos, gerr = _bars(loss_gpu, g_gpu, *_oracle_loss_and_grad(o, q, w))
    plain = _bars(loss_gpu, g_gpu, *_oracle_loss_and_grad(o, torch.ones_like(q), ones))
    print(f"[masked step {cfg_name} snr={snr_on} bg={bg}] loss gpu {loss_gpu:.6f} rel {rel:.2e}; grad cos {cos:.6f} rel "
          f"{gerr:.2e}; against the plain objective: loss rel {plain[0]:.2e} cos {plain[1]:.6f} rel {plain[2]:.2e}")
    assert rel < 1e-3, "the masked loss must match the oracle to 1e-3 relative"
    assert cos > 0.999 and gerr < 5e-2
    assert not (plain[0] < 1e-3 and plain[1] > 0.999 and plain[2] < 5e-2), "the step passes with the mask ignored"


# ================================================================================================ engine behaviour
def _masks_for(step, full=False):
    if full:
        return torch.full((B, H, W), 255, dtype=torch.uint8)
    return torch.stack([MR.blocky_mask(H, W, 8, 100 + 10 * step + b) for b in range(B)])


def _feed_masked(cfg, eng, step, micro, mode3):
    _feed(cfg, eng, step, micro, mode3)
    eng.set_loss_masks(_masks_for(step))


def test_all_foreground_masks_are_the_plain_training():
    """captured steps; every weight is exactly 1, so parameters, AdamW moments and every other state tensor are the plain
    engine's after six steps; real masks change the training and nothing of the RNG"""
    plain, _, _ = _six_steps("one-mapper")
    cfg, eng = _build(False, 1, loss_mask=True, loss_mask_background=0.25)
    _feed(cfg, eng, 0, 0, False)
    eng.set_loss_masks(_masks_for(0, full=True))
    assert bool((eng.loss_weights == 1.0).all())
    eng.capture()
    run_steps(cfg, eng, range(6), False, _feed)
    got = snapshot(eng, STATE)
    for f in STATE:
        assert torch.equal(plain[f], got[f]), f"{f} differs with all-foreground masks"
    cfg, eng = _build(False, 1, loss_mask=True)
    _feed_masked(cfg, eng, 0, 0, False)
    eng.capture()
    run_steps(cfg, eng, range(6), False, _feed_masked)
    real = snapshot(eng, STATE)
    assert not torch.equal(plain["params"], real["params"]), "masks must change the training"
    for f in ("rng_state", "opt_step"):
        assert torch.equal(plain[f], real[f])
    assert eng.memory_bytes() > eng.unet.bytes + eng.vae.bytes + eng.text.bytes  # the table is counted


_ON = dict(loss_mask=True, loss_mask_background=0.25, snr_gamma=GAMMA)


@pytest.mark.parametrize("form", ["one-mapper", "mode3"])
def test_captured_replay_equals_eager_and_resumes(form):
    """the option on (with a background weight and Min-SNR): 3 eager steps == 3 replayed steps; state_dict after 3 -> a fresh
    engine -> 3 more == 6 in one run; a state is refused by an engine without the option and the reverse, naming the field"""
    mode3 = FORMS[form][0]
    cfg, eager = _build(mode3, 1, **_ON)
    for s in range(3):
        _feed_masked(cfg, eager, s, 0, mode3)
        assert eager.step_eager()
    _, graph = _build(mode3, 1, **_ON)
    _feed_masked(cfg, graph, 0, 0, mode3)
    graph.capture()
    assert graph.graph_a is not None
    run_steps(cfg, graph, range(3), mode3, _feed_masked)
    a, b = snapshot(eager, STATE), snapshot(graph, STATE)
    for f in STATE:
        assert torch.equal(a[f], b[f]), f"{form}: {f} differs between eager and replayed steps"
    assert eager.loss() == graph.loss()
    sd = graph.state_dict()
    assert sd["meta"]["loss_mask"] is True and sd["meta"]["loss_mask_background"] == 0.25 and "loss_weights" not in sd
    run_steps(cfg, graph, range(3, 6), mode3, _feed_masked)
    want = snapshot(graph, STATE)
    _, fresh = _build(mode3, 1, **_ON)
    fresh.load_state_dict(sd)
    _feed_masked(cfg, fresh, 3, 0, mode3)
    fresh.capture()
    run_steps(cfg, fresh, range(3, 6), mode3, _feed_masked)
    got = snapshot(fresh, STATE)
    for f in STATE:
        assert torch.equal(want[f], got[f]), f"{form}: {f} differs after the resume"
    if mode3:
        return
    for field, other in (("loss_mask", dict(snr_gamma=GAMMA)), ("loss_mask_background", dict(_ON, loss_mask_background=0.0)),
                         ("loss_mask_background", dict(_ON, loss_mask_background=0.5))):
        _, e = _build(False, 1, **other)
        with pytest.raises(ValueError, match=field) as err:
            e.load_state_dict(sd)
        assert "n_params" not in str(err.value)
        with pytest.raises(ValueError, match=field):
            fresh.load_state_dict(e.state_dict())
    _, plain = _build(False, 1)
    assert "loss_mask" not in plain.state_dict()["meta"] and "loss_mask_background" not in plain.state_dict()["meta"]
    assert plain.loss_weights is None and plain.memory_bytes() == plain.unet.bytes + plain.vae.bytes + plain.text.bytes


def test_constructor_and_set_loss_mask_refusals():
    for bad in (-0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="loss_mask_background"):
            _build(False, 1, loss_mask=True, loss_mask_background=bad)
    with pytest.raises(ValueError, match="loss_mask"):
        _build(False, 1, loss_mask_background=0.25)
    with pytest.raises(ValueError, match="loss_mask"):
        _build(False, 1, loss_mask=True, need_backward=False)
    _, plain = _build(False, 1)
    m = torch.zeros(H, W, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="loss_mask"):
        plain.set_loss_mask(0, m, H, W, 1)
    _, eng = _build(False, 1, loss_mask=True)
    with pytest.raises(ValueError, match="latent"):
        eng.set_loss_mask(0, torch.zeros(32, 64, dtype=torch.uint8, device=DEV), 32, 64, 1)
    with pytest.raises(ValueError, match="sample"):
        eng.set_loss_mask(B, m, H, W, 1)
    with pytest.raises(ValueError, match="uint8"):
        eng.set_loss_mask(0, m.float(), H, W, 1)
    with pytest.raises(ValueError, match="uint8"):
        eng.set_loss_mask(0, m, H, W, 3)  # too few bytes for stride 3
    eng.set_loss_mask(1, m + 255, H, W, 1)
    torch.cuda.synchronize()
    assert bool((eng.loss_weights == 1.0).all())


@pytest.mark.parametrize("form", ["one-mapper", "mode3"])
def test_launch_counts(form, monkeypatch):
    """an eager step's ABI calls: the option swaps the loss entry (and, with the record on, the per-sample entry) for its
    weighted sibling and adds none; off, the names are the ones they always were"""
    from view_neti_amd import lib
    mode3 = FORMS[form][0]

    def calls(**kw):
        cfg, eng = _build(mode3, 1, **kw)
        _feed(cfg, eng, 0, 0, mode3)
        if eng.loss_weights is not None:
            eng.set_loss_masks(_masks_for(0))
        names, orig = [], lib.call
        with monkeypatch.context() as m:
            m.setattr(lib, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
            assert eng.step()
        torch.cuda.synchronize()
        return names, len(eng.launches())

    def back(names):
        return [n.replace("mse_loss_grad_weighted", "mse_loss_grad").replace("mse_loss_per_sample_weighted", "mse_loss_per_sample")
                for n in names]

    plain, n_plain = calls()
    assert not any("weighted" in n or "loss_weights" in n for n in plain) and plain.count("mse_loss_grad") == 1
    on, n_on = calls(loss_mask=True)
    assert len(on) == len(plain) and n_on == n_plain and on.count("mse_loss_grad_weighted") == 1
    assert "mse_loss_grad" not in on and back(on) == plain
    snr, _ = calls(snr_gamma=GAMMA)
    both, _ = calls(loss_mask=True, snr_gamma=GAMMA)
    assert len(both) == len(snr) and "mse_loss_grad_snr" not in both
    assert back(both) == [n.replace("mse_loss_grad_snr", "mse_loss_grad") for n in snr]
    rec, _ = calls(telemetry_rows=ROWS)
    rec_on, _ = calls(telemetry_rows=ROWS, loss_mask=True)
    assert len(rec_on) == len(rec) and back(rec_on) == rec
    assert rec_on.count("mse_loss_per_sample_weighted") == 1 and "mse_loss_per_sample" not in rec_on


def test_eval_losses_stay_unmasked_and_weights_give_the_masked_ones():
    from view_neti_amd import synth
    cfg, plain = _build(False, 1)
    _, eng = _build(False, 1, telemetry_rows=ROWS, **_ON)
    assert torch.equal(plain.params, eng.params)
    h, w = H // 8, W // 8
    masks = _masks_for(7)
    eng.set_loss_masks(masks)
    q = torch.stack([MR.weights_from_mask(m, 8, THR, 0.25) for m in masks])
    losses = []
    for e in (plain, eng):
        feed_device_rng(cfg, e, 0, 0, False)
        ph = cfg.clip.vocab_size - 3
        e.set_batch(synth.pixel_values(B, H, W, seed=11), synth.input_ids(B, ph, cfg.clip.vocab_size),
                    torch.full((B,), ph), for_eval=True)
        e.set_noise(synth.gaussian((B, 4, h, w), 13), synth.gaussian((B, 4, h, w), 14), torch.tensor([40, 700]))
        losses.append((e.eval_losses(graph=False), e.eval_losses(graph=True)))
    assert torch.equal(losses[0][0], losses[1][0]) and torch.equal(losses[0][1], losses[1][1])
    assert torch.equal(losses[0][0], losses[0][1]) and float(losses[0][0].min()) > 0
    # weights=: the pair (unmasked, masked); on either engine, eager or replayed, the same bits
    for e in (plain, eng):
        for graph in (False, True):
            un, ma = e.eval_losses(graph=graph, weights=eng.loss_weights)
            assert torch.equal(un, losses[0][0])
            pr = e.unet.pred[:, :4].double().cpu().reshape(B, h * w, 4).permute(0, 2, 1)
            ref = MR.per_sample(pr, e.target.cpu().view(B, 4, h * w), eng.loss_weights.cpu())
            rel = ((ma.double() - ref).abs() / ref).max().item()
            rel_q = ((ma.double() - MR.per_sample(pr, e.target.cpu().view(B, 4, h * w), q)).abs() / ref).max().item()
            print(f"[eval masked graph={graph}] {ma.tolist()} ref {ref.tolist()} rel {rel:.2e} (restated weights: {rel_q:.2e})")
            assert rel <= 1e-5 and rel_q <= 2e-5 and not torch.equal(ma, un)
        one = e.eval_losses(weights=torch.ones_like(eng.loss_weights))
        assert torch.equal(one[1], one[0]), "weights of 1 give the unmasked losses bit for bit"
    with pytest.raises(ValueError, match="weights"):
        plain.eval_losses(weights=torch.ones(B, 3, device=DEV))
    # ---- the ring row of a training micro-step: the MASKED per-sample MSE of the step's own pred / target
    cfg, eng, _, _, _, _ = build_step("tiny", B, H, W, device_rng=False, lr=4e-3, telemetry_rows=ROWS, **_ON)
    inp = _step_inputs(cfg, False, H, W)
    eng.set_batch(inp["px"], inp["ids"], torch.full((B,), cfg.clip.vocab_size - 3))
    eng.set_noise(inp["eps"], inp["noise"], inp["t"])
    eng.set_loss_masks(inp["masks"])
    eng.forward_backward()
    direct, ws = torch.zeros(B, device=DEV), torch.zeros_like(eng.eval_ws)
    _ops().mse_loss_per_sample_weighted(eng.unet.pred, eng.target, eng.loss_weights, direct, ws, B, 4, h * w)
    torch.cuda.synchronize()
    t = eng.timesteps.cpu()
    eng.optimizer_step()
    (row,), lost = eng.read_telemetry()
    assert lost == 0 and row["timesteps"] == t.tolist() and row["losses"] == direct.cpu().tolist()
    wts = LR.min_snr_weight(AC, t, GAMMA)
    assert eng.loss() == pytest.approx((wts * direct.cpu().double()).mean().item(), rel=1e-5)  # the objective


# ================================================================================================ Coach
def _toy_masks(root, names, size, full=False):
    root.mkdir(parents=True)
    for n in names:
        m = np.full((size[1], size[0]), 255 if full else 0, dtype=np.uint8)
        m[:, : size[0] // 2] = 255  # the left half-plane is the object
        Image.fromarray(m).save(root / n)


def test_coach_runs_with_masks_on_host_and_device_paths(tmp_path):
    rt.toys(tmp_path / "toys")
    names = [f"{i}.png" for i in range(3)]
    _toy_masks(tmp_path / "half", names, (120, 90))
    _toy_masks(tmp_path / "full", names, (120, 90), full=True)
    ends = {}
    for name, extra in (("plain", ()), ("full", ("--data.mask_dir", str(tmp_path / "full"))),
                        ("host", ("--data.mask_dir", str(tmp_path / "half"), "--optim.loss_mask_background", "0.25")),
                        ("device", ("--data.mask_dir", str(tmp_path / "half"), "--optim.loss_mask_background", "0.25",
                                    "--data.device_input_pipeline", "true"))):
        cfg = rt.mode0_cfg(tmp_path / "toys", tmp_path / name, "--log.train_metrics", "true", *extra, max_steps=3)
        coach = rt.coach(cfg)
        assert (coach.engine.loss_weights is not None) == (name != "plain")
        assert rt.train_counting(coach) == 3
        ends[name] = rt.end_state(coach)
        lines = [json.loads(l) for l in (cfg.log.exp_dir / "train-metrics.jsonl").read_text().splitlines()]
        assert [l["step"] for l in lines] == [1, 2, 3]
        assert all(l.get("masked") is (True if name != "plain" else None) for l in lines)
        ck = torch.load(cfg.log.exp_dir / "mapper-steps-3_object.pt", map_location="cpu", weights_only=False)
        assert "mask_dir" not in ck["cfg"]["data"] and "loss_mask_background" not in ck["cfg"]["optim"]
        ext = ck["vneti_ext"]["config_ext"]
        assert ("data.mask_dir" in ext) == (name != "plain") and ("optim.loss_mask_background" in ext) == (name in ("host", "device"))
        if name in ("host", "device"):
            # the last batch's weights: the object is the left half-plane, and augmentation_key 5 crops at 0.95 - 1.05 of
            # the frame without rotation or flip, so the three left cell columns are all object, the three right ones none
            q = coach.engine.loss_weights.cpu().view(-1, 8, 8)
            assert abs(float(q.mean()) - 1) < 1e-5 and bool((q[:, :, :3] > 1.5).all()) and bool((q[:, :, 5:] < 0.5).all())
            assert bool((q[:, :, 5:] > 0.3).all()), "the background keeps its weight of 0.25 before the normalisation"
        if name == "host":
            state3 = cfg.log.exp_dir / "mapper-steps-3"
        del coach
    # all-foreground masks: every weight is 1, the run ends in the state of the run without the option.  (This shows that
    # weights of 1 change nothing; that the run WITHOUT data.mask_dir is the parent commit's is shown by the existing Coach
    # tests, which this change leaves untouched and which run the unset path: test_coach_gpu.py, test_resume_gpu.py)
    rt.assert_end(ends["plain"], ends["full"])
    assert not torch.equal(ends["plain"]["params"], ends["host"]["params"]), "the masks must change the training"
    # (the device path's pixels are within 2 LSB of the host's, test_coach_device_input_pipeline_matches_host: no bit
    # comparison of the two runs)
    assert not torch.equal(ends["plain"]["params"], ends["device"]["params"])
    # a state saved with the option is refused without it, and the reverse
    for extra, other in ((("--data.mask_dir", str(tmp_path / "half")), "loss_mask_background"), ((), "loss_mask")):
        cfg2 = rt.mode0_cfg(tmp_path / "toys", tmp_path / f"x{len(extra)}", "--model.mapper_checkpoint_path", str(state3), *extra)
        with pytest.raises(ValueError, match=other):
            rt.coach(cfg2)
    (tmp_path / "half" / "2.png").unlink()
    with pytest.raises(FileNotFoundError, match="2.png"):
        rt.coach(rt.mode0_cfg(tmp_path / "toys", tmp_path / "gone", "--data.mask_dir", str(tmp_path / "half")))


def test_coach_heldout_loss_masked_on_the_dtu_toy(tmp_path, monkeypatch):
    from view_neti_amd.compat import heldout as HL
    from view_neti_amd.compat.dtu_metrics import get_cam_idxs
    monkeypatch.chdir(tmp_path)
    (scan,) = rt.dtu_scene(tmp_path, ["scan114"])
    _toy_masks(tmp_path / "idr" / "scan114" / "mask", [f"{c:03d}.png" for c in range(49)], (160, 120))
    common = ("--optim.max_train_steps", "2", "--eval.heldout_loss_steps", "2", "--eval.heldout_loss_timesteps", "1",
              "--data.mask_dir", str(tmp_path / "idr"))
    on = rt.train_from_cfg(rt.mode2_cfg(scan, tmp_path / "out", "on", *common, "--eval.heldout_loss_masked", "true"))
    off = rt.train_from_cfg(rt.mode2_cfg(scan, tmp_path / "out", "off", *common))
    assert torch.equal(on.engine.params, off.engine.params), "the masked evaluation must not perturb training"
    (rec,) = HL.read_records(on.cfg.log.exp_dir / HL.FILE_NAME)
    (rec_off,) = HL.read_records(off.cfg.log.exp_dir / HL.FILE_NAME)
    o = rec["objects"]["<object>"]
    assert "loss_masked" not in rec_off["objects"]["<object>"]
    assert {k: v for k, v in o.items() if k != "loss_masked"} == rec_off["objects"]["<object>"], "the unmasked numbers moved"
    cams, _, _ = get_cam_idxs(3)
    m = o["loss_masked"]
    assert sorted(m["by_view_timestep"]) == sorted(cams) and all(list(d) == [500] for d in m["by_view_timestep"].values())
    vals = [d[500] for d in m["by_view_timestep"].values()] + [m["train"], m["test"]]
    assert all(isinstance(v, float) and math.isfinite(v) and v > 0 for v in vals)
    assert m["by_view"] != o["by_view"]
    with pytest.raises(ValueError, match="mask_dir"):
        rt.mode2_cfg(scan, tmp_path / "out", "bad", "--eval.heldout_loss_masked", "true")
