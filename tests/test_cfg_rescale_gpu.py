"""Guidance rescale on the GPU: vneti_cfg_rescale_factor and the scaled sampler step entries against the float64 restatement
(tests/helpers/cfg_rescale_ref.py), their bit-identity with the existing step entries at factor = 1, their argument checks
and memory contract, and `sd_pipeline_call(..., guidance_rescale=...)` / `timestep_spacing="trailing"` end to end on the
tiny synthetic SD configs.

Precision-generic like tests/test_ddim_eta_gpu.py: the 16-bit format is `lib.act_dtype()`, and the bf16 run of every case is
a child pytest process started by the last test of this file.

Inputs of the kernel cases: a 16-bit NHWC prediction of row stride 8 > Lc = 4, drawn as (randn + 3.0) * s[b] with
s = 0.1, 1, 10 over the samples — the offset makes an rms differ from the centred deviation, the scales make a statistic
shared by the batch differ from the per-sample one.

Bars.  The factor and the scaled step are f32 results with no 16-bit store between the shared inputs and them: the f32 bar
rule of helpers.checks.check32 (1e-5, or 8x the error of the same formulas evaluated in torch float32 on the CPU where that
is larger).  The end-to-end host loop uses the bar of tests/test_ddim_eta_gpu.py::
test_latents_after_three_steps_match_a_host_loop: 4x the error the EXISTING vneti_cfg_sampler_step makes against float64
on the same recorded UNet outputs.  Every case prints its figures before it asserts (the "[...]" lines); the measured
values are recorded in profiles/LAB_NOTES.md under "Guidance rescale".
"""
import os

import pytest
import torch

from helpers import cfg_rescale_ref as R
from helpers import slabs as S
from helpers.bf16_child import run_bf16_child
from helpers.checks import DEV, DT, check32, gen as _gen

pytestmark = pytest.mark.gpu

STEPS = 5          # the 5-step DDIM table on the SD scaled_linear betas: timesteps 801, 601, 401, 201, 1
LD = 8
SCALES = (0.1, 1.0, 10.0)
MARGIN = 4.0       # of the host-loop test (see the module docstring)
F32 = torch.float32


def _pred(B, Lc, HW, seed, ld=LD):
    """[2 B HW][ld] prediction in the 16-bit format: (randn + 3) * s[b], the same scale in both CFG halves of sample b"""
    g = _gen(seed)
    s = torch.tensor([SCALES[b % 3] for b in range(B)]).view(1, B, 1, 1)
    p = (torch.randn(2, B, HW, ld, generator=g) + 3.0) * s
    return p.view(2 * B * HW, ld).to(DT)


def _state(B, Lc, HW, seed):
    g = _gen(seed)
    return (torch.randn(B, Lc, HW, generator=g), torch.randn(B, Lc, HW, generator=g),
            torch.randn(STEPS, B, Lc, HW, generator=g))


def _factor(ops, pred_d, B, Lc, HW, gs, phi, ws=None, fill=float("nan")):
    f = torch.full((B,), fill, device=DEV)
    if ws is None:
        ws = torch.full((ops.cfg_rescale_ws_doubles(B, HW),), float("nan"), dtype=torch.float64, device=DEV)
    ops.cfg_rescale_factor(pred_d[:, :Lc], f, ws, B, Lc, HW, gs, phi)
    torch.cuda.synchronize()
    return f


def _refs(pred, B, Lc, HW, gs, phi):
    """(f64 factor, f32 factor, f64 guided e, f32 guided e) of the stored prediction"""
    u, c = R.unpack(pred, B, Lc, HW)
    return (R.rescale_factor(u, c, gs, phi), R.rescale_factor(u.float(), c.float(), gs, phi, dtype=F32),
            R.guided(u, c, gs), R.guided(u.float(), c.float(), gs, dtype=F32))


def _coef(eta, kind="ddim"):
    from view_neti_amd.engine.infer import coefficient_row, inference_timesteps
    from helpers.ddim_eta_ref import scaled_linear_alphas_cumprod
    ac = scaled_linear_alphas_cumprod()
    ts = inference_timesteps(kind, STEPS)
    return [coefficient_row(kind, ac, ts, i, eta) for i in range(STEPS)]


def _run(ops, form, pred_d, x, m, noise_d, factor_d, coef, i, B, Lc, HW, gs, vpred):
    """one launch; form: 'base' (vneti_cfg_sampler_step), 'noise' (…_noise), 'scalar' / 'table' (the scaled entries; noise_d
    None: no noise).  -> (x, m_prev, x_in) on the device"""
    xd, md = x.to(DEV).clone(), m.to(DEV).clone()
    x_in = torch.full((2 * B, Lc, HW), float("nan"), device=DEV)
    a_t, s_t, cx, c0, c1, cn = coef[i]
    p = pred_d[:, :Lc]
    if form == "base":
        ops.cfg_sampler_step(p, xd, md, x_in, B, Lc, HW, gs, a_t, s_t, cx, c0, c1, vpred)
    elif form == "noise":
        ops.cfg_sampler_step_noise(p, xd, md, x_in, noise_d[i], B, Lc, HW, gs, a_t, s_t, cx, c0, c1, cn, vpred)
    elif form == "scalar":
        ops.cfg_sampler_step_scaled(p, xd, md, x_in, None if noise_d is None else noise_d[i], factor_d, B, Lc, HW, gs,
                                    a_t, s_t, cx, c0, c1, cn, vpred)
    else:
        table = torch.tensor(coef, dtype=F32, device=DEV)
        step = torch.tensor([i], dtype=torch.int32, device=DEV)
        ops.cfg_sampler_step_scaled_table(p, xd, md, x_in, B, Lc, HW, gs, table, noise_d, factor_d, step, vpred)
    torch.cuda.synchronize()
    return xd, md, x_in


# ------------------------------------------------------------------------------------------ the factor
@pytest.mark.timeout(120)
@pytest.mark.parametrize("gs", [1.0, 7.5])
@pytest.mark.parametrize("HW", [7, 1001, 48 * 64])
@pytest.mark.parametrize("B", [1, 3])
def test_factor_matches_fp64(B, HW, gs):
    """one chunk with 7 pixels, a ragged last chunk (1001), several whole chunks (48 x 64); the 8-byte pixel loads (row
    stride 8, aligned) and the element loads (the same rows through a view that starts one element in: 2-byte aligned)"""
    from view_neti_amd import ops
    Lc = 4
    pred = _pred(B, Lc, HW, 17 * B + HW % 89)
    pred_d = pred.to(DEV)
    for phi in (0.3, 0.7, 1.0):
        f64, f32, _, _ = _refs(pred, B, Lc, HW, gs, phi)
        got = _factor(ops, pred_d, B, Lc, HW, gs, phi)
        check32(f"cfg rescale factor B{B} HW{HW} g{gs} phi{phi}", got, f64, f32)
        if gs == 1.0:
            assert (got.cpu() - 1.0).abs().max().item() < 1e-6  # e = c
        # the element path on the channels 1..4 of the same buffer
        u, c = R.unpack(pred[:, 1:], B, Lc, HW)
        e64, e32 = R.rescale_factor(u, c, gs, phi), R.rescale_factor(u.float(), c.float(), gs, phi, dtype=F32)
        f = torch.full((B,), float("nan"), device=DEV)
        ws = torch.empty(ops.cfg_rescale_ws_doubles(B, HW), dtype=torch.float64, device=DEV)
        ops.cfg_rescale_factor(pred_d[:, 1:1 + Lc], f, ws, B, Lc, HW, gs, phi)
        torch.cuda.synchronize()
        check32(f"cfg rescale factor, element loads B{B} HW{HW} g{gs} phi{phi}", f, e64, e32)


@pytest.mark.timeout(120)
def test_factor_other_channel_counts():
    """Lc = 3 and Lc = 5 take the element loop (row stride 8)"""
    from view_neti_amd import ops
    for Lc in (3, 5):
        B, HW, gs, phi = 2, 777, 7.5, 0.7
        pred = _pred(B, Lc, HW, 40 + Lc)
        f64, f32, _, _ = _refs(pred, B, Lc, HW, gs, phi)
        check32(f"cfg rescale factor Lc{Lc}", _factor(ops, pred.to(DEV), B, Lc, HW, gs, phi), f64, f32)


@pytest.mark.timeout(120)
def test_factor_constant_prediction_position_and_repeat():
    from view_neti_amd import ops
    Lc, gs, phi = 4, 7.5, 0.7
    for HW in (7, 1001, 48 * 64):
        # a constant prediction: the centred sum of squares of e is 0, the factor exactly 1.0f (diffusers: NaN)
        const = torch.full((2 * 2 * HW, LD), 0.3).to(DT)
        f =_factor(ops, const.to(DEV), 2, Lc, HW, gs, phi)
        assert torch.equal(f.cpu(), torch.ones(2)), f"HW{HW}: constant prediction gives {f.tolist()}"
        # sample data -> factor, wherever the sample sits: (B = 1, b = 0) against (B = 3, b = 2), bit for bit
        p3 = _pred(3, Lc, HW, 60 + HW % 7)
        rows = p3.view(2, 3, HW, LD)
        p1 = rows[:, 2].reshape(2 * HW, LD).contiguous()
        f3 = _factor(ops, p3.to(DEV), 3, Lc, HW, gs, phi).cpu()
        f1 = _factor(ops, p1.to(DEV), 1, Lc, HW, gs, phi).cpu()
        print(f"[cfg rescale factor HW{HW}] B3: {f3.tolist()}  B1 of its sample 2: {f1.tolist()}")
        assert torch.equal(f1.view(torch.int32), f3[2:].view(torch.int32)), "f[b] depends on Bn or on b"
        # two runs, the second over a dirty workspace and a dirty output
        again = _factor(ops, p3.to(DEV), 3, Lc, HW, gs, phi, fill=5.0).cpu()
        assert torch.equal(again.view(torch.int32), f3.view(torch.int32))


# ------------------------------------------------------------------------------------------ the scaled step
@pytest.mark.timeout(240)
@pytest.mark.parametrize("vpred", [False, True])
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("B,HW", [(3, 48 * 64), (2, 1001)])
def test_scaled_step_matches_fp64(B, HW, eta, vpred):
    """factor launch + scaled step (scalar and table form) against the float64 chain; x, m_prev and both halves of x_in.
    eta = 0 runs with a null noise pointer (the cn column of the rows is 0 as well), eta = 0.5 with the noise table"""
    from view_neti_amd import ops
    Lc, gs, phi = 4, 7.5, 0.7
    pred = _pred(B, Lc, HW, 200 + HW % 97 + int(vpred))
    x, m, noise = _state(B, Lc, HW, 300 + B)
    pred_d = pred.to(DEV)
    noise_d = noise.to(DEV) if eta else None
    f64, f32, e64, e32 = _refs(pred, B, Lc, HW, gs, phi)
    factor_d = _factor(ops, pred_d, B, Lc, HW, gs, phi)
    coef = _coef(eta)
    assert all((row[5] > 0) == (eta > 0) for row in coef)
    for i in (0, 2, 4):
        nz = noise[i] if eta else None
        ref_x, ref_x0 = R.sampler_step(x, e64, m, coef[i], nz, vpred, factor=f64)
        r32_x, r32_x0 = R.sampler_step(x, e32, m, coef[i], nz, vpred, factor=f32, dtype=F32)
        plain_x, _ = R.sampler_step(x, e64, m, coef[i], nz, vpred)
        assert ((plain_x - ref_x).norm() / ref_x.norm()).item() > 1e-2, "the rescale must matter in this case"
        for form in ("scalar", "table"):
            gx, gm, gin = _run(ops, form, pred_d, x, m, noise_d, factor_d, coef, i, B, Lc, HW, gs, vpred)
            tag = f"cfg scaled step {form} B{B} HW{HW} eta{eta} vpred{int(vpred)} step{i}"
            check32(f"{tag} x", gx, ref_x, r32_x)
            check32(f"{tag} m_prev", gm, ref_x0, r32_x0)
            check32(f"{tag} x_in[:B]", gin[:B], ref_x, r32_x)
            check32(f"{tag} x_in[B:]", gin[B:], ref_x, r32_x)
            assert torch.equal(gin[:B], gx) and torch.equal(gin[B:], gx)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("vpred", [False, True])
@pytest.mark.parametrize("B,HW", [(2, 48 * 64), (2, 1001), (3, 7)])
def test_factor_one_is_the_existing_entries_bit_for_bit(B, HW, vpred):
    """factor = 1.0f: with noise the x, m_prev and x_in of vneti_cfg_sampler_step_noise (eta = 0.5 rows, and cn = 0 rows
    whatever the noise buffer holds); with a null noise those of vneti_cfg_sampler_step; DDIM rows and rows with a history
    term (c1 != 0); the 16-byte path (HW = 48 x 64) and the element path (1001, 7)"""
    from view_neti_amd import ops
    Lc = 4
    pred = _pred(B, Lc, HW, 400 + HW % 13)
    x, m, noise = _state(B, Lc, HW, 500 + HW % 13)
    pred_d, noise_d = pred.to(DEV), noise.to(DEV)
    ones = torch.ones(B, device=DEV)
    history = [(0.8366, 0.5478, 0.6547, 1.3093, -0.4364, 0.0), (0.2512, 0.9679, 1.7, -0.83, 0.291, 0.25)] + \
        [(0.5, 0.5, 1.0, 0.5, 0.1, 0.0)] * (STEPS - 2)
    for coef, steps in ((_coef(0.5), (0, 2, 4)), (_coef(0.0), (0, 4)), (history, (0, 1))):
        for gs in (1.0, 7.5):
            for i in steps:
                with_noise = _run(ops, "noise", pred_d, x, m, noise_d, None, coef, i, B, Lc, HW, gs, vpred)
                no_noise = _run(ops, "base", pred_d, x, m, None, None, coef, i, B, Lc, HW, gs, vpred)
                assert bool(torch.isfinite(with_noise[2]).all())
                for form in ("scalar", "table"):
                    for want, nd, what in ((with_noise, noise_d, "vneti_cfg_sampler_step_noise"),
                                           (no_noise, None, "vneti_cfg_sampler_step")):
                        got = _run(ops, form, pred_d, x, m, nd, ones, coef, i, B, Lc, HW, gs, vpred)
                        for name, a, b in zip(("x", "m_prev", "x_in"), got, want):
                            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                                f"{form} B{B} HW{HW} g{gs} row{i}: {name} differs from {what} at factor 1"


@pytest.mark.timeout(60)
def test_table_form_reads_row_step_of_both_tables():
    from view_neti_amd import ops
    B, Lc, HW, gs = 2, 4, 1000, 7.5
    pred = _pred(B, Lc, HW, 31)
    x, m, noise = _state(B, Lc, HW, 32)
    pred_d, noise_d = pred.to(DEV), noise.to(DEV)
    factor_d = _factor(ops, pred_d, B, Lc, HW, gs, 0.7)
    coef = _coef(1.0)
    seen = []
    for i in range(STEPS):
        s = _run(ops, "scalar", pred_d, x, m, noise_d, factor_d, coef, i, B, Lc, HW, gs, True)
        t = _run(ops, "table", pred_d, x, m, noise_d, factor_d, coef, i, B, Lc, HW, gs, True)
        assert all(torch.equal(a, b) for a, b in zip(s, t))
        seen.append(s[0].cpu())
    assert all(not torch.equal(seen[i], seen[j]) for i in range(STEPS) for j in range(i))


# ------------------------------------------------------------------------------------------ launchers
@pytest.mark.timeout(60)
def test_launchers_refuse_bad_arguments():
    """null pointers, non-positive sizes, a row stride below Lc and the 2 GiB buffer-store bound: a negative return code
    with a message (RuntimeError through the binding), before any launch — the small buffers below are never touched"""
    from view_neti_amd import ops
    B, Lc, HW = 1, 4, 64
    pred = torch.zeros(2 * B * HW, 8, dtype=DT, device=DEV)
    narrow = torch.zeros(2 * B * HW, 2, dtype=DT, device=DEV)  # row stride 2 < Lc
    x, m = torch.zeros(B, Lc, HW, device=DEV), torch.zeros(B, Lc, HW, device=DEV)
    x_in, nz = torch.zeros(2 * B, Lc, HW, device=DEV), torch.zeros(2, B, Lc, HW, device=DEV)
    table, step = torch.zeros(2, 6, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    table[:, 0] = 0.8
    f = torch.ones(B, device=DEV)
    ws = torch.zeros(ops.cfg_rescale_ws_doubles(B, HW), dtype=torch.float64, device=DEV)
    p = pred[:, :Lc]
    sc = (1.0, 0.8, 0.6, 0.9, 0.1, 0.0, 0.2, False)
    # the well-formed calls pass
    ops.cfg_rescale_factor(p, f, ws, B, Lc, HW, 7.5, 0.7)
    ops.cfg_sampler_step_scaled(p, x, m, x_in, nz[0], f, B, Lc, HW, *sc)
    ops.cfg_sampler_step_scaled(p, x, m, x_in, None, f, B, Lc, HW, *sc)
    ops.cfg_sampler_step_scaled_table(p, x, m, x_in, B, Lc, HW, 1.0, table, nz, f, step, False)
    ops.cfg_sampler_step_scaled_table(p, x, m, x_in, B, Lc, HW, 1.0, table, None, f, step, False)
    torch.cuda.synchronize()
    for kw in (dict(pred=None), dict(f=None), dict(ws=None)):
        a = dict(pred=p, f=f, ws=ws)
        a.update(kw)
        with pytest.raises(RuntimeError, match="null pointer"):
            ops.cfg_rescale_factor(a["pred"], a["f"], a["ws"], B, Lc, HW, 7.5, 0.7)
    for kw in (dict(B=0), dict(B=-1), dict(Lc=0), dict(HW=0), dict(pred=narrow)):
        a = dict(pred=p, B=B, Lc=Lc, HW=HW)
        a.update(kw)
        with pytest.raises(RuntimeError, match="bad shape"):
            ops.cfg_rescale_factor(a["pred"], f, ws, a["B"], a["Lc"], a["HW"], 7.5, 0.7)
    for bad in (-0.1, 1.5):
        with pytest.raises(RuntimeError, match="outside"):
            ops.cfg_rescale_factor(p, f, ws, B, Lc, HW, 7.5, bad)
    assert ops.cfg_rescale_ws_doubles(3, 1001) == 3 * ops.cfg_rescale_ws_doubles(1, 1001)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.cfg_rescale_ws_doubles(0, 64)
    bad = [dict(pred=None), dict(x=None), dict(m=None), dict(x_in=None), dict(f=None), dict(B=0), dict(Lc=0), dict(HW=-4),
           dict(pred=narrow)]
    for kw in bad:
        a = dict(pred=p, x=x, m=m, x_in=x_in, f=f, B=B, Lc=Lc, HW=HW)
        a.update(kw)
        with pytest.raises(RuntimeError, match="bad arguments"):
            ops.cfg_sampler_step_scaled(a["pred"], a["x"], a["m"], a["x_in"], nz[0], a["f"], a["B"], a["Lc"], a["HW"], *sc)
        if "m" in kw or "x" in kw:
            continue
        with pytest.raises(RuntimeError, match="bad arguments"):
            ops.cfg_sampler_step_scaled_table(a["pred"], x, m, a["x_in"], a["B"], a["Lc"], a["HW"], 1.0, table, nz, a["f"],
                                              step, False)
    with pytest.raises(RuntimeError, match="bad arguments"):  # alpha_t = 0 divides
        ops.cfg_sampler_step_scaled(p, x, m, x_in, nz[0], f, B, Lc, HW, 1.0, 0.0, 0.6, 0.9, 0.1, 0.0, 0.2, False)
    for kw in (dict(table=None), dict(step=None)):
        a = dict(table=table, step=step)
        a.update(kw)
        with pytest.raises(RuntimeError, match="bad arguments"):
            ops.cfg_sampler_step_scaled_table(p, x, m, x_in, B, Lc, HW, 1.0, a["table"], nz, f, a["step"], False)
    # x_in = 2 B Lc HW 4 bytes = 2 GiB: out of the buffer stores' range
    with pytest.raises(RuntimeError, match="2 GiB"):
        ops.cfg_sampler_step_scaled(p, x, m, x_in, nz[0], f, 1 << 13, 4, 1 << 13, *sc)
    with pytest.raises(RuntimeError, match="2 GiB"):
        ops.cfg_sampler_step_scaled_table(p, x, m, x_in, 1 << 13, 4, 1 << 13, 1.0, table, None, f, step, False)
    with pytest.raises(RuntimeError, match="2 GiB"):  # one noise row alone
        ops.cfg_sampler_step_scaled_table(p, x, m, x_in, 1 << 14, 4, 1 << 13, 1.0, table, nz, f, step, False)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ memory contract
def _vec_slab(values, dtype=None):
    """a contiguous operand (the ABI gives it no row stride) between front and back guards"""
    v = values.reshape(1, -1)
    s = S.Slab.matrix(1, v.shape[1], dtype or v.dtype, gap=0, device=DEV)
    return s


@pytest.mark.timeout(120)
@pytest.mark.parametrize("Lc,HW", [(4, 1000), (3, 1001)])  # 8-byte pixel loads + 16-byte step path | element paths
def test_memory_contract(Lc, HW):
    """the factor entry and the scaled step in guarded slabs (tests/helpers/slabs.py), three launches as in
    tests/test_kernel_contracts_gpu.py: clean; poisoned (NaN around every input, sentinel NaN through every output, NaN
    through the workspace); replayed on the poisoned run's buffers.  All three give the same bits in factor, the workspace,
    x, m_prev and x_in; nothing outside the logical extents is written; no input changes."""
    from view_neti_amd import ops
    B, gs, phi = 2, 7.5, 0.7
    pred = _pred(B, Lc, HW, 70 + Lc)[:, :Lc].contiguous()
    x, m, noise = _state(B, Lc, HW, 80 + Lc)
    row = _coef(0.5)[2]
    sp = S.Slab.matrix(2 * B * HW, Lc, DT, gap=8, device=DEV)           # row stride Lc + 8
    sn = _vec_slab(noise[2])
    sx, sm = _vec_slab(x), _vec_slab(m)                                  # in place
    sin_, sf = _vec_slab(torch.zeros(2 * B * Lc * HW)), _vec_slab(torch.zeros(B))
    n_ws = ops.cfg_rescale_ws_doubles(B, HW)
    sw = S.Slab.matrix(1, n_ws, torch.float64, gap=0, device=DEV)
    ins, inplace, outs = [(sp, pred), (sn, noise[2])], [(sx, x), (sm, m)], [sin_, sf]
    SENT64 = 0x7FF8A5A5A5A5A5A5

    def call():
        ops.cfg_rescale_factor(sp.view, sf.view.view(-1), sw.view.view(-1), B, Lc, HW, gs, phi)
        ops.cfg_sampler_step_scaled(sp.view, sx.view.view(B, Lc, HW), sm.view.view(B, Lc, HW),
                                    sin_.view.view(2 * B, Lc, HW), sn.view.view(B, Lc, HW), sf.view.view(-1), B, Lc, HW, gs,
                                    *row, True)
        torch.cuda.synchronize()

    def results():
        return [(s, s.logical_bits()) for s in (sf, sw, sx, sm, sin_)]

    # ---- A: clean
    for s, v in ins + inplace:
        s.fill_all(0)
        s.fill_logical(v)
    for s in outs + [sw]:
        s.fill_all(0)
    call()
    a = results()
    # ---- B: poisoned
    for s, _ in ins:
        s.fill_outside(S.QNAN[s.dtype])
    for s in outs:
        s.fill_all(S.SENTINEL[s.dtype])
    for s, v in inplace:
        s.fill_all(S.SENTINEL[s.dtype])
        s.fill_logical(v)
    sw.fill_all(SENT64)
    snaps = [s.snapshot() for s, _ in ins]

    def contract(run):
        for s in outs + [s for s, _ in inplace]:
            s.outside_intact(S.SENTINEL[s.dtype], f"run {run}")
        for s in outs:
            s.logical_has_no_sentinel(S.SENTINEL[s.dtype], f"run {run}")
        sw.outside_intact(SENT64, f"ws, run {run}")
        sw.logical_has_no_sentinel(SENT64, f"ws, run {run}")
        for (s, _), snap in zip(ins, snaps):
            s.unchanged(snap, f"input, run {run}")

    call()
    contract("B")
    b = results()
    f64, f32, e64, e32 = _refs(pred, B, Lc, HW, gs, phi)
    check32(f"contract cfg rescale factor Lc{Lc}", sf.view.view(-1), f64, f32)
    ref_x, ref_x0 = R.sampler_step(x, e64, m, row, noise[2], True, factor=f64)
    r32_x, r32_x0 = R.sampler_step(x, e32, m, row, noise[2], True, factor=f32, dtype=F32)
    check32(f"contract cfg scaled step Lc{Lc} x", sx.view.view(B, Lc, HW), ref_x, r32_x)
    check32(f"contract cfg scaled step Lc{Lc} m_prev", sm.view.view(B, Lc, HW), ref_x0, r32_x0)
    for (s, p), (_, q) in zip(a, b):
        S.first_difference(p, q, s, "run B (poisoned) differs from run A (clean)")
    # ---- C: replay on B's buffers (the in-place operands copied in again)
    for s, v in inplace:
        s.fill_logical(v)
    call()
    contract("C")
    for (s, p), (_, q) in zip(b, results()):
        S.first_difference(p, q, s, "run C (replay) differs from run B")


# ------------------------------------------------------------------------------------------ end to end
_engines = {}


def _pipeline(cfg_name, B):
    """InferencePipeline on a tiny synthetic SD config (object + view mapper), one per (config, batch) and process"""
    if (cfg_name, B) in _engines:
        return _engines[(cfg_name, B)]
    from view_neti_amd import sd_config as sc, synth
    from view_neti_amd.compat.prompt_manager import PromptEmbeds
    from view_neti_amd.compat.sd_pipeline_call import InferencePipeline
    from view_neti_amd.compat.tokenizer import HashTokenizer
    from view_neti_amd.engine.infer import InferenceEngine
    from view_neti_amd.mapper import fourier_frequencies, init_mapper_state
    cfg = sc.CONFIGS[cfg_name]()
    D = cfg.clip.hidden_size
    uw, dw, cw = synth.unet_weights(cfg.unet), synth.vae_decoder_weights(cfg.vae), synth.clip_weights(cfg.clip)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(9)
        gen = torch.Generator().manual_seed(9)
        mk = lambda: {k: v + 0.05 * torch.randn(v.shape, generator=gen) for k, v in init_mapper_state(64, 64, D).items()}
        sdo, sdv = mk(), mk()
    w_enc = fourier_frequencies([0.03, 2.0], 64, 0)
    w_enc_v = fourier_frequencies([0.03, 2.0] + [0.5] * 12, 64, 0)
    eng = InferenceEngine(cfg, uw, dw, cw, B, 64, 64, sdo, w_enc, 0.4, 0.2, mapper_view=sdv, w_enc_view=w_enc_v,
                          norm_scale_view=0.35, alpha_view=0.3)
    ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
    ids = synth.input_ids(1, ph, cfg.clip.vocab_size, view_placeholder_id=phv)
    emb = PromptEmbeds("synthetic", ids, torch.tensor([ph]), torch.tensor([phv]), synth.gaussian((1, 12), 9).clamp(-1, 1),
                       None, B)
    pipe = InferencePipeline(eng, HashTokenizer(cfg.clip.vocab_size), sampler="ddim")
    _engines[(cfg_name, B)] = (cfg, pipe, emb)
    return _engines[(cfg_name, B)]


def _errs(got, ref64):
    d = got.double().cpu() - ref64
    return (d.norm() / ref64.norm()).item(), d.abs().max().item()


def _set_prompt(pipe, emb, B):
    from view_neti_amd.compat.sd_pipeline_call import get_neg_prompt_input_ids
    eng = pipe.engine
    eng.set_negative_prompt(get_neg_prompt_input_ids(pipe).input_ids)
    rep = lambda t: t.expand(B, *t.shape[1:]) if t.dim() > 1 else t.expand(B)
    eng.set_prompt(rep(emb.input_ids), rep(emb.input_ids_placeholder_object), rep(emb.input_ids_placeholder_view),
                   rep(emb.view_params))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind,eta", [("ddim", 0.0), ("ddim", 0.5), ("dpm++2m", 0.0)])
@pytest.mark.parametrize("cfg_name", ["tiny", "tiny21"])  # epsilon / v-prediction
def test_three_steps_match_a_host_loop(cfg_name, kind, eta, monkeypatch):
    """the engine's eager loop at guidance_rescale = 0.7 with its UNet output recorded at each step; a float64 host loop (the
    helper's factor and step formulas on the recorded outputs) must land on the engine's final latents within 4x the error
    of the EXISTING vneti_cfg_sampler_step against the float64 loop without rescale on the same outputs.  The captured step
    equals the eager loop bit for bit, and sd_pipeline_call runs that same captured step."""
    from view_neti_amd import ops
    from view_neti_amd.compat.sd_pipeline_call import InferencePipeline, sd_pipeline_call
    from view_neti_amd.engine.infer import coefficient_row, inference_timesteps
    cfg, pipe, emb = _pipeline(cfg_name, 2)
    eng = pipe.engine
    B, Lc, h, w, steps, gs, phi = 2, eng.Lc, eng.h, eng.w, 3, 5.0, 0.7
    HW = h * w
    vpred = cfg.ddpm.prediction_type == "v_prediction"
    g = _gen(21)
    lat = torch.randn(B, Lc, h, w, generator=g)
    noise = torch.stack([torch.randn(B, Lc, h, w, generator=g) for _ in range(steps)])
    kw = dict(eta=eta, step_noise=noise) if eta else {}
    _set_prompt(pipe, emb, B)
    preds, factors, real = [], [], ops.cfg_sampler_step_scaled

    def recording(pred, x, m, x_in, nz, factor, *a):
        preds.append(pred.clone())
        factors.append(factor.clone())
        return real(pred, x, m, x_in, nz, factor, *a)

    monkeypatch.setattr(ops, "cfg_sampler_step_scaled", recording)
    eng.generate(lat.to(DEV), steps, gs, kind, decode=False, use_graph=False, guidance_rescale=phi, **kw)
    monkeypatch.undo()
    x_eager = eng.x.cpu().clone()
    assert len(preds) == steps and bool(torch.isfinite(x_eager).all())
    eng.generate(lat.to(DEV), steps, gs, kind, decode=False, guidance_rescale=phi, **kw)
    assert torch.equal(eng.x.cpu(), x_eager), "graph replay of the rescaled step must match the eager loop bit for bit"
    assert (gs, vpred, eta > 0, phi) in eng._graphs
    ac = eng.ac.double().cpu()
    ts = inference_timesteps(kind, steps, cfg.ddpm.num_train_timesteps)
    x1 = lat.double().view(B, Lc, HW)
    m1 = torch.zeros_like(x1)
    xb, mb = x1.clone(), m1.clone()
    bx, bm = lat.view(B, Lc, HW).to(DEV).clone(), torch.zeros(B, Lc, HW, device=DEV)
    b_in = torch.zeros(2 * B, Lc, HW, device=DEV)
    for i in range(steps):
        u, c = R.unpack(preds[i], B, Lc, HW)
        e = R.guided(u, c, gs)
        f = R.rescale_factor(u, c, gs, phi)
        print(f"[cfg rescale host loop {cfg_name} {kind} eta{eta} step{i}] factor {factors[i].tolist()} (float64 {f.tolist()})")
        x1, m1 = R.sampler_step(x1, e, m1, coefficient_row(kind, ac, ts, i, eta), noise[i].view(B, Lc, HW), vpred, factor=f)
        row0 = coefficient_row(kind, ac, ts, i, 0.0)
        xb, mb = R.sampler_step(xb, e, mb, row0, None, vpred)
        ops.cfg_sampler_step(preds[i], bx, bm, b_in, B, Lc, HW, gs, *row0[:5], vpred)
    torch.cuda.synchronize()
    base = _errs(bx, xb)
    got = _errs(x_eager.view(B, Lc, HW), x1)
    print(f"[cfg rescale host loop {cfg_name} {kind} eta{eta}] final latents vs fp64 after {steps} steps: rel {got[0]:.3e} "
          f"max {got[1]:.3e}; existing kernel, no rescale, same outputs: rel {base[0]:.3e} max {base[1]:.3e}")
    assert 0 < base[0] < 1e-4
    assert got[0] <= MARGIN * base[0] and got[1] <= MARGIN * base[1]
    # sd_pipeline_call: the same draws (latents, then one noise draw per step) through the same captured step
    p2 = InferencePipeline(eng, pipe.tokenizer, sampler=kind)
    out = sd_pipeline_call(p2, emb, num_inference_steps=steps, guidance_scale=gs, num_images_per_prompt=B, eta=eta,
                           generator=_gen(21), output_type="latent", guidance_rescale=phi).images.cpu()
    assert torch.equal(out, x_eager)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cfg_name", ["tiny", "tiny21"])
def test_off_is_bit_identical_and_graphs_are_keyed_by_phi(cfg_name):
    from view_neti_amd.compat.sd_pipeline_call import sd_pipeline_call
    cfg, pipe, emb = _pipeline(cfg_name, 2)
    eng = pipe.engine
    vpred = cfg.ddpm.prediction_type == "v_prediction"
    B, steps, gs = 2, 3, 5.0
    call = lambda **kw: sd_pipeline_call(pipe, emb, num_inference_steps=steps, guidance_scale=gs, num_images_per_prompt=B,
                                         generator=_gen(3), output_type="latent", **kw).images.cpu()
    plain = call()
    keys = set(eng._graphs)
    assert (gs, vpred, False) in keys
    assert torch.equal(call(guidance_rescale=0.0), plain) and set(eng._graphs) == keys  # no new capture, the same bits
    a = call(guidance_rescale=0.7)
    assert (gs, vpred, False, 0.7) in eng._graphs and (gs, vpred, False) in eng._graphs
    assert eng.memory_bytes() == eng.unet.bytes + eng.text.bytes + eng.decoder.bytes + \
        (0 if eng.noise_table is None else eng.noise_table.numel() * 4) + eng.rescale_factor.numel() * 4 + \
        eng.rescale_ws.numel() * 8
    b = call(guidance_rescale=0.3)
    assert (gs, vpred, False, 0.3) in eng._graphs and (gs, vpred, False, 0.7) not in eng._graphs
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert not torch.equal(a, b) and not torch.equal(a, plain) and not torch.equal(b, plain)
    assert torch.equal(call(guidance_rescale=0.7), a), "phi = 0.7 after 0.3: its own graph again, the same bits"
    assert torch.equal(call(), plain)
    # the eager loop of the reference's prompt_embeds contract (a tensor) takes the argument too
    ctx = torch.randn(B, eng.L, cfg.clip.hidden_size, generator=_gen(5)) * 0.3
    c0 = sd_pipeline_call(pipe, ctx, num_inference_steps=steps, guidance_scale=gs, num_images_per_prompt=B,
                          generator=_gen(3), output_type="latent").images.cpu()
    c7 = sd_pipeline_call(pipe, ctx, num_inference_steps=steps, guidance_scale=gs, num_images_per_prompt=B,
                          generator=_gen(3), output_type="latent", guidance_rescale=0.7).images.cpu()
    assert bool(torch.isfinite(c7).all()) and not torch.equal(c0, c7)
    with pytest.raises(ValueError, match="guidance_rescale"):
        call(guidance_rescale=1.2)
    with pytest.raises(ValueError, match="guidance_rescale"):
        eng.generate(torch.zeros(B, 4, 8, 8, device=DEV), steps, gs, "ddim", guidance_rescale=-0.1)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["ddim", "dpm++2m"])
def test_trailing_spacing_fills_the_timestep_table(kind):
    from view_neti_amd.compat.sd_pipeline_call import InferencePipeline, sd_pipeline_call
    from view_neti_amd.engine.infer import inference_timesteps
    cfg, pipe, emb = _pipeline("tiny21", 2)
    eng = pipe.engine
    steps = 3
    want = inference_timesteps(kind, steps, cfg.ddpm.num_train_timesteps, "trailing")
    assert want == [999, 666, 332]
    outs = {}
    for spacing in (None, "trailing"):
        p = InferencePipeline(eng, pipe.tokenizer, sampler=kind, timestep_spacing=spacing)
        outs[spacing] = sd_pipeline_call(p, emb, num_inference_steps=steps, guidance_scale=5.0, num_images_per_prompt=2,
                                         generator=_gen(3), output_type="latent", guidance_rescale=0.7).images.cpu()
        ts = inference_timesteps(kind, steps, cfg.ddpm.num_train_timesteps, spacing)
        assert eng.ts_table[:steps].cpu().tolist() == ts and int(eng.step_idx.item()) == steps
        assert bool(torch.isfinite(outs[spacing]).all())
    assert not torch.equal(outs[None], outs["trailing"])
    with pytest.raises(ValueError, match="timestep_spacing"):
        sd_pipeline_call(InferencePipeline(eng, pipe.tokenizer, sampler=kind, timestep_spacing="leading"), emb,
                         num_inference_steps=steps, guidance_scale=5.0, num_images_per_prompt=2, generator=_gen(3))


# ------------------------------------------------------------------------------------------ the bf16 library
@pytest.mark.timeout(300)
def test_every_case_against_the_bf16_library(tmp_path):
    """the cases above in a child process with VNETI_PRECISION=bf16 (libvneti_hip_bf16.so); one child, under its own time
    limit, nothing retried"""
    out = run_bf16_child(os.path.join("tests", os.path.basename(__file__)), "not bf16_library", 170, tmp_path, least=40,
                         extra_args=("-s",), collect_limit=120, what="cfg rescale bf16")
    print("\n".join(l for l in out.splitlines() if l.startswith("[")))
