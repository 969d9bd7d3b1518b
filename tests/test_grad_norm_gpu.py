"""Direct tests of the gradient-norm / clipping / per-step-record kernels (csrc/elementwise.hip)
through the C ABI: vneti_grad_sumsq + vneti_grad_norm_finish, vneti_adamw_flat_clipped / vneti_adamw_segments_clipped and
vneti_train_record.

References.  The norm: torch.linalg.vector_norm of the float64 gradient.  Clipped AdamW: the real torch.optim.AdamW on
float64 CPU parameters with torch.nn.utils.clip_grad_norm_ before every step.  Bars: `check32` of tests/helpers/checks.py
(1e-5 unless 8 x the error of the same computation in torch float32 is larger); nothing comes from a kernel's output.  The
kernels are f32 / f64 only, so one bar holds in both builds; `test_bf16_library_runs_this_file` runs every case against
libvneti_hip_bf16.so in a child process, as tests/test_kernels_bf16_gpu.py does for the other kernel files."""
import math
import os

import pytest
import torch

from helpers import slabs as S
from helpers.adamw_ref import ACTIVITY, N_FLAT, N_SEG, SEG_LEN, hyper_dev, i32, spread_gradients, torch_adamw
from helpers.bf16_child import run_bf16_child
from helpers.checks import DEV, check32
from helpers.checks import gen as _gen, ops as _ops

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
C = 4096          # the chunk of vneti_grad_sumsq's fixed partition (asserted below through the workspace query)
SCALE = 65536.0   # the loss scale of the inputs: a power of two, so scaling is exact
QNAN64 = 0x7FF8000000000000
SENT64 = 0x7FF8A5A5A5A5A5A5


def _dev(x, dtype=F32):
    return torch.tensor(x, dtype=dtype, device=DEV)


def _offset_copy(g, off):
    """g on the device at a base pointer `off` floats past a 16-byte aligned one"""
    buf = torch.zeros(g.numel() + 8, dtype=F32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + g.numel()]
    v.copy_(g)
    return v


def norm_launch(obj=None, view=None, seg_len=None, active=None, scale=SCALE, gdiv=1.0, max_norm=0.0, scaler=None,
                hyper=None, ring=None, count=None, rows=0, row_floats=0):
    """sumsq of the object side (flat, or the `active` segments) and the view side (flat), then the finish -> out (device)"""
    ops = _ops()
    out = torch.full((ops.NORM_OUT_FLOATS,), 7.0, device=DEV)
    ws = [None, None]
    n = [0, 0]
    if obj is not None:
        n[0] = ops.grad_sumsq_ws_doubles(seg_len, active.numel()) if active is not None else ops.grad_sumsq_ws_doubles(obj.numel())
        ws[0] = torch.full((n[0],), math.nan, dtype=F64, device=DEV)
        ops.grad_sumsq(obj, ws[0], seg_len=seg_len, active=active)
    if view is not None:
        n[1] = ops.grad_sumsq_ws_doubles(view.numel())
        ws[1] = torch.full((n[1],), math.nan, dtype=F64, device=DEV)
        ops.grad_sumsq(view, ws[1])
    scaler = _dev([scale, 0.0, 0.0]) if scaler is None else scaler
    hyper = hyper_dev(1e-3, 0.0, gdiv) if hyper is None else hyper
    ops.grad_norm_finish(ws[0], n[0], ws[1], n[1], scaler, hyper, _dev([max_norm]), out, ring, count, rows, row_floats)
    return out


def check_norm(name, got, g, div):
    ref64 = (torch.linalg.vector_norm(g.double()) / div).reshape(1)
    ref32 = (torch.linalg.vector_norm(g.float()) / torch.tensor(div, dtype=F32)).reshape(1)
    check32(name, got.reshape(1), ref64, ref32)


def test_chunk_is_what_the_cases_assume():
    ops = _ops()
    assert ops.grad_sumsq_ws_doubles(C) == 1 and ops.grad_sumsq_ws_doubles(C + 1) == 2
    assert ops.grad_sumsq_ws_doubles(3 * C + 5) == 4 and ops.grad_sumsq_ws_doubles(1031, 2) == 2
    with pytest.raises(RuntimeError):
        ops.grad_sumsq_ws_doubles(0)


@pytest.mark.parametrize("n", [1, 255, 256, 257, C - 1, C, C + 1, 3 * C + 5])
def test_grad_sumsq_flat_against_float64(n):
    """one flat range at base pointers 0..3 floats past 16-byte alignment, as the object side, as the view side, and split
    between the two; gdiv 1 and 8"""
    ops = _ops()
    g = spread_gradients(n, 1, 100 + n % 97)[0] * SCALE
    for off in (0, 1, 2, 3):
        gd = _offset_copy(g, off)
        assert gd.data_ptr() % 16 == 4 * off
        gdiv = 8.0 if off % 2 else 1.0
        out = norm_launch(obj=gd, gdiv=gdiv).cpu()
        check_norm(f"sumsq flat n={n} off={off} total", out[ops.NORM_TOTAL], g, SCALE * gdiv)
        assert out[ops.NORM_OBJECT] == out[ops.NORM_TOTAL] and out[ops.NORM_VIEW] == -1.0
        assert out[ops.NORM_FINITE] == 1.0 and out[ops.NORM_CLIP_COEF] == 1.0  # max_norm 0: clipping off
        out_v = norm_launch(view=gd, gdiv=gdiv).cpu()
        assert out_v[ops.NORM_VIEW] == out[ops.NORM_TOTAL] and out_v[ops.NORM_OBJECT] == -1.0
        assert out_v[ops.NORM_TOTAL] == out[ops.NORM_TOTAL]
    if n > 1:
        k = n // 3 + 1
        gd = _offset_copy(g, 0)
        out = norm_launch(obj=gd[:k], view=gd[k:]).cpu()  # the view side starts at an arbitrary float
        check_norm(f"sumsq split n={n} object", out[ops.NORM_OBJECT], g[:k], SCALE)
        check_norm(f"sumsq split n={n} view", out[ops.NORM_VIEW], g[k:], SCALE)
        check_norm(f"sumsq split n={n} total", out[ops.NORM_TOTAL], g, SCALE)


@pytest.mark.parametrize("active", [[0], [4], [1, 3]])
def test_grad_sumsq_segments_against_float64(active):
    """5 segments of 1031 floats; the inactive ones hold garbage (inf, nan) that must not be read"""
    ops = _ops()
    L, Sg = 1031, 5
    g = torch.full((Sg, L), math.inf)
    g[:, 1::7] = math.nan
    for s in active:
        g[s] = spread_gradients(L, 1, 200 + s)[0] * SCALE
    for off in (0, 3):
        gd = _offset_copy(g.reshape(-1), off)
        out = norm_launch(obj=gd, seg_len=L, active=i32(*active)).cpu()
        check_norm(f"sumsq segments {active} off={off}", out[ops.NORM_TOTAL], g[active].reshape(-1), SCALE)
        assert out[ops.NORM_FINITE] == 1.0 and out[ops.NORM_VIEW] == -1.0


def test_clip_coef_rule():
    """min(1, max_norm / (norm + 1e-6)) in f32, torch's clip_grad_norm_; exactly 1 when off"""
    ops = _ops()
    g = spread_gradients(1000, 1, 7)[0]
    norm = torch.linalg.vector_norm(g.double()).item()
    for max_norm in (0.0, -1.0, norm * 0.5, norm * 4.0, 1e30):
        out = norm_launch(obj=(g * SCALE).to(DEV), max_norm=max_norm).cpu()
        nt = out[ops.NORM_TOTAL]
        want = 1.0 if max_norm <= 0 else min(1.0, (torch.tensor(max_norm, dtype=F32) / (nt + 1e-6)).item())
        assert out[ops.NORM_CLIP_COEF].item() == pytest.approx(want, rel=2e-7), (max_norm, out.tolist())
        if max_norm <= 0 or max_norm > norm:
            assert out[ops.NORM_CLIP_COEF].item() == 1.0


# ------------------------------------------------------------------------------------------ non-finite gradients
@pytest.mark.parametrize("where", ["first", "last", "inactive"])
@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan])
def test_non_finite_gradient(bad, where):
    """inf / nan at element 0, at the last element, and in an inactive segment (ignored).  Non-finite: finite == 0,
    clip_coef == 1.0, the clipped AdamW leaves p, m, v untouched and the scale is halved"""
    ops = _ops()
    L, Sg, active = 1031, 5, [1, 3]
    g = spread_gradients(Sg * L, 1, 300)[0].reshape(Sg, L) * 1024.0
    seg, idx = {"first": (1, 0), "last": (3, L - 1), "inactive": (2, 17)}[where]
    g[seg, idx] = bad
    expect_finite = where == "inactive"
    p0 = torch.randn(Sg, L, generator=_gen(301)) * 0.05
    p, m, v = p0.clone().to(DEV), torch.zeros(Sg, L, device=DEV), torch.zeros(Sg, L, device=DEV)
    seg_step, step = torch.zeros(Sg, dtype=torch.int32, device=DEV), i32(0)
    scaler, hyper = _dev([1024.0, 2.0, 0.0]), hyper_dev(1e-3, 1e-2, 1.0)
    gd, act = g.to(DEV), i32(*active)
    out = norm_launch(obj=gd.reshape(-1), seg_len=L, active=act, scaler=scaler, hyper=hyper, max_norm=1e-3)
    ops.adamw_segments_clipped(p, gd, m, v, L, Sg, seg_step, act, hyper, scaler, step, out[ops.NORM_CLIP_COEF:],
                               growth_interval=4)
    o = out.cpu()
    assert o[ops.NORM_FINITE].item() == (1.0 if expect_finite else 0.0)
    if expect_finite:
        assert o[ops.NORM_CLIP_COEF].item() < 1.0 and math.isfinite(o[ops.NORM_TOTAL].item())
        assert not torch.equal(p[1].cpu(), p0[1]) and torch.equal(p[2].cpu(), p0[2])
        assert scaler.cpu().tolist() == [1024.0, 3.0, 0.0] and int(step.item()) == 1
    else:
        assert o[ops.NORM_CLIP_COEF].item() == 1.0
        assert torch.equal(p.cpu(), p0) and float(m.abs().sum()) == 0 and float(v.abs().sum()) == 0
        assert scaler.cpu().tolist() == [512.0, 0.0, 0.0] and int(step.item()) == 0
        assert seg_step.cpu().tolist() == [0] * Sg


@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_non_finite_gradient_flat(bad):
    ops = _ops()
    n = N_FLAT
    for idx in (0, n - 1):
        g = spread_gradients(n, 1, 310)[0] * 16.0
        g[idx] = bad
        p0 = torch.randn(n, generator=_gen(311)) * 0.05
        p, m, v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        scaler, hyper, step = _dev([16.0, 1.0, 0.0]), hyper_dev(1e-3, 1e-2, 1.0), i32(3)
        gd = g.to(DEV)
        out = norm_launch(obj=gd[:5000], view=gd[5000:], scaler=scaler, hyper=hyper, max_norm=1.0)
        ops.adamw_flat_clipped(p, gd, m, v, hyper, scaler, step, out[ops.NORM_CLIP_COEF:], growth_interval=4)
        o = out.cpu()
        assert o[ops.NORM_FINITE].item() == 0.0 and o[ops.NORM_CLIP_COEF].item() == 1.0
        assert torch.equal(p.cpu(), p0) and float(m.abs().sum()) == 0 and float(v.abs().sum()) == 0
        assert scaler.cpu().tolist() == [8.0, 0.0, 0.0] and int(step.item()) == 3


def test_large_finite_gradient_is_finite_and_stepped():
    """+-3.2e38 is a finite f32: its square overflows f32, not the f64 the kernel squares in"""
    ops = _ops()
    n = N_FLAT
    g = spread_gradients(n, 1, 320)[0]
    g[5], g[n - 2] = 3.2e38, -3.2e38
    p0 = torch.randn(n, generator=_gen(321)) * 0.05
    p, m, v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    scaler, hyper, step = _dev([1.0, 0.0, 0.0]), hyper_dev(1e-3, 1e-2, 1.0), i32(0)
    gd = g.to(DEV)
    out = norm_launch(obj=gd, scaler=scaler, hyper=hyper, max_norm=1.0)
    ops.adamw_flat_clipped(p, gd, m, v, hyper, scaler, step, out[ops.NORM_CLIP_COEF:], growth_interval=4)
    o = out.cpu()
    assert o[ops.NORM_FINITE].item() == 1.0
    assert 0.0 <= o[ops.NORM_CLIP_COEF].item() < 1e-30  # the f32 norm itself may round to inf: the coefficient to 0
    assert int(step.item()) == 1 and scaler.cpu().tolist() == [1.0, 1.0, 0.0]
    assert not torch.equal(p.cpu(), p0) and bool(torch.isfinite(p).all()) and bool(torch.isfinite(v).all())


# ------------------------------------------------------------------------------------------ memory contract
def _vec_slab(n, dtype, offset_extra=0):
    """contiguous `n` elements with guards in front and behind; offset_extra shifts the base off its alignment"""
    front, back = 1024 + offset_extra, 1024
    return S.Slab(front + n + back, (1, n), (n, 1), front, dtype, DEV)


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("c0", [0, 2, 3, 7])
def test_contract_record_and_norm(c0, B):
    """train_record + grad_sumsq (segments, flat) + grad_norm_finish with every operand in a guarded slab: a clean, a
    poisoned and a replayed run agree bit for bit, guards are intact, inputs unwritten, and of the ring only the addressed
    row changes — at counters before, at and past a wrap of the 3-row ring"""
    ops = _ops()
    rows, W = 3, ops.telemetry_row_floats(B)
    L, Sg, active, nv = 1031, 5, [1, 3], C + 9
    gen = _gen(400 + c0)
    g_obj = spread_gradients(Sg * L, 1, 401)[0] * SCALE
    g_view = spread_gradients(nv, 1, 402)[0] * SCALE
    t = torch.randint(0, 1000, (B,), generator=gen)
    losses = torch.rand(B, generator=gen)
    ins = {"g_obj": (_vec_slab(Sg * L, F32, 1), g_obj), "g_view": (_vec_slab(nv, F32, 3), g_view),
           "active": (_vec_slab(2, torch.int32), torch.tensor(active, dtype=torch.int32)),
           "scaler": (_vec_slab(3, F32), torch.tensor([SCALE, 5.0, 0.0])),
           "hyper": (_vec_slab(6, F32), hyper_dev(2e-3, 1e-2, 2.0).cpu()),
           "max_norm": (_vec_slab(1, F32), torch.tensor([0.25])),
           "t": (_vec_slab(B, torch.int64), t), "losses": (_vec_slab(B, F32), losses)}
    n_o, n_v = ops.grad_sumsq_ws_doubles(L, 2), ops.grad_sumsq_ws_doubles(nv)
    outs = {"ws_obj": _vec_slab(n_o, F64), "ws_view": _vec_slab(n_v, F64), "out": _vec_slab(ops.NORM_OUT_FLOATS, F32)}
    ring, count = S.Slab.matrix(rows, W, F32, gap=0, device=DEV), _vec_slab(1, torch.int32)
    row, prev = c0 % rows, (c0 + rows - 1) % rows
    pat = {F32: (S.QNAN[F32], S.SENTINEL[F32]), F64: (QNAN64, SENT64), torch.int32: (0x5A5AA5A5, 0), torch.int64: (S.INT_PATTERN, 0)}

    def launch():
        v = {k: s.view.view(-1) for k, (s, _) in ins.items()}
        ops.train_record(ring.view.view(-1), count.view.view(-1), rows, False, v["t"], v["losses"], B)
        ops.grad_sumsq(v["g_obj"], outs["ws_obj"].view.view(-1), seg_len=L, active=v["active"])
        ops.grad_sumsq(v["g_view"], outs["ws_view"].view.view(-1))
        ops.grad_norm_finish(outs["ws_obj"].view.view(-1), n_o, outs["ws_view"].view.view(-1), n_v, v["scaler"], v["hyper"],
                             v["max_norm"], outs["out"].view.view(-1), ring.view.view(-1), count.view.view(-1), rows, W)
        torch.cuda.synchronize()

    def prepare(poison):
        for s, val in ins.values():
            s.fill_all(pat[s.dtype][0] if poison else 0)
            s.fill_logical(val)
        for s in outs.values():
            s.fill_all(pat[s.dtype][1] if poison else 0)
        ring.fill_all(S.SENTINEL[F32] if poison else 0)
        ring.view[prev, ops.TEL_MICRO] = 4.0  # the one ring element the record reads: the previous row's micro index
        count.fill_all(0x5A5AA5A5 if poison else 0)
        count.fill_logical(torch.tensor([c0], dtype=torch.int32))

    def results():
        return {**{k: s.logical_bits() for k, s in outs.items()}, "row": ring.bits.view(-1)[ring.mask].view(rows, W)[row].clone()}

    res = {}
    for run in ("clean", "poisoned", "replay"):
        if run != "replay":
            prepare(run == "poisoned")
        else:
            count.fill_logical(torch.tensor([c0], dtype=torch.int32))  # the in-place counter, put back
            if prev != row:
                assert ring.view[prev, ops.TEL_MICRO].item() == 4.0
        snaps = {k: s.snapshot() for k, (s, _) in ins.items()}
        ring_before = ring.snapshot()
        launch()
        res[run] = results()
        for k, (s, _) in ins.items():
            s.unchanged(snaps[k], f"{k} after the {run} run")
        assert int(count.view.item()) == c0 + 1
        changed = (ring.bits != ring_before).nonzero().view(-1)
        lo = ring.offset + row * W
        assert bool(((changed >= lo) & (changed < lo + W)).all()), f"{run}: the ring changed outside row {row}"
        if run != "clean":
            for k, s in outs.items():
                s.outside_intact(pat[s.dtype][1], f"{k} after the {run} run")
                s.logical_has_no_sentinel(pat[s.dtype][1], f"{k} after the {run} run")
            count.outside_intact(0x5A5AA5A5, "count")
            assert not bool((res[run]["row"] == S._signed(S.SENTINEL[F32], 32)).any()), "a field of the row was never written"
    for k in res["clean"]:
        assert torch.equal(res["clean"][k], res["poisoned"][k]), f"{k}: the poisoned run differs from the clean one"
        assert torch.equal(res["poisoned"][k], res["replay"][k]), f"{k}: the replayed run differs"
    # and the values
    r = ring.view[row].cpu()
    o = outs["out"].view.view(-1).cpu()
    assert r[ops.TEL_SEQ] == c0 and r[ops.TEL_MICRO] == 5.0 and r[ops.TEL_CLOSED] == 1.0
    assert r[ops.TEL_HEADER:ops.TEL_HEADER + B].tolist() == t.tolist()
    assert torch.equal(r[ops.TEL_HEADER + B:], losses)
    assert r[ops.TEL_LOSS_SCALE] == SCALE and r[ops.TEL_LR] == torch.tensor(2e-3, dtype=F32)
    assert torch.equal(r[ops.TEL_NORM_OBJECT:ops.TEL_CLIP_COEF + 1], o)
    both = torch.cat([g_obj.view(Sg, L)[active].reshape(-1), g_view])
    check_norm("contract total norm", o[ops.NORM_TOTAL], both, SCALE * 2.0)
    assert 0.0 < o[ops.NORM_CLIP_COEF] < 1.0 and o[ops.NORM_FINITE] == 1.0


# ------------------------------------------------------------------------------------------ train_record
@pytest.mark.parametrize("B", [1, 2, 3])
def test_train_record_rows(B):
    """7 micro-steps in groups of 3, 1, 3 into a 4-row ring: timesteps and per-sample values exact, the micro index counts
    inside a group, the counter advances, the finish kernel's fields land in row (count - 1) % rows"""
    ops = _ops()
    rows, W = 4, ops.telemetry_row_floats(B)
    ring, count = torch.zeros(rows * W, device=DEV), i32(0)
    gen = _gen(500 + B)
    g = (spread_gradients(300, 1, 501)[0] * SCALE).to(DEV)
    firsts = [True, False, False, True, True, False, False]
    closes = [False, False, True, True, False, False, True]
    want = {}
    for c, (first, close) in enumerate(zip(firsts, closes)):
        t = torch.randint(0, 1000, (B,), generator=gen)
        losses = torch.rand(B, generator=gen) * 3
        ops.train_record(ring, count, rows, first, t.to(DEV), losses.to(DEV), B)
        micro = 0 if first else want[c - 1][0] + 1
        want[c] = (micro, t, losses, close)
        if close:
            out = norm_launch(obj=g, ring=ring, count=count, rows=rows, row_floats=W, scale=SCALE / (1 + c)).cpu()
        assert int(count.item()) == c + 1
        host = ring.cpu().view(rows, W)
        for k in range(max(0, c + 1 - rows), c + 1):
            r, (mi, tt, ll, cl) = host[k % rows], want[k]
            assert r[ops.TEL_SEQ] == k and r[ops.TEL_MICRO] == mi and r[ops.TEL_CLOSED] == float(cl), (c, k, r.tolist())
            assert r[ops.TEL_HEADER:ops.TEL_HEADER + B].tolist() == tt.tolist() and torch.equal(r[ops.TEL_HEADER + B:], ll)
            if cl:
                assert r[ops.TEL_LOSS_SCALE] == SCALE / (1 + k) and r[ops.TEL_FINITE] == 1.0 and r[ops.TEL_NORM_VIEW] == -1.0
            else:
                assert float(r[ops.TEL_NORM_OBJECT:ops.TEL_HEADER].abs().sum()) == 0.0
        if close:
            assert torch.equal(host[c % rows][ops.TEL_NORM_OBJECT:ops.TEL_CLIP_COEF + 1], out)
    with pytest.raises(RuntimeError, match="train_record"):
        _ops()._l.call("train_record", ring.data_ptr(), count.data_ptr(), rows, W + 1, 1, t.to(DEV).data_ptr(),
                       losses.to(DEV).data_ptr(), B, ops.stream())


# ------------------------------------------------------------------------------------------ clipped AdamW
def _clip_refs(p0s, lr, wd):
    refs = {}
    for dt in (F64, F32):
        qs = [p.to(dt).clone().requires_grad_(True) for p in p0s]
        refs[dt] = (qs, torch_adamw(qs, lr, wd))
    return refs


@pytest.mark.parametrize("gdiv", [1.0, 8.0])
def test_adamw_flat_clipped_trajectory(gdiv):
    """50 steps against float64 torch AdamW with clip_grad_norm_ before each step; max_norm = the median step norm"""
    ops = _ops()
    n, steps, lr, wd = N_FLAT, 50, 1e-3, 1e-2
    p0 = torch.randn(n, generator=_gen(600)) * 0.05
    gs = spread_gradients(n, steps, 601)
    norms = torch.linalg.vector_norm(gs.double(), dim=1)
    max_norm = float(norms.median())
    assert int((norms > max_norm * (1 + 1e-4)).sum()) >= 10 and int((norms < max_norm * (1 - 1e-4)).sum()) >= 10
    g_dev = (gs * (SCALE * gdiv)).to(DEV)
    assert torch.equal(g_dev.cpu() / (SCALE * gdiv), gs)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    scaler, step, hyper = _dev([SCALE, 0.0, 0.0]), i32(0), hyper_dev(lr, wd, gdiv)
    refs = _clip_refs([p0], lr, wd)
    coefs = []
    for s in range(1, steps + 1):
        out = norm_launch(obj=g_dev[s - 1], scaler=scaler, hyper=hyper, max_norm=max_norm)
        ops.adamw_flat_clipped(p, g_dev[s - 1], m, v, hyper, scaler, step, out[ops.NORM_CLIP_COEF:], growth_interval=100000)
        coefs.append(out)
        for dt, (qs, opt) in refs.items():
            qs[0].grad = gs[s - 1].to(dt)
            torch.nn.utils.clip_grad_norm_(qs, max_norm)
            opt.step()
        if s in (1, 2, 10, 50):
            torch.cuda.synchronize()
            assert int(step.item()) == s
            (q64, o64), (q32, o32) = refs[F64], refs[F32]
            tag = f"adamw clipped gdiv={gdiv} step {s}"
            check32(tag + " p - p0", p.cpu().double() - p0.double(), q64[0].detach() - p0.double(),
                    q32[0].detach().double() - p0.double())
            check32(tag + " m", m, o64.state[q64[0]]["exp_avg"], o32.state[q32[0]]["exp_avg"])
            check32(tag + " v", v, o64.state[q64[0]]["exp_avg_sq"], o32.state[q32[0]]["exp_avg_sq"])
    coefs = torch.stack(coefs).cpu()[:, ops.NORM_CLIP_COEF]
    assert int((coefs < 1).sum()) >= 10 and int((coefs == 1).sum()) >= 10


def test_adamw_segments_clipped_against_torch():
    """5 object segments on the active schedule of test_adamw_segments_against_torch plus a flat view bucket, one global
    norm over the active segments and the view bucket, the two-bucket phase order CHECK, CHECK, APPLY, APPLY | FINISH"""
    ops = _ops()
    L, Sg, nv = SEG_LEN, N_SEG, 1000
    lr, wd, scale = 1e-3, 1e-2, 256.0
    p0 = torch.randn(Sg, L, generator=_gen(610)) * 0.05
    pv0 = torch.randn(nv, generator=_gen(611)) * 0.05
    gs = torch.stack([spread_gradients(L, len(ACTIVITY), 612 + s) for s in range(Sg)], dim=1)  # [steps, S, L]
    gv = spread_gradients(nv, len(ACTIVITY), 620)
    norms = torch.stack([torch.linalg.vector_norm(torch.cat([gs[k, act].reshape(-1), gv[k]]).double())
                         for k, act in enumerate(ACTIVITY)])
    max_norm = float(norms.median())
    assert int((norms > max_norm * (1 + 1e-4)).sum()) >= 3 and int((norms < max_norm * (1 - 1e-4)).sum()) >= 3
    p, m, v = p0.clone().to(DEV), torch.zeros(Sg, L, device=DEV), torch.zeros(Sg, L, device=DEV)
    pv, mv, vv = pv0.clone().to(DEV), torch.zeros(nv, device=DEV), torch.zeros(nv, device=DEV)
    seg_step, step = torch.zeros(Sg, dtype=torch.int32, device=DEV), i32(0)
    scaler, hyper = _dev([scale, 0.0, 0.0]), hyper_dev(lr, wd, 1.0)
    refs = _clip_refs([p0[s] for s in range(Sg)] + [pv0], lr, wd)
    for k, act in enumerate(ACTIVITY):
        g = torch.full((Sg, L), math.inf)  # stale garbage in the inactive segments: neither in the norm nor in the update
        g[:, 1::7] = math.nan
        for s in act:
            g[s] = gs[k, s] * scale
        gd, gvd, active = g.to(DEV), (gv[k] * scale).to(DEV), i32(*act)
        out = norm_launch(obj=gd.reshape(-1), view=gvd, seg_len=L, active=active, scaler=scaler, hyper=hyper,
                          max_norm=max_norm)
        clip = out[ops.NORM_CLIP_COEF:]
        a = dict(growth_interval=100000)
        ops.adamw_flat_clipped(pv, gvd, mv, vv, hyper, scaler, step, clip, phases=ops.OPT_CHECK, **a)
        ops.adamw_segments_clipped(p, gd, m, v, L, Sg, seg_step, active, hyper, scaler, step, clip, phases=ops.OPT_CHECK, **a)
        ops.adamw_flat_clipped(pv, gvd, mv, vv, hyper, scaler, step, clip, phases=ops.OPT_APPLY, **a)
        ops.adamw_segments_clipped(p, gd, m, v, L, Sg, seg_step, active, hyper, scaler, step, clip,
                                   phases=ops.OPT_APPLY | ops.OPT_FINISH, **a)
        for dt, (qs, opt) in refs.items():
            opt.zero_grad(set_to_none=False)
            for s in act:
                qs[s].grad = gs[k, s].to(dt)
            qs[Sg].grad = gv[k].to(dt)
            torch.nn.utils.clip_grad_norm_(qs, max_norm)
            opt.step()
    torch.cuda.synchronize()
    assert int(step.item()) == len(ACTIVITY) and seg_step.cpu().tolist() == [12, 11, 0, 9, 10]
    (q64, o64), (q32, o32) = refs[F64], refs[F32]
    got = [(p[s], m[s], v[s], p0[s]) for s in range(Sg)] + [(pv, mv, vv, pv0)]
    for s, (gp, gm, gvv, start) in enumerate(got):
        if s == 2:
            assert torch.equal(gp.cpu(), start)
            continue
        tag = f"adamw segments clipped bucket {s}"
        check32(tag + " p - p0", gp.cpu().double() - start.double(), q64[s].detach() - start.double(),
                q32[s].detach().double() - start.double())
        check32(tag + " m", gm, o64.state[q64[s]]["exp_avg"], o32.state[q32[s]]["exp_avg"])
        check32(tag + " v", gvv, o64.state[q64[s]]["exp_avg_sq"], o32.state[q32[s]]["exp_avg_sq"])


def test_clipped_entries_are_the_unclipped_ones_when_nothing_clips():
    """max_norm = 1e30: the coefficient is exactly 1 and p, m, v stay torch.equal to the unclipped entries over 20 steps,
    flat and segments"""
    ops = _ops()
    n, L, Sg, steps = N_FLAT, SEG_LEN, N_SEG, 20
    gs = (spread_gradients(n, steps, 700) * 1024.0).to(DEV)
    gseg = (spread_gradients(Sg * L, steps, 701) * 1024.0).to(DEV)
    hyper = hyper_dev(1e-3, 1e-2, 2.0)

    def fresh(shape, seed):
        return [(torch.randn(*shape, generator=_gen(seed)) * 0.05).to(DEV), torch.zeros(*shape, device=DEV),
                torch.zeros(*shape, device=DEV)]
    flat = {k: (fresh((n,), 702), _dev([1024.0, 0.0, 0.0]), i32(0)) for k in ("plain", "clipped")}
    seg = {k: (fresh((Sg, L), 703), _dev([1024.0, 0.0, 0.0]), i32(0), torch.zeros(Sg, dtype=torch.int32, device=DEV))
           for k in ("plain", "clipped")}
    for s in range(steps):
        (p, m, v), sc, st = flat["plain"]
        ops.adamw_flat(p, gs[s], m, v, hyper, sc, st, growth_interval=8)
        (p, m, v), sc, st = flat["clipped"]
        out = norm_launch(obj=gs[s], scaler=sc, hyper=hyper, max_norm=1e30)
        ops.adamw_flat_clipped(p, gs[s], m, v, hyper, sc, st, out[ops.NORM_CLIP_COEF:], growth_interval=8)
        active = i32(*ACTIVITY[s % len(ACTIVITY)])
        (p, m, v), sc, st, ss = seg["plain"]
        ops.adamw_segments(p, gseg[s].view(Sg, L), m, v, L, Sg, ss, active, hyper, sc, st, growth_interval=8)
        (p, m, v), sc, st, ss = seg["clipped"]
        out2 = norm_launch(obj=gseg[s], seg_len=L, active=active, scaler=sc, hyper=hyper, max_norm=1e30)
        ops.adamw_segments_clipped(p, gseg[s].view(Sg, L), m, v, L, Sg, ss, active, hyper, sc, st, out2[ops.NORM_CLIP_COEF:],
                                   growth_interval=8)
        assert out.cpu()[ops.NORM_CLIP_COEF] == 1.0 and out2.cpu()[ops.NORM_CLIP_COEF] == 1.0
    torch.cuda.synchronize()
    for d in (flat, seg):
        for a, b in zip(d["plain"][0], d["clipped"][0]):
            assert torch.equal(a, b)
        assert torch.equal(d["plain"][1], d["clipped"][1]) and torch.equal(d["plain"][2], d["clipped"][2])
    assert flat["plain"][1].cpu().tolist()[0] == 1024.0 * 4 and int(flat["plain"][2].item()) == steps
    assert not torch.equal(flat["plain"][0][0].cpu(), fresh((n,), 702)[0].cpu())


# ------------------------------------------------------------------------------------------ the bf16 library
def test_bf16_library_runs_this_file(tmp_path):
    """every case above against libvneti_hip_bf16.so, in a child pytest process with VNETI_PRECISION=bf16 (a process
    computes in one 16-bit format): no failure, no error, nothing skipped, and as many cases as this process collects"""
    from view_neti_amd import lib
    if lib.precision() == "bf16":
        return  # this IS the bf16 run
    run_bf16_child(os.path.join("tests", os.path.basename(__file__)), "not bf16_library", 240, tmp_path, least=40)
