"""The exponential moving average of the mappers on the GPU: vneti_ema_update and vneti_swap_f32
through the C ABI, the engine's `ema` / `ema_weights()`, and a tiny Coach run.

References.  The kernels: tests/helpers/ema_ref.py, the decay and the update restated in float64 (numpy).  Bars, derived and
not measured: the coefficient is float32(1 - d64) within one f32 ulp (device f64 `pow` against numpy's); an updated element
is within 5 * 2^-24 * max(|e|, |p|) of e + (1 - d64) * (p - e) in float64 — one rounding of p - e on a difference
<= 2 * max (2), one of the fma (1), one ulp of c on that difference (2).  Everything else is bit equality.  The kernels are
f32 only; `test_bf16_library_runs_the_kernel_cases` runs them against libvneti_hip_bf16.so in a child process."""
import os

import numpy as np
import pytest
import torch

from helpers import ema_ref as ER
from helpers import slabs as S
from helpers.bf16_child import run_bf16_child
from helpers.checks import DEV
from helpers.checks import ops as _ops
from helpers import coach_runs as rt
from helpers.engines import FORMS, STATE, batch_dict, build_device_rng_engine, feed_six, run_steps, six_steps, snapshot

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
SENT = S.SENTINEL[F32]
GUARD = 256  # floats of guard on each side of a flat operand (a multiple of 4: the misalignment is the test's choice)
SIZES = (1, 3, 4, 5, 255, 256, 1027, 8193)
ALIGN = ((0, 0), (1, 1), (1, 0), (0, 1))  # (ema, p): 0 = 16-byte aligned base, 1 = a `[1:]` slice (4-byte aligned only)
BAR = 5.0 * 2.0 ** -24


def _dev(x, dtype=F32):
    return torch.tensor(x, dtype=dtype, device=DEV)


def flat_slab(n, mis):
    """n floats inside a sentinel-filled allocation, `mis` floats past a 16-byte boundary"""
    s = S.Slab(GUARD + mis + n + GUARD, (1, n), (n, 1), GUARD + mis, F32, DEV)
    assert s.buf.data_ptr() % 16 == 0 and (s.view.data_ptr() % 16 == 0) == (mis % 4 == 0)
    s.fill_all(SENT)
    return s


def values(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.tensor(10.0) ** torch.randint(-3, 3, (n,), generator=g).float()


def launch(ema, p, n_updates, last=6, opt=7, max_decay=0.9999, after=0, power=0.0):
    """one vneti_ema_update on device state written by the test -> (count, coef) on the host"""
    ops = _ops()
    count, opt_step = _dev([n_updates, last], I32), _dev([opt], I32)
    hyper, coef = _dev([max_decay, float(after), power, 0.0]), _dev([-3.0, -3.0])
    ops.ema_update(ema.view(-1), p.view(-1), opt_step, count, hyper, coef)
    torch.cuda.synchronize()
    return count.cpu().tolist(), coef.cpu()


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ================================================================================================ the kernels
@pytest.mark.parametrize("n", SIZES)
def test_kernel_update_against_float64(n):
    e0, p0 = values(n, 10 + n), values(n, 20 + n)
    big = torch.maximum(e0.abs(), p0.abs()).double().numpy()
    worst = 0.0
    for me, mp in ALIGN:
        for n_updates in (0, 1, 11, 1_000_000):
            for max_decay in (0.9999, 0.5):
                for power in (0.0, 2.0 / 3.0):
                    ema, p = flat_slab(n, me), flat_slab(n, mp)
                    ema.fill_logical(e0)
                    p.fill_logical(p0)
                    snap = p.snapshot()
                    count, coef = launch(ema.view, p.view, n_updates, max_decay=max_decay, power=power)
                    k = n_updates + 1
                    d = ER.decay(k, ER.f32(max_decay), 0, ER.f32(power))
                    what = f"n {n} align {(me, mp)} k {k} max_decay {max_decay} power {power:.3f}"
                    assert count == [k, 7], what
                    ema.outside_intact(SENT, what + " (ema)")
                    p.unchanged(snap, what + " (p)")
                    got = ema.view.reshape(-1).cpu()
                    if d == 0.0:  # k = 1: the first update is a copy
                        assert float(coef[1]) == 2.0 and float(coef[0]) == 1.0, what
                        assert torch.equal(got.view(I32), p0.view(I32)), what
                        continue
                    assert float(coef[1]) == 1.0, what
                    u = ulps(float(coef[0]), np.float32(1.0 - d))
                    assert u <= 1, f"{what}: one_minus_decay {float(coef[0])!r} is {u} ulp from float32(1 - d64) {np.float32(1.0 - d)!r}"
                    err = np.abs(got.double().numpy() - ER.update(e0.numpy(), p0.numpy(), 1.0 - d))
                    worst = max(worst, float((err / big).max()))
                    assert (err <= BAR * big).all(), f"{what}: worst error {float((err / big).max()) / 2.0 ** -24:.3f} * 2^-24 * max(|e|,|p|)"
    print(f"[ema_update n={n}] worst error {worst / 2.0 ** -24:.3f} * 2^-24 * max(|e|, |p|), bar 5")


def test_kernel_decay_schedule():
    """the coefficient over the first updates, with and without update_after_step, and where the cap takes over"""
    ema, p = flat_slab(4, 0), flat_slab(4, 0)
    ema.fill_logical(values(4, 1))
    p.fill_logical(values(4, 2))
    for after, power, max_decay in ((0, 0.0, 0.5), (3, 0.0, 0.9999), (0, 2.0 / 3.0, 0.9999), (2, 2.0 / 3.0, 0.3)):
        for k in range(1, 16):
            count, coef = launch(ema.view, p.view, k - 1, max_decay=max_decay, after=after, power=power)
            d = ER.decay(k, ER.f32(max_decay), after, ER.f32(power))
            assert count == [k, 7]
            assert float(coef[1]) == (2.0 if d == 0.0 else 1.0), (after, power, k)
            assert ulps(float(coef[0]), np.float32(1.0 - d)) <= 1, (after, power, max_decay, k, float(coef[0]), 1.0 - d)
    assert ER.decay(9, 0.5) == 0.5 and ER.decay(8, 0.5) < 0.5 and ER.decay(4, 0.9, 3) == 0.0 and ER.decay(5, 0.9, 3) == 2.0 / 11.0


@pytest.mark.parametrize("n", (5, 1027))
@pytest.mark.parametrize("align", ALIGN)
def test_kernel_copy_is_bitwise(n, align):
    """s == 0 (the first update, or any inside update_after_step): ema takes the BITS of p — a NaN payload, -0.0, an
    infinity and a denormal included — whatever ema held"""
    p0 = values(n, 3).view(I32).clone()
    special = torch.tensor([0x7FC12345, -0x80000000, 0x7F800000, 0x00000001], dtype=torch.int64)
    p0[:min(4, n)] = special[:min(4, n)].to(I32)
    for n_updates, after in ((0, 0), (3, 3), (2, 5)):
        ema, p = flat_slab(n, align[0]), flat_slab(n, align[1])
        ema.fill_logical(torch.full((n,), float("nan")))
        p.view.view(I32).copy_(p0.reshape(1, n))
        snap = p.snapshot()
        count, coef = launch(ema.view, p.view, n_updates, after=after)
        assert count == [n_updates + 1, 7] and float(coef[1]) == 2.0
        assert torch.equal(ema.view.view(I32).reshape(-1).cpu(), p0)
        ema.outside_intact(SENT, "ema")
        p.unchanged(snap, "p")


@pytest.mark.parametrize("align", ALIGN)
def test_kernel_skipped_step(align):
    """opt_step == last_opt_step: the optimizer step was skipped on found_inf — ema and ema_count keep their bits; the
    next applied step advances k by one, not two"""
    n = 1027
    ops = _ops()
    ema, p = flat_slab(n, align[0]), flat_slab(n, align[1])
    ema.fill_logical(values(n, 4))
    p.fill_logical(values(n, 5))
    before, p_snap = ema.snapshot(), p.snapshot()
    count, opt_step = _dev([5, 7], I32), _dev([7], I32)
    hyper, coef = _dev([0.9999, 0.0, 0.0, 0.0]), _dev([-3.0, -3.0])
    ops.ema_update(ema.view.view(-1), p.view.view(-1), opt_step, count, hyper, coef)
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [5, 7] and float(coef[1]) == 0.0
    ema.unchanged(before, "ema after a skipped step")
    p.unchanged(p_snap, "p")
    opt_step.fill_(8)
    ops.ema_update(ema.view.view(-1), p.view.view(-1), opt_step, count, hyper, coef)
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [6, 8] and float(coef[1]) == 1.0
    assert ulps(float(coef[0]), np.float32(1.0 - ER.decay(6, ER.f32(0.9999)))) <= 1
    assert not torch.equal(ema.snapshot(), before)
    ema.outside_intact(SENT, "ema")
    p.unchanged(p_snap, "p")


@pytest.mark.parametrize("n", (3, 256, 8193))
@pytest.mark.parametrize("align", ALIGN)
def test_kernel_memory_contract_ema(n, align):
    """apply, copy and skip launches on guarded operands: guards intact, p unchanged, a second launch from the same
    inputs bit-identical"""
    e0, p0 = values(n, 6), values(n, 7)
    for name, kw in (("apply", dict(n_updates=11)), ("copy", dict(n_updates=0)), ("skip", dict(n_updates=11, last=7))):
        runs = []
        for _ in range(2):
            ema, p = flat_slab(n, align[0]), flat_slab(n, align[1])
            ema.fill_logical(e0)
            p.fill_logical(p0)
            snap = p.snapshot()
            launch(ema.view, p.view, **kw)
            ema.outside_intact(SENT, f"{name}: ema")
            p.unchanged(snap, f"{name}: p")
            runs.append((ema, ema.logical_bits()))
        S.first_difference(runs[0][1], runs[1][1], runs[0][0], f"{name}: two launches from the same inputs")
        if name == "skip":
            assert torch.equal(runs[0][1].cpu(), e0.view(I32))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("align", ALIGN)
def test_kernel_swap_f32(n, align):
    """exchanged contents, intact guards and double swap = identity, all bitwise"""
    ops = _ops()
    a0, b0 = values(n, 8).view(I32).clone(), values(n, 9).view(I32).clone()
    a0[0], b0[-1] = 0x7FC12345, -0x80000000  # a NaN payload and -0.0 travel as bits
    a, b = flat_slab(n, align[0]), flat_slab(n, align[1])
    a.view.view(I32).copy_(a0.reshape(1, n))
    b.view.view(I32).copy_(b0.reshape(1, n))
    snap_a, snap_b = a.snapshot(), b.snapshot()
    ops.swap_f32(a.view.view(-1), b.view.view(-1))
    torch.cuda.synchronize()
    assert torch.equal(a.logical_bits().cpu(), b0) and torch.equal(b.logical_bits().cpu(), a0)
    a.outside_intact(SENT, "a")
    b.outside_intact(SENT, "b")
    ops.swap_f32(a.view.view(-1), b.view.view(-1))
    torch.cuda.synchronize()
    a.unchanged(snap_a, "a after two swaps")
    b.unchanged(snap_b, "b after two swaps")


def test_kernel_argument_checks():
    ops = _ops()
    x = torch.zeros(16, device=DEV)
    i2, i1, h, c = _dev([0, 0], I32), _dev([1], I32), _dev([0.9, 0.0, 0.0, 0.0]), _dev([0.0, 0.0])
    with pytest.raises(RuntimeError, match="overlap"):
        ops.ema_update(x[:8], x[4:12], i1, i2, h, c)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.swap_f32(x[:8], x[7:15])
    from view_neti_amd import lib
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call("ema_update", x.data_ptr(), None, 8, i1.data_ptr(), i2.data_ptr(), h.data_ptr(), c.data_ptr(), None)
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call("swap_f32", x.data_ptr(), x.data_ptr() + 32, 0, None)
    torch.cuda.synchronize()
    assert not x.any()


# ================================================================================================ the engine
DECAY = 0.9  # the cap; over 6 steps the (1 + s) / (10 + s) ramp stays under it: 0 (copy), 2/11, 3/12, 4/13, 5/14, 6/15
K = 6
_ENG = {}


def _build(form, **kw):
    mode3, accum = FORMS[form]
    return build_device_rng_engine(mode3, accum, **kw)


def _ema_run(form, captured=True):
    """6 optimizer steps of the tiny device-RNG engine with the average on, computed once per (form, captured) and left
    unchanged: (cfg, engine, [params after step k], [opt_step after step k], end state, params before step 1)"""
    key = (form, captured)
    if key not in _ENG:
        mode3 = FORMS[form][0]
        cfg, eng = _build(form, ema_decay=DECAY)
        p_init = eng.params.cpu().clone()
        assert torch.equal(eng.ema.cpu(), p_init) and eng.ema.data_ptr() != eng.params.data_ptr()
        feed_six(cfg, eng, 0, 0, mode3)
        if captured:
            eng.capture()
            assert torch.equal(eng.ema.cpu(), p_init) and eng.ema_count.cpu().tolist() == [0, 0], "the warm-up left a trace"
        ps, steps = [], []
        for s in range(K):
            run_steps(cfg, eng, [s], mode3, feed_six)
            ps.append(eng.params.cpu().clone())
            steps.append(int(eng.opt_step.item()))
        _ENG[key] = (cfg, eng, ps, steps, snapshot(eng, STATE + ("ema", "ema_count")), p_init)
    return _ENG[key]


@pytest.mark.parametrize("form", ["one-mapper", "mode3", "accum2"])
def test_engine_training_is_not_perturbed(form):
    """the average only reads `params`: everything the step trains is torch.equal to the same run without it"""
    off, _, _ = six_steps(form)
    on = _ema_run(form)[4]
    for f in STATE:
        assert torch.equal(on[f], off[f]), f"{form}: {f} differs between the run with and without the average"
    assert set(STATE) >= {"params", "exp_avg", "exp_avg_sq", "opt_step", "seg_step", "scaler", "rng_state"}


@pytest.mark.parametrize("form", ["one-mapper", "mode3", "accum2"])
def test_engine_ema_against_float64_recurrence(form):
    """the f64 recurrence over the test's own per-step snapshots of `params` (an update only where opt_step advanced)"""
    _, eng, ps, steps, end, p_init = _ema_run(form)
    e, k, last, big = p_init.double().numpy(), 0, 0, float(p_init.abs().max())
    for p, step in zip(ps, steps):
        big = max(big, float(p.abs().max()))
        if step == last:
            continue  # skipped on found_inf
        k, last = k + 1, step
        d = ER.decay(k, ER.f32(DECAY))
        e = p.double().numpy() if d == 0.0 else ER.update(e, p.numpy(), 1.0 - d)
    assert k >= 4, f"{form}: only {k} of {K} steps were applied: the recurrence is hardly exercised"
    assert end["ema_count"].tolist() == [k, steps[-1]]
    err = float(np.abs(end["ema"].double().numpy() - e).max())
    bar = K * BAR * big
    print(f"[engine ema {form}] {k} updates, max |ema - ref64| {err:.3e}, bar {bar:.3e}, max|p| {big:.3e}")
    assert err <= bar
    assert not torch.equal(end["ema"], end["params"]) and not torch.equal(end["ema"], p_init)
    if form == "mode3":  # scenes 0, 2, 0, 2, 0, 2: mapper 1 never trained, p == ema exactly, so no bit of it moved
        seg = slice(eng.n_obj, 2 * eng.n_obj)
        assert torch.equal(end["ema"][seg], p_init[seg]) and torch.equal(end["params"][seg], p_init[seg])


@pytest.mark.parametrize("form", ["one-mapper", "mode3", "accum2"])
def test_engine_replay_equals_eager(form):
    eager, replay = _ema_run(form, captured=False)[4], _ema_run(form)[4]
    for f in ("ema", "ema_count", "params", "opt_step"):
        assert torch.equal(eager[f], replay[f]), f"{form}: {f} differs between eager steps and graph replay"


@pytest.mark.parametrize("form", ["one-mapper", "mode3", "accum2"])
def test_engine_launch_counts(form, monkeypatch):
    """an eager step's ABI calls: without the average the optimizer's calls are the ones they always were; with it, exactly
    one ema_update, after the last AdamW call, and only in the micro-step that closes a group"""
    from view_neti_amd import lib
    mode3, accum = FORMS[form]

    def calls(**kw):
        cfg, eng = _build(form, **kw)
        per_micro, orig = [], lib.call
        for m in range(accum):
            feed_six(cfg, eng, 0, m, mode3)
            names = []
            with monkeypatch.context() as mp:
                mp.setattr(lib, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
                assert eng.step() is (m == accum - 1)
            per_micro.append(names)
        torch.cuda.synchronize()
        return per_micro, len(eng.launches())

    off, n_off = calls()
    on, n_on = calls(ema_decay=DECAY)
    assert n_on == n_off
    optimizer = ["adamw_flat", "adamw_segments", "adamw_flat", "adamw_segments"] if mode3 else ["adamw_flat"]
    assert off[-1][-len(optimizer):] == optimizer and not any(n.startswith("adamw") for n in off[-1][:-len(optimizer)])
    assert not any(n in ("ema_update", "swap_f32") for names in off for n in names)
    assert on[-1] == off[-1] + ["ema_update"]
    for a, b in zip(on[:-1], off[:-1]):  # the accumulating micro-steps
        assert a == b and not any(n.startswith("adamw") for n in a)


def test_engine_skipped_step_leaves_the_average_alone():
    """an inf planted in `grads`: GradScaler's ordinary found-inf handling skips the step, and the average with it"""
    cfg, eng = _build("one-mapper", ema_decay=DECAY)
    for s in range(2):
        feed_six(cfg, eng, s, 0, False)
        assert eng.step()
    before = snapshot(eng, ("ema", "ema_count", "opt_step", "params", "scaler"))
    assert before["ema_count"].tolist() == [2, 2]
    feed_six(cfg, eng, 2, 0, False)
    eng.forward_backward()
    eng.grads[5] = float("inf")
    eng.optimizer_step()
    after = snapshot(eng, ("ema", "ema_count", "opt_step", "params", "scaler"))
    for f in ("ema", "ema_count", "opt_step", "params"):
        assert torch.equal(before[f], after[f]), f
    assert float(after["scaler"][0]) == 0.5 * float(before["scaler"][0]), "the step was not skipped the GradScaler way"
    feed_six(cfg, eng, 3, 0, False)
    assert eng.step()
    torch.cuda.synchronize()
    assert eng.ema_count.cpu().tolist() == [3, 3] and not torch.equal(eng.ema.cpu(), before["ema"])


def _eval_batch(cfg, eng, mode3, seed=0):
    b = batch_dict(cfg, eng.B, eng.H, eng.W, seed=seed)
    if mode3:
        eng.set_batch(b["px"], b["ids"], b["po"], b["pv"], b["vp"], object_index=2, for_eval=True)
    else:
        from view_neti_amd import synth
        ids = synth.input_ids(eng.B, cfg.clip.vocab_size - 3, cfg.clip.vocab_size)
        eng.set_batch(b["px"], ids, b["po"], for_eval=True)
    eng.set_noise(b["eps"], b["noise"], b["t"])
    return eng.eval_losses()


@pytest.mark.parametrize("form", ["one-mapper", "mode3"])
def test_engine_ema_weights(form):
    mode3 = FORMS[form][0]
    cfg, eng, _, _, end, _ = _ema_run(form)
    raw = _eval_batch(cfg, eng, mode3)
    with eng.ema_weights() as inside:
        assert inside is eng
        assert torch.equal(eng.params.cpu(), end["ema"]) and torch.equal(eng.ema.cpu(), end["params"])
        averaged = _eval_batch(cfg, eng, mode3)
        for what, call in (("step", eng.step), ("forward_backward", eng.forward_backward),
                           ("optimizer_step", eng.optimizer_step), ("state_dict", eng.state_dict),
                           ("load_state_dict", lambda: eng.load_state_dict({})), ("capture", eng.capture),
                           ("ema_weights", eng.ema_weights)):
            with pytest.raises(RuntimeError, match="ema_weights"):
                call()
    now = snapshot(eng, STATE + ("ema", "ema_count"))
    for f in now:
        assert torch.equal(now[f], end[f]), f"{f} is not what it was before ema_weights()"
    assert torch.equal(_eval_batch(cfg, eng, mode3), raw)
    assert not torch.equal(raw, averaged), "the average and the raw mappers evaluate alike: the swap shows nothing"
    # a fresh forward-only engine loaded with the averaged mappers computes the same losses
    _, fwd = _build(form, need_backward=False)
    assert fwd.ema is None
    fwd.params.copy_(end["ema"])
    assert torch.equal(_eval_batch(cfg, fwd, mode3), averaged)
    with pytest.raises(RuntimeError, match="ema_decay"):
        fwd.ema_weights()
    # an exception inside the context still swaps back
    with pytest.raises(KeyError):
        with eng.ema_weights():
            raise KeyError("x")
    assert torch.equal(eng.params.cpu(), end["params"]) and torch.equal(eng.ema.cpu(), end["ema"])


def test_engine_ema_weights_only_between_optimizer_steps():
    cfg, eng = _build("accum2", ema_decay=DECAY)
    feed_six(cfg, eng, 0, 0, False)
    assert eng.step() is False
    with pytest.raises(RuntimeError, match="accumulation"):
        eng.ema_weights()
    feed_six(cfg, eng, 0, 1, False)
    assert eng.step() is True


def test_engine_constructor_refusals():
    for kw in (dict(ema_decay=0.0), dict(ema_decay=1.0), dict(ema_decay=-0.5), dict(ema_decay=float("nan")),
               dict(ema_decay=0.9, ema_warmup_power=0.0), dict(ema_decay=0.9, ema_warmup_power=float("inf")),
               dict(ema_decay=0.9, ema_update_after_step=-1), dict(ema_update_after_step=3), dict(ema_warmup_power=0.5),
               dict(ema_decay=0.9, need_backward=False)):
        with pytest.raises(ValueError, match="ema_"):
            _build("one-mapper", **kw)


@pytest.mark.parametrize("form", ["one-mapper", "mode3"])
def test_engine_resume(form):
    """3 + 3 steps against 6 uninterrupted ones: in place after capture, and into a fresh engine before its capture"""
    mode3 = FORMS[form][0]
    kw = dict(ema_decay=DECAY, ema_update_after_step=1, ema_warmup_power=0.75)
    cfg, eng = _build(form, **kw)
    feed_six(cfg, eng, 0, 0, mode3)
    eng.capture()
    run_steps(cfg, eng, range(3), mode3, feed_six)
    sd = eng.state_dict()
    assert sd["ema_count"].tolist()[0] == int(sd["opt_step"]) >= 2 and not sd["ema"].is_cuda
    assert (sd["meta"]["ema_decay"], sd["meta"]["ema_update_after_step"], sd["meta"]["ema_warmup_power"]) == (DECAY, 1, 0.75)
    run_steps(cfg, eng, range(3, 6), mode3, feed_six)
    want = snapshot(eng, STATE + ("ema", "ema_count"))
    assert not torch.equal(want["ema"], sd["ema"])
    graph = eng.graph_a
    eng.load_state_dict(sd)
    assert eng.graph_a is graph, "no re-capture"
    assert torch.equal(eng.ema.cpu(), sd["ema"]) and torch.equal(eng.ema_count.cpu(), sd["ema_count"])
    run_steps(cfg, eng, range(3, 6), mode3, feed_six)
    got = snapshot(eng, STATE + ("ema", "ema_count"))
    for f in want:
        assert torch.equal(want[f], got[f]), f"in place: {f} differs from the uninterrupted run"
    _, fresh = _build(form, **kw)
    fresh.load_state_dict(sd)
    feed_six(cfg, fresh, 3, 0, mode3)
    fresh.capture()
    assert torch.equal(fresh.ema.cpu(), sd["ema"]) and torch.equal(fresh.ema_count.cpu(), sd["ema_count"])
    run_steps(cfg, fresh, range(3, 6), mode3, feed_six)
    got = snapshot(fresh, STATE + ("ema", "ema_count"))
    for f in want:
        assert torch.equal(want[f], got[f]), f"fresh engine: {f} differs from the uninterrupted run"


def test_engine_state_refusals():
    """a state with the average into an engine without it, the reverse, and other settings: each refusal names the field"""
    kw = dict(ema_decay=DECAY, ema_update_after_step=1, ema_warmup_power=0.75)
    _, eng = _build("one-mapper", **kw)
    sd = eng.state_dict()
    assert set(sd) - set(STATE) == {"hyper", "meta", "ema", "ema_count"}
    _, plain = _build("one-mapper")
    assert "ema" not in plain.state_dict() and "ema_decay" not in plain.state_dict()["meta"]
    with pytest.raises(ValueError, match="ema_decay: saved 0.9, this engine None"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="ema_decay: saved None, this engine 0.9"):
        eng.load_state_dict(plain.state_dict())
    _, other = _build("one-mapper", ema_decay=DECAY, ema_warmup_power=0.75)
    with pytest.raises(ValueError, match="ema_update_after_step: saved 1, this engine None"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError, match="ema_update_after_step: saved None, this engine 1"):
        eng.load_state_dict(other.state_dict())
    _, other = _build("one-mapper", ema_decay=DECAY, ema_update_after_step=1)
    with pytest.raises(ValueError, match="ema_warmup_power: saved 0.75, this engine None"):
        other.load_state_dict(sd)
    eng.load_state_dict(sd)  # and its own state fits


# ================================================================================================ Coach
def test_coach_run_with_ema(tmp_path):
    """mode 0, 6 steps, a save and a held-out evaluation every 3"""
    from view_neti_amd.compat import heldout as H
    from view_neti_amd.compat import resume as R
    from view_neti_amd.compat.checkpoint_handler import CheckpointHandler
    from view_neti_amd.engine.text import flatten_mapper_state
    rt.toys(tmp_path / "toys")
    watch = ("--eval.heldout_loss_steps", "3", "--eval.heldout_loss_timesteps", "2")
    cfg_on = rt.mode0_cfg(tmp_path / "toys", tmp_path / "on", "--optim.ema_decay", "0.9", *watch)
    on = rt.coach(cfg_on)
    assert on.engine.ema_decay == 0.9 and on.engine.ema is not None
    at3 = {}
    save = on.save

    def saving(embeds_name, mapper_name):
        save(embeds_name, mapper_name)
        torch.cuda.synchronize()
        at3.setdefault(mapper_name, (on.engine.ema.cpu().clone(), on.engine.params.cpu().clone()))
    on.save = saving
    assert rt.train_counting(on) == 6
    off = rt.coach(rt.mode0_cfg(tmp_path / "toys", tmp_path / "off", *watch))
    assert off.engine.ema is None and rt.train_counting(off) == 6
    run, run_off = cfg_on.log.exp_dir, off.cfg.log.exp_dir
    assert torch.equal(on.engine.params, off.engine.params) and torch.equal(on.engine.rng_state, off.engine.rng_state)
    assert not list(run_off.glob("mapper-ema-*"))
    assert sorted(f.name for f in run.glob("mapper-ema-*")) == ["mapper-ema-final_object.pt", "mapper-ema-steps-3_object.pt",
                                                               "mapper-ema-steps-6_object.pt"]
    ds = on.train_dataset
    for stem in ("mapper-steps-3", "mapper-steps-6", "mapper-final"):
        ema, params = at3[stem + ".pt"]
        _, lookup = CheckpointHandler.load_mapper(run / f"{R.ema_name(stem)}_object.pt", "object",
                                                  ds.placeholder_object_tokens, on.placeholder_object_token_ids)
        (m,) = lookup.values()
        assert torch.equal(flatten_mapper_state(m.mapper_state()), ema), f"{stem}: the file is not the engine's average"
        assert not torch.equal(ema, params)
        # the raw files are what they were: the tensors of the run without the average
        raw, raw_off = rt.mapper_tensors(run / f"{stem}_object.pt"), rt.mapper_tensors(run_off / f"{stem}_object.pt")
        assert raw.keys() == raw_off.keys() and all(torch.equal(raw[k], raw_off[k]) for k in raw), stem
        _, lookup = CheckpointHandler.load_mapper(run / f"{stem}_object.pt", "object", ds.placeholder_object_tokens,
                                                  on.placeholder_object_token_ids)
        assert torch.equal(flatten_mapper_state(next(iter(lookup.values())).mapper_state()), params)
        ck = torch.load(run / f"{R.ema_name(stem)}_object.pt", map_location="cpu", weights_only=False)
        assert not any("ema" in k for k in ck["cfg"]["optim"]) and ck["vneti_ext"]["config_ext"]["optim.ema_decay"] == 0.9
    # the modules hold the raw weights again after a save
    assert torch.equal(flatten_mapper_state(next(iter(on.mapper_object_lookup.values())).mapper_state()), on.engine.params.cpu())
    # the trainer state carries the average; the held-out file has it beside the unchanged raw fields
    state = R.load_state(R.state_file(run, 3))
    assert torch.equal(state["engine"]["ema"], at3["mapper-steps-3.pt"][0]) and state["fingerprint"]["ema_decay"] == 0.9
    assert state["engine"]["ema_count"].tolist()[0] == int(state["engine"]["opt_step"])
    recs, recs_off = H.read_records(run / H.FILE_NAME), H.read_records(run_off / H.FILE_NAME)
    assert [r["step"] for r in recs] == [3, 6] == [r["step"] for r in recs_off]
    for r, r_off in zip(recs, recs_off):
        (o,), (o_off,) = r["objects"].values(), r_off["objects"].values()
        assert list(o) == ["train", "test", "by_timestep", "by_view", "ema"] and "ema" not in o_off
        assert {k: v for k, v in o.items() if k != "ema"} == o_off
        assert list(o["ema"]) == ["train", "test", "by_timestep", "by_view"] and o["ema"]["train"] > 0
        assert o["ema"]["train"] != o["train"]
    del off
    # 3 + 3: the run continued from step 3 ends with the uninterrupted run's average
    cfg_b = rt.mode0_cfg(tmp_path / "toys", tmp_path / "b", "--optim.ema_decay", "0.9", *watch, "--model.mapper_checkpoint_path",
                         str(run / "mapper-steps-3"))
    b = rt.coach(cfg_b)
    assert b.start_step == 3 and torch.equal(b.engine.ema.cpu(), at3["mapper-steps-3.pt"][0])
    assert rt.train_counting(b) == 3
    assert torch.equal(b.engine.ema, on.engine.ema) and torch.equal(b.engine.ema_count, on.engine.ema_count)
    assert torch.equal(b.engine.params, on.engine.params)
    del b
    # a run without the average (or with another decay) cannot continue that state; the switch without the average raises
    for other in ((), ("--optim.ema_decay", "0.99")):
        cfg_x = rt.mode0_cfg(tmp_path / "toys", tmp_path / f"x{len(other)}", *other, "--model.mapper_checkpoint_path",
                             str(run / "mapper-steps-3"))
        with pytest.raises(ValueError, match="ema_decay"):
            rt.coach(cfg_x)
    with pytest.raises(ValueError, match="ema_decay"):
        rt.coach(rt.mode0_cfg(tmp_path / "toys", tmp_path / "v", "--eval.validation_use_ema", "true"))
    assert not (tmp_path / "v").exists(), "refused before anything was written"


def test_coach_validation_use_ema(tmp_path):
    """eval.validation_use_ema: the validator's engine reads the live bucket, which holds the average while it renders — and
    the raw mappers with the switch off; training does not notice either way"""
    rt.toys(tmp_path / "toys")
    val = ("--eval.validation_steps", "3", "--eval.num_denoising_steps", "2", "--eval.num_validation_images", "1",
           "--eval.validation_seeds", "[0]")
    seen, end = {}, {}
    for flag in ("true", "false"):
        cfg = rt.mode0_cfg(tmp_path / "toys", tmp_path / flag, "--optim.ema_decay", "0.9", "--eval.validation_use_ema", flag,
                           *val, max_steps=3)
        coach = rt.coach(cfg)
        assert coach.validator.engine.text.mo.params.data_ptr() == coach.engine.params.data_ptr()

        def spying(step, coach=coach, infer=coach.validator.infer, flag=flag):
            eng = coach.engine
            seen[flag] = (eng._ema_swapped, eng.params.cpu().clone(), eng.ema.cpu().clone())
            infer(step)
        coach.validator.infer = spying
        assert rt.train_counting(coach) == 3
        end[flag] = snapshot(coach.engine, ("params", "ema", "ema_count"))
        assert (cfg.log.exp_dir / "validation-iter_3-denoisesteps_2_upsample_1_imgs_t2i_0.png").exists()
        assert not coach.engine._ema_swapped
        del coach
    assert seen["true"][0] is True and seen["false"][0] is False
    assert torch.equal(seen["true"][1], end["true"]["ema"]) and torch.equal(seen["true"][2], end["true"]["params"])
    assert torch.equal(seen["false"][1], end["false"]["params"]) and torch.equal(seen["false"][2], end["false"]["ema"])
    for f in end["true"]:
        assert torch.equal(end["true"][f], end["false"][f]), f
    assert not torch.equal(end["true"]["ema"], end["true"]["params"])


def test_bf16_library_runs_the_kernel_cases(tmp_path):
    """the kernel cases above against libvneti_hip_bf16.so, in a child pytest process with VNETI_PRECISION=bf16"""
    from view_neti_amd import lib
    if lib.precision() == "bf16":
        return  # this IS the bf16 run
    run_bf16_child(os.path.join("tests", os.path.basename(__file__)), "test_kernel", 240, tmp_path, least=60)
