"""Direct tests of the kernels that hold or draw the trained state (csrc/elementwise.hip) through the C ABI: AdamW with
GradScaler semantics (flat bucket and per-mapper segments), the device RNG (normals, timesteps, nested-dropout masks) and
the small inference helpers (conv1x1_nchw, table_fill_i64, counter_advance).

References.  The optimizer: the real torch.optim.AdamW on float64 CPU parameters, driven with the f32-rounded
hyper-parameters the kernel reads and the unscaled gradients; GradScaler's update rule (backoff 0.5, growth 2,
growth_interval) is restated in `Scaler` (tests/helpers/adamw_ref.py).  The RNG: `hash_u32` and the index formulas restated with numpy uint64
masking — the integer outputs (timesteps, dropout masks) must be EQUAL; the normals are compared with the float64
Box-Muller of the same uniforms, and the statistics of the device output (not of the restatement) are bounded in standard
errors.

Bars.  Everything here is f32 with no 16-bit rounding, so one bar holds in both builds: 1e-5 with `check()`'s element-wise
bound where plain f32 arithmetic can meet it; each parity check also evaluates its reference in torch float32 on the CPU,
e32 = that result's relative Frobenius error against float64, and the bar is 1e-5 if 8 * e32 <= 1e-5, else 8 * e32 (the
AdamW trajectory: 200 steps of f32 rounding in p, m, v).  No bar comes from a kernel's output.  The normals' deviation from
the float64 Box-Muller is the fast intrinsics' (__logf / __cosf) and is not derivable: NORMAL_DEV_MEASURED is the
measurement on an MI355X, the bar four times that and never above 1e-4."""
import math

import numpy as np
import pytest
import torch

from helpers.adamw_ref import (ACTIVITY, N_FLAT, N_SEG, SEG_LEN, Scaler, f32, hyper_dev, i32, spread_gradients,
                               torch_adamw)
from helpers.checks import DEV, check32  # (the f32 bar rule of the docstring: tests/helpers/checks.py)
from helpers.checks import gen as _gen, ops as _ops

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("gdiv", [1.0, 8.0])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("lr", [1e-3, 5e-2])
def test_adamw_flat_trajectory(lr, wd, gdiv):
    """200 steps against torch.optim.AdamW in float64; the displacement p_t - p_0, m and v after steps 1, 2, 10, 200"""
    ops = _ops()
    n, steps, scale = N_FLAT, 200, 65536.0
    p0 = torch.randn(n, generator=_gen(1)) * 0.05
    gs = spread_gradients(n, steps, 2)
    g_dev = (gs * (scale * gdiv)).to(DEV)  # exact: a power of two
    assert torch.equal(g_dev.cpu() / (scale * gdiv), gs)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    scaler = torch.tensor([scale, 0.0, 0.0], device=DEV)
    step, hyper = i32(0), hyper_dev(lr, wd, gdiv)
    refs = {}
    for dt in (torch.float64, torch.float32):
        q = p0.to(dt).clone().requires_grad_(True)
        refs[dt] = (q, torch_adamw([q], lr, wd))
    for s in range(1, steps + 1):
        ops.adamw_flat(p, g_dev[s - 1], m, v, hyper, scaler, step, growth_interval=100000)
        for dt, (q, opt) in refs.items():
            q.grad = gs[s - 1].to(dt)
            opt.step()
        if s in (1, 2, 10, 200):
            torch.cuda.synchronize()
            assert int(step.item()) == s and scaler.cpu().tolist() == [scale, float(s), 0.0]
            (q64, o64), (q32, o32) = refs[torch.float64], refs[torch.float32]
            tag = f"adamw lr={lr} wd={wd} gdiv={gdiv} step {s}"
            check32(tag + " p - p0", p.cpu().double() - p0.double(), q64.detach() - p0.double(),
                    q32.detach().double() - p0.double())
            check32(tag + " m", m, o64.state[q64]["exp_avg"], o32.state[q32]["exp_avg"])
            check32(tag + " v", v, o64.state[q64]["exp_avg_sq"], o32.state[q32]["exp_avg_sq"])


def test_adamw_flat_gradscaler_rule():
    """growth_interval = 4; +inf at the first element, -inf at the last, NaN in the middle of the last block: a skipped step
    leaves p, m, v, step bit-identical, halves the scale, resets the tracker and clears found_inf; four clean steps double
    the scale; the step count counts applied steps only"""
    ops = _ops()
    n, lr, wd = N_FLAT, 1e-3, 1e-2
    inject = {3: (0, math.inf), 6: (n - 1, -math.inf), 9: (256 * (n // 256) + (n % 256) // 2, math.nan)}
    p0 = torch.randn(n, generator=_gen(3)) * 0.05
    gs = spread_gradients(n, 14, 4)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    scaler, step, hyper = torch.tensor([1024.0, 0.0, 0.0], device=DEV), i32(0), hyper_dev(lr, wd, 1.0)
    rule = Scaler(1024.0, 4)
    q = p0.double().clone().requires_grad_(True)
    opt = torch_adamw([q], lr, wd)
    q32 = p0.clone().requires_grad_(True)
    opt32 = torch_adamw([q32], lr, wd)
    scales = []
    for s in range(1, 15):
        g = gs[s - 1] * rule.scale  # the loss scale of this step (a power of two: exact)
        if s in inject:
            g[inject[s][0]] = inject[s][1]
        before = [t.clone() for t in (p, m, v, step)]
        ops.adamw_flat(p, g.to(DEV), m, v, hyper, scaler, step, growth_interval=4)
        torch.cuda.synchronize()
        rule.update(s in inject)
        same = [torch.equal(a, b) for a, b in zip(before, (p, m, v, step))]
        if s in inject:
            assert all(same), f"step {s}: a skipped step changed state {same}"
        else:
            assert not any(same), f"step {s}: a clean step left state unchanged {same}"
            q.grad, q32.grad = gs[s - 1].double(), gs[s - 1].clone()
            opt.step()
            opt32.step()
        assert scaler.cpu().tolist() == [rule.scale, float(rule.tracker), 0.0], f"step {s}: {scaler.cpu().tolist()}"
        assert int(step.item()) == rule.applied
        scales.append(rule.scale)
    assert scales == [1024.0] * 2 + [512.0] * 3 + [256.0] * 3 + [128.0] * 4 + [256.0] * 2 and rule.applied == 11
    check32("adamw gradscaler p - p0 after 11 applied steps", p.cpu().double() - p0.double(), q.detach() - p0.double(),
            q32.detach().double() - p0.double())


def test_adamw_flat_static_scale():
    """growth_interval = 0 (bf16: no GradScaler): a non-finite step is skipped, the scale never moves"""
    ops = _ops()
    n = N_FLAT
    gs = spread_gradients(n, 6, 5)
    p, m, v = (torch.randn(n, generator=_gen(6)) * 0.05).to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    scaler, step, hyper = torch.tensor([8.0, 0.0, 0.0], device=DEV), i32(0), hyper_dev(1e-3, 0.0, 1.0)
    applied = 0
    for s in range(1, 7):
        g = gs[s - 1] * 8.0
        if s == 2:
            g[n // 2] = math.inf
        before = [t.clone() for t in (p, m, v)]
        ops.adamw_flat(p, g.to(DEV), m, v, hyper, scaler, step, growth_interval=0)
        torch.cuda.synchronize()
        same = [torch.equal(a, b) for a, b in zip(before, (p, m, v))]
        assert all(same) if s == 2 else not any(same)
        applied += s != 2
        assert scaler.cpu().tolist() == [8.0, 0.0, 0.0] and int(step.item()) == applied


@pytest.mark.parametrize("clean", [False, True])
def test_adamw_flat_phases_over_two_buckets(clean):
    """CHECK both buckets, APPLY both, FINISH once.  inf in the SECOND bucket: nothing is applied in either; clean: each
    bucket as one OPT_ALL update of its own, the step advanced once"""
    ops = _ops()
    ns = (1000, N_FLAT)
    hyper = hyper_dev(1e-3, 1e-2, 1.0)

    def state():
        out = []
        for i, n in enumerate(ns):
            g = spread_gradients(n, 1, 20 + i)[0] * 16.0
            if not clean and i == 1:
                g[n - 2] = math.inf
            out.append([(torch.randn(n, generator=_gen(10 + i)) * 0.05).to(DEV), g.to(DEV),
                        (torch.randn(n, generator=_gen(12 + i)) * 0.01).to(DEV),
                        (torch.rand(n, generator=_gen(14 + i)) * 1e-4).to(DEV)])
        return out
    bk = state()
    scaler, step = torch.tensor([16.0, 1.0, 0.0], device=DEV), i32(5)
    for phase in (ops.OPT_CHECK, ops.OPT_APPLY):
        for b in bk:
            ops.adamw_flat(*b, hyper, scaler, step, growth_interval=4, phases=phase)
    ops.adamw_flat(*bk[1], hyper, scaler, step, growth_interval=4, phases=ops.OPT_FINISH)
    torch.cuda.synchronize()
    fresh = state()
    if not clean:
        for b, f in zip(bk, fresh):
            assert all(torch.equal(x, y) for x, y in zip(b, f))
        assert scaler.cpu().tolist() == [8.0, 0.0, 0.0] and int(step.item()) == 5
        return
    for b, f in zip(bk, fresh):
        sc, st = torch.tensor([16.0, 1.0, 0.0], device=DEV), i32(5)
        ops.adamw_flat(*f, hyper, sc, st, growth_interval=4)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(b, f))
        assert sc.cpu().tolist() == [16.0, 2.0, 0.0] and int(st.item()) == 6
    assert scaler.cpu().tolist() == [16.0, 2.0, 0.0] and int(step.item()) == 6
    assert not torch.equal(bk[0][0], state()[0][0]) and not torch.equal(bk[1][0], state()[1][0])


def test_adamw_segments_against_torch():
    ops = _ops()
    L, S = SEG_LEN, N_SEG
    lr, wd, scale = 1e-3, 1e-2, 256.0
    p0 = torch.randn(S, L, generator=_gen(30)) * 0.05
    gs = torch.stack([spread_gradients(L, len(ACTIVITY), 31 + s) for s in range(S)], dim=1)  # [steps, S, L]
    p, m, v = p0.clone().to(DEV), torch.zeros(S, L, device=DEV), torch.zeros(S, L, device=DEV)
    seg_step, step = torch.zeros(S, dtype=torch.int32, device=DEV), i32(0)
    scaler, hyper = torch.tensor([scale, 0.0, 0.0], device=DEV), hyper_dev(lr, wd, 1.0)
    refs = {}
    for dt in (torch.float64, torch.float32):
        qs = [p0[s].to(dt).clone().requires_grad_(True) for s in range(S)]
        refs[dt] = (qs, torch_adamw(qs, lr, wd))
    for k, act in enumerate(ACTIVITY):
        active = (act * 8)[:8]
        assert len(set(active)) == len(act)
        g = torch.full((S, L), math.inf)  # stale garbage in the inactive segments must neither skip the step nor leak
        g[:, ::3] = 1e30
        g[:, 1::7] = -math.inf
        for s in act:
            g[s] = gs[k, s] * scale
        ops.adamw_segments(p, g.to(DEV), m, v, L, S, seg_step, i32(*active), hyper, scaler, step, growth_interval=100000)
        for dt, (qs, opt) in refs.items():
            opt.zero_grad(set_to_none=False)  # a segment that had a gradient once keeps a zero gradient: it is stepped
            for s in act:
                qs[s].grad = gs[k, s].to(dt)
            opt.step()
    torch.cuda.synchronize()
    assert int(step.item()) == len(ACTIVITY) and scaler.cpu().tolist() == [scale, float(len(ACTIVITY)), 0.0]
    (q64, o64), (q32, o32) = refs[torch.float64], refs[torch.float32]
    want_steps = [int(o64.state[q]["step"]) if q in o64.state and len(o64.state[q]) else 0 for q in q64]
    assert seg_step.cpu().tolist() == want_steps and want_steps == [12, 11, 0, 9, 10]
    for s in range(S):
        if want_steps[s] == 0:  # never in the update set: untouched, not even decayed
            assert torch.equal(p[s].cpu(), p0[s]) and float(m[s].abs().sum()) == 0 and float(v[s].abs().sum()) == 0
            continue
        assert bool(torch.isfinite(m[s]).all()) and bool(torch.isfinite(v[s]).all())
        tag = f"adamw segments seg {s} ({want_steps[s]} steps)"
        check32(tag + " p - p0", p[s].cpu().double() - p0[s].double(), q64[s].detach() - p0[s].double(),
                q32[s].detach().double() - p0[s].double())
        check32(tag + " m", m[s], o64.state[q64[s]]["exp_avg"], o32.state[q32[s]]["exp_avg"])
        check32(tag + " v", v[s], o64.state[q64[s]]["exp_avg_sq"], o32.state[q32[s]]["exp_avg_sq"])


def test_adamw_segments_skip_and_refusal():
    """an inf in an ACTIVE segment skips the step for every segment (state, seg_step, step bit-identical, scale halved);
    n_active = 9 is refused"""
    ops = _ops()
    L, S = SEG_LEN, N_SEG
    p0 = torch.randn(S, L, generator=_gen(40)) * 0.05
    g = spread_gradients(S * L, 1, 41)[0].reshape(S, L) * 4.0
    g[3, L - 1] = math.inf
    p, m, v = p0.clone().to(DEV), torch.zeros(S, L, device=DEV), torch.zeros(S, L, device=DEV)
    seg_step, step = torch.tensor([2, 0, 0, 1, 0], dtype=torch.int32, device=DEV), i32(2)
    scaler, hyper = torch.tensor([4.0, 3.0, 0.0], device=DEV), hyper_dev(1e-3, 1e-2, 1.0)
    ops.adamw_segments(p, g.to(DEV), m, v, L, S, seg_step, i32(0, 3, 3, 0, 0, 3, 0, 3), hyper, scaler, step, growth_interval=4)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), p0) and float(m.abs().sum()) == 0 and float(v.abs().sum()) == 0
    assert seg_step.cpu().tolist() == [2, 0, 0, 1, 0] and int(step.item()) == 2 and scaler.cpu().tolist() == [2.0, 0.0, 0.0]
    with pytest.raises(RuntimeError, match="adamw_segments"):
        ops.adamw_segments(p, g.to(DEV), m, v, L, S, seg_step, i32(*([0] * 9)), hyper, scaler, step, growth_interval=4)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), p0)


def test_adamw_segments_large_finite_gradient_is_not_skipped():
    """3.2e38 is a finite f32 (FLT_MAX = 3.4028e38): torch's isfinite and adamw_flat apply the step, so must adamw_segments"""
    ops = _ops()
    L, S = SEG_LEN, N_SEG
    lr, wd = 1e-3, 1e-2
    p0 = torch.randn(S, L, generator=_gen(50)) * 0.05
    g = spread_gradients(S * L, 1, 51)[0].reshape(S, L)
    big = 517
    g[1, big] = 3.2e38
    hyper = hyper_dev(lr, wd, 1.0)
    # the flat kernel on segment 1 alone
    pf, mf, vf = p0[1].clone().to(DEV), torch.zeros(L, device=DEV), torch.zeros(L, device=DEV)
    sc_f, st_f = torch.tensor([1.0, 0.0, 0.0], device=DEV), i32(0)
    ops.adamw_flat(pf, g[1].to(DEV), mf, vf, hyper, sc_f, st_f, growth_interval=4)
    # the segments kernel, segment 1 active
    p, m, v = p0.clone().to(DEV), torch.zeros(S, L, device=DEV), torch.zeros(S, L, device=DEV)
    seg_step, step, scaler = torch.zeros(S, dtype=torch.int32, device=DEV), i32(0), torch.tensor([1.0, 0.0, 0.0], device=DEV)
    ops.adamw_segments(p, g.to(DEV), m, v, L, S, seg_step, i32(1, 1, 1, 1, 1, 1, 1, 1), hyper, scaler, step, growth_interval=4)
    torch.cuda.synchronize()
    print(f"[adamw 3.2e38] flat: step {int(st_f.item())} scaler {sc_f.cpu().tolist()}; segments: step {int(step.item())} "
          f"seg_step {seg_step.cpu().tolist()} scaler {scaler.cpu().tolist()}")
    assert int(st_f.item()) == 1 and sc_f.cpu().tolist() == [1.0, 1.0, 0.0], "adamw_flat skipped a finite gradient"
    assert int(step.item()) == 1 and scaler.cpu().tolist() == [1.0, 1.0, 0.0] and seg_step.cpu().tolist() == [0, 1, 0, 0, 0], \
        "adamw_segments skipped a step whose gradients are all finite"
    q = p0[1].double().clone().requires_grad_(True)
    q32 = p0[1].clone().requires_grad_(True)
    for t, o in ((q, torch_adamw([q], lr, wd)), (q32, torch_adamw([q32], lr, wd))):
        t.grad = g[1].to(t.dtype)
        o.step()
    rest = torch.arange(L) != big  # (g^2 overflows f32 at the large element itself: v = inf there, in torch's f32 too)
    for name, got in (("flat", pf), ("segments", p[1])):
        check32(f"adamw 3.2e38 {name} p - p0", (got.cpu().double() - p0[1].double())[rest], (q.detach() - p0[1].double())[rest],
                (q32.detach().double() - p0[1].double())[rest])
    assert float(p[1, big]) == float(pf[big]) and float(m[1, big]) == float(mf[big]) and math.isfinite(float(p[1, big]))
    assert torch.equal(p[0].cpu(), p0[0]) and torch.equal(p[2:].cpu(), p0[2:])


# ------------------------------------------------------------------------------------------ device RNG, restated
M32 = np.uint64(0xFFFFFFFF)


def u64(x):
    return np.asarray(x, dtype=np.uint64)


def hash_u32(x):
    x = u64(x) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def mix(idx, seed, ctr, stream_id, salt):
    """hash(hash(idx * 0x9E3779B1 + seed + stream_id * 0x9E3779B9) ^ (ctr * 0x85EBCA6B + salt)), all mod 2^32"""
    s = (np.uint64(seed) + np.uint64(stream_id) * np.uint64(0x9E3779B9)) & M32
    a = hash_u32((u64(idx) * np.uint64(0x9E3779B1) + s) & M32)
    return hash_u32(a ^ ((np.uint64(ctr) * np.uint64(0x85EBCA6B) + np.uint64(salt)) & M32))


def ref_randint(n, high, seed, ctr, stream_id):
    return (mix(np.arange(n), seed, ctr, stream_id, 0x27D4EB2F) % np.uint64(high)).astype(np.int64)


def ref_normal(n, seed, ctr, stream_id):
    a = mix(np.arange(n), seed, ctr, stream_id, 0x632BE5AB)
    b = hash_u32((a + np.uint64(0x68E31DA4)) & M32)
    u1 = ((a >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 16777216.0  # (0, 1]
    u2 = (b >> np.uint64(8)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def ref_dropout_mask(nl, Bn, hidden, prob, seed, ctr, stream_id):
    hl = mix(np.arange(nl), seed, ctr, stream_id, 0x27D4EB2F)
    fire = (hl >> np.uint64(8)).astype(np.float64) / 16777216.0 < np.float64(np.float32(prob))
    idx = (mix(np.arange(nl * Bn) + 0x10000, seed, ctr, stream_id, 0x27D4EB2F) % np.uint64(hidden)).astype(np.int64)
    keep = ~np.repeat(fire, Bn)[:, None] | (np.arange(hidden)[None, :] < idx[:, None])
    return keep.astype(np.float32), fire, idx.reshape(nl, Bn)


def rng_state(seed, ctr):
    return torch.from_numpy(np.array([seed, ctr], dtype=np.uint32).view(np.int32).copy()).to(DEV)


def state_of(t):
    return t.cpu().numpy().view(np.uint32).tolist()


SEEDS = [0, 1, 77, 12345, 0xdeadbeef]


@pytest.mark.parametrize("seed", [0, 77, 0xdeadbeef])
def test_rng_randint_is_the_restated_hash(seed):
    """pins the stream that checkpoints and bit-identical reruns rely on"""
    ops = _ops()
    for ctr in (0, 1, 1000):
        st = rng_state(seed, ctr)
        for sid in range(6):
            for n in (4, 1000003):
                for high in (1000, 1):
                    out = torch.full((n + 2,), -7, dtype=torch.int64, device=DEV)
                    ops.rng_fill_randint(out[:n], high, st, sid)
                    torch.cuda.synchronize()
                    want = torch.from_numpy(ref_randint(n, high, seed, ctr, sid))
                    assert torch.equal(out[:n].cpu(), want), f"seed {seed} ctr {ctr} stream {sid} n {n} high {high}"
                    assert out[n:].cpu().tolist() == [-7, -7]
        assert state_of(st) == [seed, ctr]


def test_rng_advance_moves_the_counter_only():
    ops = _ops()
    st = rng_state(0xdeadbeef, 0xfffffffe)
    for want in (0xffffffff, 0, 1):
        ops.rng_advance(st)
        torch.cuda.synchronize()
        assert state_of(st) == [0xdeadbeef, want]


NORMAL_DEV_MEASURED = 1.91e-6  # max |z_gpu - z_float64| over 2^20 samples, measured on an MI355X
NORMAL_DEV_BAR = min(4 * NORMAL_DEV_MEASURED, 1e-4)
N_DRAW = 1 << 20


def draw_normal(seed, ctr, sid, n=N_DRAW):
    ops = _ops()
    out = torch.full((n + 2,), 9.0, device=DEV)
    ops.rng_fill_normal(out[:n], rng_state(seed, ctr), sid)
    torch.cuda.synchronize()
    assert out[n:].cpu().tolist() == [9.0, 9.0]
    return out[:n].cpu().double().numpy()


@pytest.mark.parametrize("seed", [0, 0xdeadbeef])
def test_rng_normal_is_box_muller_of_the_restated_uniforms(seed):
    for ctr, sid in ((0, 1), (1000, 2)):
        z = draw_normal(seed, ctr, sid)
        d = float(np.abs(z - ref_normal(N_DRAW, seed, ctr, sid)).max())
        print(f"[rng normal seed {seed} ctr {ctr} stream {sid}] max |z_gpu - z_f64| = {d:.3e} (bar {NORMAL_DEV_BAR:.1e})")
        assert d <= NORMAL_DEV_BAR


def corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def ks_normal(z):
    x = np.sort(z)
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(x) / math.sqrt(2.0)).numpy())
    n = x.size
    i = np.arange(1, n + 1)
    return float(max((i / n - cdf).max(), (cdf - (i - 1) / n).max()))


@pytest.mark.parametrize("seed", SEEDS)
def test_rng_normal_statistics_of_the_device_output(seed):
    """n = 2^20 per draw, counters {0, 1, 2, 1000} x the eps (1) and noise (2) streams: every statistic below 5 standard
    errors, Kolmogorov-Smirnov D sqrt(n) < 1.95 (the 0.1 % critical value), max |z| <= sqrt(2 ln 2^24) (the documented
    truncation)"""
    n, rn = N_DRAW, math.sqrt(N_DRAW)
    for ctr in (0, 1, 2, 1000):
        z = {(c, s): draw_normal(seed, c, s) for c in (ctr, ctr + 1) for s in (1, 2) if not (c == ctr + 1 and s == 2)}
        stats = {}
        for sid in (1, 2):
            x = z[(ctr, sid)]
            mu, var = x.mean(), x.var()
            stats[f"mean s{sid}"] = abs(mu) * rn
            stats[f"var s{sid}"] = abs(var - 1) * math.sqrt(n / 2)
            stats[f"kurt s{sid}"] = abs((x ** 4).mean() - 3) * math.sqrt(n / 96)
            stats[f"lag1 s{sid}"] = abs(corr(x[:-1], x[1:])) * rn
            ks, mx = ks_normal(x) * rn, float(np.abs(x).max())
            print(f"[rng stats seed {seed} ctr {ctr} stream {sid}] KS {ks:.2f} max|z| {mx:.3f}")
            assert ks < 1.95 and mx <= 5.77
        stats["streams 1 x 2"] = abs(corr(z[(ctr, 1)], z[(ctr, 2)])) * rn
        stats["counter c x c+1"] = abs(corr(z[(ctr, 1)], z[(ctr + 1, 1)])) * rn
        print(f"[rng stats seed {seed} ctr {ctr}] " + " ".join(f"{k}={v:.2f}" for k, v in stats.items()))
        bad = {k: v for k, v in stats.items() if not v < 5}
        assert not bad, f"seed {seed} counter {ctr}: beyond 5 standard errors: {bad}"


def chi2_sigma(counts):
    e = counts.sum() / counts.size
    return abs(((counts - e) ** 2 / e).sum() - (counts.size - 1)) / math.sqrt(2 * (counts.size - 1))


def test_rng_timesteps_are_uniform_and_uncorrelated():
    ops = _ops()
    for seed in SEEDS:  # 10^6 draws of one launch over 1000 bins
        out = torch.zeros(1000000, dtype=torch.int64, device=DEV)
        ops.rng_fill_randint(out, 1000, rng_state(seed, 3), 0)
        torch.cuda.synchronize()
        t = out.cpu().numpy()
        assert t.min() >= 0 and t.max() <= 999
        s = chi2_sigma(np.bincount(t, minlength=1000).astype(np.float64))
        print(f"[rng timesteps seed {seed}] chi-square {s:.2f} sigma")
        assert s < 5
    # what training does: n = 4 per step over 20 000 consecutive counters
    steps = 20000
    st = rng_state(77, 0)
    out = torch.zeros(steps, 4, dtype=torch.int64, device=DEV)
    for k in range(steps):
        ops.rng_fill_randint(out[k], 1000, st, 0)
        ops.rng_advance(st)
    torch.cuda.synchronize()
    assert state_of(st) == [77, steps]
    t = out.cpu().numpy()
    assert np.array_equal(t[123], ref_randint(4, 1000, 77, 123, 0)) and np.array_equal(t[-1], ref_randint(4, 1000, 77, steps - 1, 0))
    x = t.astype(np.float64)
    s = chi2_sigma(np.bincount(t.reshape(-1), minlength=1000).astype(np.float64))
    across = max(abs(corr(x[:, j], x[:, j + 1])) for j in range(3)) * math.sqrt(steps)
    along = max(abs(corr(x[:-1, j], x[1:, j])) for j in range(4)) * math.sqrt(steps)
    print(f"[rng timesteps 20000 counters] chi-square {s:.2f} sigma, sample-to-sample {across:.2f}, step-to-step {along:.2f}")
    assert s < 5 and across < 5 and along < 5


def test_nested_dropout_mask():
    """prob 0: all ones; prob 1: every layer fires; prob 0.5 over 2000 counters: the restated hash exactly, one decision per
    layer shared by its samples, fire rate and truncation index within 5 standard errors, mask[r][j] = 1 iff j < idx"""
    ops = _ops()
    nl, Bn, hd, sid, seed = 16, 4, 128, 3, 12345
    for prob in (0.0, 1.0):
        mask = torch.full((nl * Bn, hd), 7.0, device=DEV)
        ops.nested_dropout_mask(mask, nl, Bn, hd, prob, rng_state(seed, 9), sid)
        torch.cuda.synchronize()
        want, fire, _ = ref_dropout_mask(nl, Bn, hd, prob, seed, 9, sid)
        assert torch.equal(mask.cpu(), torch.from_numpy(want)) and bool(fire.all()) == (prob == 1.0)
        assert (float(mask.min()) == 1.0) == (prob == 0.0)
    steps = 2000
    st = rng_state(seed, 0)
    masks = torch.full((steps, nl * Bn, hd), 7.0, device=DEV)
    for k in range(steps):
        ops.nested_dropout_mask(masks[k], nl, Bn, hd, 0.5, st, sid)
        ops.rng_advance(st)
    torch.cuda.synchronize()
    got = masks.cpu().numpy()
    fires, idxs = [], []
    for k in range(steps):
        want, fire, idx = ref_dropout_mask(nl, Bn, hd, 0.5, seed, k, sid)
        assert np.array_equal(got[k], want), f"counter {k}"
        fires.append(fire)
        idxs.append(idx)
    # the structure, from the device output alone
    kept = got.sum(-1).astype(np.int64).reshape(steps, nl, Bn)
    assert np.array_equal(got, (np.arange(hd)[None, None, :] < kept.reshape(steps, nl * Bn, 1)).astype(np.float32))  # prefixes
    fired = kept < hd
    assert np.array_equal(fired.all(-1), fired.any(-1))  # one decision per layer, shared by its samples
    nf = steps * nl
    rate = fired[:, :, 0].mean()
    print(f"[nested dropout] fire rate {rate:.4f} over {nf} layer draws")
    assert abs(rate - 0.5) < 5 * math.sqrt(0.25 / nf)
    ix = kept[fired[:, :, 0]]  # [n_fired, Bn] truncation indices
    assert ix.min() == 0 and ix.max() == hd - 1  # idx = 0 (an all-zero row) occurs
    s = chi2_sigma(np.bincount(ix.reshape(-1), minlength=hd).astype(np.float64))
    eq = (ix[:, 0] == ix[:, 1]).mean()
    print(f"[nested dropout] index chi-square {s:.2f} sigma; samples 0 and 1 of a layer share an index in {eq:.4f} of draws")
    assert s < 5 and abs(eq - 1 / hd) < 5 * math.sqrt((1 / hd) * (1 - 1 / hd) / ix.shape[0])


# ------------------------------------------------------------------------------------------ inference helpers
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("HW", [81, 4096])
def test_conv1x1_nchw(HW, with_bias):
    ops = _ops()
    Bn, scale = 2, f32(1 / 0.18215)
    for Ci in range(1, 9):
        for Co in range(1, 9):
            g = _gen(1000 + 10 * Ci + Co)
            x, W = torch.randn(Bn, Ci, HW, generator=g), torch.randn(Co, Ci, generator=g) * 0.5
            bias = torch.randn(Co, generator=g) if with_bias else None
            out = torch.full((Bn * Co * HW + 3,), 6.0, device=DEV)
            ops.conv1x1_nchw(x.to(DEV), W.to(DEV), None if bias is None else bias.to(DEV), out, Bn, Ci, Co, HW, in_scale=scale)
            torch.cuda.synchronize()
            assert out[Bn * Co * HW:].cpu().tolist() == [6.0] * 3

            def ref(dt):
                r = torch.einsum("oc,bcp->bop", W.to(dt), x.to(dt)) * scale
                return r if bias is None else r + bias.to(dt)[None, :, None]
            check32(f"conv1x1 Ci{Ci} Co{Co} HW{HW} bias={with_bias}", out[:Bn * Co * HW].view(Bn, Co, HW), ref(torch.float64),
                    ref(torch.float32))


def test_table_fill_and_counter_advance():
    ops = _ops()
    table = (torch.randint(0, 1000, (50,), generator=_gen(60)) + (torch.arange(50) << 33)).to(torch.int64)
    step = i32(46)
    t_dev = table.to(DEV)
    for k in range(4):  # the start and three advances: rows 46 .. 49, the last of the table
        dst = torch.full((302,), -1, dtype=torch.int64, device=DEV)
        ops.table_fill_i64(dst[:300], t_dev, step)
        torch.cuda.synchronize()
        assert int(step.item()) == 46 + k
        assert dst.cpu().tolist() == [int(table[46 + k])] * 300 + [-1, -1]
        if k < 3:
            ops.counter_advance(step)
