"""csrc/attention.hip at its edges, against float64: the forward, `attn_bwd_delta`, dQ in both delta forms, dK/dV with and
without the query split, and the one-launch `attn_bwd_small`, at the tile edges, data and refusals where these kernels can
go wrong and tests/test_kernels_gpu.py (unit Gaussians with one spiked key, float32 references) does not look.

References, data and case lists: tests/helpers/attn_ref.py — float64 formulas on the SAME 16-bit-rounded inputs the kernel
gets.  tests/test_attn_ref_cpu.py proves this file FAIR (a float32 model of the kernels' algorithm meets every bar below
with half of it to spare) and SHARP (a tail mask off by one, a moved diagonal, an unwritten row, an overflowing P each
fail it, on this file's own data).

Bars (the suite's own, helpers/checks.py; nothing new): O at t16(3e-3), lse at 1e-3, dQ / dK / dV at t16(6e-3), the
in-kernel delta against the separate launch at 1e-4.  Two stated exceptions (attn_ref.spec has the reasons): on `negative`
data column 0 of every head of dQ is left out of the element-wise bound, not of the Frobenius one; with one key the true
dQ and dK are exactly 0 and are bounded by 1e-4 in absolute value.

Common setup: Bn = 2, H = 3 (odd: head offsets are no multiples of 128 bytes), scale = D^-1/2, every output and the
workspace NaN before the launch (so an element that is not written fails its check), D in {40, 64, 80, 160}.
Operand strides and poisoned surroundings are tests/test_kernel_contracts_gpu.py's subject, not this file's.

What the data kinds reach:
  gauss      the suite's usual data.  It sees a moved causal diagonal (the first rows have few keys) and little else.
  negative   every real score near -6 nat: a key or query that should not be there has weight e^6.  A zero key admitted at
             Nk (`key <= Nk`; loads past the end return zeros), a pad row of an LDS tile taken for a key, a query row past Nq
             that reaches dK / dV.
  staircase  the tile maximum rises 7.5 nat per 64-key tile: P reaches e^7.5 against a STALE maximum (no rescale: under
             the 8-nat threshold), then one rescale.  lse = stale max + log l; the denominator from the "ones" column of the
             PV product (D = 40, 80) sums 16-bit P of magnitude 1e3.
  descend    the first tile holds the maximum; the later tiles' P underflow in 16 bits, never a rescale.

What the shapes reach (Nq, Nk):
  ragged, non-causal  (1, 1) one live lane; (1, 65) one key in the second tile; (33, 1) a second wave with one query;
             (31, 33), (32, 64), (33, 63), (64, 32) either side of the 32-query wave, the 64-key tile and the 32- / 64-query
             stage of dK/dV; (65, 129), (127, 65), (128, 128), (129, 127), (129, 193) either side of the 128-query block of
             forward / dQ and the 128-key block of dK/dV, one row or key into the next
  ragged, causal      (1, 1), (2, 2) rows with one key; (33, 33), (65, 65), (129, 129), (193, 193) the diagonal through the
             last tile, one past a tile edge; (65, 129) keys no query sees (the tile loop stops early, dK/dV blocks with
             nothing to do write zeros); (129, 65) queries that see every key
  softmax    (33, 257), (65, 193) five and four key tiles, the last with one key; (257, 257) causal: three query blocks
             whose tile loops end at different steps of the staircase
  qsplit     the query split of dK/dV: the least that splits, uneven ranges, an EMPTY last range, 64-row stages, two key
             blocks, a workspace that bounds the split, one float short of any split, causal (never split).  Each case
             first asserts its split through `attn_dkv_qsplit`, the function the launcher calls.
  small      N = 1 .. 96 either side of the 32-row roles of `attn_bwd_small`, q / k / v strided views of one qkv buffer

Only O, lse and dV are asserted in the softmax group.  The backward kernels take lse as given and have no running max;
dQ and dK on this data are ill-conditioned BY THE ALGORITHM: with a common component in K, sum_j dS_j = 0 cancels it
exactly in the truth, and the 16-bit rounding of O inside delta leaves k0 * scale * (delta error) behind — the correct
model misses the dQ bar 3.7 x and the dK bar 1.4 x on `staircase`.  They are asserted finite, not with a wider bar.

The file is precision-generic like tests/test_kernels_gpu.py: tests/test_kernels_bf16_gpu.py re-runs it against
libvneti_hip_bf16.so."""
import pytest
import torch

from helpers import attn_ref as A
from helpers.checks import DEV, DT, check
from helpers.checks import ops as _ops
from view_neti_amd import lib as _lib  # (ctypes only: importing it loads no library and touches no GPU)

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAN = float("nan")


@pytest.fixture(autouse=True)
def _no_default_workspace():
    """the default q-split workspace another test of the process may have installed is set aside (and put back): a case
    reaches the split only through the workspace it passes"""
    ops = _ops()
    saved, ops._default_ws = ops._default_ws, None
    yield
    assert ops._default_ws is None, "a case installed a default workspace"
    ops._default_ws = saved


def _nan(*shape, dtype=DT):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rc(name, *args):
    """the raw status of `vneti_<name>` (ops.* raises on a negative one)"""
    return int(getattr(_lib.load(), "vneti_" + name)(*args))


def _upload(cs, Cc):
    return tuple(cs[n].to(DEV).view(-1, Cc) for n in ("q", "k", "v", "do"))


def _forward(qd, kd, vd, Bn, H, Nq, Nk, D, causal):
    o, lse = _nan(Bn * Nq, H * D), _nan(Bn, H, Nq, dtype=F32)
    _ops().attn_fwd(qd, kd, vd, o, lse, Bn, H, Nq, Nk, D, D ** -0.5, causal)
    return o, lse


def _rows(t, Bn):
    return t.view(Bn, -1, t.shape[-1])


# ------------------------------------------------------------------------------------------ ragged tile edges
@pytest.mark.parametrize("kind", A.RAGGED_KINDS)
@pytest.mark.parametrize("shape", A.RAGGED, ids=lambda s: f"{s[0]}x{s[1]}c{s[2]}")
@pytest.mark.parametrize("D", A.HEAD_DIMS)
def test_edges_attn_ragged(D, shape, kind):
    ops = _ops()
    Nq, Nk, causal = shape
    Bn, H, Cc, scale = A.BN, A.H_EDGE, A.H_EDGE * D, D ** -0.5
    cs = A.case(kind, Bn, H, Nq, Nk, D, causal, DT)
    qd, kd, vd, dod = _upload(cs, Cc)
    o, lse = _forward(qd, kd, vd, Bn, H, Nq, Nk, D, causal)
    delta, delta2 = _nan(Bn, H, Nq, dtype=F32), _nan(Bn, H, Nq, dtype=F32)
    dq, dq2 = _nan(Bn * Nq, Cc), _nan(Bn * Nq, Cc)
    ops.attn_bwd_delta(dod, o, delta, Bn, H, Nq, D)
    ops.attn_bwd_dq(qd, kd, vd, dod, lse, delta, dq, Bn, H, Nq, Nk, D, scale, causal)
    ops.attn_bwd_dq(qd, kd, vd, dod, lse, delta2, dq2, Bn, H, Nq, Nk, D, scale, causal, O=o)  # (delta formed in the kernel)
    ws = _nan(2 * 2 * Bn * Nk * Cc, dtype=F32)  # (room for two query ranges)
    assert ops.attn_dkv_qsplit(Bn, H, Nq, Nk, D, causal, ws.numel()) == 1, "fewer than eight query stages: no split"
    dk, dv, dk0, dv0 = (_nan(Bn * Nk, Cc) for _ in range(4))
    ops.attn_bwd_dkv(qd, kd, vd, dod, lse, delta2, dk, dv, Bn, H, Nq, Nk, D, scale, causal, workspace=ws)
    ops.attn_bwd_dkv(qd, kd, vd, dod, lse, delta2, dk0, dv0, Bn, H, Nq, Nk, D, scale, causal)
    torch.cuda.synchronize()
    tag = f"ragged {kind} D{D} {Nq}x{Nk} c{causal}"
    got = {"o": _rows(o, Bn), "lse": lse, "dq": _rows(dq, Bn), "dk": _rows(dk, Bn), "dv": _rows(dv, Bn)}
    A.assert_outputs(tag, "ragged", kind, Nk, H, D, DT, got, cs["ref"])
    A.assert_outputs(tag + " (delta in-kernel)", "ragged", kind, Nk, H, D, DT, {"dq": _rows(dq2, Bn)}, cs["ref"], only=("dq",))
    check(f"{tag} delta(in-kernel)", delta2, delta, 1e-4)
    assert torch.equal(dk, dk0) and torch.equal(dv, dv0), f"{tag}: dK/dV with and without a workspace differ (no split here)"
    assert bool(torch.isnan(ws).all()), f"{tag}: the workspace was written without a split"


# ------------------------------------------------------------------------------------------ the online softmax
@pytest.mark.parametrize("kind", A.SOFTMAX_KINDS)
@pytest.mark.parametrize("shape", A.SOFTMAX_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}c{s[2]}")
@pytest.mark.parametrize("D", A.HEAD_DIMS)
def test_edges_attn_softmax(D, shape, kind):
    ops = _ops()
    Nq, Nk, causal = shape
    Bn, H, Cc, scale = A.BN, A.H_EDGE, A.H_EDGE * D, D ** -0.5
    cs = A.case(kind, Bn, H, Nq, Nk, D, causal, DT)
    qd, kd, vd, dod = _upload(cs, Cc)
    o, lse = _forward(qd, kd, vd, Bn, H, Nq, Nk, D, causal)
    delta, dq = _nan(Bn, H, Nq, dtype=F32), _nan(Bn * Nq, Cc)
    dk, dv = _nan(Bn * Nk, Cc), _nan(Bn * Nk, Cc)
    ops.attn_bwd_dq(qd, kd, vd, dod, lse, delta, dq, Bn, H, Nq, Nk, D, scale, causal, O=o)
    ops.attn_bwd_dkv(qd, kd, vd, dod, lse, delta, dk, dv, Bn, H, Nq, Nk, D, scale, causal)
    torch.cuda.synchronize()
    tag = f"softmax {kind} D{D} {Nq}x{Nk} c{causal}"
    got = {"o": _rows(o, Bn), "lse": lse, "dv": _rows(dv, Bn)}
    A.assert_outputs(tag, "softmax", kind, Nk, H, D, DT, got, cs["ref"])
    assert bool(torch.isfinite(dq.float()).all()) and bool(torch.isfinite(dk.float()).all()), f"{tag}: dQ / dK not finite"


# ------------------------------------------------------------------------------------------ the query split of dK/dV
@pytest.mark.parametrize("kind", A.RAGGED_KINDS)
@pytest.mark.parametrize("case", A.QSPLIT_CASES, ids=lambda c: c[0])
def test_edges_attn_qsplit(case, kind):
    ops = _ops()
    name, D, Nq, Nk, causal, ws_of, split = case
    Bn, H, Cc, scale = A.QSPLIT_BN, A.QSPLIT_H, A.QSPLIT_H * D, D ** -0.5
    plane = Bn * Nk * Cc
    ws = _nan(ws_of(plane) if ws_of else 2 * 32 * plane, dtype=F32)
    assert ops.attn_dkv_qsplit(Bn, H, Nq, Nk, D, causal, ws.numel()) == split, f"{name}: the heuristic changed; the case is empty"
    cs = A.case(kind, Bn, H, Nq, Nk, D, causal, DT)
    qd, kd, vd, dod = _upload(cs, Cc)
    o, lse = _forward(qd, kd, vd, Bn, H, Nq, Nk, D, causal)
    delta, dq = _nan(Bn, H, Nq, dtype=F32), _nan(Bn * Nq, Cc)
    ops.attn_bwd_dq(qd, kd, vd, dod, lse, delta, dq, Bn, H, Nq, Nk, D, scale, causal, O=o)
    dk, dv = _nan(Bn * Nk, Cc), _nan(Bn * Nk, Cc)
    ops.attn_bwd_dkv(qd, kd, vd, dod, lse, delta, dk, dv, Bn, H, Nq, Nk, D, scale, causal, workspace=ws)
    torch.cuda.synchronize()
    tag = f"qsplit {name} {kind}"
    A.assert_outputs(tag, "qsplit", kind, Nk, H, D, DT, {"dk": _rows(dk, Bn), "dv": _rows(dv, Bn)}, cs["ref"])
    if split == 1:
        dk0, dv0 = _nan(Bn * Nk, Cc), _nan(Bn * Nk, Cc)
        ops.attn_bwd_dkv(qd, kd, vd, dod, lse, delta, dk0, dv0, Bn, H, Nq, Nk, D, scale, causal)
        torch.cuda.synchronize()
        assert torch.equal(dk, dk0) and torch.equal(dv, dv0), f"{tag}: split 1 differs from the run without a workspace"
        assert bool(torch.isnan(ws).all()), f"{tag}: the workspace was written without a split"
    else:  # exactly `split` pairs of planes are written, nothing behind them
        used = 2 * split * plane
        assert bool(torch.isfinite(ws[:used]).all()) and bool(torch.isnan(ws[used:]).all()), f"{tag}: partials outside [0, {used})"


# ------------------------------------------------------------------------------------------ attn_bwd_small
def _small_run(cs, Bn, H, N, D, causal, pair):
    """q / k / v as column slices of one [Bn * N, 3 * H * D] buffer, the gradients into the slices of a NaN one -> that
    buffer, from the one-launch kernel or (pair) from dQ (O given) + dK/dV"""
    ops = _ops()
    Cc, scale = H * D, D ** -0.5
    qkv = torch.cat([cs[n].view(Bn * N, Cc) for n in ("q", "k", "v")], 1).to(DEV)
    qd, kd, vd = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
    dod = cs["do"].to(DEV).view(-1, Cc)
    o, lse = _forward(qd, kd, vd, Bn, H, N, N, D, causal)
    dqkv = _nan(Bn * N, 3 * Cc)
    dq, dk, dv = dqkv[:, :Cc], dqkv[:, Cc:2 * Cc], dqkv[:, 2 * Cc:]
    if pair:
        delta = _nan(Bn, H, N, dtype=F32)
        ops.attn_bwd_dq(qd, kd, vd, dod, lse, delta, dq, Bn, H, N, N, D, scale, causal, O=o)
        ops.attn_bwd_dkv(qd, kd, vd, dod, lse, delta, dk, dv, Bn, H, N, N, D, scale, causal)
    else:
        assert ops.attn_bwd_small_ok(N, D)
        ops.attn_bwd_small(qd, kd, vd, dod, o, lse, dq, dk, dv, Bn, H, N, D, scale, causal)
    torch.cuda.synchronize()
    return dqkv


@pytest.mark.parametrize("kind", A.RAGGED_KINDS)
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("N", A.SMALL_N)
def test_edges_attn_small(N, causal, kind):
    Bn, H, D = A.BN, A.H_EDGE, A.SMALL_D
    Cc = H * D
    cs = A.case(kind, Bn, H, N, N, D, causal, DT)
    one, pair = _small_run(cs, Bn, H, N, D, causal, False), _small_run(cs, Bn, H, N, D, causal, True)
    tag = f"small {kind} N{N} c{causal}"
    got = {n: one[:, i * Cc:(i + 1) * Cc].reshape(Bn, N, Cc) for i, n in enumerate(("dq", "dk", "dv"))}
    A.assert_outputs(tag, "small", kind, N, H, D, DT, got, cs["ref"])
    assert torch.equal(one, pair), f"{tag}: the one-launch backward differs from the dQ + dK/dV pair"


@pytest.mark.parametrize("N,D", [(97, 64), (33, 40), (97, 40)], ids=["N97", "D40", "N97_D40"])
def test_edges_attn_small_too_long_or_wide(N, D):
    """sizes the one-launch kernel does not carry: status -2 (the caller takes the two kernels), not one byte written"""
    Bn, H = A.BN, A.H_EDGE
    Cc = H * D
    x = torch.ones(Bn * N, Cc, dtype=DT, device=DEV)
    lse = torch.zeros(Bn, H, N, dtype=F32, device=DEV)
    out = _nan(3, Bn * N, Cc)
    p = lambda t: t.data_ptr()
    rc = _rc("attn_bwd_small", p(x), Cc, p(x), Cc, p(x), Cc, p(x), Cc, p(x), Cc, p(lse), p(out[0]), Cc, p(out[1]), Cc,
             p(out[2]), Cc, Bn, H, N, D, D ** -0.5, 1, _stream())
    torch.cuda.synchronize()
    assert rc == -2 and not _ops().attn_bwd_small_ok(N, D)
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------ refusals
class _Refusal:
    """one-value operands of a (Bn, H, N, N, D) launch with per-operand ld, NaN outputs, and the raw status of the six
    forms of the five entries (dQ with delta given and with O given)"""

    def __init__(self, Bn, H, Nq, Nk, D, pad=0):
        self.shape = (Bn, H, Nq, Nk, D)
        Cc = H * D
        rq, rk = Bn * max(Nq, 1), Bn * max(Nk, 1)
        self.ld = {n: Cc + pad for n in ("q", "k", "v", "do", "o")}
        self.ins = {n: torch.ones(rq if n in ("q", "do", "o") else rk, Cc + pad, dtype=DT, device=DEV) for n in self.ld}
        self.lse = torch.zeros(Bn, H, max(Nq, 1), dtype=F32, device=DEV)
        self.delta_in = torch.zeros_like(self.lse)
        self.outs = {"o": _nan(rq, Cc), "dq": _nan(rq, Cc), "dk": _nan(rk, Cc), "dv": _nan(rk, Cc)}
        self.f32 = {"lse": _nan(Bn, H, max(Nq, 1), dtype=F32), "delta": _nan(Bn, H, max(Nq, 1), dtype=F32)}
        self.ws = _nan(1024, dtype=F32)

    def statuses(self, entries=None):
        Bn, H, Nq, Nk, D = self.shape
        Cc, sc, st = H * D, D ** -0.5, _stream()
        p = lambda t: t.data_ptr()
        i, ld, o, f = self.ins, self.ld, self.outs, self.f32
        qkv = (p(i["q"]), ld["q"], p(i["k"]), ld["k"], p(i["v"]), ld["v"])
        calls = {
            "fwd": lambda: _rc("attn_fwd", *qkv, p(o["o"]), Cc, p(f["lse"]), Bn, H, Nq, Nk, D, sc, 0, st),
            "delta": lambda: _rc("attn_bwd_delta", p(i["do"]), ld["do"], p(i["o"]), ld["o"], p(f["delta"]), Bn, H, Nq, D, st),
            "dq": lambda: _rc("attn_bwd_dq", *qkv, p(i["do"]), ld["do"], p(self.lse), p(self.delta_in), None, 0, p(o["dq"]),
                              Cc, Bn, H, Nq, Nk, D, sc, 0, st),
            "dq_o": lambda: _rc("attn_bwd_dq", *qkv, p(i["do"]), ld["do"], p(self.lse), p(f["delta"]), p(i["o"]), ld["o"],
                                p(o["dq"]), Cc, Bn, H, Nq, Nk, D, sc, 0, st),
            "dkv": lambda: _rc("attn_bwd_dkv", *qkv, p(i["do"]), ld["do"], p(self.lse), p(self.delta_in), p(o["dk"]), Cc,
                               p(o["dv"]), Cc, Bn, H, Nq, Nk, D, sc, 0, p(self.ws), self.ws.numel(), st),
            "small": lambda: _rc("attn_bwd_small", *qkv, p(i["do"]), ld["do"], p(i["o"]), ld["o"], p(self.lse), p(o["dq"]),
                                 Cc, p(o["dk"]), Cc, p(o["dv"]), Cc, Bn, H, Nq, D, sc, 0, st),
        }
        assert Nq == Nk, "the one-launch entry takes one N"
        rcs = {e: calls[e]() for e in (entries or calls)}
        msg = _lib.last_error()
        torch.cuda.synchronize()
        return rcs, msg

    def untouched(self):
        return all(bool(torch.isnan(t).all()) for t in (*self.outs.values(), *self.f32.values(), self.ws))


# which entries read which operand
_TAKES = {"q": ("fwd", "dq", "dq_o", "dkv", "small"), "k": ("fwd", "dq", "dq_o", "dkv", "small"),
          "v": ("fwd", "dq", "dq_o", "dkv", "small"), "do": ("delta", "dq", "dq_o", "dkv", "small"),
          "o": ("delta", "dq_o", "small")}


@pytest.mark.parametrize("D", [48, 128])
def test_edges_attn_refuse_head_dim(D):
    r = _Refusal(2, 3, 33, 33, D)
    rcs, msg = r.statuses()
    print(f"D {D}: {rcs}; last message: {msg}")
    assert all(rc < 0 for rc in rcs.values()) and len(rcs) == 6, rcs
    assert r.untouched()
    assert _lib.query("attn_dkv_qsplit", 2, 3, 33, 33, D, 0, 1 << 20) < 0


def test_edges_attn_refuse_no_queries():
    r = _Refusal(2, 3, 0, 0, 64)
    rcs, msg = r.statuses()
    print(f"Nq 0: {rcs}; last message: {msg}")
    assert all(rc < 0 for rc in rcs.values()) and len(rcs) == 6, rcs
    assert r.untouched()


@pytest.mark.parametrize("which", list(_TAKES))
def test_edges_attn_refuse_ld_not_multiple_of_8(which):
    """16-byte row loads: every input ld must be a multiple of 8.  Each operand in turn, through every entry that reads it
    (the rows are allocated 8 wider, so ld = H * D + 4 would address nothing out of range)"""
    r = _Refusal(2, 3, 33, 33, 64, pad=8)
    r.ld[which] = 3 * 64 + 4
    rcs, msg = r.statuses(_TAKES[which])
    print(f"ld({which}) = {r.ld[which]}: {rcs}; last message: {msg}")
    assert all(rc < 0 for rc in rcs.values()) and set(rcs) == set(_TAKES[which]), rcs
    assert r.untouched()


@pytest.mark.parametrize("which", list(_TAKES))
def test_edges_attn_refuse_operand_of_2_gib(which):
    """the size guard: Q, K, V, dO and O are read through 32-bit buffer descriptors, so Bn * N * ld * 2 bytes must stay
    under 0x7fffffff.  One batch, one head, one query, one key, D = 64, one-row tensors, ld = 2^30 for the operand under
    test: 2^31 bytes by the formula, while only row 0 exists and only row 0 can be addressed — the case forms no address
    out of range even on a library without the guard.  ld = 2^30 - 8 (2^31 - 16 bytes) is accepted."""
    r = _Refusal(1, 1, 1, 1, 64)
    r.ld[which] = 1 << 30
    rcs, msg = r.statuses(_TAKES[which])
    print(f"ld({which}) = 2^30: {rcs}; last message: {msg}")
    assert all(rc < 0 for rc in rcs.values()) and set(rcs) == set(_TAKES[which]), rcs
    assert "2 GiB" in msg
    assert r.untouched()
    r.ld[which] = (1 << 30) - 8
    rcs, _ = r.statuses(_TAKES[which])
    assert all(rc == 0 for rc in rcs.values()), rcs
