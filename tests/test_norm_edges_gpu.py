"""csrc/norms.hip at its edges, against float64: GroupNorm (one-launch, three-launch and two-launch forms, and the forward
that consumes producer-fused sums), LayerNorm and the row softmax, at the group geometries, capacities, dtype paths and
input statistics where these kernels can go wrong and tests/test_kernels_gpu.py (the train step's own shapes, identically
distributed groups, float32 references) does not look.

References and data: tests/helpers/norm_ref.py — float64 formulas on the SAME 16-bit-rounded inputs the kernel gets, and
`group_data`, whose groups all differ in mean and spread; tests/test_norm_ref_cpu.py proves on every GroupNorm shape below
that ONE channel normalised with its neighbour group's statistics fails `check` even at the bf16 bar.

Bars (the suite's own, helpers/checks.py; nothing new): y at t16(2e-3); dx at t16(4e-3), or 4e-3 when dx is f32; f32 mean /
rstd on benign data by the `check32` rule.  Offset-dominated groups (|mean| = 64 std): y and dx at the same bars, mean at
1e-5, rstd at 1e-3 — an rstd error e moves every y by a relative e, so half the fp16 y bar is what rstd may spend.  The
statistics are formed from f32 partial sums of x and x^2 (include/vneti.h states the contract); ratios 16, 128 and 256 are
measured and printed (DESIGN.md section 6 holds the table), only finiteness is asserted there.

The file is precision-generic like tests/test_kernels_gpu.py: tests/test_kernels_bf16_gpu.py re-runs it against
libvneti_hip_bf16.so."""
import itertools
import math

import pytest
import torch

from helpers import norm_ref as R
from helpers.checks import DEV, DT, check, check32, rel, rnd, t16
from helpers.checks import ops as _ops
from view_neti_amd import lib as _lib  # (ctypes only: importing it loads no library and touches no GPU)

pytestmark = pytest.mark.gpu

EPS = 1e-5
SLOTS = 8


def _rc(name, *args):
    """the raw status of `vneti_<name>` (ops.* raises on a negative one)"""
    return int(getattr(_lib.load(), "vneti_" + name)(*args))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------ GroupNorm: geometry
# what each (Bn, HW, C, G) of R.GN_EDGE_SHAPES reaches:
#   (2, 64, 128, 32)    cpg 4: two whole groups per 8-channel chunk
#   (2, 50, 192, 32)    cpg 6: chunks straddle at offsets 2 and 4; the one-launch kernel
#   (2, 50, 224, 32)    cpg 7 (odd: the slab kernels only): a straddle at every offset
#   (2, 36, 96, 8)      cpg 12, Bn * G < 64: `auto` takes the slab kernels
#   (1, 81, 320, 32)    a batch-1 inference level
#   (2, 108, 640, 32)   the 12 x 9 level of the 768 x 576 evaluation
#   (2, 7, 256, 64)     the largest G: gacc[64 * 4] full
#   (2, 2560, 256, 32), (2, 2048, 320, 32)   the forward one-launch kernel exactly full (10240 pairs); backward: slabs
#   (2, 2048, 256, 32)  the backward one-launch kernel exactly full (8192 pairs)
#   (2, 2049, 256, 32)  one pixel past that
#   (2, 16, 4096, 32)   cpg 128: sga[128] full; C / 8 = 512 > TX (the cb += TX walk in the slab kernels)
#   (2, 16, 4160, 32)   cpg 130: too wide for the one-launch kernel
#   (1, 5, 8320, 64)    C > 8192: rows per slab clamped to 1
def _gn_run(c, shape, silu, form, x=None, mean_rstd=None):
    """forward + backward (with accum) of one form on the case's data -> y, dx, mean, rstd (device tensors)"""
    ops = _ops()
    Bn, HW, C, G = shape
    xd = (c["x"] if x is None else x).to(DEV).view(Bn * HW, C)
    dyd, acc = c["dy"].to(DEV).view(Bn * HW, C), c["acc"].to(DEV).view(Bn * HW, C)
    ga, be = c["gamma"].to(DEV), c["beta"].to(DEV)
    y, dx = torch.zeros_like(xd), torch.zeros_like(xd)
    mean = torch.zeros(Bn * G, dtype=torch.float32, device=DEV)
    rstd = torch.zeros_like(mean)
    ws = torch.zeros(ops.groupnorm_ws_floats(Bn, HW, C, G), dtype=torch.float32, device=DEV)
    if form == "2l":
        fs = torch.zeros(Bn, SLOTS, G, 4, dtype=torch.int64, device=DEV)
        bs = torch.zeros(Bn, SLOTS, G, 4, dtype=torch.int64, device=DEV)
        ops.groupnorm_fwd_2l(xd, y, ga, be, fs, SLOTS, mean, rstd, Bn, HW, C, G, EPS, silu)
        ops.groupnorm_bwd_2l(dyd, xd, ga, be, mean, rstd, dx, bs, SLOTS, ws, Bn, HW, C, G, silu, accum=acc)
    else:
        if mean_rstd is None:
            ops.groupnorm_fwd(xd, y, ga, be, mean, rstd, ws, Bn, HW, C, G, EPS, silu)
        else:  # (the forward ran elsewhere: a producer-fused one)
            y, mean, rstd = None, *mean_rstd
        ops.groupnorm_bwd(dyd, xd, ga, be, mean, rstd, dx, ws, Bn, HW, C, G, silu, accum=acc)
    torch.cuda.synchronize()
    return y, dx, mean, rstd


def _dx_minus_acc(dx, c, shape):
    Bn, HW, C, _ = shape
    return dx.view(Bn, HW, C).float().cpu() - c["acc"].float()


@pytest.mark.parametrize("form", ["auto", "no_small", "2l"])
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("shape", R.GN_EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edges_groupnorm_geometry(shape, silu, form, monkeypatch):
    Bn, HW, C, G = shape
    if form == "no_small":
        monkeypatch.setenv("VNETI_GN_NO_SMALL", "1")
    c = R.gn_case(shape, bool(silu), DT)
    ref, ref32 = c["ref"], c["ref32"]
    y, dx, mean, rstd = _gn_run(c, shape, silu, form)
    tag = f"gn {form} {shape} silu{silu}"
    check(f"{tag} y", y.view(Bn, HW, C), ref["y"], t16(2e-3))
    check(f"{tag} dx", _dx_minus_acc(dx, c, shape), ref["dx"], t16(4e-3))
    check32(f"{tag} mean", mean.view(Bn, G), ref["mean"], ref32["mean"])
    check32(f"{tag} rstd", rstd.view(Bn, G), ref["rstd"], ref32["rstd"])
    if form == "2l":
        _, _, mean_a, rstd_a = _gn_run(c, shape, silu, "auto")
        check(f"{tag} mean == auto", mean, mean_a, 1e-5)
        check(f"{tag} rstd == auto", rstd, rstd_a, 1e-5)


@pytest.mark.parametrize("why", list(R.GN_REFUSED))
def test_edges_groupnorm_refusals(why):
    """shapes outside the kernels' geometry: a negative status from every entry, a negative workspace size, and not one
    byte of the outputs written.  cpg = 5 is the shape the slab kernels would compute WRONGLY (three groups in one
    8-channel chunk); the others would index out of their tables."""
    Bn, HW, C, G = R.GN_REFUSED[why]
    ld = (C + 7) // 8 * 8
    st = _stream()
    x = rnd(Bn * HW, ld, seed=1).to(DEV)
    dy = rnd(Bn * HW, ld, seed=2).to(DEV)
    out = torch.full((Bn * HW, ld), 7.0, dtype=DT, device=DEV)
    ga, be = torch.ones(ld, device=DEV), torch.zeros(ld, device=DEV)
    stats = torch.full((2, Bn * max(G, 64)), 3.0, device=DEV)
    ws = torch.zeros(1 << 16, device=DEV)
    sums = torch.zeros(Bn, SLOTS, max(G, 64), 4, dtype=torch.int64, device=DEV)
    p = lambda t: t.data_ptr()
    m, r = p(stats[0]), p(stats[1])
    assert _lib.query("groupnorm_ws_floats", Bn, HW, C, G) < 0
    rcs = {
        "fwd": _rc("groupnorm_fwd", p(x), ld, p(out), ld, p(ga), p(be), m, r, p(ws), Bn, HW, C, G, EPS, 1, st),
        "fwd_sums": _rc("groupnorm_fwd_sums", p(x), ld, p(out), ld, p(ga), p(be), p(sums), SLOTS, m, r, Bn, HW, C, G, EPS, 1, st),
        "fwd_2l": _rc("groupnorm_fwd_2l", p(x), ld, p(out), ld, p(ga), p(be), p(sums), SLOTS, m, r, Bn, HW, C, G, EPS, 1, st),
        "bwd": _rc("groupnorm_bwd", p(dy), ld, p(x), ld, p(ga), p(be), m, r, p(out), ld, None, 0, p(ws), Bn, HW, C, G, 1, st),
        "bwd_2l": _rc("groupnorm_bwd_2l", p(dy), ld, p(x), ld, p(ga), p(be), m, r, p(out), ld, None, 0, p(sums), SLOTS, p(ws),
                      Bn, HW, C, G, 1, st),
    }
    msg = _lib.last_error()
    torch.cuda.synchronize()
    print(f"{why} {(Bn, HW, C, G)}: {rcs}; last message: {msg}")
    assert all(rc < 0 for rc in rcs.values()), rcs
    assert bool((out == 7.0).all()) and bool((stats == 3.0).all()) and int(sums.abs().sum()) == 0
    if why == "cpg5":
        assert "three groups" in msg


# ------------------------------------------------------------------------------------------ GroupNorm: offset-dominated
def _producer_gemm(ratio, hint):
    """x [2, 256, 320] as ops.gemm stores it (M 512, K 64, N 320), the per-channel f32 bias carrying the group means and
    every column of A B^T scaled to std 0.25; the epilogue's slot sums"""
    ops = _ops()
    Bn, HW, C, G = R.GN_RATIO_SHAPE
    M, K = Bn * HW, 64
    A = rnd(M, K, seed=61)
    B0 = rnd(C, K, scale=1.0 / math.sqrt(K), seed=62, dtype=torch.float64)
    B = (B0 * (R.RATIO_STD / (A.double() @ B0.T).std(0, unbiased=False)).reshape(C, 1)).to(DT)
    bias = R.group_stats(1, G, ratio)[0].reshape(G, 1).expand(G, C // G).reshape(C).float()
    out = torch.zeros(M, C, dtype=DT, device=DEV)
    sums = torch.zeros(Bn, SLOTS, G, 4, dtype=torch.int64, device=DEV)
    ops.gemm(A.to(DEV), B.to(DEV), out, bias=bias.to(DEV), tile_hint=hint, split_k=1, gn_sums=sums, gn_hw=HW, gn_groups=G,
             gn_slots=SLOTS)
    return (Bn, HW, C, G), out, sums


def _producer_conv_in(ratio):
    """x [1, 256, 128] as ops.conv3x3_in stores it (3 channels, 16 x 16), bias and scaling as in `_producer_gemm`"""
    import torch.nn.functional as F
    from view_neti_amd import packing
    ops = _ops()
    Bn, Ci, H, W, Co, G = 1, 3, 16, 16, 128, 32
    x = rnd(Bn, Ci, H, W, seed=21, dtype=torch.float32)
    w0 = rnd(Co, Ci, 3, 3, scale=0.3, seed=22, dtype=torch.float64)
    s = F.conv2d(x.to(DT).double(), w0, None, padding=1).std((0, 2, 3), unbiased=False)
    w = (w0 * (R.RATIO_STD / s).reshape(Co, 1, 1, 1)).to(DT)
    bias = R.group_stats(1, G, ratio)[0].reshape(G, 1).expand(G, Co // G).reshape(Co).float()
    out = torch.zeros(Bn * H * W, Co, dtype=DT, device=DEV)
    sums = torch.zeros(Bn, SLOTS, G, 4, dtype=torch.int64, device=DEV)
    xd = x.to(DEV)
    ops.conv3x3_in(xd, packing.conv_in_direct(w).to(DEV), bias.to(DEV), out, Bn, Ci, H, W, xd.stride(), gn_sums=sums,
                   gn_hw=H * W, gn_groups=G, gn_slots=SLOTS)
    return (Bn, H * W, Co, G), out, sums


def _producer_case(shape, x, silu):
    """the case dict of R.gn_case for a tensor a producer stored (the reference is of the STORED values)"""
    Bn, HW, C, G = shape
    gamma, beta = R.gn_affine(C)
    dy, acc = rnd(Bn, HW, C, seed=22), rnd(Bn, HW, C, seed=23)
    return {"x": x, "dy": dy, "acc": acc, "gamma": gamma, "beta": beta,
            "ref": R.groupnorm_ref(x, gamma, beta, G, EPS, silu, dy=dy)}


RATIO_PATHS = ["small", "slab", "2l", "gemm3", "gemm7", "gemm17", "conv_in"]


@pytest.mark.parametrize("ratio", R.GN_RATIOS)
@pytest.mark.parametrize("path", RATIO_PATHS)
def test_edges_groupnorm_offset_dominated(path, ratio, monkeypatch):
    """every group's |mean| = `ratio` x its std (0.25): what the f32 partial sums of x and x^2 leave of the variance.
    ratio 64 is held to the bars of the module docstring; 16, 128 and 256 are measured, printed and must be finite."""
    ops = _ops()
    silu = 1
    if path in ("small", "slab", "2l"):
        shape = R.GN_RATIO_SHAPE
        c = R.gn_case(shape, True, DT, ratio)
        if path != "small":
            monkeypatch.setenv("VNETI_GN_NO_SMALL", "1")  # (also for 2l: without it this shape takes the one-launch kernel)
        y, dx, mean, rstd = _gn_run(c, shape, silu, "2l" if path == "2l" else "auto")
    else:
        shape, x, sums = _producer_conv_in(ratio) if path == "conv_in" else _producer_gemm(ratio, int(path[4:]))
        Bn, HW, C, G = shape
        torch.cuda.synchronize()
        c = _producer_case(shape, x.cpu().view(Bn, HW, C), True)
        y = torch.zeros_like(x)
        mean = torch.zeros(Bn * G, dtype=torch.float32, device=DEV)
        rstd = torch.zeros_like(mean)
        ops.groupnorm_fwd_sums(x, y, c["gamma"].to(DEV), c["beta"].to(DEV), sums, SLOTS, mean, rstd, Bn, HW, C, G, EPS, silu)
        _, dx, _, _ = _gn_run(c, shape, silu, "auto", mean_rstd=(mean, rstd))
    Bn, HW, C, G = shape
    ref = c["ref"]
    got_ratio = R.achieved_ratio(c["x"], G)
    dxm = _dx_minus_acc(dx, c, shape)
    ey, edx = rel(y.view(Bn, HW, C).cpu(), ref["y"]), rel(dxm, ref["dx"])
    em, er = rel(mean.view(Bn, G).cpu(), ref["mean"]), rel(rstd.view(Bn, G).cpu(), ref["rstd"])
    print(f"[ratio-table] {path} ratio {ratio} (achieved {got_ratio.min().item():.0f}..{got_ratio.max().item():.0f}): "
          f"y {ey:.2e} dx {edx:.2e} mean {em:.2e} rstd {er:.2e}")
    assert all(math.isfinite(e) for e in (ey, edx, em, er))
    if ratio != 64:
        return
    assert got_ratio.min() >= 40 and got_ratio.max() <= 90, "the data drifted from the stated ratio: a defect of the test"
    tag = f"gn {path} ratio 64"
    check(f"{tag} y", y.view(Bn, HW, C), ref["y"], t16(2e-3))
    check(f"{tag} dx", dxm, ref["dx"], t16(4e-3))
    check(f"{tag} mean", mean.view(Bn, G), ref["mean"], 1e-5)
    check(f"{tag} rstd", rstd.view(Bn, G), ref["rstd"], 1e-3)


# ------------------------------------------------------------------------------------------ LayerNorm
def _ln_inputs(rows, C, x_dt, dy_dt, dx_dt, offset=0.5, seed=24):
    x = (rnd(rows, C, seed=seed, dtype=torch.float32) * 2 + offset).to(x_dt)
    gamma = 1 + 0.1 * rnd(C, seed=25, dtype=torch.float32)
    beta = 0.1 * rnd(C, seed=26, dtype=torch.float32)
    dy = rnd(rows, C, seed=27, dtype=torch.float32).to(dy_dt)
    acc = rnd(rows, C, seed=28, dtype=torch.float32).to(dx_dt)
    return x, gamma, beta, dy, acc


def _ln_run_and_check(tag, rows, C, x_dt, dy_dt, dx_dt, offset=0.5, copy=False):
    ops = _ops()
    x, gamma, beta, dy, acc = _ln_inputs(rows, C, x_dt, dy_dt, dx_dt, offset)
    ref = R.layernorm_ref(x, gamma, beta, EPS, dy=dy)
    ref32 = R.layernorm_ref(x, gamma, beta, EPS, dtype=torch.float32)
    xd = x.to(DEV)
    y = torch.zeros(rows, C, dtype=DT, device=DEV)
    mean = torch.zeros(rows, dtype=torch.float32, device=DEV)
    rstd = torch.zeros_like(mean)
    ops.layernorm_fwd(xd, y, gamma.to(DEV), beta.to(DEV), mean, rstd, EPS)
    dx = torch.zeros(rows, C, dtype=dx_dt, device=DEV)
    c16 = torch.full((rows, C + 8), 7.0, dtype=DT, device=DEV) if copy else None
    ops.layernorm_bwd(dy.to(DEV), xd, gamma.to(DEV), mean, rstd, dx, accum=acc.to(DEV),
                      f16_copy=c16[:, :C] if copy else None)
    torch.cuda.synchronize()
    check(f"{tag} y", y, ref["y"], t16(2e-3))
    check32(f"{tag} mean", mean, ref["mean"], ref32["mean"])
    check32(f"{tag} rstd", rstd, ref["rstd"], ref32["rstd"])
    check(f"{tag} dx", dx.float().cpu() - acc.float(), ref["dx"], 4e-3 if dx_dt == torch.float32 else t16(4e-3))
    if copy:
        want = dx.to(DT) if dx_dt == torch.float32 else dx
        assert torch.equal(c16[:, :C], want), f"{tag}: the 16-bit copy is not dx rounded to {DT}"
        assert bool((c16[:, C:] == 7.0).all()), f"{tag}: the 16-bit copy wrote past its columns"


# (1, 8) one live lane; (5, 520) NC 2 with a ragged second chunk row (65 chunks), the last block one row; (3, 1544) NC 4
# ragged; (2, 2048) NC 4 full
@pytest.mark.parametrize("f32", [False, True], ids=["x16", "x32"])
@pytest.mark.parametrize("rows,C", [(1, 8), (5, 520), (3, 1544), (2, 2048)])
def test_edges_layernorm_shapes(rows, C, f32):
    dt = torch.float32 if f32 else DT
    _ln_run_and_check(f"ln ({rows}, {C}) f32={f32}", rows, C, dt, DT, dt)


@pytest.mark.parametrize("dy32,x32,dx32", list(itertools.product([False, True], repeat=3)),
                         ids=lambda v: "32" if v else "16")
def test_edges_layernorm_bwd_dtype_paths(dy32, x32, dx32):
    """all eight (dy, x, dx) instantiations of the backward kernel, with the accumulator and the 16-bit copy (the text
    engine's own combination is 16 / 32 / 32 with the copy)"""
    f = lambda is32: torch.float32 if is32 else DT
    _ln_run_and_check(f"ln bwd dy{'32' if dy32 else '16'} x{'32' if x32 else '16'} dx{'32' if dx32 else '16'}", 5, 520,
                      f(x32), f(dy32), f(dx32), copy=True)


def test_edges_layernorm_offset_dominated_rows():
    """row mean = 50 x the row std, f32 x: the kernel is two-pass (mean first, then the squares of x - mean), so the
    ordinary bars hold"""
    _ln_run_and_check("ln mean 50 std", 5, 520, torch.float32, DT, torch.float32, offset=100.0)


@pytest.mark.parametrize("rows,C", [(2, 2056), (2, 12), (0, 64)], ids=["C2056", "C12", "rows0"])
def test_edges_layernorm_refusals(rows, C):
    st = _stream()
    ld = (C + 7) // 8 * 8
    x = rnd(2, ld, seed=1).to(DEV)
    out = torch.full((2, ld), 7.0, dtype=DT, device=DEV)
    ga, be = torch.ones(ld, device=DEV), torch.zeros(ld, device=DEV)
    stats = torch.full((2, 2), 3.0, device=DEV)
    p = lambda t: t.data_ptr()
    rc_f = _rc("layernorm_fwd", p(x), 0, ld, p(out), ld, p(ga), p(be), p(stats[0]), p(stats[1]), rows, C, EPS, st)
    rc_b = _rc("layernorm_bwd", p(x), 0, ld, p(x), 0, ld, p(ga), p(stats[0]), p(stats[1]), p(out), 0, ld, None, 0, None, 0,
               rows, C, st)
    torch.cuda.synchronize()
    print(f"rows {rows} C {C}: fwd {rc_f} bwd {rc_b}: {_lib.last_error()}")
    assert rc_f < 0 and rc_b < 0
    assert bool((out == 7.0).all()) and bool((stats == 3.0).all())


# ------------------------------------------------------------------------------------------ softmax rows
def _softmax_rows(cols, which, seed):
    """three rows of one launch.  'dominant': a +40 entry at column 0 / at the last column / a constant row;
    'underflow': every third entry -60000 (its exp is 0) / a plain row / -60000 entries AND the +40 at the last column"""
    x = rnd(3, cols, seed=seed, dtype=torch.float32)
    if which == "dominant":
        x[0, 0] = 40.0
        x[1, -1] = 40.0
        x[2] = 1.25
    else:
        x[0, 1::3] = -60000.0
        x[2, 0::3] = -60000.0
        x[2, -1] = 40.0
    return x.to(DT)


# 8: one live thread; 520: 65 chunks; 2056: 257 chunks, the second chunk of thread 0 alone; 16384: every register in use
@pytest.mark.parametrize("which", ["dominant", "underflow"])
@pytest.mark.parametrize("cols,pad", [(8, 0), (520, 8), (2056, 0), (16384, 0)])
def test_edges_softmax_rows(cols, pad, which):
    ops = _ops()
    x = _softmax_rows(cols, which, seed=30 + cols % 7)
    ref = R.softmax_ref(x)
    buf = torch.full((3, cols + pad), 7.0, dtype=DT, device=DEV)
    buf[:, :cols] = x.to(DEV)
    ops.softmax_rows(buf[:, :cols], 3, cols)
    torch.cuda.synchronize()
    check(f"softmax {cols} ld {cols + pad} {which}", buf[:, :cols], ref, t16(2e-3))
    assert bool((buf[:, cols:] == 7.0).all())


@pytest.mark.parametrize("cols", [16392, 12])
def test_edges_softmax_refusals(cols):
    ld = (cols + 7) // 8 * 8
    buf = torch.full((3, ld), 7.0, dtype=DT, device=DEV)
    rc = _rc("softmax_rows_f16", buf.data_ptr(), ld, 3, cols, _stream())
    torch.cuda.synchronize()
    print(f"cols {cols}: {rc}: {_lib.last_error()}")
    assert rc < 0 and bool((buf == 7.0).all())
