"""Memory contracts of the tiled kernels: what a kernel may read, what it must write, and that nothing is carried from one
launch to the next.  The parity files run every kernel once, on exact-size tensors, into zeroed outputs; the engines run
them on views into wider buffers (include/vneti.h: "views into wider buffers"), over scratch that is never zeroed, on
buffers that are dirty from the previous graph replay.  Here every operand lives in a guarded slab (tests/helpers/slabs.py:
64 guard rows in front, 256 behind, an `ld` gap of its own) and every case is launched three times:

  run A, clean      the surroundings of the inputs, the outputs and the scratch buffers are all zero
  run B, poisoned   same buffers and offsets; the surroundings of every input are NaN, every output is a sentinel NaN
                    throughout (logical region included), every scratch / workspace buffer is NaN throughout; what the
                    header says "the caller zeroes" (gn_sums) is zero inside and an integer pattern in its guards
  run C, replay     the same launch again on B's buffers as they are (only the caller-zeroed sums are zeroed again and the
                    input of an in-place kernel is copied in again)

and asserts: B against the fp32 / fp64 CPU reference at the tolerance of the matching parity test; B's output bits == A's (the
result depends on nothing outside the logical extents and on no prior contents of outputs or scratch); C's bits == B's
(no race, no carried state); after B and after C the surroundings of every output still hold the sentinel, no logical
element does (everything owned was written, nothing else), and every input slab is bit-identical to what was uploaded.
A stray store these cases can detect lands inside the case's own slab by construction.

Precision-generic like tests/test_kernels_gpu.py (the bf16 build runs it through tests/test_kernels_bf16_gpu.py).  Every
case passes its workspace explicitly; the process-wide default workspace is set aside for the duration of a case, so the
file neither depends on nor changes the order of the tests."""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import slabs as S
from helpers.checks import DEV, DT, check, t16, rnd  # the kernel files' bars
from helpers.checks import attn_ref as _attn_ref, ops as _ops

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(autouse=True)
def _no_default_workspace():
    """the default split-K / q-split workspace another test of the process may have installed is set aside (and put back):
    a case reaches a split path only through the workspace it passes"""
    ops = _ops()
    saved, ops._default_ws = ops._default_ws, None
    yield
    assert ops._default_ws is None, "a contract case installed a default workspace"
    ops._default_ws = saved


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


class Case:
    """the slabs of one case and its three runs"""

    def __init__(self):
        self.ins, self.outs, self.zeroed, self.inplace, self.scratch = [], [], [], [], []
        self.gaps = set()

    def _gap(self, gap):
        if gap is None:  # a different ld gap for every operand of the call: the smallest multiple of 8 not yet taken
            gap = next(g for g in range(8, 8 * 64, 8) if g not in self.gaps)
        if gap:
            assert gap not in self.gaps, "two operands of one call share an ld gap"
            self.gaps.add(gap)
        return gap

    def inp(self, name, values, gap=None, batch=1):
        """input matrix `[rows, cols]` (`[batch, rows, cols]`) with row stride cols + gap; gap = 0: contiguous (vectors)"""
        rows, cols = values.shape[-2:] if values.dim() >= 2 else (1, values.shape[0])
        s = S.Slab.matrix(rows, cols, values.dtype, gap=self._gap(gap), batch=batch, device=DEV)
        s.name = name
        self.ins.append((s, values))
        return s.view if values.dim() >= 2 else s.view.view(-1)

    def vec(self, name, values):
        """contiguous f32 input (bias, gamma, beta): guards in front and behind"""
        return self.inp(name, values.reshape(1, -1), gap=0).view(values.shape)

    def image(self, name, values):
        s = S.Slab.image(*values.shape, values.dtype, device=DEV)
        s.name = name
        self.ins.append((s, values))
        return s.view

    def out(self, name, rows, cols, dtype=None, gap=None, batch=1):
        s = S.Slab.matrix(rows, cols, DT if dtype is None else dtype, gap=self._gap(gap), batch=batch, device=DEV)
        s.name = name
        self.outs.append(s)
        return s.view

    def outvec(self, name, *shape):
        """contiguous f32 output (mean, rstd, lse, delta)"""
        return self.out(name, math.prod(shape[:-1]), shape[-1], dtype=F32, gap=0).view(*shape)

    def sums(self, name, Bn, slots, G):
        """caller-zeroed 64-bit fixed-point GroupNorm slot sums [Bn][slots][G][4]"""
        s = S.Slab.matrix(Bn * slots * G, 4, torch.int64, gap=0, device=DEV)
        s.name, s.sums_shape = name, (Bn, slots, G, 4)
        self.zeroed.append(s)
        return s.view.view(Bn, slots, G, 4)

    def inout(self, name, values, gap=None):
        s = S.Slab.matrix(*values.shape, values.dtype, gap=self._gap(gap), device=DEV)
        s.name = name
        self.inplace.append((s, values))
        return s.view

    def ws(self, nfloats):
        w = torch.empty(int(nfloats), dtype=F32, device=DEV)
        self.scratch.append(w)
        return w

    # ------------------------------------------------------------------------------------------------------------------
    def _results(self):
        ops = _ops()
        res = [(s, s.logical_bits()) for s in self.outs + [s for s, _ in self.inplace]]
        dec = [(s, ops.gn_sums_decode(s.view.view(s.sums_shape).sum(1))) for s in self.zeroed]
        return res, dec

    def _compare(self, what, a, b):
        for (s, x), (_, y) in zip(a[0], b[0]):
            S.first_difference(x, y, s, f"{s.name}: {what}")
        for (s, x), (_, y) in zip(a[1], b[1]):
            assert torch.equal(x, y), f"{s.name}: {what}: the decoded GroupNorm sums differ by {(x - y).abs().max().item()}"

    def _contract(self, run, snaps):
        for s in self.outs:
            s.outside_intact(S.SENTINEL[s.dtype], f"{s.name} after run {run}")
            s.logical_has_no_sentinel(S.SENTINEL[s.dtype], f"{s.name} after run {run}")
        for s, _ in self.inplace:
            s.outside_intact(S.SENTINEL[s.dtype], f"{s.name} after run {run}")
        for s in self.zeroed:
            s.outside_intact(S.INT_PATTERN, f"{s.name} after run {run}")
        for (s, _), snap in zip(self.ins, snaps):
            s.unchanged(snap, f"{s.name} after run {run}")

    def run(self, call, verify):
        # ---- A: clean
        for s, v in self.ins + self.inplace:
            s.fill_all(0)
            s.fill_logical(v)
        for s in self.outs + self.zeroed:
            s.fill_all(0)
        for w in self.scratch:
            w.zero_()
        call()
        torch.cuda.synchronize()
        a = self._results()
        # ---- B: poisoned
        for s, _ in self.ins:
            s.fill_outside(S.QNAN[s.dtype])
        for s in self.outs:
            s.fill_all(S.SENTINEL[s.dtype])
        for s, v in self.inplace:
            s.fill_all(S.SENTINEL[s.dtype])
            s.fill_logical(v)
        for s in self.zeroed:
            s.fill_all(S.INT_PATTERN)
            s.fill_logical(0)
        for w in self.scratch:
            w.fill_(float("nan"))
        snaps = [s.snapshot() for s, _ in self.ins]
        call()
        torch.cuda.synchronize()
        self._contract("B", snaps)
        b = self._results()
        verify()
        self._compare("run B (poisoned surroundings, sentinel outputs, NaN scratch) differs from run A (all clean)", a, b)
        # ---- C: replay on B's buffers
        for s in self.zeroed:
            s.fill_logical(0)
        for s, v in self.inplace:
            s.fill_logical(v)
        call()
        torch.cuda.synchronize()
        self._contract("C", snaps)
        self._compare("run C (replay) differs from run B", b, self._results())


# ------------------------------------------------------------------------------------------ GEMM
GM, GN, GK = 300, 328, 512   # ragged M and N tiles for every tile shape, 8 K-tiles, more than one block each way


def _gemm_operands(c, M=GM, batch=1, seedbase=100):
    A = rnd(*((batch, M, GK) if batch > 1 else (M, GK)), seed=seedbase + 1)
    B = rnd(GN, GK, scale=1.0 / math.sqrt(GK), seed=seedbase + 2)
    return A, B, c.inp("A", A, gap=24, batch=batch), c.inp("B", B)


@pytest.mark.parametrize("hint", [3, 4, 7, 13, 16, 17, 103])
def test_contract_gemm_plain(hint):
    """bias + residual + row-add (rows_per_group 75), one hint per kernel structure"""
    ops, c = _ops(), Case()
    A, B, Ad, Bd = _gemm_operands(c)
    bias, res, radd = rnd(GN, seed=103, dtype=F32), rnd(GM, GN, seed=104), rnd(GM // 75, GN, seed=105)
    biasd, resd, raddd = c.vec("bias", bias), c.inp("resid", res), c.inp("rowadd", radd)
    out = c.out("C", GM, GN)
    ref = (A.float() @ B.float().t() + bias).to(DT).float() + radd.float().repeat_interleave(75, 0) + res.float()
    c.run(lambda: ops.gemm(Ad, Bd, out, bias=biasd, resid=resd, rowadd=raddd, rows_per_group=75, tile_hint=hint, split_k=1),
          lambda: check(f"contract gemm hint{hint}", out, ref, t16(2e-3)))


@pytest.mark.parametrize("hint", [3, 17])
@pytest.mark.parametrize("f32", [False, True], ids=["f16out", "f32out"])
def test_contract_gemm_split_k(hint, f32):
    """split_k = 3: the partials go through a NaN workspace; the reduce kernel's epilogue"""
    ops, c = _ops(), Case()
    A, B, Ad, Bd = _gemm_operands(c)
    bias = rnd(GN, seed=103, dtype=F32)
    res = rnd(GM, GN, seed=104, dtype=F32 if f32 else DT)
    biasd, resd = c.vec("bias", bias), c.inp("resid", res)
    out = c.out("C", GM, GN, dtype=F32 if f32 else DT)
    ws = c.ws(3 * GM * GN)
    ref = A.float() @ B.float().t() + bias
    ref = ref + res if f32 else ref.to(DT).float() + res.float()
    c.run(lambda: ops.gemm(Ad, Bd, out, bias=biasd, resid=resd, workspace=ws, split_k=3, tile_hint=hint),
          lambda: check(f"contract gemm split3 hint{hint} f32={f32}", out, ref, 2e-3 if f32 else t16(2e-3)))


def test_contract_gemm_batched_shared_b():
    """batch = 3 with a shared B: every batch matrix has guard rows of its own, the space between batches is poison"""
    ops, c = _ops(), Case()
    M = 100
    A, B, Ad, Bd = _gemm_operands(c, M=M, batch=3)
    out = c.out("C", M, GN, batch=3)
    c.run(lambda: ops.gemm(Ad, Bd, out, batch=3, strideA=Ad.stride(0), strideB=0, strideC=out.stride(0), M=M,
                           lda=Ad.stride(1), ldc=out.stride(1), split_k=1),
          lambda: check("contract gemm batched", out, A.float() @ B.float().t(), t16(2e-3)))


@pytest.mark.parametrize("hint", [3, 17])
def test_contract_gemm_gate_and_second_output(hint):
    ops, c = _ops(), Case()
    A, B, Ad, Bd = _gemm_operands(c)
    bias, pre = rnd(GN, seed=103, dtype=F32), rnd(GM, GN, seed=106, scale=1.5)
    biasd, pred = c.vec("bias", bias), c.inp("gate", pre)
    out, out2 = c.out("C", GM, GN), c.out("C2", GM, GN)
    x = pre.float().requires_grad_(True)
    F.silu(x).sum().backward()
    ref = ((A.float() @ B.float().t() + bias).to(DT).float() * x.grad).to(DT).float()

    def verify():
        check(f"contract gemm gate hint{hint}", out, ref, t16(2e-3))
        check(f"contract gemm out2 hint{hint}", out2, F.silu(out.float().cpu()), t16(1e-3))
    c.run(lambda: ops.gemm(Ad, Bd, out, bias=biasd, gate=pred, gate_act=1, out2=out2, act2=1, split_k=1, tile_hint=hint), verify)


@pytest.mark.parametrize("hint", [3, 17])
def test_contract_gemm_geglu(hint):
    """GEGLU forward (pre-activation + gated output from one launch) and backward (d_h | d_g) at M = 300, C = 64"""
    from view_neti_amd import packing
    ops, c = _ops(), Case()
    M, Cc = 300, 64
    F4 = 4 * Cc
    x, W = rnd(M, Cc, seed=61), rnd(2 * F4, Cc, scale=1.0 / math.sqrt(Cc), seed=62)
    b = rnd(2 * F4, seed=63, dtype=F32)
    dy, W2 = rnd(M, Cc, seed=64), rnd(Cc, F4, scale=1.0 / math.sqrt(F4), seed=65)
    idx = packing.geglu_interleave_index(2 * F4)
    xd, Wd, bd = c.inp("x", x), c.inp("W", packing.geglu_interleave(W)), c.vec("bias", packing.geglu_interleave(b))
    dyd, W2d = c.inp("dy", dy), c.inp("W2t", W2.t().contiguous())
    p, gg, dp = c.out("pre", M, 2 * F4), c.out("gated", M, F4), c.out("dpre", M, 2 * F4)

    def call():
        ops.gemm(xd, Wd, p, bias=bd, out2=gg, geglu=1, split_k=1, tile_hint=hint)
        ops.gemm(dyd, W2d, dp, gate=p, gate_act=ops.ACT_GELU, geglu=2, split_k=1, tile_hint=hint)

    def verify():
        pre = (x.float() @ W.float().t() + b).to(DT).float()
        check(f"contract geglu pre hint{hint}", p, pre[:, idx], t16(2e-3))
        inv = torch.empty_like(idx)
        inv[idx] = torch.arange(2 * F4)
        pu = p.float().cpu()[:, inv]
        check(f"contract geglu gate hint{hint}", gg, pu[:, :F4] * F.gelu(pu[:, F4:]), t16(1e-3))
        d = (dy.float() @ W2.float()).to(DT).float()
        hg = pu.clone().requires_grad_(True)
        (hg[:, :F4] * F.gelu(hg[:, F4:]) * d).sum().backward()
        check(f"contract geglu bwd hint{hint}", dp, hg.grad[:, idx], t16(2e-3))
    c.run(call, verify)


@pytest.mark.parametrize("hint", [7, 17])
def test_contract_gemm_gn_sums_and_fwd_sums(hint):
    """GroupNorm statistics from the epilogue into caller-zeroed slot sums (integer pattern in their guards) and the
    one-launch GroupNorm that consumes them"""
    ops, c = _ops(), Case()
    Bn, HW, Cc, G, slots, K = 2, 256, 320, 32, 8, 512
    M = Bn * HW
    A, B = rnd(M, K, seed=61), rnd(Cc, K, scale=1.0 / math.sqrt(K), seed=62)
    bias, res = rnd(Cc, seed=63, dtype=F32) * 2, rnd(M, Cc, seed=64)
    gamma, beta = rnd(Cc, seed=65, dtype=F32) * 0.1 + 1, rnd(Cc, seed=66, dtype=F32) * 0.1
    Ad, Bd, biasd, resd = c.inp("A", A, gap=24), c.inp("B", B), c.vec("bias", bias), c.inp("resid", res)
    gd, bd = c.vec("gamma", gamma), c.vec("beta", beta)
    out, y = c.out("C", M, Cc), c.out("y", M, Cc)
    mean, rstd = c.outvec("mean", 1, Bn * G), c.outvec("rstd", 1, Bn * G)
    sums = c.sums("gn_sums", Bn, slots, G)

    def call():
        ops.gemm(Ad, Bd, out, bias=biasd, resid=resd, tile_hint=hint, split_k=1, gn_sums=sums, gn_hw=HW, gn_groups=G,
                 gn_slots=slots)
        ops.groupnorm_fwd_sums(out, y, gd, bd, sums, slots, mean, rstd, Bn, HW, Cc, G, 1e-5, True)

    def verify():
        ref = (A.float() @ B.float().t() + bias).to(DT).float() + res.float()
        check(f"contract gemm+gn out hint{hint}", out, ref, t16(2e-3))
        x = out.float().cpu().reshape(Bn, HW, G, Cc // G)
        got = ops.gn_sums_decode(sums.sum(1))
        check(f"contract gn sums hint{hint}", got[..., 0], x.sum((1, 3)), 1e-3)
        check(f"contract gn sumsq hint{hint}", got[..., 1], (x * x).sum((1, 3)), 1e-5)
        xn = out.float().cpu().reshape(Bn, HW, Cc).permute(0, 2, 1)
        yr = F.silu(F.group_norm(xn, G, gamma, beta, 1e-5)).permute(0, 2, 1).reshape(M, Cc)
        check(f"contract gn fwd_sums hint{hint}", y, yr, t16(2e-3))
        xg = xn.reshape(Bn, G, -1)
        check("contract gn mean", mean.cpu().reshape(Bn, G), xg.mean(-1), 1e-4)
        check("contract gn rstd", rstd.cpu().reshape(Bn, G), (xg.var(-1, unbiased=False) + 1e-5).rsqrt(), 1e-4)
    c.run(call, verify)


# ------------------------------------------------------------------------------------------ conv
def _conv_fwd_case(case, x, w, bias):
    Bn, Ci, H, W = x.shape
    xf, wf = x.float(), w.float()
    base = dict(mode=1, Hi=H, Wi=W, Ci=Ci, ups=0)
    if case == "s1":
        return F.conv2d(xf, wf, bias, padding=1), dict(base, Ho=H, Wo=W, stride=1, pad_t=1, pad_l=1)
    if case == "s2p1":
        return F.conv2d(xf, wf, bias, stride=2, padding=1), dict(base, Ho=H // 2, Wo=W // 2, stride=2, pad_t=1, pad_l=1)
    if case == "s2vae":
        return (F.conv2d(F.pad(xf, (0, 1, 0, 1)), wf, bias, stride=2, padding=0),
                dict(base, Ho=H // 2, Wo=W // 2, stride=2, pad_t=0, pad_l=0))
    return (F.conv2d(F.interpolate(xf, scale_factor=2.0, mode="nearest"), wf, bias, padding=1),
            dict(base, Ho=2 * H, Wo=2 * W, stride=1, pad_t=1, pad_l=1, ups=1))


def _image_rows(c, name, x):
    """NCHW reference tensor -> the NHWC rows `[Bn*H*W, Ci]` as a channel slice [:, :Ci] of a slab with ldx = Ci + 64 (the way
    a skip concat is read)"""
    Bn, Ci, H, W = x.shape
    return c.inp(name, _nhwc(x).reshape(Bn * H * W, Ci), gap=64)


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("korder", [0, 1], ids=["tap-major", "chunk-major"])
@pytest.mark.parametrize("hint", [7, 17])
@pytest.mark.parametrize("case", ["s1", "s2p1", "s2vae", "ups"])
def test_contract_conv_fwd(case, hint, korder, split):
    """the row-major implicit GEMM forward, fused and split-K, with an explicit (NaN) workspace"""
    from view_neti_amd import packing
    ops, c = _ops(), Case()
    Bn, Ci, Co, H, W = 2, 128, 128, 12, 20
    x, w = rnd(Bn, Ci, H, W, seed=11), rnd(Co, Ci, 3, 3, scale=1 / math.sqrt(9 * Ci), seed=12)
    bias = rnd(Co, seed=13, dtype=F32)
    ref, conv = _conv_fwd_case(case, x, w, bias)
    M = Bn * conv["Ho"] * conv["Wo"]
    xd, wd, bd = _image_rows(c, "x", x), c.inp("w", packing.conv3x3_fwd(w, cm=bool(korder))), c.vec("bias", bias)
    conv.update(ldx=xd.stride(0), korder=korder)
    out = c.out("C", M, Co)
    ws = c.ws(3 * M * Co)
    c.run(lambda: ops.gemm(xd, wd, out, bias=bd, conv=conv, M=M, tile_hint=hint, workspace=ws, split_k=split),
          lambda: check(f"contract conv {case} hint{hint} korder{korder} split{split}", out.view(Bn, conv["Ho"], conv["Wo"], Co),
                        _nhwc(ref), t16(2e-3)))


def test_contract_conv_fwd_deep_level_heuristic_split():
    """a deep UNet level (1280 -> 320 channels on an 8 x 8 grid): split_k = 0 with a 16 MiB workspace must really split"""
    from view_neti_amd import packing
    ops, c = _ops(), Case()
    Bn, Ci, Co, H, W = 1, 1280, 320, 8, 8
    x, w = rnd(Bn, Ci, H, W, seed=11), rnd(Co, Ci, 3, 3, scale=1 / math.sqrt(9 * Ci), seed=12)
    bias = rnd(Co, seed=13, dtype=F32)
    ref, conv = _conv_fwd_case("s1", x, w, bias)
    M = Bn * H * W
    xd, wd, bd = _image_rows(c, "x", x), c.inp("w", packing.conv3x3_fwd(w, cm=True)), c.vec("bias", bias)
    conv.update(ldx=xd.stride(0), korder=1)
    out = c.out("C", M, Co)
    ws = c.ws(4 * 2 ** 20)
    assert ops.gemm_select_split(M, Co, 9 * Ci, 1, 17, ws.numel() * 4) > 1, "the heuristic does not split this shape"
    c.run(lambda: ops.gemm(xd, wd, out, bias=bd, conv=conv, M=M, tile_hint=17, workspace=ws, split_k=0),
          lambda: check("contract conv deep level", out.view(Bn, H, W, Co), _nhwc(ref), t16(2e-3)))


@pytest.mark.parametrize("shape,epi,split", [((2, 128, 128, 16, 32), "bias", 1), ((2, 128, 128, 16, 32), "resid+rowadd+gn", 1),
                                             ((1, 192, 320, 16, 32), "resid", 2)], ids=["plain", "resid+rowadd+gn", "split2"])
def test_contract_conv_halo_tile(shape, epi, split):
    """tile 18 (the 18 x 18 input patch of a 64-channel chunk resident in LDS): plain, with the resnet epilogue, split-K"""
    from view_neti_amd import packing
    ops, c = _ops(), Case()
    Bn, Ci, Co, H, W = shape
    x, w = rnd(Bn, Ci, H, W, seed=21), rnd(Co, Ci, 3, 3, scale=1 / math.sqrt(9 * Ci), seed=22)
    bias = rnd(Co, seed=23, dtype=F32)
    M, G, slots = Bn * H * W, Co // 8, 4
    ref = F.conv2d(x.float(), w.float(), bias, padding=1)
    xd, wd, bd = _image_rows(c, "x", x), c.inp("w", packing.conv3x3_fwd(w, cm=True)), c.vec("bias", bias)
    kw = dict(bias=bd)
    if epi != "bias":
        res = rnd(M, Co, seed=24)
        ref = ref + res.float().view(Bn, H, W, Co).permute(0, 3, 1, 2)
        kw.update(resid=c.inp("resid", res))
    sums = None
    if epi == "resid+rowadd+gn":
        temb = rnd(Bn, Co, seed=25)
        ref = ref + temb.float()[:, :, None, None]
        sums = c.sums("gn_sums", Bn, slots, G)
        kw.update(rowadd=c.inp("rowadd", temb), rows_per_group=H * W, gn_sums=sums, gn_hw=H * W, gn_groups=G, gn_slots=slots)
    conv = dict(mode=1, Hi=H, Wi=W, Ci=Ci, Ho=H, Wo=W, stride=1, pad_t=1, pad_l=1, ups=0, ldx=xd.stride(0), korder=1)
    out = c.out("C", M, Co)
    ws = c.ws(max(split, 2) * M * Co)

    def verify():
        check(f"contract conv halo {epi}", out.view(Bn, H, W, Co), _nhwc(ref), t16(3e-3) if split > 1 else t16(2e-3))
        if sums is not None:
            got = ops.gn_sums_decode(sums.sum(1))
            xg = out.double().cpu().view(Bn, H * W, G, Co // G)
            check("contract halo gn sum", got[..., 0].float(), xg.sum((1, 3)).float(), 1e-4)
            check("contract halo gn sumsq", got[..., 1].float(), (xg * xg).sum((1, 3)).float(), 1e-4)
    c.run(lambda: ops.gemm(xd, wd, out, conv=conv, M=M, tile_hint=18, split_k=split, workspace=ws, **kw), verify)


@pytest.mark.parametrize("hint", [3, 17])
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("stride,vae", [(1, False), (2, False), (2, True)], ids=["s1", "s2p1", "s2vae"])
def test_contract_conv_dgrad(stride, vae, split, hint):
    """the transposed gather of the input gradient (tap-major K for hint 3, chunk-major for 17)"""
    from view_neti_amd import packing
    ops, c = _ops(), Case()
    Bn, Ci, Co, H, W = 2, 64, 128, 12, 20
    korder = 1 if hint == 17 else 0
    x = rnd(Bn, Ci, H, W, seed=14).float().requires_grad_(True)
    w = rnd(Co, Ci, 3, 3, scale=1 / math.sqrt(9 * Ci), seed=15)
    y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w.float(), None, stride=2, padding=0) if vae else \
        F.conv2d(x, w.float(), None, stride=stride, padding=1)
    pt = 0 if vae else 1
    dy = rnd(*y.shape, seed=16)
    y.backward(dy.float())
    Ho, Wo, M = y.shape[2], y.shape[3], Bn * H * W
    dyd, wd = _image_rows(c, "dy", dy), c.inp("w", packing.conv3x3_dgrad(w, cm=bool(korder)))
    conv = dict(mode=2, Hi=Ho, Wi=Wo, Ci=Co, Ho=H, Wo=W, stride=stride, pad_t=pt, pad_l=pt, ups=0, ldx=dyd.stride(0), korder=korder)
    dx = c.out("dx", M, Ci)
    ws = c.ws(3 * M * Ci)
    c.run(lambda: ops.gemm(dyd, wd, dx, conv=conv, M=M, workspace=ws, split_k=split, tile_hint=hint),
          lambda: check(f"contract dgrad s{stride} vae={vae} split{split} hint{hint}", dx.view(Bn, H, W, Ci), _nhwc(x.grad),
                        t16(2e-3)))


def test_contract_conv_dgrad_halo_silu_gate():
    from view_neti_amd import packing
    ops, c = _ops(), Case()
    Bn, Co, Ci, H, W = 2, 128, 64, 16, 32  # dy has Co channels, dx has Ci
    x = rnd(Bn, Ci, H, W, seed=31).float().requires_grad_(True)
    w = rnd(Co, Ci, 3, 3, scale=1 / math.sqrt(9 * Ci), seed=32)
    y = F.conv2d(x, w.float(), None, padding=1)
    dy = rnd(*y.shape, seed=33)
    y.backward(dy.float())
    M = Bn * H * W
    pre = rnd(M, Ci, seed=34)
    s = torch.sigmoid(pre.float())
    ref = x.grad * (s * (1 + pre.float() * (1 - s))).view(Bn, H, W, Ci).permute(0, 3, 1, 2)
    dyd, wd, pred = _image_rows(c, "dy", dy), c.inp("w", packing.conv3x3_dgrad(w, cm=True)), c.inp("gate", pre)
    conv = dict(mode=2, Hi=H, Wi=W, Ci=Co, Ho=H, Wo=W, stride=1, pad_t=1, pad_l=1, ups=0, ldx=dyd.stride(0), korder=1)
    dx = c.out("dx", M, Ci)
    c.run(lambda: ops.gemm(dyd, wd, dx, conv=conv, M=M, split_k=1, tile_hint=18, gate=pred, gate_act=1),
          lambda: check("contract dgrad halo gate", dx.view(Bn, H, W, Ci), _nhwc(ref), t16(3e-3)))


@pytest.mark.parametrize("H,W,gn", [(9, 21, False), (16, 16, True)], ids=["9x21", "16x16+gn_sums"])
def test_contract_conv_in_direct(H, W, gn):
    """conv_in straight from a strided f32 pixel window (channel, row and batch strides): the ragged 9 x 21 image (567 rows:
    a partly filled last block of 256 pixels), and — the entry point takes gn_sums only when H * W % 256 == 0 and refuses 9 x 21
    with them — the smallest image it takes them for, 16 x 16, with the GroupNorm sums"""
    from view_neti_amd import packing
    ops, c = _ops(), Case()
    Bn, Ci, Co, G, slots = 3, 3, 128, 32, 8
    x = rnd(Bn, Ci, H, W, seed=21, dtype=F32)
    w, bias = rnd(Co, Ci, 3, 3, scale=0.3, seed=22), rnd(Co, seed=23, dtype=F32)
    xd, wd, bd = c.image("pixels", x), c.inp("w", packing.conv_in_direct(w), gap=0), c.vec("bias", bias)
    out = c.out("C", Bn * H * W, Co)
    sums = c.sums("gn_sums", Bn, slots, G) if gn else None

    def verify():
        ref = F.conv2d(x.to(DT).float(), w.float(), bias, padding=1)
        check(f"contract conv_in direct {H}x{W}", out.reshape(Bn, H, W, Co), _nhwc(ref), t16(2e-3))
        if gn:
            xo = out.float().cpu().reshape(Bn, H * W, G, Co // G)
            got = ops.gn_sums_decode(sums.sum(1))
            check("contract conv_in gn sums", got[..., 0], xo.sum((1, 3)), 1e-3)
            check("contract conv_in gn sumsq", got[..., 1], (xo * xo).sum((1, 3)), 1e-5)
    c.run(lambda: ops.conv3x3_in(xd, wd, bd, out, Bn, Ci, H, W, xd.stride(), gn_sums=sums, gn_hw=H * W if gn else 0,
                                 gn_groups=G if gn else 0, gn_slots=slots if gn else 0), verify)


def test_contract_conv_im2col_small():
    """the 64-wide im2col rows of a 4-channel image (the ABI takes them contiguous: the zero padding 36..63 is written)"""
    ops, c = _ops(), Case()
    Bn, Ci, H, W = 2, 4, 16, 16
    x = rnd(Bn, Ci, H, W, seed=17, dtype=F32)
    xd = c.image("x", x)
    col = c.out("col", Bn * H * W, 64, gap=0)
    ref = torch.zeros(Bn * H * W, 64)
    u = F.unfold(x.to(DT).float(), 3, padding=1).view(Bn, Ci, 9, H * W)          # [b][c][tap][pixel]
    ref[:, :9 * Ci] = u.permute(0, 3, 2, 1).reshape(Bn * H * W, 9 * Ci)          # k = tap * C + c

    def verify():
        check("contract im2col", col, ref, t16(2e-3))
        assert float(col[:, 9 * Ci:].abs().max()) == 0
    c.run(lambda: ops.im2col3x3_small(xd, col, Bn, Ci, H, W, H, W, 1, 1, 1, xd.stride()), verify)


# ------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("silu", [True, False], ids=["silu", "nosilu"])
@pytest.mark.parametrize("Cc,HW", [(320, 256), (320, 4096), (960, 100)])
@pytest.mark.parametrize("form", ["auto", "no_small", "2l"])
def test_contract_norm_groupnorm_fwd_bwd(form, Cc, HW, silu, monkeypatch):
    """forward + backward (with accum) in the three forms; x, y, dy, dx, accum are column slices of wider rows"""
    ops, c = _ops(), Case()
    if form == "no_small":
        monkeypatch.setenv("VNETI_GN_NO_SMALL", "1")
    Bn, G, eps, slots = 2, 32, 1e-5, 8
    M = Bn * HW
    x = (rnd(Bn, HW, Cc, seed=19).float() * 1.5 + 0.3).to(DT)
    gamma, beta = 1 + 0.1 * rnd(Cc, seed=20, dtype=F32), 0.1 * rnd(Cc, seed=21, dtype=F32)
    dy, acc = rnd(Bn, HW, Cc, seed=22), rnd(M, Cc, seed=23)
    xr = x.float().permute(0, 2, 1).requires_grad_(True)
    yr = F.group_norm(xr, G, gamma, beta, eps)
    yr = F.silu(yr) if silu else yr
    yr.backward(dy.float().permute(0, 2, 1))
    xd, dyd, accd = c.inp("x", x.view(M, Cc)), c.inp("dy", dy.view(M, Cc)), c.inp("accum", acc)
    gd, bd = c.vec("gamma", gamma), c.vec("beta", beta)
    y, dx = c.out("y", M, Cc), c.out("dx", M, Cc)
    mean, rstd = c.outvec("mean", 1, Bn * G), c.outvec("rstd", 1, Bn * G)
    ws = c.ws(max(ops.groupnorm_ws_floats(Bn, HW, Cc, G), 1))
    if form == "2l":
        fs, bs = c.sums("fwd sums", Bn, slots, G), c.sums("bwd sums", Bn, slots, G)

    def call():
        if form == "2l":
            ops.groupnorm_fwd_2l(xd, y, gd, bd, fs, slots, mean, rstd, Bn, HW, Cc, G, eps, silu)
            ops.groupnorm_bwd_2l(dyd, xd, gd, bd, mean, rstd, dx, bs, slots, ws, Bn, HW, Cc, G, silu, accum=accd)
        else:
            ops.groupnorm_fwd(xd, y, gd, bd, mean, rstd, ws, Bn, HW, Cc, G, eps, silu)
            ops.groupnorm_bwd(dyd, xd, gd, bd, mean, rstd, dx, ws, Bn, HW, Cc, G, silu, accum=accd)

    def verify():
        check(f"contract gn {form} fwd C{Cc} HW{HW}", y.view(Bn, HW, Cc), yr.detach().permute(0, 2, 1), t16(2e-3))
        check(f"contract gn {form} bwd C{Cc} HW{HW}", dx.view(Bn, HW, Cc).float().cpu() - acc.view(Bn, HW, Cc).float(),
              xr.grad.permute(0, 2, 1), t16(4e-3))
    c.run(call, verify)


@pytest.mark.parametrize("Cc", [320, 1280])
@pytest.mark.parametrize("f32", [False, True], ids=["x16", "x32"])
def test_contract_norm_layernorm_fwd_bwd(Cc, f32):
    ops, c = _ops(), Case()
    rows, dt = 77, F32 if f32 else DT
    x = (rnd(rows, Cc, seed=24, dtype=F32) * 2 + 0.5).to(dt)
    gamma, beta = 1 + 0.1 * rnd(Cc, seed=25, dtype=F32), 0.1 * rnd(Cc, seed=26, dtype=F32)
    dy, acc = rnd(rows, Cc, seed=27), rnd(rows, Cc, seed=28, dtype=F32).to(dt)
    xr = x.float().requires_grad_(True)
    yr = F.layer_norm(xr, (Cc,), gamma, beta, 1e-5)
    yr.backward(dy.float())
    xd, dyd, accd, gd, bd = c.inp("x", x), c.inp("dy", dy), c.inp("accum", acc), c.vec("gamma", gamma), c.vec("beta", beta)
    y, dx = c.out("y", rows, Cc), c.out("dx", rows, Cc, dtype=dt)
    mean, rstd = c.outvec("mean", 1, rows), c.outvec("rstd", 1, rows)

    def call():
        ops.layernorm_fwd(xd, y, gd, bd, mean, rstd, 1e-5)
        ops.layernorm_bwd(dyd, xd, gd, mean, rstd, dx, accum=accd)

    def verify():
        check(f"contract ln fwd C{Cc} f32={f32}", y, yr.detach(), t16(2e-3))
        check(f"contract ln bwd C{Cc} f32={f32}", dx.float().cpu() - acc.float(), xr.grad, 4e-3 if f32 else t16(4e-3))
    c.run(call, verify)


def test_contract_norm_softmax_rows():
    """in place on [50, 1000] rows of stride 1024: the 24 pad columns keep their sentinel"""
    ops, c = _ops(), Case()
    s = rnd(50, 1000, scale=3.0, seed=30)
    sd = c.inout("scores", s, gap=24)
    assert sd.stride(0) == 1024
    c.run(lambda: ops.softmax_rows(sd, 50, 1000), lambda: check("contract softmax rows", sd, torch.softmax(s.float(), -1), t16(2e-3)))


def _transpose_operands(c, tag, x, ldo):
    """in [Bn, rows, cols] (rows of stride cols + gap, guard rows between the batches) -> out [Bn, cols, ldo]: the contract is
    that columns [rows, ldo) are ZERO FILLED, so the whole ldo width is the logical output"""
    Bn, rows, cols = x.shape
    xd, out = c.inp("in" + tag, x, batch=Bn), c.out("out" + tag, cols, ldo, gap=0, batch=Bn)
    return xd, out, (xd, out, rows, cols, Bn, xd.stride(1), xd.stride(0), ldo, out.stride(0))


def _transpose_verify(x, out):
    rows = x.shape[1]
    assert torch.equal(out[:, :, :rows].cpu(), x.transpose(1, 2)), "transpose differs"
    assert float(out[:, :, rows:].abs().max()) == 0, "the pad columns [rows, ld_out) are not zero filled"


def test_contract_norm_transpose():
    ops, c = _ops(), Case()
    x = rnd(3, 77, 320, seed=29)
    xd, out, args = _transpose_operands(c, "", x, 80)
    c.run(lambda: ops.transpose(*args), lambda: _transpose_verify(x, out))


def test_contract_norm_transpose_multi():
    ops, c = _ops(), Case()
    a, b = rnd(3, 77, 64, seed=40), rnd(2, 130, 40, seed=41)
    _, at, args_a = _transpose_operands(c, " a", a, 80)
    _, bt, args_b = _transpose_operands(c, " b", b, 136)
    c.run(lambda: ops.transpose_multi([args_a, args_b]), lambda: (_transpose_verify(a, at), _transpose_verify(b, bt)))


# ------------------------------------------------------------------------------------------ attention
def _attention_case(D, Nq, Nk, causal, use_ws, small=False):
    """fwd, attn_bwd_delta, attn_bwd_dq in both delta forms, attn_bwd_dkv (and attn_bwd_small): every operand in a slab of
    its own with ld = H * D + 24, + 32, ...; the spike key of the parity test keeps the online-softmax rescale path in"""
    ops, c = _ops(), Case()
    Bn, H = 2, 2
    Cc, scale = H * D, D ** -0.5
    q, k, v, do = (rnd(Bn, n, Cc, seed=s) for n, s in ((Nq, 31), (Nk, 32), (Nk, 33), (Nq, 34)))
    k[0, Nk - 3] = (q[0, 5].float() * 3).to(DT)
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    o_ref, lse_ref = _attn_ref(qr, kr, vr, H, D, scale, causal)
    o_ref.backward(do.float())
    c.gaps.update((8, 16))
    qd, kd, vd, dod = (c.inp(n, t.view(-1, Cc)) for n, t in (("Q", q), ("K", k), ("V", v), ("dO", do)))
    assert qd.stride(0) == Cc + 24
    o, dq, dq2 = c.out("O", Bn * Nq, Cc), c.out("dQ", Bn * Nq, Cc), c.out("dQ (fused delta)", Bn * Nq, Cc)
    dk, dv = c.out("dK", Bn * Nk, Cc), c.out("dV", Bn * Nk, Cc)
    lse, delta, delta2 = (c.outvec(n, Bn, H, Nq) for n in ("lse", "delta", "delta (in-kernel)"))
    ws = c.ws(2 * 4 * Bn * Nk * Cc) if use_ws else None
    if small:
        dq3, dk3, dv3 = c.out("dQ small", Bn * Nq, Cc), c.out("dK small", Bn * Nk, Cc), c.out("dV small", Bn * Nk, Cc)

    def call():
        ops.attn_fwd(qd, kd, vd, o, lse, Bn, H, Nq, Nk, D, scale, causal)
        ops.attn_bwd_delta(dod, o, delta, Bn, H, Nq, D)
        ops.attn_bwd_dq(qd, kd, vd, dod, lse, delta, dq, Bn, H, Nq, Nk, D, scale, causal)
        ops.attn_bwd_dq(qd, kd, vd, dod, lse, delta2, dq2, Bn, H, Nq, Nk, D, scale, causal, O=o)
        ops.attn_bwd_dkv(qd, kd, vd, dod, lse, delta2, dk, dv, Bn, H, Nq, Nk, D, scale, causal, workspace=ws)
        if small:
            ops.attn_bwd_small(qd, kd, vd, dod, o, lse, dq3, dk3, dv3, Bn, H, Nq, D, scale, causal)

    def verify():
        tag = f"contract D{D} Nq{Nq} Nk{Nk} c{int(causal)} ws{int(use_ws)}"
        check(f"attn fwd {tag}", o.view(Bn, Nq, Cc), o_ref.detach(), t16(3e-3))
        check(f"attn lse {tag}", lse, lse_ref.detach(), 1e-3)
        check(f"attn delta(in-kernel) {tag}", delta2, delta, 1e-4)
        check(f"attn dq(fused delta) {tag}", dq2, dq, t16(1e-3))
        check(f"attn dq {tag}", dq.view(Bn, Nq, Cc), qr.grad, t16(6e-3))
        check(f"attn dk {tag}", dk.view(Bn, Nk, Cc), kr.grad, t16(6e-3))
        check(f"attn dv {tag}", dv.view(Bn, Nk, Cc), vr.grad, t16(6e-3))
        if small:
            assert ops.attn_bwd_small_ok(Nq, D)
            assert torch.equal(dq3, dq2) and torch.equal(dk3, dk) and torch.equal(dv3, dv), \
                "fused small backward differs from the dQ + dK/dV pair"
    c.run(call, verify)


@pytest.mark.parametrize("Nq,Nk", [(200, 200), (200, 77)])
@pytest.mark.parametrize("D", [40, 64, 80, 160])
def test_contract_attn_fwd_bwd(D, Nq, Nk):
    _attention_case(D, Nq, Nk, False, True)


@pytest.mark.parametrize("use_ws", [True, False], ids=["nan-ws", "no-ws"])
@pytest.mark.parametrize("D", [40, 160])
def test_contract_attn_query_split_dkv(D, use_ws):
    """Nq = 520 against 77 keys: with a workspace the dK/dV query range is split and the f32 partials go through it"""
    _attention_case(D, 520, 77, False, use_ws)


@pytest.mark.parametrize("N", [77, 96])
def test_contract_attn_causal_and_small(N):
    _attention_case(64, N, N, True, True, small=True)
