"""Direct parity of the NeTI text-path kernels (csrc/text.hip) through the C ABI: the mapper forward / backward, the legacy
input layer, mapper_inputs, the embedding splice and the bypass + final LayerNorm pair, each against a plain float64 CPU
statement of the operation written here from the formulas in include/vneti.h (torch autograd in float64 for every backward).

Bars.  The outputs are f32 and no 16-bit rounding lies between the shared inputs and them, so the bar is the kernel file's f32
bar, 1e-5 with `check()`'s element-wise bound, in both builds — where plain f32 arithmetic can meet it: every parity check
also evaluates its reference in torch float32 on the CPU from the same inputs, e32 = that result's relative Frobenius error
against float64, and the bar is 1e-5 if 8 * e32 <= 1e-5, else 8 * e32 (the kernels sum in another order — 16-lane partials,
64-lane trees, column partitions — and use rsqrtf).  No bar comes from a kernel's output.  `ctx_k` / `ctx_v` of
text_final_fwd and the cast are stored in the 16-bit format: they get `t16()` (x8 in bf16), as the LayerNorm test of
tests/test_kernels_gpu.py.  Every case runs against libvneti_hip_bf16.so too (tests/test_kernels_bf16_gpu.py)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers.checks import DEV, DT, F32_BAR, check, check32, t16
from helpers.checks import gen as _gen, ops as _ops

pytestmark = pytest.mark.gpu

NAMES = ("net.0.weight", "net.0.bias", "net.1.weight", "net.1.bias", "net.3.weight", "net.3.bias", "net.4.weight",
         "net.4.bias", "output_layer.0.weight", "output_layer.0.bias")


def randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=_gen(seed)) * scale


def dev(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------------------------------ the mapper, restated
def mapper_shapes(E, hd, D, has_bypass):
    OD = 2 * D if has_bypass else D
    return [(hd, E), (hd,), (hd,), (hd,), (hd, hd), (hd,), (hd,), (hd,), (OD, hd), (OD,)]


def mapper_params(E, hd, D, has_bypass, seed):
    """ten f32 tensors in state_dict order; LayerNorm weights / biases away from (1, 0) so that they matter"""
    shp = mapper_shapes(E, hd, D, has_bypass)
    g = _gen(seed)
    P = []
    for i, s in enumerate(shp):
        if i in (2, 6):
            P.append(1.0 + 0.2 * torch.randn(*s, generator=g))
        elif i in (3, 7):
            P.append(0.2 * torch.randn(*s, generator=g))
        else:
            bound = 1.0 / math.sqrt(shp[i - 1][1] if len(s) == 1 else s[1])
            P.append((torch.rand(*s, generator=g) * 2 - 1) * bound)
    return P


def flat(P):
    return torch.cat([p.reshape(-1) for p in P])


def unflat(v, shapes):
    out, o = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(v[o:o + n].reshape(s))
        o += n
    assert o == v.numel()
    return out


def mapper_ref(P, enc, hmask, norm_scale, D, has_bypass):
    """models/neti_mapper.py:165-197 from the first layer's input on: Linear - LayerNorm - LeakyReLU twice, the 0/1 mask of
    nested dropout, the output layer, F.normalize(word) * norm_scale; dtype = that of the arguments"""
    w0, b0, g1, be1, w3, b3, g2, be2, wo, bo = P
    hd = w0.shape[0]
    h = F.leaky_relu(F.layer_norm(enc @ w0.t() + b0, (hd,), g1, be1, 1e-5), 0.01)
    h = F.leaky_relu(F.layer_norm(h @ w3.t() + b3, (hd,), g2, be2, 1e-5), 0.01)
    if hmask is not None:
        h = h * hmask
    out = h @ wo.t() + bo
    raw = out[:, :D]
    wnorm = raw.norm(dim=1)
    word = raw / wnorm.clamp_min(1e-12)[:, None] * norm_scale if norm_scale > 0 else raw
    return word, (out[:, D:] if has_bypass else None), wnorm


def fourier(data, w_enc):
    ph = data @ w_enc.t()  # models/positional_encoding.py:174-195
    return torch.cat([torch.sin(ph), torch.cos(ph)], dim=1)


def prefix_masks(R, hd, seed):
    """random prefix masks; row 0 is all zero (idx = 0: |word_raw| = |bias|), row 1 all ones"""
    idx = torch.randint(0, hd + 1, (R,), generator=_gen(seed))
    idx[0] = 0
    if R > 1:
        idx[1] = hd
    return (torch.arange(hd)[None, :] < idx[:, None]).float()


# (E, hidden, D, nfeat (0 = legacy: the first layer's input is given), nl, Bn)
SHAPES = {
    "sd15_object": (64, 128, 768, 2, 16, 4),
    "sd21_view": (64, 128, 1024, 14, 16, 4),
    "legacy160": (160, 128, 768, 0, 16, 2),
    "r48": (64, 64, 64, 2, 16, 3),
    "r80": (64, 64, 64, 2, 16, 5),
    "r3": (64, 64, 64, 2, 1, 3),
    "e6_nonvector": (6, 32, 40, 2, 16, 2),
}


class Case:
    """inputs of one mapper problem (f32, CPU) and the device-side call"""

    def __init__(self, shape, has_bypass=True, masked=True, norm_scale=0.4, seed=0):
        self.E, self.hd, self.D, self.nfeat, self.nl, self.Bn = SHAPES[shape]
        self.R = self.nl * self.Bn
        self.has_bypass, self.norm_scale = has_bypass, norm_scale
        self.P = mapper_params(self.E, self.hd, self.D, has_bypass, 100 + seed)
        self.shapes = mapper_shapes(self.E, self.hd, self.D, has_bypass)
        if self.nfeat:
            self.data = torch.rand(self.R, self.nfeat, generator=_gen(200 + seed)) * 2 - 1
            sig = torch.tensor([0.03, 2.0] + [1.0] * (self.nfeat - 2))
            self.w_enc = randn(self.E // 2, self.nfeat, seed=201 + seed) * sig
            self.enc_in = None
        else:
            self.data = self.w_enc = None
            self.enc_in = randn(self.R, self.E, seed=202 + seed, scale=0.5)
        self.hmask = prefix_masks(self.R, self.hd, 203 + seed) if masked else None

    def enc(self, dt):
        return self.enc_in.to(dt) if self.enc_in is not None else fourier(self.data.to(dt), self.w_enc.to(dt))

    def ref(self, dt):
        hm = None if self.hmask is None else self.hmask.to(dt)
        return mapper_ref([p.to(dt) for p in self.P], self.enc(dt), hm, self.norm_scale, self.D, self.has_bypass)

    def n_params(self):
        return sum(int(np.prod(s)) for s in self.shapes)

    def forward(self, params_dev, slot=None, slot_stride=0):
        ops = _ops()
        R, D = self.R, self.D
        assert ops.mapper_num_params(self.E, self.hd, D, self.has_bypass) == self.n_params()
        word = torch.full((R, D), 7.0, device=DEV)
        byp = torch.full((R, D), 7.0, device=DEV) if self.has_bypass else None
        save = torch.zeros(ops.mapper_save_floats(R, self.E, self.hd), device=DEV)
        self.dev_in = (dev(self.data), dev(self.w_enc), dev(self.hmask), dev(self.enc_in))
        data, w_enc, hm, enc_in = self.dev_in
        ops.mapper_fwd(params_dev, data, w_enc, hm, self.norm_scale, word, byp, save, R, self.E, self.hd, D,
                       self.has_bypass, slot=slot, slot_stride=slot_stride, enc_in=enc_in)
        torch.cuda.synchronize()
        return word, byp, save

    def backward(self, params_dev, word, save, dword_src, rows, ld_src, dbyp, grads, accumulate, slot=None, slot_stride=0,
                 denc=None):
        ops = _ops()
        rg = torch.zeros(ops.mapper_rowgrad_floats(self.R, self.hd, self.D, self.has_bypass), device=DEV)
        ops.mapper_bwd(params_dev, self.dev_in[2], self.norm_scale, word, dword_src, rows, ld_src, dbyp, save, rg, grads,
                       accumulate, self.R, self.E, self.hd, self.D, self.has_bypass, slot=slot, slot_stride=slot_stride,
                       denc=denc)
        torch.cuda.synchronize()

    def upstream(self, seed, with_dbyp):
        """random d(word) rows addressed through a shuffled dword_rows with ld_src > D, two rows dead (-1)"""
        R, D = self.R, self.D
        ld = D + 8
        src = randn(R + 5, ld, seed=300 + seed)
        rows = torch.randperm(R + 5, generator=_gen(301 + seed))[:R].to(torch.int32)
        rows[R // 2] = -1
        if R >= 8:  # (R = 3 keeps two live rows, one of them with a non-empty mask)
            rows[R - 1] = -1
        dbyp = randn(R, D, seed=302 + seed) if (with_dbyp and self.has_bypass) else None
        live = (rows >= 0)
        dword = src[rows.clamp_min(0).long(), :D] * live[:, None]
        dbyp_eff = None if dbyp is None else dbyp * live[:, None]
        return src, rows, ld, dbyp, dword, dbyp_eff

    def ref_grads(self, dt, dword, dbyp_eff):
        P = [p.to(dt).requires_grad_(True) for p in self.P]
        enc = self.enc(dt).requires_grad_(True)
        hm = None if self.hmask is None else self.hmask.to(dt)
        word, byp, _ = mapper_ref(P, enc, hm, self.norm_scale, self.D, self.has_bypass)
        loss = (word * dword.to(dt)).sum()
        if dbyp_eff is not None:
            loss = loss + (byp * dbyp_eff.to(dt)).sum()
        gs = torch.autograd.grad(loss, P + [enc], allow_unused=True)
        gs = [torch.zeros_like(p) if g is None else g for g, p in zip(gs, P + [enc])]
        return gs[:-1], gs[-1]


def wnorm_of(save, c):
    return save.view(c.R, c.E + 4 * c.hd + 4)[:, c.E + 4 * c.hd + 2]


@pytest.mark.parametrize("has_bypass", [1, 0])
@pytest.mark.parametrize("norm_scale", [0.4, -1.0])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_mapper_fwd(shape, masked, norm_scale, has_bypass):
    c = Case(shape, bool(has_bypass), masked, norm_scale)
    word, byp, save = c.forward(dev(flat(c.P)))
    w64, b64, n64 = c.ref(torch.float64)
    w32, b32, n32 = c.ref(torch.float32)
    tag = f"mapper fwd {shape} mask={masked} ns={norm_scale} byp={has_bypass}"
    check32(tag + " word", word, w64, w32)
    check32(tag + " wnorm", wnorm_of(save, c), n64, n32)
    if has_bypass:
        check32(tag + " bypass", byp, b64, b32)
    if masked:  # the all-zero row: the raw word is the output bias
        nb = c.P[9][:c.D].double().norm().item()
        assert abs(wnorm_of(save, c)[0].item() - nb) <= 1e-6 * nb


@pytest.mark.parametrize("variant", ["full", "no_dbypass", "plain"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_mapper_bwd(shape, variant):
    """all ten parameter gradients separately; accumulate = 1 is previous + fresh in one f32 add; d(enc) for the legacy shape"""
    plain = variant == "plain"  # no bypass half, no mask, no output normalisation
    c = Case(shape, has_bypass=not plain, masked=not plain, norm_scale=-1.0 if plain else 0.4, seed=1)
    params = dev(flat(c.P))
    word, _, save = c.forward(params)
    src, rows, ld, dbyp, dword, dbyp_eff = c.upstream(1, with_dbyp=variant == "full")
    n = c.n_params()
    grads = torch.full((n + 8,), 3.0, device=DEV)  # the 8 floats behind the bucket must keep their value
    legacy = c.enc_in is not None
    denc = torch.zeros(c.R, c.E, device=DEV) if legacy else None
    args = (params, word, save, dev(src), dev(rows), ld, dev(dbyp))
    c.backward(*args, grads, 0, denc=denc)
    assert bool((grads[n:] == 3.0).all())
    g64, e64 = c.ref_grads(torch.float64, dword, dbyp_eff)
    g32, e32 = c.ref_grads(torch.float32, dword, dbyp_eff)
    got = unflat(grads[:n].cpu(), c.shapes)
    for name, g, r64, r32 in zip(NAMES, got, g64, g32):
        check32(f"mapper bwd {shape} {variant} d {name}", g, r64, r32)
    if legacy:
        check32(f"mapper bwd {shape} {variant} denc", denc, e64, e32)
    prev = randn(n, seed=77)
    acc = torch.cat([prev, torch.full((8,), 3.0)]).to(DEV)
    c.backward(*args, acc, 1)
    assert torch.equal(acc[:n].cpu(), prev + grads[:n].cpu()) and bool((acc[n:] == 3.0).all())


def test_mapper_slot_of_a_bucket():
    """slot = 2 of a 3-mapper bucket: outputs as the single-mapper run bit for bit, gradients in segment 2 only"""
    c = Case("sd15_object", seed=2)
    n = c.n_params()
    stride = n + 4  # a multiple of 4: the vector body
    assert stride % 4 == 0
    single = dev(flat(c.P))
    word1, byp1, save1 = c.forward(single)
    bucket = randn(3 * stride + 16, seed=5, scale=0.05)
    bucket[2 * stride:2 * stride + n] = flat(c.P)
    bucket = bucket.to(DEV)
    slot = torch.tensor([2], dtype=torch.int32, device=DEV)
    word, byp, save = c.forward(bucket, slot=slot, slot_stride=stride)
    assert torch.equal(word, word1) and torch.equal(byp, byp1) and torch.equal(save, save1)
    src, rows, ld, dbyp, _, _ = c.upstream(2, True)
    g1 = torch.zeros(n, device=DEV)
    c.backward(single, word1, save1, dev(src), dev(rows), ld, dev(dbyp), g1, 0)
    gb = torch.full((3 * stride + 16,), -5.5, device=DEV)
    c.backward(bucket, word, save, dev(src), dev(rows), ld, dev(dbyp), gb, 0, slot=slot, slot_stride=stride)
    assert torch.equal(gb[2 * stride:2 * stride + n], g1)
    assert bool((gb[:2 * stride] == -5.5).all()) and bool((gb[2 * stride + n:] == -5.5).all())
    assert float(g1.abs().sum()) > 0


@pytest.mark.parametrize("shape", ["sd15_object", "legacy160", "r3"])
def test_mapper_non_vector_body(shape):
    """params (and grads) one float into a larger allocation: 4-byte but not 16-byte aligned, so the non-vector bodies of the
    forward and the backward run; vs float64 at the same bar and vs the vector body at the f32 bar"""
    c = Case(shape, seed=3)
    n = c.n_params()
    big = torch.zeros(n + 9, device=DEV)
    big[1:1 + n] = flat(c.P).to(DEV)
    pv = big[1:1 + n]
    assert pv.data_ptr() % 16 == 4
    word, byp, save = c.forward(pv)
    aligned = dev(flat(c.P))
    assert aligned.data_ptr() % 16 == 0
    word_v, byp_v, save_v = c.forward(aligned)
    w64, b64, _ = c.ref(torch.float64)
    w32, b32, _ = c.ref(torch.float32)
    check32(f"non-vector {shape} word", word, w64, w32)
    check32(f"non-vector {shape} bypass", byp, b64, b32)
    check(f"non-vector vs vector {shape} word", word, word_v, F32_BAR)
    check(f"non-vector vs vector {shape} bypass", byp, byp_v, F32_BAR)
    src, rows, ld, dbyp, dword, dbyp_eff = c.upstream(3, True)
    gbig = torch.full((n + 9,), 2.0, device=DEV)
    legacy = c.enc_in is not None
    denc = torch.zeros(c.R, c.E, device=DEV) if legacy else None
    c.backward(pv, word, save, dev(src), dev(rows), ld, dev(dbyp), gbig[1:1 + n], 0, denc=denc)
    assert float(gbig[0]) == 2.0 and bool((gbig[1 + n:] == 2.0).all())
    gv = torch.zeros(n, device=DEV)
    c.backward(aligned, word_v, save_v, dev(src), dev(rows), ld, dev(dbyp), gv, 0)
    g64, e64 = c.ref_grads(torch.float64, dword, dbyp_eff)
    g32, e32 = c.ref_grads(torch.float32, dword, dbyp_eff)
    for name, g, v, r64, r32 in zip(NAMES, unflat(gbig[1:1 + n].cpu(), c.shapes), unflat(gv.cpu(), c.shapes), g64, g32):
        check32(f"non-vector {shape} d {name}", g, r64, r32)
        check(f"non-vector vs vector {shape} d {name}", g, v, F32_BAR)
    if legacy:
        check32(f"non-vector {shape} denc", denc, e64, e32)


# ------------------------------------------------------------------------------------------ legacy input layer
def legacy_v(w_pe, t, nl, dt):
    """models/positional_encoding.py:23-41: v = cat[sin(w x), cos(w x)] / |.| of the RAW x = (t_b, l), rows r = l * Bn + b.
    w_pe is the f32 tensor the kernel reads; t and l are exact in either dtype."""
    Bn = t.numel()
    tt = t.to(dt).repeat(nl)
    ll = torch.arange(nl).repeat_interleave(Bn).to(dt)
    ph = tt[:, None] * w_pe.to(dt)[None, :, 0] + ll[:, None] * w_pe.to(dt)[None, :, 1]
    v = torch.cat([torch.sin(ph), torch.cos(ph)], dim=1)
    return v / v.norm(dim=1, keepdim=True)


def legacy_setup(Bn, seed=0):
    E, P2 = 160, 2048
    w_pe = randn(P2 // 2, 2, seed=400 + seed) * torch.tensor([0.03, 2.0])  # NeTIPositionalEncoding(sigma_t, sigma_l)
    t = torch.tensor([0, 1, 500, 999], dtype=torch.int64)
    if Bn > 4:
        t = torch.cat([t, torch.randint(0, 1000, (Bn - 4,), generator=_gen(401 + seed))])
    t = t[:Bn].contiguous()
    pin = torch.cat([randn(E, P2, seed=402 + seed, scale=1 / math.sqrt(P2)).reshape(-1), randn(E, seed=403 + seed, scale=0.1)])
    return E, P2, w_pe, t, pin


def test_legacy_input_fwd():
    ops = _ops()
    nl, Bn = 16, 4
    E, P2, w_pe, t, pin = legacy_setup(Bn)
    assert ops.mapper_legacy_input_params(E, P2) == pin.numel()
    out = torch.zeros(nl * Bn, E, device=DEV)
    ops.mapper_legacy_input_fwd(dev(pin), dev(t), dev(w_pe), out, nl, Bn, E, P2)
    torch.cuda.synchronize()

    def ref(dt):
        return legacy_v(w_pe, t, nl, dt) @ pin[:E * P2].reshape(E, P2).to(dt).t() + pin[E * P2:].to(dt)
    check32("legacy input fwd", out, ref(torch.float64), ref(torch.float32))


@pytest.mark.parametrize("nl,Bn", [(8, 4), (16, 4), (13, 5), (16, 8)])
def test_legacy_input_bwd(nl, Bn):
    """dW_in = sum_r denc[r] (x) v_r, db_in = sum_r denc[r] for 32, 64, 65 and 128 rows (above 64: the LDS opt-in)"""
    ops = _ops()
    E, P2, w_pe, t, _ = legacy_setup(Bn, seed=1)
    R = nl * Bn
    denc = randn(R, E, seed=410)
    n = E * P2 + E
    g = torch.full((n + 4,), 9.0, device=DEV)
    ops.mapper_legacy_input_bwd(dev(t), dev(w_pe), dev(denc), g, 0, nl, Bn, E, P2)
    torch.cuda.synchronize()
    assert bool((g[n:] == 9.0).all())

    def ref(dt):
        return torch.cat([(denc.to(dt).t() @ legacy_v(w_pe, t, nl, dt)).reshape(-1), denc.to(dt).sum(0)])
    r64, r32 = ref(torch.float64), ref(torch.float32)
    check32(f"legacy input bwd R={R} dW_in", g[:E * P2], r64[:E * P2], r32[:E * P2])
    check32(f"legacy input bwd R={R} db_in", g[E * P2:n], r64[E * P2:], r32[E * P2:])
    prev = randn(n, seed=411)
    acc = prev.to(DEV)
    ops.mapper_legacy_input_bwd(dev(t), dev(w_pe), dev(denc), acc, 1, nl, Bn, E, P2)
    torch.cuda.synchronize()
    assert torch.equal(acc.cpu(), prev + g[:n].cpu())


def test_legacy_input_bwd_refuses_129_rows():
    ops = _ops()
    E, P2, w_pe, t, _ = legacy_setup(3)
    g = torch.zeros(E * P2 + E, device=DEV)
    with pytest.raises(RuntimeError, match="mapper_legacy_input_bwd"):
        ops.mapper_legacy_input_bwd(dev(t), dev(w_pe), torch.zeros(129, E, device=DEV), g, 0, 43, 3, E, P2)
    torch.cuda.synchronize()
    assert float(g.abs().sum()) == 0


@pytest.mark.parametrize("nv", [0, 12])
def test_mapper_inputs(nv):
    """t / 1000 * 2 - 1 and l / nl * 2 - 1 in f32 in that order, all 1000 timesteps: at most 1 ulp per element (the product
    and the subtraction round identically fused or not; only the division's rounding is the compiler's); the view
    parameters are copied bit for bit"""
    ops = _ops()
    nl, Bn = 16, 1000
    t = torch.arange(1000, dtype=torch.int64)
    vp = randn(Bn, nv, seed=420) if nv else None
    data = torch.full((nl * Bn, 2 + nv), 5.0, device=DEV)
    ops.mapper_inputs(dev(t), dev(vp), data, nl, Bn)
    torch.cuda.synchronize()
    got = data.cpu().numpy().reshape(nl, Bn, 2 + nv)
    one, two = np.float32(1), np.float32(2)
    rt = np.arange(1000).astype(np.float32) / np.float32(1000) * two - one
    rl = np.arange(nl).astype(np.float32) / np.float32(nl) * two - one
    for name, g, r in (("t", got[:, :, 0], np.broadcast_to(rt[None, :], (nl, Bn))),
                       ("l", got[:, :, 1], np.broadcast_to(rl[:, None], (nl, Bn)))):
        ulps = np.abs(g.astype(np.float64) - r.astype(np.float64)) / np.spacing(np.abs(r)).astype(np.float64)
        print(f"[mapper_inputs nv={nv}] {name}: worst {ulps.max():.2f} ulp")
        assert ulps.max() <= 1.0
    if nv:
        assert np.array_equal(got[:, :, 2:], np.broadcast_to(vp.numpy()[None], (nl, Bn, nv)))


# ------------------------------------------------------------------------------------------ embedding splice
@pytest.mark.parametrize("mode", ["object", "view", "both", "neither", "same_position"])
@pytest.mark.parametrize("D", [768, 1024])
def test_text_embed(D, mode):
    """E[ids] (+ overwrite: object, then view) + P: one f32 add, bit for bit; sample 1 has no object placeholder (-1)"""
    ops = _ops()
    nl, Bn, L, V = 16, 3, 77, 3001
    tok, pos = randn(V, D, seed=500, scale=0.02), randn(L, D, seed=501, scale=0.02)
    ids = torch.randint(0, V, (Bn, L), generator=_gen(502))
    ids[0, 0], ids[0, 1], ids[2, 76], ids[2, 75] = 0, V - 1, V - 1, 0  # both ends of the table
    w_obj, w_view = randn(nl * Bn, D, seed=503), randn(nl * Bn, D, seed=504)
    p_obj = torch.tensor([0, -1, 76], dtype=torch.int32) if mode in ("object", "both", "same_position") else None
    p_view = torch.tensor([5, 40, 76 if mode == "same_position" else 3], dtype=torch.int32) if mode != "object" and \
        mode != "neither" else None
    X = torch.full((nl * Bn * L, D), 9.0, device=DEV)
    ops.text_embed(dev(tok), dev(pos), dev(ids), dev(p_obj), dev(w_obj) if p_obj is not None else None, dev(p_view),
                   dev(w_view) if p_view is not None else None, X, nl, Bn, L, D)
    torch.cuda.synchronize()
    ref = tok[ids][None].repeat(nl, 1, 1, 1)  # [nl, Bn, L, D]
    for p, w in ((p_obj, w_obj), (p_view, w_view)):  # the view overwrites last
        if p is not None:
            for b in range(Bn):
                if p[b] >= 0:
                    ref[:, b, int(p[b])] = w.view(nl, Bn, D)[:, b]
    ref = ref + pos[None, None]
    assert torch.equal(X.cpu().view(nl, Bn, L, D), ref)


# ------------------------------------------------------------------------------------------ bypass + final LayerNorm
EPS = 1e-5


def final_ref(last, gamma, beta, obj, view, nl, Bn, L, D):
    """models/neti_clip_text_encoder.py:121-185: ctx_k = LN(last); ctx_v = LN(last with the placeholder rows rewritten),
    object first, then view.  obj / view = None or (pos[Bn], bypass[nl*Bn, D], alpha, unconstrained).  Returns ctx_k, ctx_v
    and the two detached normalising terms [2, nl*Bn] (mean over the L rows of |row| of the tensor as it is at that mapper's
    turn)."""
    x = last.view(nl, Bn, L, D)
    y = x.clone()
    terms = []
    for m in (obj, view):
        term = y.detach().norm(dim=-1).mean(dim=-1)  # [nl, Bn]
        terms.append(term.reshape(-1))
        if m is None:
            continue
        pos, byp, alpha, unc = m
        u = byp / byp.norm(dim=-1, keepdim=True)
        u = u.view(nl, Bn, D)
        for b in range(Bn):
            p = int(pos[b])
            if p < 0:
                continue
            if unc:
                y[:, b, p] = u[:, b] * term[:, b, None]
            else:
                xr = y[:, b, p].clone()
                y[:, b, p] = xr + alpha * u[:, b] * xr.norm(dim=-1, keepdim=True)
    ln = lambda z: F.layer_norm(z, (D,), gamma, beta, EPS).reshape(nl * Bn * L, D)
    return ln(x), ln(y), torch.stack(terms)


def final_inputs(D, nl, Bn, L, seed):
    last = randn(nl * Bn * L, D, seed=600 + seed) * (1 + 2 * torch.rand(nl * Bn * L, 1, generator=_gen(601 + seed)))
    last = last + 0.3 * randn(1, D, seed=602 + seed)
    gamma, beta = 1 + 0.2 * randn(D, seed=603 + seed), 0.2 * randn(D, seed=604 + seed)
    b_obj, b_view = randn(nl * Bn, D, seed=605 + seed), randn(nl * Bn, D, seed=606 + seed, scale=3.0)
    p_obj = torch.tensor([0, 76, 38], dtype=torch.int32)[:Bn]   # different placeholder positions per sample
    p_view = torch.tensor([76, 5, 39], dtype=torch.int32)[:Bn]
    return last, gamma, beta, b_obj, b_view, p_obj, p_view


FINAL_CASES = [(D, nl, uo, uv, "both") for D in (768, 1024, 64) for nl in (16, 1) for uo in (0, 1) for uv in (0, 1)] + \
              [(768, 16, u, u, who) for u in (0, 1) for who in ("object", "view")]


@pytest.mark.parametrize("D,nl,unc_obj,unc_view,who", FINAL_CASES)
def test_text_final_fwd_bwd(D, nl, unc_obj, unc_view, who):
    """nl = 1: 231 rows, the 4-rows-per-block tail.  The backward is float64 autograd of the forward with the unconstrained
    term detached, from 16-bit dctx_k / dctx_v; its outputs are f32 and keep the f32 bar in both builds."""
    ops = _ops()
    Bn, L = 3, 77
    rows = nl * Bn * L
    last, gamma, beta, b_obj, b_view, p_obj, p_view = final_inputs(D, nl, Bn, L, D + nl)
    a_obj, a_view = 0.2, 0.35
    has_o, has_v = who in ("both", "object"), who in ("both", "view")
    dk, dv = randn(rows, D, seed=610).to(DT), randn(rows, D, seed=611).to(DT)

    def ref(dt):
        ls = last.to(dt).requires_grad_(True)
        bo, bv = b_obj.to(dt).requires_grad_(True), b_view.to(dt).requires_grad_(True)
        k, v, terms = final_ref(ls, gamma.to(dt), beta.to(dt), (p_obj, bo, a_obj, unc_obj) if has_o else None,
                                (p_view, bv, a_view, unc_view) if has_v else None, nl, Bn, L, D)
        loss = (k * dk.to(dt)).sum() + (v * dv.to(dt)).sum()
        g = torch.autograd.grad(loss, [ls, bo, bv], allow_unused=True)
        g = [torch.zeros_like(t) if x is None else x for x, t in zip(g, (ls, bo, bv))]
        return k.detach(), v.detach(), terms, g
    k64, v64, t64, g64 = ref(torch.float64)
    k32, v32, t32, g32 = ref(torch.float32)

    ctx_k = torch.zeros(rows, D, dtype=DT, device=DEV)
    ctx_v = torch.zeros(rows, D, dtype=DT, device=DEV)
    nt = torch.zeros(2, nl * Bn, device=DEV)
    d_last, d_gamma, d_beta = dev(last), dev(gamma), dev(beta)
    po, bo = (dev(p_obj), dev(b_obj)) if has_o else (None, None)
    pv, bv = (dev(p_view), dev(b_view)) if has_v else (None, None)
    ops.text_final_fwd(d_last, d_gamma, d_beta, EPS, po, bo, a_obj, pv, bv, a_view, ctx_k, ctx_v, nl, Bn, L, D,
                       unconstrained_obj=bool(unc_obj), unconstrained_view=bool(unc_view), norm_terms=nt)
    torch.cuda.synchronize()
    tag = f"text_final D{D} nl{nl} unc=({unc_obj},{unc_view}) {who}"
    check(tag + " ctx_k", ctx_k, k64, t16(2e-3))
    check(tag + " ctx_v", ctx_v, v64, t16(2e-3))
    plain = torch.ones(nl, Bn, L, dtype=torch.bool)
    for has, p in ((has_o, p_obj), (has_v, p_view)):
        if has:
            for b in range(Bn):
                plain[:, b, int(p[b])] = False
    plain = plain.reshape(-1)
    assert torch.equal(ctx_k.cpu()[plain], ctx_v.cpu()[plain])  # only placeholder rows differ
    assert not torch.equal(ctx_k.cpu()[~plain], ctx_v.cpu()[~plain])
    if (unc_obj and has_o) or (unc_view and has_v):  # the scratch is written when an unconstrained flag is set
        check32(tag + " norm_terms object", nt[0], t64[0], t32[0])
        check32(tag + " norm_terms view", nt[1], t64[1], t32[1])
    dX = torch.full((rows, D), 4.0, device=DEV)
    dbo = torch.zeros(nl * Bn, D, device=DEV) if has_o else None
    dbv = torch.zeros(nl * Bn, D, device=DEV) if has_v else None
    ops.text_final_bwd(d_last, d_gamma, EPS, po, bo, a_obj, dbo, pv, bv, a_view, dbv, dev(dk), dev(dv), dX, nl, Bn, L, D,
                       unconstrained_obj=bool(unc_obj), unconstrained_view=bool(unc_view), norm_terms=nt)
    torch.cuda.synchronize()
    check32(tag + " dX", dX, g64[0], g32[0])
    if has_o:
        check32(tag + " dbypass_obj", dbo, g64[1], g32[1])
    if has_v:
        check32(tag + " dbypass_view", dbv, g64[2], g32[2])


def test_text_final_refuses_a_width_that_is_no_multiple_of_8():
    ops = _ops()
    D, nl, Bn, L = 60, 1, 1, 4
    z = torch.zeros(nl * Bn * L, D, device=DEV)
    h = torch.zeros(nl * Bn * L, D, dtype=DT, device=DEV)
    g = torch.ones(D, device=DEV)
    with pytest.raises(RuntimeError, match="text_final_fwd"):
        ops.text_final_fwd(z, g, g, EPS, None, None, 0.0, None, None, 0.0, h, h, nl, Bn, L, D)
    with pytest.raises(RuntimeError, match="text_final_bwd"):
        ops.text_final_bwd(z, g, EPS, None, None, 0.0, None, None, None, 0.0, None, h, h, z, nl, Bn, L, D)
    torch.cuda.synchronize()


def test_text_cast_is_round_to_nearest_even():
    """vneti_cast_f32_f16: f32 -> the build's 16-bit format, bit for bit torch's conversion (normal range of both formats)"""
    ops = _ops()
    n = 8 * 4099
    x = (1 + torch.rand(n, generator=_gen(700))) * torch.exp2(torch.randint(-10, 13, (n,), generator=_gen(701)).float())
    x = x * (torch.randint(0, 2, (n,), generator=_gen(702)) * 2 - 1)
    x[:4] = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11])  # ties of the fp16 grid
    y = torch.zeros(n + 8, dtype=DT, device=DEV)
    ops.cast_f32_f16(dev(x), y)
    torch.cuda.synchronize()
    assert torch.equal(y[:n].cpu().view(torch.int16), x.to(DT).view(torch.int16)) and float(y[n:].float().abs().sum()) == 0
