"""Every (tile, split-K, K-order) variant the autotuner may pin, on the engines' own GEMM launches, against float64.

`Schedule.autotune()` times every variant `gemm_variants()` lists for a launch and keeps the fastest; which one that is
depends on the machine and the day, and only the winner's numbers ever reach a parity check.  Here each engine is built with
`autotune=False` (Schedule._tile_cache is then neither read nor written), its inputs are filled as its own engine test fills
them, and `fwd_pre`, `fwd`, `bwd` are walked in order, every entry executed.  For the FIRST `ops.gemm` launch of each
signature (`signature()` below) the walk stops and, on the live operands the schedule has produced so far,

  1. snapshots the whole base tensor of `out`, `out2` and `gn_sums`,
  2. computes the float64 reference once (tests/helpers/gemm_ref.py, pinned without a kernel by tests/test_gemm_ref_cpu.py),
  3. for every reachable variant: restores the snapshots, runs `eng._pin(f, variant)` and compares
       values        out / out2 with the two bounds of tests/test_kernels_gpu.py's `check` (relative Frobenius norm and the
                     element-wise bound) at that file's bars: t16(2e-3) for a 16-bit output, 1e-3 for an f32 output; the decoded
                     GroupNorm sums as test_gemm_groupnorm_sums_and_fused_apply does — against the float64 sums of the values
                     the variant stored, sum at 1e-3, sum of squares at 1e-5;
       surroundings  every byte of the snapshotted base tensors outside the launch's logical output is bit-identical to the
                     snapshot: a variant must not write into the `ld` gap or the neighbouring slice of a concat buffer;
  4. restores the snapshots and runs the launch as the schedule has it, so the walk continues on the schedule's own data.

Reachable variants: `gemm_variants(key, conv, geglu, CANDIDATES)`, CANDIDATES being Schedule.autotune's default as a literal.
Two rules, both read off engine/schedule.py:
  * a launch that carries `gn_sums` got them from `fuse_gn_stats` after tuning and only with split_k = 1: its split_k == 1
    variants run with the statistics, all the others with the gn_* arguments stripped (the form a splitting pick leaves);
  * a launch whose builder pinned `tile_hint` itself (the UNet's three time-embedding linears) is skipped by the autotuner
    (`autotune()`: `f.keywords.get("tile_hint")` -> continue): its only reachable form is the scheduled one, which is compared
    as one variant.
No variant is left out: each case asserts tested == enumerated and prints the launches, signatures and variants it covered
and the variant that came closest to its bar per output kind.  Comparisons run on the device; data comes to the host only
to describe a failure (and the few dozen GroupNorm words, which `ops.gn_sums_decode` decodes on the host).

A status error of the library (RuntimeError) on a reachable variant fails the case at once."""
import time
from functools import partial

import pytest
import torch

from helpers import gemm_ref as G
from helpers.checks import DEV, DT, ELEM_K, t16  # the kernel files' bars

pytestmark = pytest.mark.gpu

CANDIDATES = (1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18)  # Schedule.autotune's default
TOL_16, TOL_F32, TOL_GN_SUM, TOL_GN_SUMSQ = 2e-3, 1e-3, 1e-3, 1e-5
GN_KEYS = ("gn_sums", "gn_hw", "gn_groups", "gn_slots")


# ---------------------------------------------------------------------------------------------- which launches, which variants
def _storage_ptr(t):
    return t.untyped_storage().data_ptr()


def signature(f):
    """Schedule._gemm_key plus the epilogue features and layouts of the launch; the first launch of each is the one tested"""
    from view_neti_amd.engine.schedule import Schedule
    kw = f.keywords
    A, _, out = f.args[:3]
    g = G.geometry(f)
    conv = kw.get("conv")
    resid = kw.get("resid")
    has = tuple(kw.get(k) is not None for k in ("bias", "rowadd", "resid", "gate", "out2", "gn_sums"))
    nums = (kw.get("act") or 0, kw.get("act2") or 0, kw.get("gate_act") or 0, kw.get("geglu") or 0,
            float(kw.get("alpha", 1.0)) != 1.0, g.batch > 1, kw.get("tile_hint") or 0)
    alias = resid is not None and _storage_ptr(resid) == _storage_ptr(out)
    wide_in = (int(conv["ldx"]) > int(conv["Ci"])) if conv else \
        ((kw.get("lda") if kw.get("lda") is not None else A.stride(-2)) > g.K)
    return (Schedule._gemm_key(f), has, nums, alias, g.out_strides[1] > g.out_shape[2], wide_in)


def variants_of(f):
    """[(form, variant)]: form 'gn' = with the statistics, 'plain' = the launch without gn_* arguments (or one that never had
    them), 'scheduled' = a builder-pinned launch as it stands"""
    from view_neti_amd.engine.schedule import Schedule, gemm_variants
    kw = f.keywords
    if kw.get("tile_hint"):
        return [("scheduled", None)]
    vs = gemm_variants(Schedule._gemm_key(f), kw.get("conv"), kw.get("geglu"), CANDIDATES)
    assert vs and len(set(vs)) == len(vs)
    if kw.get("gn_sums") is None:
        return [("plain", v) for v in vs]
    return [("gn", v) for v in vs if v[1] == 1] + [("plain", v) for v in vs if v[1] != 1]


def describe(lst_name, idx, f):
    key, has, nums, alias, wide_out, wide_in = signature(f)
    names = [n for n, h in zip(("bias", "rowadd", "resid", "gate", "out2", "gn_sums"), has) if h]
    names += [f"{n}={v}" for n, v in zip(("act", "act2", "gate_act", "geglu"), nums[:4]) if v]
    names += [n for n, v in (("alpha", nums[4]), ("batch", nums[5]), ("resid-is-out", alias), ("ldc>N", wide_out),
                             ("ld-in>K", wide_in)) if v]
    return f"{lst_name}[{idx}] key={key} {'+'.join(names) or 'plain'}"


# ---------------------------------------------------------------------------------------------- comparison, on the device
class Bar:
    """the two bounds of test_kernels_gpu.check against one reference: rel = |got - ref|_F / (|ref|_F + 1e-12) < tol and
    |got - ref| <= ELEM_K * tol * (rms(ref) + |ref|) element-wise — the same float32 arithmetic, on the reference's device"""

    def __init__(self, ref, tol):
        self.tol = tol
        self.b = ref.float()
        self.norm = self.b.norm() + 1e-12
        self.bound = ELEM_K * tol * (self.b.pow(2).mean().sqrt() + self.b.abs())

    def measure(self, got):
        """device tensor [rel / tol, max(|diff| - bound), max(|diff| / bound)]: passes iff [0] < 1 and [1] <= 0"""
        d = (got.float() - self.b).abs()
        rel = torch.linalg.vector_norm(d) / self.norm
        return torch.stack((rel / self.tol, (d - self.bound).max(), (d / self.bound.clamp_min(1e-30)).max()))

    def where(self, got):
        """host-side description of the worst element (failure path only)"""
        a, b = got.float().cpu(), self.b.cpu()
        ex = (a - b).abs() - self.bound.cpu()
        idx = tuple(int(i) for i in torch.unravel_index(ex.argmax(), ex.shape))
        return f"worst element {list(idx)}: got {a[idx].item():.6e}, ref {b[idx].item():.6e}, bound {self.bound.cpu()[idx].item():.3e}"


def _bits(t):
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Surroundings:
    """the base tensors of a launch's outputs: snapshot, restore, and 'nothing outside the logical views changed'"""

    def __init__(self):
        self.bases = {}  # storage pointer -> [base, snapshot, [(offset, shape, strides)]]

    def add(self, t, shape, strides):
        base = t._base if t._base is not None else t
        assert base.is_contiguous() and base._base is None
        rec = self.bases.setdefault(_storage_ptr(base), [base, base.clone(), []])
        assert rec[0].dtype == t.dtype
        rec[2].append((t.storage_offset() - base.storage_offset(), tuple(shape), tuple(strides)))
        # the logical view lies inside the base (else the snapshot would not cover what the launch may write)
        last = rec[2][-1][0] + sum((n - 1) * s for n, s in zip(shape, strides))
        assert 0 <= rec[2][-1][0] and last < base.numel(), (shape, strides, base.shape)

    def restore(self):
        for base, snap, _ in self.bases.values():
            base.copy_(snap)

    def changed_outside(self):
        """device bool: some byte outside the logical views differs from the snapshot"""
        bad = None
        for base, snap, views in self.bases.values():
            cur = base.clone()
            for off, shape, strides in views:
                torch.as_strided(cur, shape, strides, off).copy_(torch.as_strided(snap, shape, strides, off))
            b = (_bits(cur) != _bits(snap)).any()
            bad = b if bad is None else (bad | b)
        return bad

    def where(self):
        out = []
        for base, snap, views in self.bases.values():
            cur = base.clone()
            for off, shape, strides in views:
                torch.as_strided(cur, shape, strides, off).copy_(torch.as_strided(snap, shape, strides, off))
            flat = (_bits(cur) != _bits(snap)).reshape(-1).nonzero().reshape(-1)
            if flat.numel():
                out.append(f"{flat.numel()} elements of a {tuple(base.shape)} {base.dtype} base changed outside the output, "
                           f"first flat indices {flat[:8].tolist()} (views {views})")
        return "; ".join(out)


def _view(t, shape, strides):
    return torch.as_strided(t, shape, strides, t.storage_offset())


# ---------------------------------------------------------------------------------------------- one tested launch
def _test_launch(eng, f, where, stats, failures):
    """every reachable variant of the launch `f`; returns the number of variants run and compared"""
    from view_neti_amd import ops, packing
    from view_neti_amd.engine.schedule import _chunk_major_ok
    kw = f.keywords
    out = f.args[2]
    g = G.geometry(f)
    sur = Surroundings()
    sur.add(out, g.out_shape, g.out_strides)
    if kw.get("out2") is not None:
        sur.add(kw["out2"], g.out2_shape, g.out2_strides)
    sums = kw.get("gn_sums")
    if sums is not None:
        sur.add(sums, sums.shape, sums.stride())
    ref = G.reference(f)  # from the live inputs, before anything is overwritten (resid may be `out` itself)
    f32 = out.dtype == torch.float32
    kind = "out f32" if f32 else "out 16-bit"
    bar_out = Bar(ref.out.reshape(g.out_shape), TOL_F32 if f32 else t16(TOL_16))
    bar_out2 = Bar(ref.out2, t16(TOL_16)) if ref.out2 is not None else None
    conv = kw.get("conv")
    B_cm = packing._chunk_major(f.args[1], f.args[1].shape[0], conv["Ci"]) if _chunk_major_ok(conv) else None
    stripped = None
    if sums is not None:
        stripped = partial(ops.gemm, *f.args, **{k: v for k, v in kw.items() if k not in GN_KEYS})
    checked_cm = False
    n = 0
    for form, v in variants_of(f):
        sur.restore()
        if form == "scheduled":
            run = f
        else:
            run = eng._pin(f if form == "gn" else (stripped or f), v, B_cm)
            if v[2] and not checked_cm:
                # the chunk-major pick runs on a re-ordered copy of the packed weight: the same problem, stated twice
                r2 = G.reference(run).out
                assert ((r2 - ref.out).norm() <= 1e-12 * ref.out.norm()).item(), f"{where}: chunk-major weights differ"
                checked_cm = True
        run()
        res = [bar_out.measure(_view(out, g.out_shape, g.out_strides))]
        if bar_out2 is not None:
            res.append(bar_out2.measure(_view(kw["out2"], g.out2_shape, g.out2_strides)))
        res.append(sur.changed_outside().float().reshape(1))
        vals = torch.cat(res).tolist()  # the one synchronisation of this variant
        tag = f"{where} variant={v} form={form}"
        for name, nums, bar, t in ((kind, vals[0:3], bar_out, out), ("out2", vals[3:6], bar_out2, kw.get("out2"))):
            if bar is None:
                continue
            r, ex, ratio = nums
            worst = max(r, ratio)
            if not (worst <= stats["closest"].get(name, (-1.0, ""))[0]):
                stats["closest"][name] = (worst, tag)
            if not (r < 1.0 and ex <= 0.0):
                shape, strides = (g.out_shape, g.out_strides) if name != "out2" else (g.out2_shape, g.out2_strides)
                failures.append(f"{tag}: {name} rel/bar {r:.3f}, element/bound {ratio:.3f} (bar {bar.tol:g}); "
                                + bar.where(_view(t, shape, strides)))
        if vals[-1] != 0.0:
            failures.append(f"{tag}: wrote outside its output: {sur.where()}")
        if form == "gn":
            hw, G_ = int(kw["gn_hw"]), int(kw["gn_groups"])
            got = ops.gn_sums_decode(sums.sum(1))                                   # [img, G, 2] float64, host
            want = G.gn_sums(_view(out, g.out_shape, g.out_strides)[0], hw, G_).cpu()  # of the values the variant stored
            for q, (name, tol) in enumerate((("gn sum", TOL_GN_SUM), ("gn sumsq", TOL_GN_SUMSQ))):
                bar = Bar(want[..., q], tol)
                r, ex, ratio = bar.measure(got[..., q]).tolist()
                if not (max(r, ratio) <= stats["closest"].get(name, (-1.0, ""))[0]):
                    stats["closest"][name] = (max(r, ratio), tag)
                if not (r < 1.0 and ex <= 0.0):
                    failures.append(f"{tag}: {name} rel/bar {r:.3f}, element/bound {ratio:.3f} (bar {tol:g}); "
                                    + bar.where(got[..., q]))
        n += 1
    sur.restore()
    f()
    return n


def _walk(eng, test_lists, label):
    """execute fwd_pre, fwd, bwd in order; in the lists named by `test_lists` test the first launch of every signature"""
    from view_neti_amd import ops
    lists = [(n, getattr(eng, n)) for n in ("fwd_pre", "fwd", "bwd") if getattr(eng, n)]
    is_gemm = lambda f: getattr(f, "func", None) is ops.gemm
    # what is to be covered, counted before anything runs (signatures and variants are static properties of the launches)
    seen, enumerated, n_gemm = set(), 0, 0
    for name, lst in lists:
        for f in lst:
            if name in test_lists and is_gemm(f):
                n_gemm += 1
                s = signature(f)
                if s not in seen:
                    seen.add(s)
                    enumerated += len(variants_of(f))
    stats, failures = dict(closest={}), []
    done, tested = set(), 0
    t0 = time.time()
    for name, lst in lists:
        for idx, f in enumerate(lst):
            if name in test_lists and is_gemm(f) and signature(f) not in done:
                done.add(signature(f))
                tested += _test_launch(eng, f, describe(name, idx, f), stats, failures)
            else:
                f()
    torch.cuda.synchronize()
    dt = time.time() - t0
    print(f"[variants {label} {'+'.join(test_lists)}] {n_gemm} GEMM launches, {len(seen)} signatures, {tested} variants "
          f"(enumerated {enumerated}), {dt:.2f} s")
    for kind, (worst, tag) in sorted(stats["closest"].items()):
        print(f"[variants {label}] closest to its bar, {kind}: error/bar {worst:.3g} at {tag}")
    assert n_gemm > 0 and len(done) == len(seen)
    assert tested == enumerated, f"{tested} variants ran, {enumerated} are reachable"
    assert not failures, f"{len(failures)} variant checks failed:\n" + "\n".join(failures[:40])


# ---------------------------------------------------------------------------------------------- the engines
def _r16(w, pred=lambda k, v: True):
    """weights rounded to the 16-bit format once (as the engines' own tests do)"""
    return {k: (v.to(DT).float() if pred(k, v) else v) for k, v in w.items()}


def _unet(cfg_name, B, H, W):
    from view_neti_amd import sd_config as sc, synth
    from view_neti_amd.engine.unet import UNetEngine
    cfg = sc.CONFIGS[cfg_name]().unet
    eng = UNetEngine(cfg, _r16(synth.unet_weights(cfg)), B, H, W, autotune=False)
    L, Dc, nl = 77, cfg.cross_attention_dim, cfg.n_cross_layers
    eng.x_in.copy_(synth.gaussian((B, 4, H, W), 5))
    eng.timesteps.copy_(synth.timesteps(B))
    eng.ctx_k.copy_(synth.gaussian((nl, B * L, Dc), 6))
    eng.ctx_v.copy_(synth.gaussian((nl, B * L, Dc), 7))
    eng.dpred.copy_(synth.gaussian((B, 4, H, W), 8).permute(0, 2, 3, 1).reshape(B * H * W, 4))
    return eng


def _vae_encoder(B, H, W):
    from view_neti_amd import sd_config as sc, synth
    from view_neti_amd.engine.vae import VAEEncoderEngine
    cfg = sc.tiny().vae
    eng = VAEEncoderEngine(cfg, _r16(synth.vae_weights(cfg)), B, H, W, autotune=False)
    eng.x_in.copy_(synth.pixel_values(B, H, W))
    return eng


def _vae_decoder(B, h, w):
    from view_neti_amd import sd_config as sc, synth
    from view_neti_amd.engine.vae import VAEDecoderEngine
    cfg = sc.tiny().vae
    wts = _r16(synth.vae_decoder_weights(cfg), lambda k, v: v.dim() >= 2 and not k.startswith("post_quant"))
    eng = VAEDecoderEngine(cfg, wts, B, h, w, autotune=False)
    eng.z_in.copy_(synth.gaussian((B, 4, h, w), 21) * cfg.scaling_factor)
    return eng


def _text():
    """tests/test_text_gpu.py's engine: 16 passes of the tiny CLIP, B = 2, object mapper only"""
    from view_neti_amd import sd_config as sc, synth
    from view_neti_amd.engine.text import MapperState, TextEngine, flatten_mapper_state
    from view_neti_amd.mapper import fourier_frequencies
    cfg = sc.tiny().clip
    D, L, nl, B = cfg.hidden_size, cfg.max_positions, 16, 2
    wr = _r16(synth.clip_weights(cfg), lambda k, v: k.endswith("weight") and v.dim() == 2 and "embedding" not in k)
    ph_obj = cfg.vocab_size - 3
    ids = synth.input_ids(B, ph_obj, cfg.vocab_size, L)
    ids[1] = torch.roll(ids[1], 3)
    gen = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=gen)
    sd = {"net.0.weight": rn(64, 64) * 0.15, "net.0.bias": rn(64) * 0.1, "net.1.weight": 1 + 0.1 * rn(64),
          "net.1.bias": 0.1 * rn(64), "net.3.weight": rn(64, 64) * 0.15, "net.3.bias": rn(64) * 0.1,
          "net.4.weight": 1 + 0.1 * rn(64), "net.4.bias": 0.1 * rn(64), "output_layer.0.weight": rn(2 * D, 64) * 0.15,
          "output_layer.0.bias": rn(2 * D) * 0.1}
    w_enc = fourier_frequencies([0.03, 2.0], 64, 0, preserve_rng=True)
    ctx_k = torch.zeros(nl, B * L, D, dtype=DT, device=DEV)
    ctx_v = torch.zeros_like(ctx_k)
    dk = (synth.gaussian((nl, B * L, D), 11) * 0.5).to(DT).to(DEV)
    dv = (synth.gaussian((nl, B * L, D), 12) * 0.5).to(DT).to(DEV)
    po = flatten_mapper_state(sd).to(DEV)
    mo = MapperState(po, w_enc.to(DEV), 0.4, 0.2)
    eng = TextEngine(cfg, wr, nl, B, torch.tensor([17, 803]).to(DEV), ctx_k, ctx_v, dk, dv, mo, torch.zeros_like(po),
                     autotune=False)
    eng.set_batch(ids, torch.full((B,), ph_obj), None, None)
    return eng


ENGINES = {
    "unet-tiny-B2-16x16": lambda: _unet("tiny", 2, 16, 16),
    "unet-tiny-B1-8x16": lambda: _unet("tiny", 1, 8, 16),        # the deepest level is 1 x 2 tokens: M = 2
    "unet-tiny21-B2-16x16": lambda: _unet("tiny21", 2, 16, 16),  # linear proj_in / proj_out weights
    "unet-tiny21-B1-8x16": lambda: _unet("tiny21", 1, 8, 16),
    "vae-encoder-tiny-B2-64x64": lambda: _vae_encoder(2, 64, 64),
    "vae-decoder-tiny-B1-8x8": lambda: _vae_decoder(1, 8, 8),
    "text-tiny": _text,
}
# (engine, lists tested): a backward case replays the forward lists as the schedule has them first
_dead = None  # set once by a case that ended in an error other than a failed comparison; later cases then fail at once
CASES = [(e, ls) for e in ENGINES for ls in ((("fwd_pre", "fwd"), ("bwd",)) if not e.startswith("vae") else (("fwd_pre", "fwd"),))]


@pytest.mark.parametrize("engine,lists", CASES, ids=[f"{e}-{'fwd' if 'fwd' in ls else 'bwd'}" for e, ls in CASES])
def test_autotune_variants(engine, lists):
    global _dead
    from view_neti_amd.engine.schedule import Schedule
    assert _dead is None, f"not run: {_dead}"
    cache_before = dict(Schedule._tile_cache)
    try:
        eng = ENGINES[engine]()
        _walk(eng, lists, engine)
    except AssertionError:
        raise
    except BaseException as e:
        # a status or HIP error: the device may be in no state to be handed the remaining cases
        _dead = f"{engine} ended with {type(e).__name__}: {e}"
        raise
    assert Schedule._tile_cache == cache_before, "autotune=False: the pick cache is neither read nor written"
