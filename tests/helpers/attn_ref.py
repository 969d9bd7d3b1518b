"""The attention edge tests' reference, data, model and case lists (no GPU; tests/test_attn_ref_cpu.py pins all of it).

`attn_ref64`   O, lse, dQ, dK, dV in float64 from the SAME 16-bit-rounded inputs the kernel gets; top-left aligned causal
               mask (`key <= q`).
`attn_data`    four kinds of (q, k, v, dO).  `gauss`: unit Gaussians, the suite's usual data.  `negative`: component 0 of
               every head is 8 in q and -6 sqrt(D) / 8 in k, the rest 0.5 N(0,1): every real score is near -6 nat, so a key
               or query that should not be there (score 0) outweighs a real one by e^6 instead of being one of N equals.
               `staircase`: q0 = 8, k0 = (key // 64) 7.5 sqrt(D) / 8: the maximum of each 64-key tile of the forward
               kernel is 7.5 nat above the previous one's — under the 8-nat rescale threshold once, over it the next time.
               `descend`: the same steps reversed: the first tile holds the maximum, the later ones underflow.
`attn_model16` a float32 emulation of the kernels' ALGORITHM (csrc/attention.hip): f32 scores, the running max advanced
               per 32-query wave only when some row's tile maximum grew by more than the threshold, P rounded to 16 bits
               in front of the PV product, the denominator from those rounded P for D = 40 and 80 (the "ones" column of
               the V tile) and from the f32 P for D = 64 and 160, lse = stale max + log l, delta from the 16-bit O, f32 P in
               dS, 16-bit dS and P in front of the dQ / dK / dV products, 16-bit outputs.  Not a port: no MFMA order.
               Switches for the CPU file only: a zero key admitted at Nk, the causal diagonal moved, the threshold, and
               plain float32 summation in place of once-rounded dot products.
`spec`         which outputs a group asserts, at which of the suite's bars, with the two stated exceptions.
The shape lists at the end are the ones both test files use."""
import functools
import math

import torch

from helpers.checks import ELEM_K, check

HEAD_DIMS = (40, 64, 80, 160)
KINDS = ("gauss", "negative", "staircase", "descend")
RESCALE_THR = 8.0  # nat (csrc/attention.hip: RESCALE_THR_LOG2)
STEP = 7.5         # nat per 64-key tile of the staircase


def _heads(t, H, D):
    Bn, N, _ = t.shape
    return t.view(Bn, N, H, D).transpose(1, 2)


def _rows(t):
    Bn, H, N, D = t.shape
    return t.transpose(1, 2).reshape(Bn, N, H * D)


def _mask(Nq, Nk, causal, shift=0):
    m = torch.ones(Nq, Nk, dtype=torch.bool)
    if causal:
        m = torch.arange(Nk).view(1, Nk) <= torch.arange(Nq).view(Nq, 1) + shift
    return m


def attn_ref64(q, k, v, do, H, D, scale, causal):
    """q, do [Bn, Nq, H * D], k, v [Bn, Nk, H * D] (any dtype: the values as they are) -> dict of float64 o, lse, dq, dk, dv"""
    qh, kh, vh, doh = (_heads(t.double(), H, D) for t in (q, k, v, do))
    Nq, Nk = qh.shape[2], kh.shape[2]
    s = (qh @ kh.transpose(-1, -2)) * scale
    s = s.masked_fill(~_mask(Nq, Nk, causal), float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = p @ vh
    dv = p.transpose(-1, -2) @ doh
    dp = doh @ vh.transpose(-1, -2)
    ds = p * (dp - (doh * o).sum(-1, keepdim=True))
    dq = (ds @ kh) * scale
    dk = (ds.transpose(-1, -2) @ qh) * scale
    return {"o": _rows(o), "lse": lse, "dq": _rows(dq), "dk": _rows(dk), "dv": _rows(dv)}


def attn_data(kind, Bn, H, Nq, Nk, D, dtype, seed):
    """-> q, k, v, do (CPU, `dtype`), rows [Bn, N, H * D]"""
    g = torch.Generator().manual_seed(seed)
    q, do = (torch.randn(Bn, Nq, H, D, generator=g) for _ in range(2))
    k, v = (torch.randn(Bn, Nk, H, D, generator=g) for _ in range(2))
    if kind != "gauss":
        q *= 0.5
        k *= 0.5
        q[..., 0] = 8.0
        unit = math.sqrt(D) / 8.0  # k0 = x * unit gives the score x
        tile = torch.arange(Nk) // 64
        if kind == "negative":
            k[..., 0] = -6.0 * unit
        elif kind == "staircase":
            k[..., 0] = (tile * STEP * unit).view(1, Nk, 1)
        elif kind == "descend":
            k[..., 0] = ((tile.max() - tile) * STEP * unit).view(1, Nk, 1)
        else:
            raise ValueError(kind)
    return tuple(t.reshape(t.shape[0], t.shape[1], H * D).to(dtype) for t in (q, k, v, do))


def attn_model16(q, k, v, do, H, D, scale, causal, dtype, phantom_key=False, diag_shift=0, threshold=RESCALE_THR,
                 f32_order=False):
    """the kernels' algorithm in float32 (module docstring) -> dict of o, dq, dk, dv (`dtype`) and lse (float32)"""
    r16 = lambda t: t.to(dtype).float()
    # every dot product is an f32 value rounded ONCE, so that the model shows the algorithm's 16-bit roundings and no
    # summation order of its own; f32_order = True: plain float32 matmuls and sums instead (one possible order)
    mm = (lambda a, b: a @ b) if f32_order else (lambda a, b: (a.double() @ b.double()).float())
    qh, kh, vh, doh = (_heads(t.float(), H, D).contiguous() for t in (q, k, v, do))
    Bn, _, Nq, _ = qh.shape
    Nk = kh.shape[2]
    if phantom_key:  # what `key <= Nk` in place of `key < Nk` admits: loads past the end return zeros
        zero = torch.zeros(Bn, H, 1, D)
        kh, vh, Nk = torch.cat([kh, zero], 2), torch.cat([vh, zero], 2), Nk + 1
    mask = _mask(Nq, Nk, causal, diag_shift)
    s = mm(qh, kh.transpose(-1, -2)).masked_fill(~mask, float("-inf"))  # unscaled f32 scores, as the MFMA leaves them
    ones = D in (40, 80)
    # ---- forward: 64-key tiles, the running max per query, advanced per 32-query wave
    nw = (Nq + 31) // 32
    m = torch.full((Bn, H, Nq), float("-inf"))
    l = torch.zeros(Bn, H, Nq)
    o = torch.zeros(Bn, H, Nq, D)
    for k0 in range(0, Nk, 64):
        st = s[..., k0:k0 + 64]
        mx = st.max(-1).values
        grew = ~((mx - m) * scale <= threshold)  # (NaN from -inf - -inf counts as grown, as in the kernel)
        grew = torch.nn.functional.pad(grew, (0, nw * 32 - Nq)).view(Bn, H, nw, 32).any(-1, keepdim=True)
        grew = grew.expand(Bn, H, nw, 32).reshape(Bn, H, nw * 32)[..., :Nq]
        m_new = torch.maximum(m, mx)
        m_use = torch.where(m_new == float("-inf"), torch.zeros_like(m_new), m_new)
        alpha = torch.where(grew, torch.exp((m - m_use) * scale), torch.ones_like(m))
        m = torch.where(grew, m_use, m)
        l, o = l * alpha, o * alpha.unsqueeze(-1)
        p = torch.exp((st - m.unsqueeze(-1)) * scale)
        p16 = r16(p)
        l = l + (p16 if ones else p).sum(-1)
        o = o + mm(p16, vh[:, :, k0:k0 + 64])
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    o16 = r16(o * inv.unsqueeze(-1))
    lse = m * scale + torch.log(l)
    # ---- backward: lse and the 16-bit O as given
    delta = (doh * o16).sum(-1, keepdim=True) if f32_order else (doh.double() * o16.double()).sum(-1, keepdim=True).float()
    p = torch.exp(s * scale - lse.unsqueeze(-1)).masked_fill(~mask, 0.0)
    ds = p * (mm(doh, vh.transpose(-1, -2)) - delta)
    p16, ds16 = r16(p), r16(ds)
    dq = r16(mm(ds16, kh) * scale)
    dk = r16(mm(ds16.transpose(-1, -2), qh) * scale)
    dv = r16(mm(p16.transpose(-1, -2), doh))
    if phantom_key:
        dk, dv = dk[:, :, :-1], dv[:, :, :-1]
    out = {"o": o16, "dq": dq, "dk": dk, "dv": dv}
    out = {n: _rows(t).to(dtype) for n, t in out.items()}
    out["lse"] = lse
    return out


# ------------------------------------------------------------------------------------------ bars
def bar16(tol, dtype):
    """the tolerance of a check through a 16-bit store in `dtype` (helpers.checks.t16 for a given format)"""
    return tol * (8.0 if dtype == torch.bfloat16 else 1.0)


def margins(got, ref, tol, skip_cols=None):
    """helpers.checks.check as two ratios: (relative Frobenius error / tol, max |got - ref| / its element-wise bound);
    check passes iff both are finite, the first < 1 and the second <= 1.  skip_cols: last-axis columns left out of the
    element-wise bound (they stay in the Frobenius one)."""
    a, b = got.float().cpu(), ref.float().cpu()
    r = ((a - b).norm() / (b.norm() + 1e-12)).item()
    rms = b.pow(2).mean().sqrt()
    ratio = (a - b).abs() / (ELEM_K * tol * (rms + b.abs()))
    if skip_cols is not None:
        ratio[..., skip_cols] = 0.0
    e = ratio.max().item() if bool(torch.isfinite(ratio).all()) else float("nan")
    return r / tol, e


def spec(group, kind, Nk, H, D, dtype):
    """the outputs `group` asserts against float64 -> list of (name, tol, skip_cols, abs_bound).  The suite's bars: O
    t16(3e-3), lse 1e-3, dQ / dK / dV t16(6e-3).  Two exceptions.  (1) `negative` data: column 0 of every head of dQ is left
    out of the element-wise bound.  sum_j dS_j = 0 cancels the common k0 exactly in the true dQ; delta is formed from the
    16-bit O, which leaves k0 * scale * (delta error) behind in that column alone — the algorithm's conditioning on this
    data, not a kernel's tail.  (2) Nk = 1: the true dQ and dK are exactly zero, so a relative bound is meaningless:
    abs_bound 1e-4 instead (the model gives <= 1e-5, a mis-formed delta O(0.1))."""
    o = ("o", bar16(3e-3, dtype), None, None)
    lse = ("lse", 1e-3, None, None)
    g = bar16(6e-3, dtype)
    col0 = [h * D for h in range(H)] if kind == "negative" else None
    dq = ("dq", g, col0, None) if Nk > 1 else ("dq", None, None, 1e-4)
    dk = ("dk", g, None, None) if Nk > 1 else ("dk", None, None, 1e-4)
    dv = ("dv", g, None, None)
    return {"ragged": [o, lse, dq, dk, dv], "softmax": [o, lse, dv], "qsplit": [dk, dv], "small": [dq, dk, dv]}[group]


def failing_outputs(tag, group, kind, Nk, H, D, dtype, got, ref, only=None):
    """every entry of `spec` (or those named in `only`) through helpers.checks.check, or its stated exception -> the
    messages of those that fail"""
    bad = []
    for name, tol, skip_cols, abs_bound in spec(group, kind, Nk, H, D, dtype):
        if only is not None and name not in only:
            continue
        g, r = got[name].detach().cpu(), ref[name]
        try:
            if abs_bound is not None:
                worst = g.float().abs().max().item()
                print(f"[{tag} {name}] max abs {worst:.3e} (the truth is 0; bound {abs_bound})")
                assert bool(torch.isfinite(g.float()).all()) and worst <= abs_bound, \
                    f"{tag} {name}: |{name}| reaches {worst} where the truth is exactly 0 (bound {abs_bound})"
                continue
            rel_m, elem_m = margins(g, r, tol, skip_cols)
            print(f"[attn-margin] {tag} {name}: rel/bar {rel_m:.3f} elem/bound {elem_m:.3f}")
            if skip_cols is None:
                check(f"{tag} {name}", g, r, tol)
            else:
                assert math.isfinite(rel_m) and rel_m < 1, f"{tag} {name}: rel err {rel_m * tol} >= {tol}"
                g = g.float()
                g[..., skip_cols] = r[..., skip_cols].float()
                check(f"{tag} {name} (element-wise, without column 0 of each head)", g, r, tol)
        except AssertionError as e:
            bad.append(str(e))
    return bad


def assert_outputs(tag, group, kind, Nk, H, D, dtype, got, ref, only=None):
    bad = failing_outputs(tag, group, kind, Nk, H, D, dtype, got, ref, only)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------ the cases of both test files
BN, H_EDGE = 2, 3  # (H odd: head offsets are no multiples of 128 bytes)
# either side of the 32-query wave, the 128-query block, the 64-key tile of the forward / dQ kernels, the 128-key block
# and the 32- / 64-query stage of dK/dV
RAGGED_NONCAUSAL = [(1, 1), (1, 65), (33, 1), (31, 33), (32, 64), (33, 63), (64, 32), (65, 129), (127, 65), (128, 128),
                    (129, 127), (129, 193)]
RAGGED_CAUSAL = [(1, 1), (2, 2), (33, 33), (65, 65), (129, 129), (65, 129), (129, 65), (193, 193)]
RAGGED = [(nq, nk, 0) for nq, nk in RAGGED_NONCAUSAL] + [(nq, nk, 1) for nq, nk in RAGGED_CAUSAL]
RAGGED_KINDS = ("gauss", "negative")
SOFTMAX_SHAPES = [(33, 257, 0), (65, 193, 0), (257, 257, 1)]
SOFTMAX_KINDS = ("staircase", "descend")
# dK/dV query split, Bn = 2, H = 2: (id, D, Nq, Nk, causal, workspace floats as a function of the plane Bn * Nk * H * D
# (None: ample), the split count the case expects)
QSPLIT_BN, QSPLIT_H = 2, 2
QSPLIT_CASES = [
    ("d80_8stages", 80, 225, 77, 0, None, 2),         # eight 32-row stages: the least that splits
    ("d160_9stages", 160, 257, 77, 0, None, 2),       # nine stages: uneven ranges (5 + 4)
    ("d160_25stages", 160, 800, 77, 0, None, 6),      # 25 stages, 5 per range: the sixth range is empty
    ("d40_449", 40, 449, 77, 0, None, 2),             # 64-row stages: 8 of them
    ("d64_2keyblocks", 64, 513, 129, 0, None, 2),     # two key blocks
    ("d160_ws3", 160, 800, 77, 0, lambda plane: 2 * 3 * plane, 3),      # the workspace holds exactly three ranges
    ("d160_ws_short", 160, 800, 77, 0, lambda plane: 2 * 2 * plane - 1, 1),  # one float short of two: no split
    ("d160_causal", 160, 800, 77, 1, None, 1),        # causal never splits
]
SMALL_N = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96)
SMALL_D = 64


def seed_of(kind, Nq, Nk, D, causal):
    return (((KINDS.index(kind) * 1024 + Nq) * 1024 + Nk) * 2 + causal) * 256 + D  # (no two cases share one)


@functools.lru_cache(maxsize=8)
def case(kind, Bn, H, Nq, Nk, D, causal, dtype):
    """data and float64 reference of one case, computed once per process and shared (do not modify)"""
    q, k, v, do = attn_data(kind, Bn, H, Nq, Nk, D, dtype, seed_of(kind, Nq, Nk, D, causal))
    return {"q": q, "k": k, "v": v, "do": do, "ref": attn_ref64(q, k, v, do, H, D, D ** -0.5, bool(causal))}


def all_cases():
    """(group, kind, Bn, H, Nq, Nk, D, causal) of every float64 comparison of tests/test_attn_edges_gpu.py, each once (the
    three workspace sizes of the 800-query split case share their data)"""
    out = []
    for D in HEAD_DIMS:
        out += [("ragged", kind, BN, H_EDGE, nq, nk, D, c) for kind in RAGGED_KINDS for nq, nk, c in RAGGED]
        out += [("softmax", kind, BN, H_EDGE, nq, nk, D, c) for kind in SOFTMAX_KINDS for nq, nk, c in SOFTMAX_SHAPES]
    out += [("qsplit", kind, QSPLIT_BN, QSPLIT_H, nq, nk, D, c) for kind in RAGGED_KINDS
            for _, D, nq, nk, c, _, _ in QSPLIT_CASES]
    out += [("small", kind, BN, H_EDGE, n, n, SMALL_D, c) for kind in RAGGED_KINDS for n in SMALL_N for c in (0, 1)]
    return list(dict.fromkeys(out))
