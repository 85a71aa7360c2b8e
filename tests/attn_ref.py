"""fp64 torch restatement of the fused attention kernels' contract (csrc/attention.hip, csrc/attention_wide.hip), a model of where
they round to bf16, the per-element error bounds both are held to, and the test inputs.  Test helper only; imports no project code.

Contract (per image b and head h; q, k, v = the head's columns of the packed qkv[B*S][3C]):
    t = (q k^T) * scale * log2(e)        lse = log2 sum_j 2^t_j        P = 2^(t - lse)
    o = P v       y = o + x              D = rowsum(dO * o)            dP = dO v^T       dS = P * (dP - D) * scale
    dQ = dS k     dK = dS^T q            dV = P^T dO

Error scales (what one relative rounding of an operand of each product can move its result by):
    A   = P |v|                               forward
    G_V = P^T |dO|                            dV
    G_Q = scale * (P * (|dP| + |D|)) |k|      dQ
    G_K = scale * (P * (|dP| + |D|))^T |q|    dK

Bounds, per element.  bf16 carries 8 significant bits, so one rounding moves a value v by at most 2^-8 |v| (2^-9 |v| at the top of a
binade); each budget is the sum of the roundings the model makes, worst case:
    y    : 2^-8 |y| + 2^-7 A         output rounding 2^-8 |y|, P rounding 2^-8 A, partial-output rounding 2^-8 A (split runs)
    lse  : 2^-8 + 2^-22 |lse|        twice what a relative error of 2^-9 in the sum l does to log2(l); the fp32 store of lse
    dsum : 2^-8 sum_j |dy_j| |y_j| + 1e-5     o is rebuilt as bf16(y) - x, off by at most 2^-8 |y| per element
    dV     : 2^-8 |ref| + KAPPA 2^-8 G_V      KAPPA measured on the rounding model, see below
    dQ, dK : 2^-8 |ref| + KAPPA 2^-8 G + E    E_Q = scale * (P * b) |k|,  E_K = scale * (P * b)^T |q|,  b = the dsum bound of the row

Why E.  dS = P * (dP - D) * scale takes D from the rebuilt o, so an error e_i in D_i moves dS_ij by scale * P_ij * e_i, and e_i is
bounded by the dsum bound, not by u|D_i|: the rebuilt o is off by u|y| = u|o + x|, which |D| does not see (where dO . o nearly
cancels, D is tiny and its error is not).  G alone therefore cannot bound dQ / dK for the kernels' own design: on near-one-hot inputs
the rounding model misses 2^-8 |ref| + KAPPA 2^-8 G by factors up to 1.9e5 for any usable KAPPA, with every one of those elements
explained by a dsum error inside the dsum bound.  E is that propagation, worst case, and is exact about what it covers: a dsum at its
bound.  dV does not depend on D and gets no such term.

Split against single pass on the same data (split_bound): 2^-7 |y| + 3 * 2^-8 A.  Both runs round their output (2^-8 |y| each).  Both
round P, and against different running maxima -- a split restarts its maximum, and bf16(p * a) != a * bf16(p) unless a is a power of
two -- so the two P roundings are independent (2^-8 A each); the split run also rounds its partial outputs (2^-8 A).  Counting the
partial rounding alone (2^-8 |y| + 2^-8 A) does not hold: the rounding model itself exceeds it by up to 1.8x at every split shape.
"""
import math

import torch

F64 = torch.float64
LOG2E = 1.0 / math.log(2.0)
U8, U7, U22 = 2.0 ** -8, 2.0 ** -7, 2.0 ** -22

# Worst (err - 2^-8 |ref| - E) / (2^-8 G) of rounding_model over every shape of CASES x every input kind of KINDS, split as expected
# and unsplit, is 1.74 (dV of a 2-way split, near-one-hot inputs: P rounding + partial rounding + output rounding; EXPERIMENTS.md has
# the table).  Doubled and rounded up to a power of two.  The margin is for what the model leaves out: fp32 accumulation order and
# the hardware exp2.
KAPPA = 4.0

# (d, B, H, S, expected split count): the smallest shapes at which each path of the kernels exists
NARROW = [(d, 1, 1, S, 1) for d in (32, 64) for S in (1, 31, 33, 63, 64, 65, 127, 129, 255, 257)] + \
         [(d, 2, 2, 65, 1) for d in (32, 64)] + \
         [(d, 1, 1, 513, 2) for d in (32, 64)] + [(d, 1, 1, 769, 3) for d in (32, 64)] + [(d, 2, 2, 520, 2) for d in (32, 64)] + \
         [(32, 2, 2, 1000, 4)] + [(d, 1, 1, 2048, 8) for d in (32, 64)]
WIDE = [(512, 1, 1, S, 1) for S in (1, 31, 33, 63, 65, 255, 257)] + [(512, 1, 1, 512, 2), (512, 1, 1, 513, 2), (512, 2, 1, 513, 2)] + \
       [(768, 1, 1, 33, 1), (768, 1, 1, 257, 1), (768, 1, 1, 513, 2)]
CASES = NARROW + WIDE
KINDS = ("gauss", "rising", "onehot", "qzero")
# the subset the non-Gaussian inputs run on: one row past a tile, every split count, B * H > 1 with a split, both wide dims
KIND_CASES = [(d, 1, 1, 65, 1) for d in (32, 64)] + [(d, 2, 2, 520, 2) for d in (32, 64)] + [(32, 1, 1, 769, 3), (32, 2, 2, 1000, 4)] + \
             [(64, 1, 1, 2048, 8), (512, 1, 1, 65, 1), (512, 2, 1, 513, 2), (768, 1, 1, 33, 1), (768, 1, 1, 513, 2)]


def key_tile(d):
    """Rows of the reduction axis per tile: 64 for head dims 32 / 64, 32 for the one wide head."""
    return 64 if d <= 64 else 32


def bf(t):
    """Round to bf16 (nearest even), back in fp64."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def make_inputs(kind, B, H, S, d, seed=None, resid=True):
    """bf16 qkv [B, S, 3C], x [B, S, C] (None without residual), dy [B, S, C], and the softmax scale."""
    C = H * d
    g = torch.Generator().manual_seed(S + d if seed is None else seed)
    qkv = torch.randn(B, S, 3 * C, generator=g) * 1.5   # the Gaussian of test_flash_attention_fwd_bwd
    x = torch.randn(B, S, C, generator=g)
    dy = torch.randn(B, S, C, generator=g)
    scale = 1 / math.sqrt(d)
    if kind == "rising":
        # every query ~ the all-ones direction, key j = ramp(j) * ones: the score climbs with j from about -60 to +60 in the exp2
        # domain, so each tile raises the running max and the early splits end up with vanishing weights in the merge
        ramp = torch.linspace(-1, 1, S) if S > 1 else torch.ones(1)
        beta = 60.0 / (LOG2E * math.sqrt(d))
        noise = torch.randn(B, S, 2 * C, generator=g) * 0.1
        qkv[..., :C] = 1.0 + noise[..., :C]
        qkv[..., C:2 * C] = beta * ramp[None, :, None] + noise[..., C:]
    elif kind == "onehot":
        qkv[..., :2 * C] *= 4.0   # amplitude 6: scores of std 36, each query attends to one or two keys
    elif kind == "qzero":
        qkv[..., :C] = 0.0
    else:
        assert kind == "gauss", kind
    return qkv.bfloat16(), (x.bfloat16() if resid else None), dy.bfloat16(), scale


def _heads(t, B, H, S, d):  # [B, S, H*d] -> [B, H, S, d]
    return t.reshape(B, S, H, d).permute(0, 2, 1, 3)


def _merge(t, B, H, S, d):  # [B, H, S, d] -> [B, S, H*d]
    return t.permute(0, 2, 1, 3).reshape(B, S, H * d)


def _split_qkv(qkv, B, H, S, d):
    C = H * d
    w = qkv.reshape(B, S, 3 * C).to(F64)
    return (_heads(w[..., i * C:(i + 1) * C], B, H, S, d) for i in range(3))


def reference(qkv, x, dy, B, H, S, d, scale):
    """Everything the kernels emit, in fp64 on the bf16-rounded operands, plus the error scales.  Channel quantities are [B, S, C],
    row quantities (lse in the log2 domain, dsum) are [B*H, S]."""
    C = H * d
    q, k, v = _split_qkv(qkv, B, H, S, d)
    do = _heads(dy.to(F64), B, H, S, d)
    t = q @ k.transpose(-1, -2) * (scale * LOG2E)
    lse = torch.logsumexp(t * math.log(2.0), dim=-1) * LOG2E
    P = torch.exp2(t - lse[..., None])
    o = P @ v
    D = (do * o).sum(-1)
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP - D[..., None]) * scale
    om = _merge(o, B, H, S, d)
    y = om + (x.to(F64) if x is not None else 0.0)
    y_abs = y.abs()
    W = P * (dP.abs() + D.abs()[..., None]) * scale
    dsum_scale = _heads(dy.to(F64).abs() * y_abs, B, H, S, d).sum(-1)
    WD = P * (U8 * dsum_scale + 1e-5)[..., None] * scale   # |dS| moved by a dsum that sits at its own bound
    return dict(
        y=y, o=om, lse=lse.reshape(B * H, S), dsum=D.reshape(B * H, S),
        dQ=_merge(dS @ k, B, H, S, d), dK=_merge(dS.transpose(-1, -2) @ q, B, H, S, d), dV=_merge(P.transpose(-1, -2) @ do, B, H, S, d),
        A=_merge(P @ v.abs(), B, H, S, d), G_V=_merge(P.transpose(-1, -2) @ do.abs(), B, H, S, d),
        G_Q=_merge(W @ k.abs(), B, H, S, d), G_K=_merge(W.transpose(-1, -2) @ q.abs(), B, H, S, d),
        E_Q=_merge(WD @ k.abs(), B, H, S, d), E_K=_merge(WD.transpose(-1, -2) @ q.abs(), B, H, S, d), dsum_scale=dsum_scale.reshape(B * H, S))


def split_ranges(S, d, nsplit):
    """The reduction-axis ranges of an nsplit-way run: whole tiles, ceil(tiles / nsplit) per split (AttnArgs: `tps` tiles each)."""
    tile = key_tile(d)
    ntiles = -(-S // tile)
    tps = -(-ntiles // nsplit)
    out = [(z * tps * tile, min(S, (z + 1) * tps * tile)) for z in range(nsplit)]
    assert all(a < b for a, b in out), "an empty split: no such launch exists"
    return out


FAULTS = ("pad_unmasked", "key_dropped", "merge_wrong_max", "dsum_from_y", "row_unwritten", "row_unwritten_nan")


def rounding_model(qkv, x, dy, B, H, S, d, scale, nsplit=1, fault=None):
    """The same math with a bf16 rounding wherever the kernels hold a bf16 value: P as the operand of P v and P^T dO, dS as the operand
    of the dQ / dK products, each split's normalised partial O and partial dQ | dK | dV, o = bf16(y) - x, and the outputs.  Sums and
    exponentials stay exact (fp64): accumulation order and the hardware exp2 are what KAPPA's margin is for.

    fault: one of FAULTS, a planted defect of the kind a wrong kernel would have (tests/test_attention_cpu.py)."""
    assert fault is None or fault in FAULTS, fault
    C = H * d
    q, k, v = _split_qkv(qkv, B, H, S, d)
    do = _heads(dy.to(F64), B, H, S, d)
    xr = x.to(F64) if x is not None else torch.zeros(B, S, C, dtype=F64)
    ranges = split_ranges(S, d, nsplit)
    tile = key_tile(d)
    t = q @ k.transpose(-1, -2) * (scale * LOG2E)

    # ---- forward: per split the max m, the sum l of 2^(t - m) and O = (bf16(p) v) / l
    tf = t
    if fault == "key_dropped":  # key 17 of every tile never counts
        tf = t.clone()
        tf[..., 17::tile] = -math.inf
    ms, ls, parts = [], [], []
    for z, (k0, k1) in enumerate(ranges):
        tz = tf[..., k0:k1]
        m = tz.max(-1).values
        p = torch.exp2(tz - m[..., None])
        l = p.sum(-1)
        if fault == "pad_unmasked" and z == nsplit - 1:  # the zero rows that pad the last tile score t = 0 and carry v = 0
            npad = -(-S // tile) * tile - S
            m2 = m.clamp_min(0.0)
            p, l = p * torch.exp2(m - m2)[..., None], l * torch.exp2(m - m2) + npad * torch.exp2(-m2)
            m = m2
        o = (bf(p) @ v[..., k0:k1, :]) / l[..., None]
        ms.append(m), ls.append(l), parts.append(bf(o) if nsplit > 1 else o)
    if nsplit > 1:
        M = torch.stack(ms).max(0).values
        wm = list(ms)
        if fault == "merge_wrong_max":  # the first split's weight takes the last split's running max
            wm[0] = ms[-1]
        w = [l * torch.exp2(m - M) for l, m in zip(ls, wm)]
        L = sum(w)
        o = sum(wi[..., None] * pi for wi, pi in zip(w, parts)) / L[..., None]
    else:
        M, L, o = ms[0], ls[0], parts[0]
    lse = (M + torch.log2(L)).to(torch.float32).to(F64)
    y = bf(_merge(o, B, H, S, d) + xr)
    if fault in ("row_unwritten", "row_unwritten_nan"):
        y[:, S - 1] = 0.0 if fault == "row_unwritten" else math.nan

    # ---- backward
    orb = _heads(y - xr if fault != "dsum_from_y" else y, B, H, S, d)
    D = (do * orb).sum(-1).to(torch.float32).to(F64)
    P = torch.exp2(t - lse[..., None])
    dP = do @ v.transpose(-1, -2)
    Pb, dSb = bf(P), bf(P * (dP - D[..., None]) * scale)
    dq, dk, dv = [], [], []
    for a, b in ranges:  # dQ splits the keys; dK, dV split the queries
        dq.append(dSb[..., a:b] @ k[..., a:b, :])
        dk.append(dSb[..., a:b, :].transpose(-1, -2) @ q[..., a:b, :])
        dv.append(Pb[..., a:b, :].transpose(-1, -2) @ do[..., a:b, :])
    fin = lambda parts: _merge(bf(sum(bf(p) for p in parts)) if nsplit > 1 else bf(parts[0]), B, H, S, d)
    out = dict(y=y, lse=lse.reshape(B * H, S), dsum=D.reshape(B * H, S), dQ=fin(dq), dK=fin(dk), dV=fin(dv))
    if fault in ("row_unwritten", "row_unwritten_nan"):
        for n in ("dQ", "dK", "dV"):
            out[n][:, S - 1] = 0.0 if fault == "row_unwritten" else math.nan
    return out


QUANTITIES = ("y", "lse", "dsum", "dQ", "dK", "dV")
_SCALE = dict(dQ="G_Q", dK="G_K", dV="G_V")


def bounds(ref, kappa=KAPPA):
    """Per-element error bound of every quantity (module docstring)."""
    b = dict(y=U8 * ref["y"].abs() + U7 * ref["A"], lse=U8 + U22 * ref["lse"].abs(), dsum=U8 * ref["dsum_scale"] + 1e-5)
    for n, g in _SCALE.items():
        b[n] = U8 * ref[n].abs() + kappa * U8 * ref[g] + (ref["E" + g[1:]] if n != "dV" else 0.0)
    return b


def ratios(got, ref, kappa=KAPPA, names=QUANTITIES):
    """Worst err / bound per quantity over EVERY element; an element that is not a number counts as infinitely wrong."""
    bnd, out = bounds(ref, kappa), {}
    for n in names:
        g = got[n].to(F64).reshape(ref[n].shape)
        err = (g - ref[n]).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / bnd[n])   # a zero bound (dK at q = 0) admits exactly the reference
        out[n] = float(torch.where(torch.isfinite(g), r, torch.full_like(r, math.inf)).max())
    return out


def kappa_ratios(got, ref):
    """(err - 2^-8 |ref|) / (2^-8 G) per gradient: what KAPPA is measured from."""
    out = {}
    for n, g in _SCALE.items():
        err = (got[n].to(F64).reshape(ref[n].shape) - ref[n]).abs()
        num, den = err - U8 * ref[n].abs() - (ref["E" + g[1:]] if n != "dV" else 0.0), U8 * ref[g]
        ok = num > 0
        out[n] = float((num[ok] / den[ok]).max()) if bool(ok.any()) else 0.0
    return out


def failed(got, ref, kappa=KAPPA, names=QUANTITIES):
    """Names of the quantities with at least one element outside its bound."""
    return [n for n, r in ratios(got, ref, kappa, names).items() if not r <= 1.0]


def qzero_failed(got, qkv, x, B, H, S, d):
    """q = 0 makes attention uniform whatever k holds: lse = log2(S) to 1e-5 and o = mean(v) within the forward bound, for every row.
    A key that is masked and should not be, or the reverse, moves lse by log2(1 +- 1/S) >= 7e-4 at S <= 2048."""
    C = H * d
    v = qkv.reshape(B, S, 3 * C)[..., 2 * C:].to(F64)
    mean = v.mean(1, keepdim=True).expand(B, S, C)
    y = mean + (x.to(F64) if x is not None else 0.0)
    bad = []
    if not float((got["lse"].to(F64).reshape(B * H, S) - math.log2(S)).abs().max()) <= 1e-5:
        bad.append("lse")
    bound = U8 * y.abs() + U7 * v.abs().mean(1, keepdim=True)
    if not bool(((got["y"].to(F64).reshape(B, S, C) - y).abs() <= bound).all()):
        bad.append("y")
    return bad


def split_bound(ref):
    """How far the outputs of a split run and of a single pass on the same data may sit apart (module docstring)."""
    return 2 * U8 * ref["y"].abs() + 3 * U8 * ref["A"]
