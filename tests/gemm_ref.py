"""fp64 torch restatement of the contracts of csrc/gemm.hip (k_gemm_nt<1|2>, k_transpose, k_softmax_fwd / _bwd) and csrc/transformer.hip
(LayerNorm and GEGLU, forward and backward), the test inputs and the per-element bounds.  Test helper only; imports no project code.  The
fenced buffers, the comparer and the integer / Gaussian generators are those of tests/conv_ref.py; this module adds the 2-D
[.., rows, cols] placement on top of them.

Contracts, on the kernels' own operands (bf16 activations, fp32 bias / gamma / beta / scores):
    GEMM       C = alpha * A @ B^T (+ bias[n]) (+ R) (+ C_old when accumulating); a bf16 output is rounded once, an fp32 output not at all
    transpose  a move of bits, plus zeros in output columns R .. P
    softmax    p = softmax(s) over the last axis, columns cols .. ld zero;  dS = P * (dP - sum_k dP_k P_k) * scale, same padding
    LayerNorm  mean and BIASED variance (two-pass in fp64), y = (x - mean) * rstd * gamma + beta;
               dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma;  dgamma += sum_rows dy * xhat, dbeta += sum_rows dy
    GEGLU      y = a * gelu(g), erf form;  da = dy * gelu(g), dg = dy * a * (Phi(g) + g * phi(g))

Input kind `ints` (GEMM only): integers in [-4, 4] times one power of two per tensor (GSCALE), alpha in {1, 0.5, 0.125}.  Every product and,
while check_exact_range() holds, every partial sum in any order is exact in fp32, and so are `* alpha`, `+ bias`, `+ R`, `+ C_old` (all
multiples of one unit, alpha * 2^-7, below 2^24 units).  bf16 outputs must equal RNE_bf16(ref) bit for bit, fp32 outputs the reference.

Input kind `gauss`: bf16-rounded normal values; each row (and for B each output column) has its own offset and amplitude, so a row, column,
head or batch taken from a neighbour changes the answer by far more than any bound below.

Bounds, per element.  Term 1 is the output rounding, half_ulp_bf16(ref) (round to nearest; absent for fp32 outputs).  It is taken at the
reference, not at the kernel's fp32 value v: rounding is monotone and binade edges are bf16 numbers, so a v that the fp32 error pushed
across an edge rounds to the edge, which is nearer to ref than v.  Term 2 is the fp32 work, always scaled by the ABSOLUTE-VALUE form of
the expression (written A_.. below), never by |ref| where the expression cancels.  u = 2^-24 is the unit roundoff of fp32.
    GEMM        (K + 3) 2^-23 A_c,  A_c = |alpha| |A| |B|^T + |bias| + |R| + |C_old|:  K additions in any order, each off by at most one
                ulp of a partial sum that never exceeds A_c (covers a truncating MFMA adder), three more for alpha, bias / R, C_old.
    softmax     ref * (cols 2^-23 + (|s - max| + 4) 2^-22).  x = s - max is one rounding (x u); __expf(x) is exp2(x * log2 e): the
                rounded constant and the rounded product move the exponent by 2 |x| log2(e) u, i.e. the value by a factor 2 |x| u, and
                v_exp_f32 adds 1 ulp (2 u, common.h) -- 3 |x| u + 2 u, under (|x| + 1/2) 2^-22, for the numerator.  The denominator
                sums cols such terms: cols 2^-23 for its additions, and its terms' own errors average with the weights p_k to
                (3/4 E_p|x| + 1/2) 2^-22.  1 / sum and the last product add 1.5 u = 3/8 * 2^-22.  So the constant 4 holds while
                1/2 + 3/4 E_p|x| + 1/2 + 3/8 <= 4, i.e. E_p|x| <= 3.5 (E_p|x| <= ln cols always, from the entropy; one-hot rows
                have ~0): softmax_fwd() asserts that premise on the inputs it is given, as check_exact_range() does for `ints`.
                Both softmax bounds carry + 2^-126: the tail of a nearly one-hot row is a denormal number, which hardware may flush.
    softmax bwd scale * P * (cols 2^-23 sum_k |dP_k P_k| + 2^-22 (|dP| + |dot|)): the dot product as the GEMM's, then one subtraction
                and two products (3 u of |dP| + |dot|).
    LayerNorm   statistics record, as test_gn_kernels_gpu.check_stats: |mean - ref| <= 1e-5 rms, |rstd / ref - 1| <= 1e-4.  y, dx, dgamma
                and dbeta are compared with the fp64 expression evaluated WITH THE KERNEL'S OWN RECORD (the record's error is bounded
                by the line above and must not be counted twice):
                y       2^-22 ((|x| + |mean|) rstd |gamma| + |beta|): a subtraction, two products, an addition (4 u);
                dx      rstd 2^-22 (|g| + |m1| + |xhat m2|), m1 = mean(g), m2 = mean(g xhat): the expression's own roundings (dy * gamma,
                        two subtractions, the products with m2 and rstd).  The two means are fp32 sums that are not in the record; the
                        bound has no term of its own for them.  Each value passes 8 NP serial additions on its lane and a 6-level
                        wave tree, at most (8 NP + 6) u of mean|g| resp. mean|g xhat| -- 22 u at C > 512, against the 4 u the terms
                        |m1| and |xhat m2| carry only where the means do not cancel.  The kernel is measured against this form
                        as it stands (fp32 torch uses 0.54 - 1.13 of the fp32 term before the output rounding and passes after it: test_gemm_ref_cpu);
                dgamma  M 2^-23 A, A = |dgamma_0| + sum_rows |dy xhat|;  dbeta M 2^-23 (|dbeta_0| + sum_rows |dy|).  The kernel forms and
                        sums dy * (x - mean) * rstd in fp64 per wave (in fp32 each term alone carries 3 u, more than the 2 u the
                        bound has at M = 1), so what counts is: one conversion per wave (together u A), at most two fold additions
                        in LDS (2 u A) and one atomic addition per block of 4 rows_per_wave rows (u A each): (3 + ceil(M / 4)) u A,
                        and with fewer than four rows fewer folds (M = 1: 2 u, M = 2: 3 u, M = 3: 4 u) -- at most 2 M u A for every
                        M.  dbeta sums bf16 values: a wave's fp32 additions, the same folds and atomics.
    GEGLU       y:  2^-22 |a g|.  gelu(g) = g/2 (1 + erf(g / sqrt 2)) cancels for negative gates, so the term is NOT relative to |ref|:
                the absolute error of 1 + erf is about u whatever its value, and g / 2 scales it.
                da: 2^-22 |dy g|.   dg: 2^-22 |dy a| (1 + |g| phi(g) (1 + g^2 / 2)): Phi as above; phi(g) = exp(-g^2 / 2) / sqrt(2 pi)
                through __expf has the relative error (g^2 / 2 + 1/2) 2^-22 derived for the softmax numerator.
"""
import math

import torch

from tests.conv_ref import (AMAX, BF16, F32, F64, FENCE_ROWS, GAP, SENT, SENT_F32, U23, Slot, SlotF32, _gauss, _ints, bf, bf_trunc,  # noqa: F401
                            compare, old_measure_passes)

U22 = 2.0 ** -22
TINY = 2.0 ** -126        # the smallest normal fp32 / bf16 number: a result below it may be flushed to zero (softmax tails, e^-90)
GSCALE = dict(a=2.0 ** -2, b=2.0 ** -5, bias=2.0 ** -4, res=2.0 ** -1, c0=2.0 ** -2)
ALPHAS = (1.0, 0.5, 0.125)
EPS = 1e-5
SQRT2, SQRT2PI = math.sqrt(2.0), math.sqrt(2.0 * math.pi)


def half_ulp_bf16(ref):
    """Half a unit in the last place of bf16 (8 significant bits) at |ref|: 2^(floor(log2 |ref|) - 8); 0 at 0."""
    _, e = torch.frexp(ref.abs())                       # |ref| = m 2^e, m in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


# ----------------------------------------------------------------------------------------------------------------- fenced 2-D buffers
def slot2d(batch, rows, cols, placement, data=None, device="cpu"):
    """conv_ref.Slot holding a bf16 [..batch, rows, cols] matrix: dense, or the first / last `cols` columns of a buffer GAP wider, with
    FENCE_ROWS rows behind.  data: fp64, bf16-exact (an input: gaps NaN); None: an output (payload NaN, gaps and fence the sentinel)."""
    z = math.prod(batch)
    return Slot((z, 1, 1, rows, cols), placement, None if data is None else data.reshape(z * rows, cols), device)


def view2d(slot, batch):
    """The [..batch, rows, cols] view of a slot2d buffer that a kernel is handed."""
    v = slot.view()[:, 0, 0]
    return v.unflatten(0, batch) if batch else v[0]


def slot2d_f32(batch, rows, cols, pitched, prefill=None, device="cpu"):
    """conv_ref.SlotF32 holding an fp32 [..batch, rows, cols] output; prefill fp64 (accumulated into) or None (NaN poison)."""
    z = math.prod(batch)
    pre = torch.full((z * rows, cols), math.nan, dtype=F64) if prefill is None else prefill.reshape(z * rows, cols)
    return SlotF32(pre, pitched, device)


def view2d_f32(slot, batch, rows):
    return slot.view().unflatten(0, tuple(batch) + (rows,))


# ----------------------------------------------------------------------------------------------------------------- inputs
def ints(g, shape, what):
    """Integers times GSCALE[what]; every index of all but the last dim (batch, row) has its own amplitude and offset."""
    return _ints(g, tuple(shape), GSCALE[what], rows=len(shape) - 1)


def gauss_rows(g, shape, sigma=1.0, offset=0.0, round_bf16=True):
    """Normal values; every index of all but the last dim gets its own amplitude in [0.5, 1.5) sigma and its own offset (N(0, sigma), or
    with `offset` that many of the row's standard deviations: LayerNorm's rows with the mean at 8 sigma).  bf16-rounded, or fp32."""
    lead = tuple(shape[:-1]) + (1,)
    amp = (0.5 + torch.rand(lead, generator=g)) * sigma
    off = offset * amp if offset else torch.randn(lead, generator=g) * sigma
    t = torch.randn(tuple(shape), generator=g) * amp + off
    return (t.to(BF16) if round_bf16 else t.to(F32)).to(F64)


def check_exact_range(k, alpha, bias=False, res=False, c_old=False):
    """The `ints` premise of one GEMM: the absolute-value form of the whole expression stays below 2^24 units of alpha * a * b (every
    addend is a multiple of that unit).  Asserted before anything runs; returns the worst count of units."""
    assert alpha in ALPHAS
    unit = alpha * GSCALE["a"] * GSCALE["b"]
    worst = k * AMAX * AMAX
    for on, what in ((bias, "bias"), (res, "res"), (c_old, "c0")):
        if on:
            assert GSCALE[what] / unit == int(GSCALE[what] / unit)
            worst += AMAX * GSCALE[what] / unit
    assert worst < 2 ** 24, f"ints inputs are not exact here: {worst} units"
    return worst


# ----------------------------------------------------------------------------------------------------------------- GEMM
def gemm(a, b, alpha=1.0, bias=None, res=None, c_old=None, with_abs=False):
    """fp64 C [..batch, M, N] before any rounding (operands broadcast over the batch like torch.matmul); with_abs: (C, A_c)."""
    def run(a, b, al, bias, res, c_old):
        c = al * (a @ b.transpose(-1, -2))
        for t in (bias, res, c_old):
            if t is not None:
                c = c + t
        return c
    c = run(a, b, alpha, bias, res, c_old)
    if not with_abs:
        return c
    ab = lambda t: None if t is None else t.abs()  # noqa: E731
    return c, run(a.abs(), b.abs(), abs(alpha), ab(bias), ab(res), ab(c_old))


def gemm_bound(c, a_c, k, out_f32):
    acc = (k + 3) * U23 * a_c
    return acc if out_f32 else half_ulp_bf16(c) + acc


# ----------------------------------------------------------------------------------------------------------------- transpose
def transpose(x_i16, p):
    """int16 bit patterns [.., R, C] -> [.., C, P]: the move, zeros in columns R .. P."""
    r = x_i16.shape[-2]
    out = torch.zeros(tuple(x_i16.shape[:-2]) + (x_i16.shape[-1], p), dtype=torch.int16)
    out[..., :r] = x_i16.transpose(-1, -2)
    return out


def finite_bf16_bits(g, shape):
    """Random FINITE bf16 bit patterns as int16 (an exponent field of all ones, inf / NaN, is redrawn as a small number)."""
    v = torch.randint(-32768, 32768, tuple(shape), generator=g, dtype=torch.int32)
    v = torch.where((v & 0x7F80) == 0x7F80, v & ~0x4000, v)
    return v.to(torch.int16)


# ----------------------------------------------------------------------------------------------------------------- softmax
def _pad(t, ld):
    out = torch.zeros(tuple(t.shape[:-1]) + (ld,), dtype=F64)
    out[..., :t.shape[-1]] = t
    return out


def softmax_fwd(s, ld):
    """(p, bound) [rows, ld] from fp64 scores [rows, cols]; pad columns: value 0, bound 0."""
    cols = s.shape[-1]
    x = s - s.max(dim=-1, keepdim=True).values
    p = torch.softmax(x, dim=-1)
    assert float((p * x.abs()).sum(dim=-1).max()) <= 3.5, "the bound's constant needs E_p|s - max| <= 3.5 (module docstring)"
    bound = half_ulp_bf16(p) + p * (cols * U23 + (x.abs() + 4) * U22) + TINY
    return _pad(p, ld), _pad(bound, ld)                  # padded AFTER the floor is added: the pad columns keep a bound of exactly 0


def softmax_bwd(p, dp, scale, ld):
    """(dS, bound) [rows, ld] from the bf16 probabilities p [rows, cols] (fp64 values) and fp64 dp."""
    cols = p.shape[-1]
    dot = (dp * p).sum(dim=-1, keepdim=True)
    ds = p * (dp - dot) * scale
    a_dot = (dp * p).abs().sum(dim=-1, keepdim=True)
    bound = half_ulp_bf16(ds) + abs(scale) * p * (cols * U23 * a_dot + U22 * (dp.abs() + dot.abs())) + TINY
    return _pad(ds, ld), _pad(bound, ld)                 # as above: pad columns must be exactly 0


# ----------------------------------------------------------------------------------------------------------------- LayerNorm
def layernorm_stats(x):
    """Two-pass fp64 (mean, biased variance) per row."""
    return x.mean(dim=-1), x.var(dim=-1, unbiased=False)


def stats_ratios(mean, rstd, mean_ref, var_ref, eps=EPS):
    """(worst |mean - ref| / (1e-5 rms), worst |rstd / ref - 1| / 1e-4) of a statistics record; not-a-number counts as infinite."""
    rms = (var_ref + mean_ref.square()).sqrt()
    rstd_ref = 1.0 / (var_ref + eps).sqrt()
    rm = (mean - mean_ref).abs() / (1e-5 * rms + 1e-300)
    rr = (rstd / rstd_ref - 1).abs() / 1e-4
    fin = lambda r: float(torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf)).max())  # noqa: E731
    return fin(rm), fin(rr)


def layernorm_fwd(x, gamma, beta, mean, rstd):
    """(y, bound) with the given record (fp64 values of the kernel's fp32 mean / rstd)."""
    m, r = mean[:, None], rstd[:, None]
    y = (x - m) * r * gamma + beta
    return y, half_ulp_bf16(y) + U22 * ((x.abs() + m.abs()) * r * gamma.abs() + beta.abs())


def layernorm_bwd(x, dy, gamma, mean, rstd, dgamma0, dbeta0):
    """dict dx, dgamma, dbeta and their bounds b_dx, b_dgamma, b_dbeta, with the given record; dgamma0 / dbeta0 the fp32 prefills."""
    rows, c = x.shape
    m, r = mean[:, None], rstd[:, None]
    xh = (x - m) * r
    g = dy * gamma
    m1, m2 = g.mean(dim=-1, keepdim=True), (g * xh).mean(dim=-1, keepdim=True)
    dx = r * (g - m1 - xh * m2)
    b_dx = half_ulp_bf16(dx) + r * U22 * (g.abs() + m1.abs() + (xh * m2).abs())
    a_dg, a_db = dgamma0.abs() + (dy * xh).abs().sum(dim=0), dbeta0.abs() + dy.abs().sum(dim=0)
    return dict(dx=dx, b_dx=b_dx, dgamma=dgamma0 + (dy * xh).sum(dim=0), dbeta=dbeta0 + dy.sum(dim=0), a_dgamma=a_dg, a_dbeta=a_db,
                b_dgamma=rows * U23 * a_dg, b_dbeta=rows * U23 * a_db)


# ----------------------------------------------------------------------------------------------------------------- GEGLU
def _phis(g):
    return 0.5 * (1.0 + torch.erf(g / SQRT2)), torch.exp(-0.5 * g * g) / SQRT2PI


def geglu_fwd(h):
    """(y, bound) [M, F] from h [M, 2F] = [a | gate]."""
    f = h.shape[-1] // 2
    a, g = h[..., :f], h[..., f:]
    y = a * g * _phis(g)[0]
    return y, half_ulp_bf16(y) + U22 * (a * g).abs()


def geglu_bwd(h, dy):
    """(dh, bound) [M, 2F] = [da | dg]."""
    f = h.shape[-1] // 2
    a, g = h[..., :f], h[..., f:]
    cdf, pdf = _phis(g)
    da, dg = dy * g * cdf, dy * a * (cdf + g * pdf)
    b_da = half_ulp_bf16(da) + U22 * (dy * g).abs()
    b_dg = half_ulp_bf16(dg) + U22 * (dy * a).abs() * (1.0 + g.abs() * pdf * (1.0 + 0.5 * g * g))
    return torch.cat([da, dg], dim=-1), torch.cat([b_da, b_dg], dim=-1)
