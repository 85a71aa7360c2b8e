"""fp64 torch restatement of the convolution kernels' contract (csrc/conv.hip, conv27*.h/.hip, convph.hip, conv1x1.hip, conv_c1.hip), the
test inputs, the fenced buffers the kernels are run in and the per-element comparer.  Test helper only; imports no project code.

Contract (x [N, Cin, D, H, W], w [Cout, Cin, kd, kh, kw], dy the gradient of y; the kernels hold activations channels-last in bf16):
    y  = bf16(bf16(conv(x, w) + addvec) + res)        (one rounding without a residual: the two roundings conv27.hip documents)
    dx = bf16(conv_transpose(dy, w))                  (the Upsample fallback alone: bf16(fold(bf16(fine-grid dx))), see folded_dx)
    dw += sum over images and voxels of x (x) dy      fp32, accumulated into what the buffer holds
    cs += per-image [N, Cout] or batch [Cout] column sums of dy, fp32, accumulated
An Upsample + conv plan computes the same on F.interpolate(x, 2, "nearest").

Input kind `ints` (the main one).  Every tensor holds small integers times one power of two (SCALE): all bf16-exact, and so is every sum
of up to 8 weight taps (the phase kernels' summed weights: |sum| <= 32 needs 6 bits).  Every product is exact in fp32, and while the
sum of absolute values stays below 2^24 units every partial sum IN ANY ORDER is exact too, so the fp32 accumulator of a correct kernel
equals the fp64 reference whatever its tiling, split or MFMA order.  Zero tolerance: bf16 outputs must equal RNE_bf16(reference) bit for
bit, fp32 outputs the reference itself.  check_exact_range() asserts the 2^24 premise per case before anything runs, from the term
count and the largest operands (an upper bound of the absolute-value convolution: 512 -> 512 k3 gives 512 * 27 * 16 + 32 = 221 216
units, a weight gradient over 2 x 20x32x32 voxels 655 360 + 32).

Input kind `gauss`.  bf16-rounded normal x / dy, an fp32 master weight that is NOT bf16-representable; the reference multiplies
RNE_bf16(w).  Per-element bound 2^-8 |ref| + n 2^-23 A with n the number of accumulated terms and A the same operation on absolute
values: one output rounding (two with a residual, derived at gauss_bounds) plus the worst case of n fp32 additions in any order, each
off by at most one unit in the last place of a partial sum that never exceeds A -- covers truncating adders as well as round-to-nearest.
fp32 outputs get the second term only.  Measured: fp32 torch on the CPU sits at 3.5e-4 of the accumulation term.  The bound is coarse
(at 20x32x32 it admits a dropped product: n 2^-23 A ~ 30 against a product of ~1); it is there for the rounding of real-valued
weights, the exact kind carries the indexing.
"""
import math
import os
import re

import torch
import torch.nn.functional as F

F64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32
U8, U23 = 2.0 ** -8, 2.0 ** -23
# power-of-two scale per tensor: nothing is a round number, every product is a multiple of one unit per output
SCALE = dict(x=2.0 ** -2, dy=2.0 ** -3, w=2.0 ** -5, bias=2.0 ** -4, res=2.0 ** -1, dw0=2.0 ** -2, cs0=2.0 ** -1)
AMAX = 4                  # |integer| <= AMAX in every tensor
SENT = 0x5A3C             # int16 sentinel of fence rows and output gap columns (as bf16: a finite 1.3e13, never a result)
SENT_F32 = 0x5A3C5A3C     # int32 sentinel behind fp32 outputs
FENCE_ROWS = 64
GAP = 32                  # channels a pitched placement is wider by
PLACEMENTS = ("dense", "first", "last")

torch.set_num_threads(16)


def bf(t):
    """Round to bf16 (nearest even), back in fp64."""
    return t.to(F32).to(BF16).to(F64)


def bf_trunc(t):
    """Round to bf16 by truncation (what a kernel that drops the low half of the fp32 word does), back in fp64."""
    i = t.to(F32).contiguous().view(torch.int32)
    return (i & -65536).view(F32).to(F64)


# ----------------------------------------------------------------------------------------------------------------- inputs
def _ints(g, shape, scale, rows=2):
    """Integers in [-AMAX, AMAX] * scale; each index of the first `rows` dims (image, channel) gets its own amplitude and its own
    offset so that a wrong image / channel / tap index changes the answer; non-zero with probability >= 0.85."""
    lead = tuple(shape[:rows]) + (1,) * (len(shape) - rows)
    amp = torch.randint(2, AMAX + 1, lead, generator=g)
    off = torch.randint(-1, 2, lead, generator=g)
    v = (torch.rand(shape, generator=g) * (2 * amp + 1)).floor().long() - amp + off
    v = v.clamp(-AMAX, AMAX)
    fill = torch.where(torch.rand(shape, generator=g) < 0.5, amp, -amp).expand(shape)
    v = torch.where((v == 0) & (torch.rand(shape, generator=g) < 0.7), fill, v)   # a = 2: P(0) = 0.2 * 0.3
    return v.to(F64) * scale


def _gauss(g, shape, scale=1.0, round_bf16=True):
    t = torch.randn(shape, generator=g) * scale
    return (t.to(BF16) if round_bf16 else t).to(F64)


def make_inputs(kind, n, cin, cout, dims, kernel, out_dims, seed=0, up=False):
    """fp64 tensors x [N, Cin, dims], w [Cout, Cin, k], bias [Cout], addrows [N, Cout], dy / res [N, Cout, out_dims], prefills dw0, cs0_img
    [N, Cout], cs0 [Cout].  `w` is the fp32 MASTER weight (gauss: not bf16-representable; the reference multiplies bf(w))."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + 3 * cin + 5 * cout + sum(dims) + 11 * sum(kernel) + (1 if up else 0))
    kt = kernel[0] * kernel[1] * kernel[2]
    xs, ys, ws = (n, cin) + tuple(dims), (n, cout) + tuple(out_dims), (cout, cin) + tuple(kernel)
    if kind == "ints":
        return dict(x=_ints(g, xs, SCALE["x"]), w=_ints(g, ws, SCALE["w"]), bias=_ints(g, (cout,), SCALE["bias"], 1),
                    addrows=_ints(g, (n, cout), SCALE["bias"]), dy=_ints(g, ys, SCALE["dy"]), res=_ints(g, ys, SCALE["res"]),
                    dw0=_ints(g, ws, SCALE["dw0"]), cs0_img=_ints(g, (n, cout), SCALE["cs0"]), cs0=_ints(g, (cout,), SCALE["cs0"], 1))
    assert kind == "gauss", kind
    return dict(x=_gauss(g, xs), w=_gauss(g, ws, 1.0 / math.sqrt(cin * kt), round_bf16=False).to(F32).to(F64), bias=_gauss(g, (cout,), 1.0, False).to(F32).to(F64),
                addrows=_gauss(g, (n, cout), 1.0, False).to(F32).to(F64), dy=_gauss(g, ys), res=_gauss(g, ys),
                dw0=_gauss(g, ws, 1.0, False).to(F32).to(F64), cs0_img=_gauss(g, (n, cout), 1.0, False).to(F32).to(F64),
                cs0=_gauss(g, (cout,), 1.0, False).to(F32).to(F64))


def check_exact_range(n, cin, cout, out_dims, kernel, up=False):
    """The `ints` premise: every absolute-value sum stays below 2^24 units of its output (asserted before anything runs)."""
    kt = kernel[0] * kernel[1] * kernel[2]
    a2 = AMAX * AMAX
    fwd = cin * kt * a2 + AMAX * SCALE["bias"] / (SCALE["x"] * SCALE["w"])
    dgr = cout * kt * a2 * (8 if up else 1)            # (the coarse dx of an Upsample + conv folds 8 fine voxels)
    vox = n * out_dims[0] * out_dims[1] * out_dims[2]
    wgr = vox * a2 + AMAX * SCALE["dw0"] / (SCALE["x"] * SCALE["dy"])
    csm = vox * AMAX + AMAX * SCALE["cs0"] / SCALE["dy"]
    worst = max(fwd, dgr, wgr, csm)
    assert worst < 2 ** 24, f"ints inputs are not exact here: {worst} units"
    return worst


# ----------------------------------------------------------------------------------------------------------------- reference
def reference(t, stride, padding, up=False, addvec="bias", with_abs=False):
    """fp64 reference of everything the kernels emit, on the kernels' operands (the weight rounded to bf16).  y1 = conv + addvec before any
    rounding; dx, dw (WITHOUT prefill), cs_img [N, Cout], cs [Cout].  with_abs: also A_y, A_dx, A_dw, A_cs_img, A_cs (gauss bounds)."""
    wq = bf(t["w"])
    add = t["bias"][None, :] if addvec == "bias" else t["addrows"]

    def run(x, w, dy, a):
        x = x.clone().requires_grad_(True)
        w = w.clone().requires_grad_(True)
        xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x
        if up:
            xin.retain_grad()
        y = F.conv3d(xin, w, None, stride=stride, padding=padding) + a[:, :, None, None, None]
        assert y.shape == dy.shape, (y.shape, dy.shape)
        y.backward(dy)
        return y.detach(), x.grad, w.grad, (xin.grad if up else None)

    y1, dx, dw, dx_fine = run(t["x"], wq, t["dy"], add)
    out = dict(y1=y1, dx=dx, dw=dw, dx_fine=dx_fine, cs_img=t["dy"].sum(dim=(2, 3, 4)), cs=t["dy"].sum(dim=(0, 2, 3, 4)))
    if with_abs:
        ay, adx, adw, _ = run(t["x"].abs(), wq.abs(), t["dy"].abs(), add.abs())
        out.update(A_y=ay, A_dx=adx, A_dw=adw, A_cs_img=t["dy"].abs().sum(dim=(2, 3, 4)), A_cs=t["dy"].abs().sum(dim=(0, 2, 3, 4)))
    return out


def expected_y(ref, res=None, kind="ints"):
    """fp64 value the forward output is compared with BEFORE its last rounding.  Without a residual: conv + addvec.  With one, `ints`:
    bf16(conv + addvec) + res, the kernels' two roundings modelled exactly (the accumulator is exact, so the first rounding is the
    reference's own).  `gauss`: the unrounded conv + addvec + res -- an accumulator that is off by an ulp can round the first time to the
    bf16 neighbour of the reference's choice, a whole bf16 ulp away; gauss_bounds carries the first rounding as a term instead."""
    if res is None:
        return ref["y1"]
    return (bf(ref["y1"]) if kind == "ints" else ref["y1"]) + res


def folded_dx(ref):
    """The data gradient of an Upsample + conv plan on its FALLBACK route (conv.hip: dgrad_upconv_fallback), before its last rounding: the
    inner plan stores the fine-grid gradient in bf16, mi_upsample_nearest_bwd folds its 2x2x2 blocks and rounds again.  Two kernels, two
    roundings by construction -- as the residual's; the phase kernel (and every other route) rounds the exact sum once."""
    f = bf(ref["dx_fine"])
    n, c, d, h, w = f.shape
    return f.view(n, c, d // 2, 2, h // 2, 2, w // 2, 2).sum(dim=(3, 5, 7))


def terms(n, cin, cout, out_dims, kernel, up=False):
    """Accumulated terms per output element of each quantity (the n of the gauss bound)."""
    kt = kernel[0] * kernel[1] * kernel[2]
    vox = n * out_dims[0] * out_dims[1] * out_dims[2]
    return dict(y=cin * kt + 1, dx=cout * kt * (8 if up else 1), dw=vox + 1, cs_img=vox // n + 1, cs=vox + 1)


# ----------------------------------------------------------------------------------------------------------------- fenced buffers
def cl(t):
    """[N, C, D, H, W] -> channels-last rows [N*D*H*W, C]"""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])


class Slot:
    """A channels-last bf16 tensor [N, D, H, W, C] inside a buffer of `rows + FENCE_ROWS` rows of `C` (dense) or `C + GAP` channels (the
    first / last C of them).  Inputs: payload = data, gap columns and the rows behind NaN (a kernel that reads a neighbour's channel or
    runs past the end computes NaN).  Outputs: payload NaN (an element the kernel forgets stays NaN), gap columns and the rows behind hold
    the int16 sentinel (a store that lands there changes it)."""

    def __init__(self, shape5, placement, data=None, device="cpu"):
        assert placement in PLACEMENTS
        n, d, h, w, c = shape5
        self.shape5, self.rows, self.c = tuple(shape5), n * d * h * w, c
        self.width = c if placement == "dense" else c + GAP
        self.c0 = self.width - c if placement == "last" else 0
        self.is_input = data is not None
        buf = torch.full((self.rows + FENCE_ROWS, self.width), math.nan, dtype=BF16)
        if self.is_input:
            buf[:self.rows, self.c0:self.c0 + c] = data.to(BF16)
            assert torch.equal(buf[:self.rows, self.c0:self.c0 + c].to(F64), data), "input is not bf16-exact"
        else:
            i16 = buf.view(torch.int16)
            i16[self.rows:] = SENT
            i16[:self.rows, :self.c0] = SENT
            i16[:self.rows, self.c0 + c:] = SENT
        self.buf = buf.to(device)

    def view(self):
        """The [N, D, H, W, C] tensor a kernel is handed: dense, or a channel slice of the wider buffer."""
        n, d, h, w, c = self.shape5
        return self.buf[:self.rows].view(n, d, h, w, self.width)[..., self.c0:self.c0 + c]

    def payload(self):
        return self.buf[:self.rows, self.c0:self.c0 + self.c]

    def fences_intact(self):
        i16 = self.buf.view(torch.int16)
        ok = bool((i16[self.rows:] == SENT).all())
        if self.c0:
            ok = ok and bool((i16[:self.rows, :self.c0] == SENT).all())
        if self.c0 + self.c < self.width:
            ok = ok and bool((i16[:self.rows, self.c0 + self.c:] == SENT).all())
        return ok


class SlotF32:
    """An fp32 output [R, C] (dw flattened to one row, column sums) starting from a prefill, at a row pitch of C or C + GAP, with sentinel
    gap columns and FENCE_ROWS sentinel floats behind."""

    def __init__(self, prefill2d, pitched=False, device="cpu"):
        r, c = prefill2d.shape
        self.r, self.c, self.width = r, c, c + GAP if pitched else c
        flat = torch.full((r * self.width + FENCE_ROWS,), SENT_F32, dtype=torch.int32)
        buf = flat[:r * self.width].view(r, self.width)
        buf[:, :c] = prefill2d.to(F32).view(torch.int32)
        self.flat = flat.to(device)

    def view(self):
        return self.flat[:self.r * self.width].view(F32).view(self.r, self.width)[:, :self.c]

    def payload(self):
        return self.view()

    def fences_intact(self):
        ok = bool((self.flat[self.r * self.width:] == SENT_F32).all())
        if self.width > self.c:
            ok = ok and bool((self.flat[:self.r * self.width].view(self.r, self.width)[:, self.c:] == SENT_F32).all())
        return ok


# ----------------------------------------------------------------------------------------------------------------- comparer
def compare(kind, slot, ref2d, bound2d=None):
    """(worst, fences_intact) over EVERY element of the slot's payload against ref2d [rows, C] (fp64, before the output rounding).
    ints: worst = the COUNT of elements that differ from RNE_bf16(ref) (bf16 slots) / from ref (fp32 slots); gauss: worst = max err / bound.
    An element that is not a number counts as infinitely wrong; nothing is excluded."""
    got = slot.payload().detach().to("cpu").to(F64)
    ref2d = ref2d.reshape(got.shape)
    finite = torch.isfinite(got)
    if kind == "ints":
        want = bf(ref2d) if isinstance(slot, Slot) else ref2d
        bad = (got != want) | ~finite
        worst = math.inf if not bool(finite.all()) else float(bad.sum())
    else:
        err = (got - ref2d).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / bound2d.reshape(got.shape))
        worst = float(torch.where(finite, r, torch.full_like(r, math.inf)).max())
    return worst, slot.fences_intact()


def gauss_bounds(ref, nterms, res=None):
    """Per-element bounds of the gauss kind (module docstring).  With a residual, against the unrounded s = conv + addvec + res: the
    accumulator is off by e_a <= n 2^-23 A, the first rounding by e_1 <= 2^-8 (|conv + addvec| + e_a), and the last rounds a value within
    e_a + e_1 of s, so |err| <= 2^-8 |s| + (1 + 2^-8) (e_a + e_1) <= 2^-8 |s| + (1 + 2^-7) (2^-8 |conv + addvec| + n 2^-23 A)."""
    y = expected_y(ref, res, "gauss")
    acc = nterms["y"] * U23 * ref["A_y"]
    b = dict(y=U8 * y.abs() + ((1 + 2 * U8) * (U8 * ref["y1"].abs() + acc) if res is not None else acc),
             dx=U8 * ref["dx"].abs() + nterms["dx"] * U23 * ref["A_dx"])
    for q in ("dw", "cs_img", "cs"):
        b[q] = nterms[q] * U23 * (ref["A_" + q] + 1e-30)
    return b


def old_measure_passes(got, ref, tol=1e-2):
    """The measure of test_conv_fwd_dgrad_wgrad: max |err| <= 1e-2 * max |ref| over the tensor."""
    err = float((got - ref).abs().max())
    return math.isfinite(err) and err <= tol * (float(ref.abs().max()) + 1e-12)


def kernel_ids():
    """name -> value of `enum mi_conv_kernel`, read from include/medimgen_hip.h"""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "medimgen_hip.h")).read()
    body = re.search(r"enum mi_conv_kernel \{(.*?)\};", hdr, re.S).group(1)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(MI_CK_[A-Z0-9_]+)\s*=\s*(\d+)", body)}
