"""tests/glue_ref.py is right and its bounds bite (no GPU).  Per op: the fp64 restatement against an independent formulation (the aten
operator with its autograd backward, torch.optim, oracle.nets, or an element-by-element loop); an fp32 / bf16 emulation of the kernel in
torch on the CPU, with the same roundings in the same places, inside the bound on the inputs of the rows of test_glue_kernels_gpu.py (the
multi-megabyte wrap rows are emulated where that takes under a second); and at least one deliberately wrong emulation outside the bound.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import glue_ref as G

F64, F32, BF16, I16, I32, I64 = G.F64, G.F32, G.BF16, G.I16, G.I32, G.I64
r32 = lambda t: t.to(F32)  # noqa: E731


def inside(got, ref, bound):
    w = G.ratio(got.to(F64), ref if torch.is_tensor(ref) else torch.tensor([ref], dtype=F64), bound if torch.is_tensor(bound) else torch.tensor([bound], dtype=F64))
    assert w <= 1.0, w
    return w


def outside(got, ref, bound):
    w = G.ratio(got.to(F64), ref if torch.is_tensor(ref) else torch.tensor([ref], dtype=F64), bound if torch.is_tensor(bound) else torch.tensor([bound], dtype=F64))
    assert w > 1.0, w


def to_bf(t32):
    return t32.to(BF16)


def trunc_bits(x):
    return (x.to(F32).contiguous().view(I32) >> 16).to(I16)


# ----------------------------------------------------------------------------------------------------------------- buffers
def test_buf_fences_and_poison():
    b = G.Buf(BF16, 3, 8, pitch=16)
    assert b.fences_ok() and bool((b.bits() == G.POISON16).all()) and b.ptr % 16 == 0
    b.flat[G.FENCE + 8] = 0
    assert not b.fences_ok()                                   # a gap column
    for where in (G.FENCE - 1, G.FENCE + 3 * 16):
        b = G.Buf(F32, 3, 8, pitch=16)
        b.flat[where] = 0
        assert not b.fences_ok()                               # the element before the payload, the element behind it
    i = G.Buf(F32, 1, 5, data=torch.arange(5, dtype=F64)[None])
    assert bool(torch.isnan(i.flat.view(F32)[:G.FENCE]).all()) and bool(torch.isnan(i.flat.view(F32)[G.FENCE + 5:]).all())
    assert torch.equal(i.got(), torch.arange(5, dtype=F64)[None])
    assert G.ratio(torch.tensor([math.nan]), torch.tensor([0.0]), torch.tensor([1.0])) == math.inf
    assert G.ratio(torch.tensor([1.0]), torch.tensor([0.0]), torch.tensor([0.0])) == math.inf
    assert G.ratio(torch.tensor([0.0]), torch.tensor([0.0]), torch.tensor([0.0])) == 0.0


# ----------------------------------------------------------------------------------------------------------------- moves
@pytest.mark.parametrize("name", [k for k in G.LAYOUT_ROWS if k != "wrap"] + ["wrap"])
def test_cast_and_layout(name):
    n, c, v = G.LAYOUT_ROWS[name]
    x = G.cast_inputs(G.gen("layout" + name), n * c * v).view(n, c, v)
    cl = G.to_ndhwc(x)
    assert torch.equal(cl, x.permute(0, 2, 1)) and torch.equal(G.to_ncdhw(cl), x)
    want = G.rne_bf16_bits(cl)
    assert torch.equal(want, cl.to(F32).bfloat16().view(I16))                # the integer rule is torch's RNE
    assert int((trunc_bits(cl) != want).sum()) > 0                           # truncation instead of RNE shows
    assert int((G.rne_bf16_bits(x.reshape(n, v, c)) != want).sum()) > 0 or c == 1   # the layout left as it was shows


def test_cast_edges_round_as_documented():
    w = torch.tensor(G.CAST_EDGES[:4], dtype=I64).to(I32).view(F32).to(F64)
    assert [int(b) & 0xFFFF for b in G.rne_bf16_bits(w)] == [0x3F80, 0x3F82, 0x3F80, 0x7F80]


@pytest.mark.parametrize("n", G.ADD_N[:-1])
def test_add_bf16(n):
    g = G.gen(f"add{n}")
    a = G.finite_bf16(g, (n,))
    b = G.bf(G.finite_bf16(g, (n,)) * torch.exp2(torch.randint(-10, 4, (n,), generator=g).to(F64)))
    want = G.add_bf16_bits(a, b)
    assert torch.equal(want, (r32(a) + r32(b)).bfloat16().view(I16))
    if n > 100:
        assert int((trunc_bits(r32(a) + r32(b)) != want).sum()) > 0


def test_copy_channels_and_space_depth_against_element_loops():
    g = G.gen("copy")
    src, dst = G.special_bf16_bits(g, (5, 40)), G.special_bf16_bits(g, (5, 64))
    got = G.copy_channels(src, 16, dst, 24, 16)
    for v in range(5):
        for c in range(64):
            assert got[v, c] == (src[v, 16 + c - 24] if 24 <= c < 40 else dst[v, c])
    assert not torch.equal(G.copy_channels(src, 8, dst, 24, 16), got)                   # a source offset one group off
    for f, dims in (((2, 2, 2), (5, 3, 7)), ((1, 2, 2), (4, 2, 6)), ((2, 1, 1), (5, 3, 7))):
        n, c = 2, 8
        x = G.special_bf16_bits(g, (n,) + dims + (c,))
        y = G.space_to_depth(x, f)
        p = G._sd_dims(dims, f)
        want = torch.zeros_like(y)
        wrong = torch.zeros_like(y)
        for i in range(y.numel() // c):                                                # the index arithmetic of k_space_depth
            t, q = divmod(i, math.prod(f))
            t, w = divmod(t, p[2])
            t, h = divmod(t, p[1])
            nn, d = divmod(t, p[0])
            qw, qh, qd = q % f[2], (q // f[2]) % f[1], q // (f[2] * f[1])
            sd, sh, sw = d * f[0] + qd, h * f[1] + qh, w * f[2] + qw
            if sd < dims[0] and sh < dims[1] and sw < dims[2]:
                want[nn, d, h, w, q * c:(q + 1) * c] = x[nn, sd, sh, sw]
                q2 = (qw * f[1] + qh) * f[0] + qd                                      # wrong: q enumerated w-major
                wrong[nn, d, h, w, q2 * c:(q2 + 1) * c] = x[nn, sd, sh, sw]
        assert torch.equal(y, want)
        assert f == (2, 1, 1) or not torch.equal(y, wrong)
        poison = torch.full(x.shape, G.POISON16, dtype=I16)
        assert torch.equal(G.depth_to_space(y, dims, f, poison), x)                    # the round trip; every space position written


# ----------------------------------------------------------------------------------------------------------------- resampling
def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def ndhwc(t):
    return t.permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("name", [k for k in G.UP_ROWS if not k.startswith("wrap")])
def test_upsample(name):
    n, (d, h, w), c, f = G.UP_ROWS[name]
    g = G.gen("up" + name)
    bits = G.special_bf16_bits(g, (n, d, h, w, c))
    x = bits.to(F64)
    assert torch.equal(G.upsample_fwd(x, f), ndhwc(F.interpolate(ncdhw(x), scale_factor=tuple(float(k) for k in f), mode="nearest")))
    dy = G.finite_bf16(g, (n, d * f[0], h * f[1], w * f[2], c))
    ref, bound = G.upsample_bwd(dy, f)
    xx = torch.zeros(n, c, d, h, w, dtype=F64, requires_grad=True)
    F.interpolate(xx, scale_factor=tuple(float(k) for k in f), mode="nearest").backward(ncdhw(dy))
    assert torch.allclose(ref, ndhwc(xx.grad), rtol=1e-14, atol=1e-14)
    t = r32(dy).reshape(n, d, f[0], h, f[1], w, f[2], c)
    acc = torch.zeros(n, d, h, w, c)
    for a in range(f[0]):
        for b in range(f[1]):
            for e in range(f[2]):
                acc = acc + t[:, :, a, :, b, :, e]
    inside(to_bf(acc), ref, bound)
    outside(G.bf_trunc(acc), ref, bound)                                              # truncation instead of RNE
    outside(to_bf(acc - t[:, :, -1, :, -1, :, -1]), ref, bound)                        # one replica dropped


def _pool_emul(x, k, s, shift=0):
    dims = x.shape[1:4]
    o = G.pool_out(dims, k, s)
    acc = torch.zeros((x.shape[0],) + o + (x.shape[-1],))
    xs = torch.roll(r32(x), shifts=-shift, dims=3) if shift else r32(x)
    for sl in G._windows(dims, k, s):
        acc = acc + xs[(slice(None),) + sl]
    return acc * (torch.tensor(1.0) / torch.tensor(float(math.prod(k))))


@pytest.mark.parametrize("name", [k for k in G.POOL_ROWS if k != "wrap"])
def test_avgpool(name):
    n, dims, c, k, s = G.POOL_ROWS[name]
    g = G.gen("pool" + name)
    x = G.finite_bf16(g, (n,) + tuple(dims) + (c,))
    ref, bound = G.avgpool_fwd(x, k, s)
    xx = ncdhw(x).clone().requires_grad_(True)
    y = F.avg_pool3d(xx, k, s)
    assert torch.allclose(ref, ndhwc(y), rtol=1e-14, atol=1e-14)
    dy = G.finite_bf16(g, tuple(ref.shape))
    y.backward(ncdhw(dy))
    refb, boundb = G.avgpool_bwd(dy, dims, k, s)
    assert torch.allclose(refb, ndhwc(xx.grad), rtol=1e-14, atol=1e-14)
    inside(to_bf(_pool_emul(x, k, s)), ref, bound)
    outside(to_bf(_pool_emul(x, k, s, shift=1)), ref, bound)                           # a window start off by one along W
    outside(G.bf_trunc(_pool_emul(x, k, s)), ref, bound)                              # truncation instead of RNE
    # backward, gather form in fp32; wrong: the gaps keep stale bytes (poison) / the window count off by one
    acc = torch.zeros(refb.shape)
    for sl in G._windows(dims, k, s):
        acc[(slice(None),) + sl] += r32(dy)
    emul = to_bf(acc * (torch.tensor(1.0) / torch.tensor(float(math.prod(k)))))
    inside(emul, refb, boundb)
    outside(to_bf(acc * (torch.tensor(1.0) / torch.tensor(float(math.prod(k) + 1)))), refb, boundb)
    if name.startswith("gaps"):
        stale = emul.clone()
        stale[refb == 0] = 1e-3
        assert bool((boundb == 0).any())
        outside(stale, refb, boundb)


# ----------------------------------------------------------------------------------------------------------------- model boundary
@pytest.mark.parametrize("name", [k for k in G.QS_ROWS if k != "wrap"])
def test_qsample(name):
    n, c, cc, v, vel, dr = G.QS_ROWS[name]
    g = G.gen("qs" + name)
    x0, noise = G.gauss(g, (n, c, v), round_bf16=False), G.gauss(g, (n, c, v), round_bf16=False)
    cond = G.gauss(g, (n, cc, v), round_bf16=False) if cc else None
    t = torch.tensor(([-5, 1003, 517] if vel else [0, 999, 517])[:n], dtype=I64)
    drop = torch.tensor([1, 0, 1][:n], dtype=torch.uint8) if dr else None
    sa, sb = G.schedule(1000)
    r = G.qsample(x0, noise, sa, sb, t, cond, drop)
    tn = torch.tensor([min(max(int(i), 0), 999) for i in t])
    for i in range(n):                                                                 # the closed form, sample by sample
        xt = sa[tn[i]] * x0[i] + sb[tn[i]] * noise[i]
        assert torch.equal(r["out"][i, :, :c], xt.t())
        assert torch.equal(r["vel"][i], sa[tn[i]] * noise[i] - sb[tn[i]] * x0[i])
        if cc:
            assert torch.equal(r["out"][i, :, c:], (cond[i] * (0.0 if dr and drop[i] else 1.0)).t())

    def emul(tt):
        a, b = r32(sa)[tt][:, None, None], r32(sb)[tt][:, None, None]
        return G.to_ndhwc(a * r32(x0) + b * r32(noise)), a * r32(noise) - b * r32(x0)
    o, ve = emul(tn)
    inside(to_bf(o), r["out"][..., :c], r["b_out"][..., :c])
    inside(ve, r["vel"], r["b_vel"])
    outside(G.bf_trunc(o), r["out"][..., :c], r["b_out"][..., :c])
    if vel:
        o2, _ = emul(t % 1000)                                                         # no clamp: the index wraps instead
        outside(to_bf(o2), r["out"][..., :c], r["b_out"][..., :c])
    if cc:
        assert bool((r["b_out"][..., c:] == 0).all())


@pytest.mark.parametrize("name", list(G.LOSS_ROWS))
def test_mse_l1(name):
    n, c, v = G.LOSS_ROWS[name]
    pred, target = G.loss_inputs(name, n, c, v)
    tg = target.permute(0, 2, 1)
    numel = pred.numel()
    for gs in (1.0, 0.5):
        r = G.mse(pred, target, gs)
        pp = pred.clone().requires_grad_(True)
        loss = F.mse_loss(pp, tg)
        (loss * gs).backward()
        assert abs(float(loss.detach()) - r["loss"]) <= 1e-13 * r["loss"] and torch.allclose(pp.grad, r["dpred"], rtol=1e-13, atol=0)
        d = r32(pred) - r32(tg)
        inv = torch.tensor(1.0) / torch.tensor(float(numel))
        gsf = torch.tensor(2.0) * inv * torch.tensor(gs)
        inside(to_bf(d * gsf), r["dpred"], r["b_dpred"])
        inside((d * d).sum() * inv, r["loss"], r["b_loss"])
        outside(G.bf_trunc(d * gsf), r["dpred"], r["b_dpred"])
        if c > 1:                                                                      # 1 / numel taken over N V instead of N V C
            inv_w = torch.tensor(1.0) / torch.tensor(float(numel // c))
            outside(to_bf(d * (torch.tensor(2.0) * inv_w * torch.tensor(gs))), r["dpred"], r["b_dpred"])
            outside((d * d).sum() * inv_w, r["loss"], r["b_loss"])
        outside((d * d).reshape(-1)[:-1].sum() * inv, r["loss"], r["b_loss"]) if numel < 4096 else None      # the last element dropped
    for loss0 in (0.0, 3.25):
        r = G.l1(pred, target, loss0)
        pp = pred.clone().requires_grad_(True)
        loss = F.l1_loss(pp, tg)
        loss.backward()
        assert abs(float(loss.detach()) + loss0 - r["loss"]) <= 1e-13 * r["loss"] and torch.equal(pp.grad, r["dpred"])
        d = r32(pred) - r32(tg)
        inv = torch.tensor(1.0) / torch.tensor(float(numel))
        z = torch.zeros_like(d)
        inside(to_bf(torch.where(d > 0, inv, torch.where(d < 0, -inv, z))), r["dpred"], r["b_dpred"])
        inside(torch.tensor(loss0) + d.abs().sum() * inv, r["loss"], r["b_loss"])
        assert int((d == 0).sum()) >= numel // 7
        outside(to_bf(torch.where(d >= 0, inv, -inv)), r["dpred"], r["b_dpred"])       # sign of a zero difference = +1
        outside(d.abs().sum() * inv, r["loss"], r["b_loss"]) if loss0 else None        # accumulate = 1 that overwrote the prefill


@pytest.mark.parametrize("name", list(G.KL_ROWS))
def test_reparam_kl(name):
    n, c, v = G.KL_ROWS[name]
    mu, sigma, eps, dz = G.kl_inputs(name, n, c, v)
    assert len(set(sigma.reshape(-1).tolist())) == len(G.SIGMAS)
    e = eps.permute(0, 2, 1)
    for klw in (G.f32s(1.0), G.f32s(1e-6)):
        r, rb = G.reparam_fwd(mu, sigma, eps, klw, 0.75), G.reparam_bwd(mu, sigma, eps, dz, klw)
        m, s = mu.clone().requires_grad_(True), sigma.clone().requires_grad_(True)
        z = m + e * s
        kl = 0.5 * (m.pow(2) + s.pow(2) - torch.log(s.pow(2)) - 1).reshape(n, -1).sum(dim=1)
        loss = klw * kl.sum() / n
        ((z * dz).sum() + loss).backward()
        assert torch.equal(z.detach(), r["z"]) and abs(float(loss.detach()) + 0.75 - r["loss"]) <= 1e-12 * abs(r["loss"])
        assert torch.allclose(m.grad, rb["dmu"], rtol=1e-12, atol=0) and torch.allclose(s.grad, rb["dsigma"], rtol=1e-12, atol=1e-300)
        m32, s32, e32, g32 = r32(mu), r32(sigma), r32(e), r32(dz)
        k32 = torch.tensor(klw, dtype=F32) / torch.tensor(float(n))
        inside(to_bf(m32 + e32 * s32), r["z"], r["b_z"])
        term = 0.5 * (m32 * m32 + s32 * s32 - torch.log(s32 * s32) - 1.0)
        inside(torch.tensor(0.75) + term.sum() * k32, r["loss"], r["b_loss"])
        outside(torch.tensor(0.75) + term.sum() * (torch.tensor(klw, dtype=F32) / torch.tensor(float(n * v))), r["loss"], r["b_loss"])   # KL / (N V)
        inside(to_bf(g32 + k32 * m32), rb["dmu"], rb["b_dmu"])
        inside(to_bf(g32 * e32 + k32 * (s32 - 1.0 / s32)), rb["dsigma"], rb["b_dsigma"])
        outside(G.bf_trunc(m32 + e32 * s32), r["z"], r["b_z"])
        outside(to_bf(g32 * e32 + k32 * (s32 + 1.0 / s32)), rb["dsigma"], rb["b_dsigma"]) if klw == 1.0 else None                       # a sign


@pytest.mark.parametrize("n", [8, 1000])
def test_logvar_to_sigma(n):
    g = G.gen(f"logvar{n}")
    lv = G.logvar_inputs(g, n)
    ref, bound = G.logvar_fwd(lv)
    sigma, ds = G.bf(ref), G.finite_bf16(g, (n,))
    ds[:8] = 1.5
    refb, boundb = G.logvar_bwd(ds, lv, sigma)
    x = lv.clone().requires_grad_(True)
    y = torch.exp(torch.clamp(x, -30.0, 20.0) / 2)
    assert torch.equal(y.detach(), ref)
    # the backward of the kernel uses the ROUNDED sigma; autograd with that sigma substituted: d/dlv = 0.5 sigma inside the closed interval
    (torch.clamp(x, -30.0, 20.0) * 0.5 * ds * sigma).sum().backward()
    assert torch.equal(x.grad, refb) and x.grad[1] != 0 and x.grad[5] != 0 and x.grad[0] == 0 and x.grad[6] == 0
    v32 = torch.clamp(r32(lv), -30.0, 20.0)
    inside(to_bf(torch.exp(0.5 * v32)), ref, bound)
    outside(G.bf_trunc(torch.exp(0.5 * v32)), ref, bound)
    outside(to_bf(torch.exp(0.5 * r32(lv).clamp(-29.0, 20.0))), ref, bound)             # a clamp edge moved
    pas = (r32(lv) >= -30) & (r32(lv) <= 20)
    inside(to_bf(torch.where(pas, 0.5 * r32(ds) * r32(sigma), torch.zeros(n))), refb, boundb)
    blocked = (r32(lv) >= -30) & (r32(lv) < 20)                                        # the gradient blocked at logvar = 20
    outside(to_bf(torch.where(blocked, 0.5 * r32(ds) * r32(sigma), torch.zeros(n))), refb, boundb)


@pytest.mark.parametrize("dim", [7, 256, 257])
@pytest.mark.parametrize("b", [1, 5])
def test_embedding(b, dim):
    g = G.gen(f"emb{b}_{dim}")
    labels = torch.tensor([0, 5, 2, 5, 0][:b] if b > 1 else [5 if dim == 256 else 0], dtype=I64)
    emb, w = G.gauss(g, (b, dim), round_bf16=False), G.gauss(g, (6, dim), round_bf16=False)
    ref, bound = G.embedding_add(emb, w, labels)
    ww = w.clone().requires_grad_(True)
    y = emb + F.embedding(labels, ww)
    assert torch.equal(y.detach(), ref)
    d_emb, dw0 = G.gauss(g, (b, dim), round_bf16=False), G.gauss(g, (6, dim), round_bf16=False)
    y.backward(d_emb)
    refb, boundb, named = G.embedding_bwd(d_emb, labels, dw0)
    assert torch.allclose(refb, dw0 + ww.grad, rtol=1e-15, atol=1e-15) and sorted(named.nonzero().reshape(-1).tolist()) == sorted(set(labels.tolist()))
    assert bool((boundb[~named] == 0).all())
    inside(r32(emb) + r32(w)[labels], ref, bound)
    outside(r32(emb) + r32(w)[(labels + 1) % 6], ref, bound)
    acc = r32(dw0).clone()
    for i in range(b):
        acc[labels[i]] += r32(d_emb)[i]
    inside(acc, refb, boundb)
    lost = r32(dw0).clone()
    lost[labels] += r32(d_emb)                                                         # a plain store: repeated labels lose terms
    outside(lost, refb, boundb) if b > 1 else None
    touched = acc.clone()
    touched[1] += 1e-6                                                                 # a row no label names
    outside(touched, refb, boundb)


def test_select_labels_and_cast_drop():
    g = G.gen("sel")
    labels = torch.randint(0, 6, (300,), generator=g)
    drop = (torch.arange(300) % 3 == 0).to(torch.uint8)
    want = G.select_labels(labels, drop, 6)
    assert all(int(want[i]) == (6 if drop[i] else int(labels[i])) for i in range(300))
    assert not torch.equal(G.select_labels(labels, 1 - drop, 6), want)
    x = G.cast_inputs(g, 300 * 77).view(300, 77)
    bits = G.cast_drop(x, drop)
    assert bool((bits[drop != 0] == 0).all()) and torch.equal(bits[drop == 0], x[drop == 0].to(F32).bfloat16().view(I16))
    assert not torch.equal(G.cast_drop(x, 1 - drop), bits)


# ----------------------------------------------------------------------------------------------------------------- small fp32 vectors
@pytest.mark.parametrize("tv,dim", G.TE_ROWS)
def test_timestep_embedding(tv, dim, monkeypatch):
    from oracle.nets import timestep_embedding as oracle_te
    t = torch.tensor(tv, dtype=I64)
    ref, bound = G.timestep_embedding(t, dim)
    if dim > 1:
        with monkeypatch.context() as mp:              # the oracle names fp32 in its body: run the same statements in fp64
            mp.setattr(torch, "float32", torch.float64)
            mp.setattr(torch.Tensor, "float", torch.Tensor.double)
            want = oracle_te(t, dim)
        assert want.dtype == F64 and torch.allclose(ref, want, rtol=0, atol=1e-12)
    if dim % 2:
        assert bool((ref[:, -1] == 0).all()) and bool((bound[:, -1] == 0).all())
    half = dim // 2
    nlp = -torch.log(torch.tensor(10000.0))                                             # fp32, as -logf on the host

    def emul(swap=False, all_f32=False):
        k = torch.arange(half, dtype=F32)
        if all_f32:
            freq = torch.exp(nlp * k / half)
        else:
            freq = torch.exp((nlp * k).to(F64) / half).to(F32)
        arg = r32(t)[:, None] * freq
        a, b = (torch.sin(arg), torch.cos(arg)) if swap else (torch.cos(arg), torch.sin(arg))
        return torch.cat([a, b, torch.zeros(len(tv), dim - 2 * half)], -1)
    inside(emul(), ref, bound)
    if half:
        outside(emul(swap=True), ref, bound)                                           # the sine half first
        shifted = emul().clone()
        shifted[-1, :half] = torch.cos(torch.tensor(998.0) * torch.exp((nlp * torch.arange(half)).to(F64) / half).to(F32))
        outside(shifted, ref, bound)                                                   # t off by one in one row
    assert float(bound.max()) < 2e-4                                                   # far below the 1e-2 steps of a bf16 consumer


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_silu(n):
    g = G.gen(f"silu{n}")
    x = G.f32((torch.rand(n, generator=g, dtype=F64) * 2 - 1) * 40)
    x[:min(n, 5)] = torch.tensor([40.0, -40.0, 0.0, -1.278, 1e-3], dtype=F32).to(F64)[:min(n, 5)]
    dy = G.gauss(g, (n,), round_bf16=False)
    ref, bound = G.silu(x)
    refb, boundb = G.silu_bwd(x, dy)
    xx = x.clone().requires_grad_(True)
    y = F.silu(xx)
    y.backward(dy)
    assert torch.allclose(y.detach(), ref, rtol=1e-13, atol=1e-300) and torch.allclose(xx.grad, refb, rtol=1e-12, atol=1e-300)
    x32 = r32(x)
    s = 1.0 / (1.0 + torch.exp(-x32))
    inside(x32 * s, ref, bound)
    inside(r32(dy) * (s * (1.0 + x32 * (1.0 - s))), refb, boundb)
    outside(x32 * s * (1 + 2.0 ** -19), ref, bound)                                    # 16 ulp off
    outside(r32(dy) * (s * (1.0 + x32 * (1.0 - s))) * (1 + 2.0 ** -12) + 2.0 ** -14 * r32(dy), refb, boundb)
    assert bool((bound <= 2.0 ** -17 * ref.abs() + 2 * G.TINY).all())                  # relative, also where silu(x) ~ 1e-16


# ----------------------------------------------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("c", G.COLSUM_C8[:3] + G.COLSUM_CR)
def test_colsum(c):
    for i, v in enumerate(G.COLSUM_V):
        n, _, acc = G.colsum_case(c, i, v)
        g = G.gen(f"colsum{c}_{v}")
        x = G.gauss(g, (n, v, c))
        out0 = G.gauss(g, (n, c), sigma=4.0, round_bf16=False) if acc else None
        ref, bound = G.colsum(x, out0)
        want = torch.einsum("nvc,v->nc", x, torch.ones(v, dtype=F64)) + (out0 if acc else 0)
        assert torch.allclose(ref, want, rtol=1e-13, atol=1e-13)
        emul = r32(x).sum(dim=1) + (r32(out0) if acc else 0)
        inside(emul, ref, bound)
        outside(r32(x)[:, :-1].sum(dim=1) + (r32(out0) if acc else 0), ref, bound) if v > 1 else None     # the last voxel dropped
        outside(r32(x).sum(dim=1), ref, bound) if acc else None                                           # the prefill overwritten


def test_colsum_depth_restates_the_launch_rules():
    assert G.colsum_depth(8, 16) == 1 + 4 + 256 + 1 + 1            # rows = 256, one chunk at the floor
    assert G.colsum_depth(2056, 17) == 16 + 4 + 1 + 2 + 1          # 320 threads, rows = 1, two chunks
    assert G.colsum_depth(520, 8195) == 6 + 4 + 3 + 483 + 1        # rows = 256 // 65 = 3, vchunk = 17
    assert G.colsum_depth(63, 8195) == 32 + 9 + 2 + 1              # two 8192-voxel chunks of the ragged kernel


@pytest.mark.parametrize("rows,cols", G.F32_2D)
def test_f32_2d(rows, cols):
    g = G.gen(f"f32_2d{rows}_{cols}")
    x, y0, row = (G.gauss(g, s, round_bf16=False) for s in ((rows, cols), (rows, cols), (1, cols)))
    ref = G.f32(y0 + x) + row
    inside((r32(y0) + r32(x)) + r32(row), ref, G.U * ref.abs())
    outside((r32(y0) + r32(x)) + r32(row).roll(1, 1), ref, G.U * ref.abs()) if cols > 1 else None
    for acc in (0, 1):
        o0 = G.gauss(g, (1, cols), sigma=3.0, round_bf16=False) if acc else None
        ref, bound = G.sum_rows(x, o0[0] if acc else None)
        assert torch.allclose(ref, torch.ones(rows, dtype=F64) @ x + (o0[0] if acc else 0), rtol=1e-14, atol=1e-14)
        s = r32(o0[0]).clone() if acc else torch.zeros(cols)
        for r in range(rows):
            s = s + r32(x)[r]
        inside(s, ref, bound)
        outside(s - r32(x)[rows - 1], ref, bound)                                      # the last row dropped


@pytest.mark.parametrize("n", G.VEC_N)
def test_sumsq_scale_axpy(n):
    x = G.vec_inputs(f"sumsq{n}", n)
    for o0 in (0.0, 2.5):
        ref, bound = G.sumsq(x, o0)
        assert abs(ref - o0 - float(torch.dot(x, x))) <= 1e-13 * ref
        inside(torch.tensor(o0) + (r32(x) * r32(x)).sum(), ref, bound)
        outside(torch.tensor(o0) + (r32(x) * r32(x))[:-1].sum(), ref, bound)           # one element of the tail dropped
    g = G.gen(f"vec{n}")
    x, y = G.gauss(g, (n,), round_bf16=False), G.gauss(g, (n,), round_bf16=False)
    al = G.f32s(0.18215)
    inside(r32(y) * torch.tensor(al, dtype=F32), y * al, G.U * (y * al).abs())
    ref, bound = G.axpy(y, x, -al)
    inside(r32(y) + torch.tensor(-al, dtype=F32) * r32(x), ref, bound)
    wrong = r32(y) + torch.tensor(-al, dtype=F32) * r32(x)
    wrong[-1] = r32(y)[-1]                                                             # the last element of the tail left as it was
    outside(wrong, ref, bound)


# ----------------------------------------------------------------------------------------------------------------- Adam
def _adam_emul(p, g, m, v, t, hp, dec, ssq, max_norm, gs, t_bias=None):
    f = lambda x: torch.tensor(x, dtype=F32)  # noqa: E731
    lr, b1, b2, eps, wd = (f(hp[k]) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    tb = f(float(t if t_bias is None else t_bias))
    bc1, bc2 = 1.0 - torch.pow(b1, tb), 1.0 - torch.pow(b2, tb)
    step, isb = lr / bc1, torch.rsqrt(bc2)
    clip = f(gs)
    if ssq is not None:
        c = f(max_norm) / (f(gs) * torch.sqrt(f(ssq)) + f(1e-6))
        clip = torch.minimum(c, f(1.0)) * f(gs)
    p, g, m, v = r32(p), r32(g) * clip, r32(m), r32(v)
    if dec:
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - step * m / (torch.sqrt(v) * isb + eps)
    return p, m, v


@pytest.mark.parametrize("name", [k for k in G.ADAM_ROWS if "n10007" in k])
def test_adam(name):
    dec, t0, clip, gs, n = G.ADAM_ROWS[name]
    s, hp = G.adam_inputs(name, n), G.ADAM_HP
    hp32 = {k: G.f32s(x) for k, x in hp.items()}
    p, m, v = s["p"], s["m"], s["v"]
    # torch.optim in fp64 from the same state, three steps, against the chained fp64 recurrence
    tp = p.clone().requires_grad_(True)
    opt = (torch.optim.AdamW if dec else torch.optim.Adam)([tp], lr=hp32["lr"], betas=(hp32["beta1"], hp32["beta2"]), eps=hp32["eps"], weight_decay=hp32["wd"])
    opt.state[tp] = dict(step=torch.tensor(float(t0)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    pe, me, ve = p, m, v
    for i, grad in enumerate(s["grads"]):
        ssq = G.f32s(float((grad * grad).sum())) if clip is not None else None
        max_norm = 0.5 * gs * math.sqrt(ssq) if clip else 1e9
        r = G.adam_step(p, grad, m, v, t0 + i + 1, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], dec, ssq, max_norm, gs)
        tp.grad = grad * G.f32s(gs)
        if clip is not None:                           # torch takes the norm in fp64, the kernel is handed the fp32 sum of squares: 1e-7 apart
            norm = torch.nn.utils.clip_grad_norm_([tp], G.f32s(max_norm))
            assert abs(float(norm) - G.f32s(gs) * math.sqrt(ssq)) <= 1e-6 * float(norm)
            assert bool(float(norm) > G.f32s(max_norm)) == bool(clip)
        before = tp.detach().clone()
        opt.step()
        st = opt.state[tp]
        # with a clip the 1e-7 of the norm moves every term of m by 1e-7 of |g|, which is absolute where m cancels (updates are ~1e-3)
        rt, at = (1e-12, 1e-5) if clip is None else (1e-6, 1.0)
        assert torch.allclose(r["p"] - p, tp.detach() - before, rtol=rt, atol=1e-9 * at) and torch.allclose(r["m"], st["exp_avg"], rtol=rt, atol=1e-10 * at)
        assert torch.allclose(r["v"], st["exp_avg_sq"], rtol=rt, atol=1e-12 * at)
        # the fp32 emulation from the same state: inside; the bias correction taken at t - 1: outside
        ep, em, ev = _adam_emul(p, grad, m, v, t0 + i + 1, hp, dec, ssq, max_norm, gs)
        inside(ep, r["p"], r["b_p"]), inside(em, r["m"], r["b_m"]), inside(ev, r["v"], r["b_v"])
        wp, _, _ = _adam_emul(p, grad, m, v, t0 + i + 1, hp, dec, ssq, max_norm, gs, t_bias=t0 + i)
        outside(wp, r["p"], r["b_p"])
        outside(em * (1 + 2.0 ** -20), r["m"], r["b_m"]), outside(ev * (1 + 2.0 ** -19), r["v"], r["b_v"])
        assert float((r["b_p"] / ((r["p"] - p).abs() + 1e-30)).median()) < 1e-3
        p, m, v = ep.to(F64), em.to(F64), ev.to(F64)       # as on the GPU: the next step starts from the fp32 state the last one left
        with torch.no_grad():
            tp.copy_(p), st["exp_avg"].copy_(m), st["exp_avg_sq"].copy_(v)
