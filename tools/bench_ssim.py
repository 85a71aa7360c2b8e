"""Time metrics.pairwise (SSIM / MS-SSIM of every sample pair, train_ldm.py:315-321) against the per-pair torch fp32 loop on the same GPU.

Cases: the reference's 3-D setting (40 x 1x128^3, kernel_size=4, 780 pairs, MS-SSIM and SSIM), the 2-D setting (100 x 1x256^2,
4,950 pairs, MS-SSIM and SSIM) and the 3-D setting with the default kernel_size=11 (SSIM only: MS-SSIM's size rule needs extents
> 16 * (11 - 1) = 160).

Per case: milliseconds of one pairwise() call (pyramids included), the implied GB/s (each pair reads both images at every scale once:
the minimum traffic) and fp32 TFLOP/s (separable work: per output voxel and scale, 3 products, 5 moments x 2 flops x (kD + kH + kW)
taps, ~20 for ssim / cs), and the torch loop (grouped F.conv2d / F.conv3d with the full kernel, F.avg_pool, one pair per call, as
upstream computes it), timed on a subset of pairs and scaled to all of them.

    python tools/bench_ssim.py [--reps 5] [--torch-pairs 10]
"""
import argparse
import itertools
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medical_image_generation_amd import metrics as M  # noqa: E402


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    out.sort()
    return out[len(out) // 2]


def _torch_pair(x, y, sd, ker, weights, want_ms):
    """Upstream's arithmetic in fp32: grouped conv with the full kernel, one pair."""
    conv = F.conv3d if sd == 3 else F.conv2d
    pool = F.avg_pool3d if sd == 3 else F.avg_pool2d
    w = ker[None, None]
    c1, c2 = 0.01 ** 2, 0.03 ** 2

    def ssim_cs(a, b):
        mx, my = conv(a, w), conv(b, w)
        sx, sy, sxy = conv(a * a, w) - mx * mx, conv(b * b, w) - my * my, conv(a * b, w) - mx * my
        cs = (2 * sxy + c2) / (sx + sy + c2)
        return ((2 * mx * my + c1) / (mx * mx + my * my + c1)) * cs, cs

    s, _ = ssim_cs(x, y)
    out = [s.flatten(1).mean(1)]
    if want_ms:
        ms = []
        a, b = x, y
        for _ in weights:
            s, cs = ssim_cs(a, b)
            ms.append(torch.relu(cs.flatten(1).mean(1)))
            a, b = pool(a, 2), pool(b, 2)
        ms[-1] = torch.relu(s.flatten(1).mean(1))
        out.append(torch.prod(torch.stack(ms) ** torch.tensor(weights, device=x.device).view(-1, 1), 0))
    return out


def case(name, n, sp, k, want_ms, reps, torch_pairs):
    sd = len(sp)
    g = torch.Generator(device="cuda").manual_seed(0)
    imgs = torch.rand((n, 1) + sp, generator=g, device="cuda")
    metrics = [M.SSIMMetric(sd, data_range=1.0, kernel_size=k)]
    if want_ms:
        metrics.insert(0, M.MultiScaleSSIMMetric(sd, data_range=1.0, kernel_size=k))
    pairs = list(itertools.combinations(range(n), 2))
    P = len(pairs)
    ms = _timed(lambda: M.pairwise(imgs, *metrics), reps)

    levels = len(M.MS_SSIM_WEIGHTS) if want_ms else 1
    byts, flops = 0, 0
    ks = (k,) * sd
    for s in range(levels):
        e = [v >> s for v in sp]
        vox_in, vox_out = 1, 1
        for v, kk in zip(e, ks):
            vox_in *= v
            vox_out *= v - kk + 1
        byts += 2 * 4 * vox_in
        flops += vox_in * 3 + vox_out * (10 * sum(ks) + 20)  # (the W / H passes also run on halo rows: a lower bound)
    byts *= P
    flops *= P

    taps = [torch.tensor(t, device="cuda", dtype=torch.float32) for t in metrics[0].taps()]
    ker = taps[0]
    for t in taps[1:]:
        ker = ker[..., None] * t
    sub = pairs[:torch_pairs]
    fn = lambda: [_torch_pair(imgs[[a]], imgs[[b]], sd, ker, M.MS_SSIM_WEIGHTS, want_ms) for a, b in sub]
    t_sub = _timed(fn, max(1, reps // 2))
    t_torch = t_sub * P / len(sub)
    res = dict(case=name, images=n, shape=list(sp), kernel_size=k, pairs=P, metrics="MS-SSIM+SSIM" if want_ms else "SSIM",
               ms=round(ms, 3), GBps=round(byts / ms / 1e6, 1), TFLOPs=round(flops / ms / 1e9, 2),
               torch_loop_ms=round(t_torch, 1), torch_pairs_timed=len(sub), speedup=round(t_torch / ms, 1))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-pairs", type=int, default=10)
    a = ap.parse_args()
    t0 = time.time()
    case("3-D reference (k=4)", 40, (128, 128, 128), 4, True, a.reps, a.torch_pairs)
    case("2-D reference (k=4)", 100, (256, 256), 4, True, a.reps, a.torch_pairs)
    case("3-D default kernel (k=11)", 40, (128, 128, 128), 11, False, a.reps, a.torch_pairs)
    print(f"total {time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main()
