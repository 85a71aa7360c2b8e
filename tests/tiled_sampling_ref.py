"""fp64 restatement of tiled (sliding-window) diffusion sampling (MultiDiffusion, Bar-Tal et al. 2023; not part of the reference: PARITY
UNPINNED), over any callable model.  TEST INFRASTRUCTURE: written from the text below, on tests/sliding_ref.py (windows, importance
map, blend and its bound); it does not import the product.

Given the sample x [N, C, *S], an optional concat condition cond [N, Cc, *S], the windows o_k and extent roi of the window plan of
(S, roi_size, overlap), the importance map imp rounded to fp32, the model f and a step at timestep t:

    p_k      = f(cat(x[n, :, o_k : o_k+roi], cond[n, :, o_k : o_k+roi]), t, n, null)
    guided:    p_k = p_k(null) + w * (p_k(condition) - p_k(null))        per window, before the blend
    acc[n,c,v] = sum_k imp[v-o_k] * p_k[c, v-o_k];   wsum[v] = sum_k imp[v-o_k];   m = acc / wsum
    x <- update(i, t, x, m, z_i)

There is no padding: a case smaller than roi on any axis is a ValueError.  The model is called as f(inp, t, n, null) with inp fp32
[1, C + Cc, *roi], n the image the window belongs to (its label / context) and null True for the unconditional branch (whose condition
channels are zero); it returns [1, C, *roi].  x is carried in fp64 and handed to the model as fp32."""
import torch

from tests import guidance_ref
from tests import sliding_ref as R


def windows(spatial, roi_size, overlap):
    """(roi, windows in enumeration order) of a case of extent `spatial`; ValueError when the case is smaller than the window."""
    spatial = tuple(int(s) for s in spatial)
    roi = (roi_size,) * len(spatial) if isinstance(roi_size, int) else tuple(roi_size)
    roi = tuple(r if r > 0 else s for r, s in zip(roi, spatial))
    if any(s < r for s, r in zip(spatial, roi)):
        raise ValueError(f"case {spatial} is smaller than the window {roi}")
    _, _, wins = R.window_starts(spatial, roi, overlap)
    return roi, wins


def blended_prediction(x, f, t, roi_size, overlap, mode="constant", sigma_scale=0.125, cond=None, w=None):
    """(m, bound), both fp64 [N, C, *S]: the blended model output of one step and the fp32 error bound of the blend
    (sliding_ref.blend: (2 K + 4) 2^-24 sum_k w_k |p_k| / sum_k w_k)."""
    n_images, c, sp = x.shape[0], x.shape[1], tuple(x.shape[2:])
    roi, wins = windows(sp, roi_size, overlap)
    imp = R.importance(roi, mode, sigma_scale).float().double()  # the fp32-rounded map, as the product uses
    preds = []
    for n in range(n_images):
        for o in wins:
            sl = (slice(n, n + 1), slice(None)) + tuple(slice(a, a + r) for a, r in zip(o, roi))
            tile = x[sl].float()

            def run(null):
                inp = tile
                if cond is not None:
                    inp = torch.cat([tile, torch.zeros_like(cond[sl]).float() if null else cond[sl].float()], dim=1)
                return f(inp, t, n, null)[0]

            p = run(False)
            if w is not None:
                p = guidance_ref.combine(p, run(True), w)
            preds.append(p.double())
    return R.blend(preds, imp, wins, n_images, c, sp, (0,) * len(sp), sp)


def sample(x, f, timesteps, update, roi_size, overlap, mode="constant", sigma_scale=0.125, cond=None, w=None, noises=None):
    """The loop: update(i, t, x fp64, m fp64, z or None) -> the next x (fp64).  Returns the final sample, fp64."""
    x = x.double()
    for i, t in enumerate(timesteps):
        m, _ = blended_prediction(x, f, t, roi_size, overlap, mode, sigma_scale, cond, w)
        x = update(i, t, x, m, None if noises is None else noises[i]).double()
    return x
