// Memory-bound helpers of the train step: layout changes at the model boundary, nearest up-sampling,
// space<->depth rearrangements (strided convs), channel-range copies (skip concat), q-sample, MSE,
// timestep embedding, column sums.  All HBM-bound: 16-byte accesses, grid-stride, no LDS except reductions.
#include "common.h"
#include "diffusion_update.h"
#include "medimgen_hip.h"

namespace {

constexpr int kThreads = 256;
inline int grid_for(int64_t work, int cap = 256 * 16) {
  int64_t g = (work + kThreads - 1) / kThreads;
  if (g < 1) g = 1;
  return (int)(g > cap ? cap : g);
}

// ---------------------------------------------------------------- NCDHW fp32 <-> NDHWC bf16
__global__ void k_ncdhw_to_ndhwc(const float* __restrict__ src, bf16* __restrict__ dst, int C, int64_t V, int64_t total) {
  // one thread per (n, v): strided-by-V reads are coalesced across the wave, writes are 2C contiguous bytes
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t n = i / V, v = i - n * V;
    const float* s = src + n * C * V + v;
    bf16* d = dst + i * C;
    for (int c = 0; c < C; ++c) d[c] = f2bf(s[(int64_t)c * V]);
  }
}
__global__ void k_ndhwc_to_ncdhw(const bf16* __restrict__ src, float* __restrict__ dst, int C, int64_t V, int64_t total) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t n = i / V, v = i - n * V;
    const bf16* s = src + i * C;
    float* d = dst + n * C * V + v;
    for (int c = 0; c < C; ++c) d[(int64_t)c * V] = bf2f(s[c]);
  }
}

// ---------------------------------------------------------------- flat elementwise (8 bf16 per thread-step)
__global__ void k_add_bf16(const u32x4* __restrict__ a, const u32x4* __restrict__ b, u32x4* __restrict__ o, int64_t n8) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    F8 x = unpack8(a[i]), y = unpack8(b[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) x.v[j] += y.v[j];
    o[i] = pack8(x);
  }
}
__global__ void k_add_bf16_tail(const bf16* a, const bf16* b, bf16* o, int64_t start, int64_t n) {
  int64_t i = start + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) o[i] = f2bf(bf2f(a[i]) + bf2f(b[i]));
}
__global__ void k_cast_f32_bf16(const float* __restrict__ s, bf16* __restrict__ d, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = f2bf(s[i]);
}

// ---------------------------------------------------------------- channel-range copy (concat / split)
// dst[v][c0d + c] = src[v][c0s + c], c in [0, nC); nC, Cs, Cd, c0s, c0d all multiples of 8
__global__ void k_copy_channels(const bf16* __restrict__ src, int Cs, int c0s, bf16* __restrict__ dst, int Cd, int c0d,
                                int nC8, int64_t total) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t v = i / nC8;
    int c = (int)(i - v * nC8) * 8;
    *(u32x4*)(dst + v * Cd + c0d + c) = *(const u32x4*)(src + v * Cs + c0s + c);
  }
}

// ---------------------------------------------------------------- nearest up-sampling (integer factors per axis)
// fwd: y[n, d, h, w, :] = x[n, d/fd, h/fh, w/fw, :]
__global__ void k_upsample_fwd(const bf16* __restrict__ x, bf16* __restrict__ y, int D, int H, int W, int C8, int fd, int fh,
                               int fw, int64_t total) {
  int Do = D * fd, Ho = H * fh, Wo = W * fw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int c = (int)(i % C8);
    int64_t t = i / C8;
    int w = (int)(t % Wo); t /= Wo;
    int h = (int)(t % Ho); t /= Ho;
    int d = (int)(t % Do);
    int64_t n = t / Do;
    int64_t src = (((n * D + d / fd) * H + h / fh) * W + w / fw) * C8 + c;
    ((u32x4*)y)[i] = ((const u32x4*)x)[src];
  }
}
// bwd: dx[n, d, h, w, :] = sum over the fd*fh*fw replicas (fp32 accumulate)
__global__ void k_upsample_bwd(const bf16* __restrict__ dy, bf16* __restrict__ dx, int D, int H, int W, int C8, int fd, int fh,
                               int fw, int64_t total) {
  int Ho = H * fh, Wo = W * fw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int c = (int)(i % C8);
    int64_t t = i / C8;
    int w = (int)(t % W); t /= W;
    int h = (int)(t % H); t /= H;
    int d = (int)(t % D);
    int64_t n = t / D;
    F8 acc;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc.v[j] = 0.f;
    for (int a = 0; a < fd; ++a)
      for (int b = 0; b < fh; ++b)
        for (int e = 0; e < fw; ++e) {
          int64_t src = (((n * D * fd + d * fd + a) * Ho + h * fh + b) * Wo + w * fw + e) * C8 + c;
          F8 g = unpack8(((const u32x4*)dy)[src]);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc.v[j] += g.v[j];
        }
    ((u32x4*)dx)[i] = pack8(acc);
  }
}

// ---------------------------------------------------------------- average pooling (nn.AvgPool{2,3}d(kernel, stride), no padding, floor mode)
// ResnetBlock(down=True) resamples with Pool[AVG](kernel_size, stride) (UNet:522, 640-644, 679-687).
// fwd: y[n, od, oh, ow, :] = mean over the kd*kh*kw window starting at (od*sd, oh*sh, ow*sw)
__global__ void k_avgpool_fwd(const bf16* __restrict__ x, bf16* __restrict__ y, int D, int H, int W, int C8, int kd, int kh, int kw, int sd,
                              int sh, int sw, int Do, int Ho, int Wo, int64_t total) {
  const float inv = 1.0f / (float)(kd * kh * kw);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int c = (int)(i % C8);
    int64_t t = i / C8;
    int w = (int)(t % Wo); t /= Wo;
    int h = (int)(t % Ho); t /= Ho;
    int d = (int)(t % Do);
    int64_t n = t / Do;
    F8 acc;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc.v[j] = 0.f;
    for (int a = 0; a < kd; ++a)
      for (int b = 0; b < kh; ++b)
        for (int e = 0; e < kw; ++e) {
          int64_t src = (((n * D + d * sd + a) * H + h * sh + b) * W + w * sw + e) * C8 + c;
          F8 g = unpack8(((const u32x4*)x)[src]);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc.v[j] += g.v[j];
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc.v[j] *= inv;
    ((u32x4*)y)[i] = pack8(acc);
  }
}
// bwd (gather form, windows may overlap or leave gaps): dx[n, d, h, w, :] = sum over the windows that contain (d, h, w) of dy / volume
__global__ void k_avgpool_bwd(const bf16* __restrict__ dy, bf16* __restrict__ dx, int D, int H, int W, int C8, int kd, int kh, int kw, int sd,
                              int sh, int sw, int Do, int Ho, int Wo, int64_t total) {
  const float inv = 1.0f / (float)(kd * kh * kw);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int c = (int)(i % C8);
    int64_t t = i / C8;
    int w = (int)(t % W); t /= W;
    int h = (int)(t % H); t /= H;
    int d = (int)(t % D);
    int64_t n = t / D;
    // outputs o with o*s <= i <= o*s + k - 1
    int d0 = max(0, (d - kd + sd) / sd), d1 = min(Do - 1, d / sd);
    int h0 = max(0, (h - kh + sh) / sh), h1 = min(Ho - 1, h / sh);
    int w0 = max(0, (w - kw + sw) / sw), w1 = min(Wo - 1, w / sw);
    F8 acc;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc.v[j] = 0.f;
    for (int a = d0; a <= d1; ++a)
      for (int b = h0; b <= h1; ++b)
        for (int e = w0; e <= w1; ++e) {
          F8 g = unpack8(((const u32x4*)dy)[(((n * Do + a) * Ho + b) * Wo + e) * C8 + c]);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc.v[j] += g.v[j];
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc.v[j] *= inv;
    ((u32x4*)dx)[i] = pack8(acc);
  }
}

// ---------------------------------------------------------------- space <-> depth (per-axis factor 1 or 2)
// s2d: out[n, d', h', w', q*C + c] = in[n, d'*fd + qd, h'*fh + qh, w'*fw + qw, c], q = (qd*fh + qh)*fw + qw
// (positions beyond the input extent read as zero: odd sizes).  d2s is the inverse scatter.
// scs8: voxel pitch of the SPACE-side tensor in 16-byte units (>= C8: it may be a channel slice of a wider buffer)
__global__ void k_space_depth(const bf16* __restrict__ in, bf16* __restrict__ out, int D, int H, int W, int C8, int fd, int fh,
                              int fw, int Dp, int Hp, int Wp, int to_depth, int64_t total, int scs8) {
  int Q = fd * fh * fw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    // i enumerates the DEPTH-side tensor: [n, Dp, Hp, Wp, Q, C8]
    int c = (int)(i % C8);
    int64_t t = i / C8;
    int q = (int)(t % Q); t /= Q;
    int w = (int)(t % Wp); t /= Wp;
    int h = (int)(t % Hp); t /= Hp;
    int d = (int)(t % Dp);
    int64_t n = t / Dp;
    int qw = q % fw, qh = (q / fw) % fh, qd = q / (fw * fh);
    int sd = d * fd + qd, sh = h * fh + qh, sw = w * fw + qw;
    bool inside = sd < D && sh < H && sw < W;
    int64_t sp = (((n * D + sd) * H + sh) * W + sw) * scs8 + c;
    if (to_depth) {
      u32x4 z = {0u, 0u, 0u, 0u};
      ((u32x4*)out)[i] = inside ? ((const u32x4*)in)[sp] : z;
    } else if (inside) {
      ((u32x4*)out)[sp] = ((const u32x4*)in)[i];
    }
  }
}

// ---------------------------------------------------------------- patch cutter of the data path (medimgen/data_processing.py)
// crop_and_pad_nd (DATA:148-225) fused with the cheap tail of MedicalDataset.__getitem__ (DATA:586-595): the volume stays resident
// in HBM (fp32 or fp16, [C][D][H][W]); one launch cuts one [C][oD][oH][oW] fp32 patch whose lower corner is `lo` (may be negative /
// run past the volume: pad_value there), optionally mirrors it along the axes of flip_mask (bit 0 = D, 1 = H, 2 = W), multiplies
// by `scale` and clamps to [0, 1].  HBM-bound: one read and one write per output element, the W axis on the lanes.
template <typename T>
__global__ void k_crop_pad(const T* __restrict__ src, float* __restrict__ out, int C, int D, int H, int W, int l0, int l1, int l2, int oD, int oH,
                           int oW, float pad, int flip, float scale, int clamp01, int64_t total) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int x = (int)(i % oW);
    int64_t t = i / oW;
    int y = (int)(t % oH); t /= oH;
    int z = (int)(t % oD);
    const int64_t c = t / oD;
    if (flip & 1) z = oD - 1 - z;
    if (flip & 2) y = oH - 1 - y;
    if (flip & 4) x = oW - 1 - x;
    const int sz = l0 + z, sy = l1 + y, sx = l2 + x;
    float v = pad;
    if ((unsigned)sz < (unsigned)D && (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W)
      v = (float)src[((c * D + sz) * H + sy) * (int64_t)W + sx];
    v *= scale;
    if (clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
    out[i] = v;
  }
}

// ---------------------------------------------------------------- q-sample and MSE at the model boundary
// x_t = a[n] * x0 + b[n] * noise, NCDHW fp32 in, NDHWC bf16 out (T-LDM:160; closed form oracle/step.py)
// velocity (optional, fp32 NCDHW): the v-prediction target a * noise - b * x0 (scheduler.get_velocity, T-LDM:163-165)
__global__ void k_qsample(const float* __restrict__ x0, const float* __restrict__ noise, const float* __restrict__ sqrt_acp,
                          const float* __restrict__ sqrt_1macp, const int64_t* __restrict__ t, const float* __restrict__ cond,
                          bf16* __restrict__ out, float* __restrict__ velocity, int C, int Cc, int64_t V, int64_t total, int T,
                          const uint8_t* __restrict__ drop) {
  // drop (optional, [N]): condition dropout of classifier-free guidance -- the condition channels of a sample with drop[n] != 0 are zeros
  const int Co = C + Cc;  // voxel pitch of the model input: C noised channels, then Cc condition channels as they are
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t n = i / V, v = i - n * V;
    int64_t tn = t[n];
    tn = tn < 0 ? 0 : (tn >= T ? T - 1 : tn);  // an out-of-range timestep must not index past the schedule tables
    float a = sqrt_acp[tn], b = sqrt_1macp[tn];
    for (int c = 0; c < C; ++c) {
      int64_t s = (n * C + c) * V + v;
      const float xv = x0[s], nv = noise[s];
      out[i * Co + c] = f2bf(a * xv + b * nv);
      if (velocity) velocity[s] = a * nv - b * xv;
    }
    const bool dropped = drop && drop[n];
    for (int c = 0; c < Cc; ++c) out[i * Co + C + c] = f2bf(dropped ? 0.f : cond[(n * Cc + c) * V + v]);
  }
}
// The per-element arithmetic of a step -- ddpm_update, ddim_update, cfg_combine -- is in diffusion_update.h: the tiled sampler's
// kernels (sliding.hip) apply the same functions.
// THE update launch of the sample loop, on either scheduler (DDIM: ddim_update on row index[0] of the rows, else ddpm_update on row t =
// index[0] of the coefficients; index is a device scalar, so every step replays one graph).  x (fp32 NCDHW, batch N) is updated in
// place and also written, as bf16, into the sample channels of the next model input x_cl (NDHWC, voxel pitch x_cl_cs >= C: the
// condition channels behind them stay as they are); mo_cl is the model output (NDHWC bf16), z fp32 NCDHW noise.
// GUIDED -- classifier-free guidance (Ho & Salimans 2022; not part of the reference: PARITY UNPINNED): the model ran ONCE at batch 2N --
// rows [0, N) of mo_cl with the condition, rows [N, 2N) with the null condition -- and the step continues from
//   m = m_uncond + w (m_cond - m_uncond)      (fp32, from the two bf16 outputs; w = guidance[0], a device scalar: one graph, every scale)
// with exactly the unguided arithmetic; the bf16 copy goes into BOTH halves of x_cl (batch 2N; the condition in the first half, zeros
// in the second).
// INPAINT -- image-conditioned sampling (masked inpainting in the manner of RePaint, Lugmayr et al. 2022; not part of the reference:
// PARITY UNPINNED): compositing inside the update launch, so a step stays ONE forward plus ONE launch.  known: [rows][4] beside the
// step table, indexed by the same device scalar; q0 = sqrt(A_next), q1 = sqrt(1 - A_next), the level the step arrives at.
//   m >= 1:  x_next = ddpm_update / ddim_update(...)            (image and known_noise are not read)
//   m <= 0:  x_next = q0 image + q1 known_noise                 (the model output, x and z are not read)
//   else:    x_next = m x_gen + (1 - m) x_known
// A selection, not a lerp evaluated everywhere: a NaN in a buffer the rule does not read (the model's bf16 overflow inside a region
// that is overwritten anyway) does not reach the output, and mask-1 voxels carry the bits of the plain step.  mask fp32 [N][V] (one
// value per voxel, every channel), image / known_noise fp32 NCDHW.  Without INPAINT none of the four is read: every voxel is m = 1.
template <bool DDIM, bool GUIDED, bool INPAINT>
__device__ __forceinline__ void diffusion_step(float* __restrict__ x, const bf16* __restrict__ mo_cl, const float* __restrict__ z,
                                               const float* __restrict__ table, const int64_t* __restrict__ index,
                                               const float* __restrict__ guidance, const float* __restrict__ mask,
                                               const float* __restrict__ image, const float* __restrict__ known_noise,
                                               const float* __restrict__ known, bf16* __restrict__ x_cl, int x_cl_cs, int C, int64_t V,
                                               int64_t total, int flags, unsigned block_dim, unsigned grid_dim) {
  const float* k = table + index[0] * 5;
  const float k0 = k[0], k1 = k[1], k2 = k[2], k3 = k[3], k4 = k[4];
  float q0 = 0.f, q1 = 0.f;
  if (INPAINT) {
    const float* q = known + index[0] * 4;
    q0 = q[0], q1 = q[1];
  }
  const float w = GUIDED ? guidance[0] : 0.f;
  for (int64_t i = blockIdx.x * (int64_t)block_dim + threadIdx.x; i < total; i += (int64_t)grid_dim * block_dim) {
    int64_t n = i / V, v = i - n * V;
    const int64_t iu = i + total;  // the same voxel of the unconditional half (GUIDED)
    const float m = INPAINT ? mask[i] : 1.f;
    for (int c = 0; c < C; ++c) {
      const int64_t s = (n * C + c) * V + v;
      float xg = 0.f, xk = 0.f;
      if (!(m <= 0.f)) {  // regenerated, at least in part
        float mo = bf2f(mo_cl[i * C + c]);
        if (GUIDED) {
          mo = cfg_combine(mo, bf2f(mo_cl[iu * C + c]), w);
        }
        xg = DDIM ? ddim_update(x[s], mo, z, s, k0, k1, k2, k3, k4, flags) : ddpm_update(x[s], mo, z, s, k0, k1, k2, k3, k4, flags);
      }
      if (!(m >= 1.f)) {  // known, at least in part (INPAINT only)
        xk = q0 * image[s];
        if (q1 != 0.f) xk += q1 * known_noise[s];
      }
      const float xn = m >= 1.f ? xg : (m <= 0.f ? xk : m * xg + (1.f - m) * xk);
      x[s] = xn;
      if (x_cl) {
        const bf16 b = f2bf(xn);
        x_cl[i * x_cl_cs + c] = b;
        if (GUIDED) x_cl[iu * x_cl_cs + c] = b;
      }
    }
  }
}
// (block_dim, grid_dim: blockDim.x and gridDim.x as the kernel itself reads them -- inside a device function the compiler does not
// assume uniform workgroups and reads them the long way)
// The one body under the three argument blocks it is launched with: a kernel whose block also carries the pointers it never reads ran
// 1 - 3 % slower at sampling shapes (EXPERIMENTS.md, 2026-10-20), so each form is passed only what it reads.  Eight instantiations.
template <bool DDIM>
__global__ void k_diffusion_step(float* __restrict__ x, const bf16* __restrict__ mo_cl, const float* __restrict__ z,
                                 const float* __restrict__ table, const int64_t* __restrict__ index, bf16* __restrict__ x_cl, int x_cl_cs, int C,
                                 int64_t V, int64_t total, int flags) {
  diffusion_step<DDIM, false, false>(x, mo_cl, z, table, index, nullptr, nullptr, nullptr, nullptr, nullptr, x_cl, x_cl_cs, C, V, total, flags,
                                     blockDim.x, gridDim.x);
}
template <bool DDIM>
__global__ void k_diffusion_step_guided(float* __restrict__ x, const bf16* __restrict__ mo_cl, const float* __restrict__ z,
                                        const float* __restrict__ table, const int64_t* __restrict__ index,
                                        const float* __restrict__ guidance, bf16* __restrict__ x_cl, int x_cl_cs, int C, int64_t V,
                                        int64_t total, int flags) {
  diffusion_step<DDIM, true, false>(x, mo_cl, z, table, index, guidance, nullptr, nullptr, nullptr, nullptr, x_cl, x_cl_cs, C, V, total, flags,
                                     blockDim.x, gridDim.x);
}
template <bool DDIM, bool GUIDED>
__global__ void k_diffusion_step_inpaint(float* __restrict__ x, const bf16* __restrict__ mo_cl, const float* __restrict__ z,
                                         const float* __restrict__ table, const int64_t* __restrict__ index,
                                         const float* __restrict__ guidance, const float* __restrict__ mask,
                                         const float* __restrict__ image, const float* __restrict__ known_noise,
                                         const float* __restrict__ known, bf16* __restrict__ x_cl, int x_cl_cs, int C, int64_t V,
                                         int64_t total, int flags) {
  diffusion_step<DDIM, GUIDED, true>(x, mo_cl, z, table, index, guidance, mask, image, known_noise, known, x_cl, x_cl_cs, C, V, total, flags,
                                     blockDim.x, gridDim.x);
}
// One forward-diffusion move between two replays of the step above (resampling): x = a x + b z in place, a = sqrt(A_t / A_next) and
// b = sqrt(1 - A_t / A_next) of the step being undone, by value.  No model and no mask: a known region renoised this way is a valid
// sample of the higher level.  The bf16 copy goes into the sample channels of `halves` (1, or 2 when guided) batches of x_cl.
__global__ void k_renoise(float* __restrict__ x, const float* __restrict__ z, float a, float b, bf16* __restrict__ x_cl, int x_cl_cs, int halves,
                          int C, int64_t V, int64_t total) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t n = i / V, v = i - n * V;
    for (int c = 0; c < C; ++c) {
      const int64_t s = (n * C + c) * V + v;
      const float xn = a * x[s] + b * z[s];
      x[s] = xn;
      if (x_cl) {
        const bf16 h = f2bf(xn);
        x_cl[i * x_cl_cs + c] = h;
        if (halves == 2) x_cl[(i + total) * x_cl_cs + c] = h;
      }
    }
  }
}
// loss = mean((pred - target)^2) over all elements; dpred = 2 (pred - target) / numel * loss_scale.
// pred NDHWC bf16, target NCDHW fp32, dpred NDHWC bf16.  loss accumulated with one atomic per block into *loss_sum.
__global__ void k_mse(const bf16* __restrict__ pred, const float* __restrict__ target, bf16* __restrict__ dpred,
                      float* __restrict__ loss_sum, int C, int64_t V, int64_t total, float inv_numel, float grad_scale) {
  __shared__ float red[4];
  float acc = 0.f;
  const float gs = 2.f * inv_numel * grad_scale;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t n = i / V, v = i - n * V;
    for (int c = 0; c < C; ++c) {
      float d = bf2f(pred[i * C + c]) - target[(n * C + c) * V + v];
      acc += d * d;
      if (dpred) dpred[i * C + c] = f2bf(d * gs);
    }
  }
  float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) atomicAdd(loss_sum, s * inv_numel);
}

// loss = mean(|pred - target|) (F.l1_loss, T-AE:414); dpred = sign(pred - target) / numel.  Same layouts as k_mse.
__global__ void k_l1(const bf16* __restrict__ pred, const float* __restrict__ target, bf16* __restrict__ dpred, float* __restrict__ loss_sum,
                     int C, int64_t V, int64_t total, float inv_numel) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t n = i / V, v = i - n * V;
    for (int c = 0; c < C; ++c) {
      float d = bf2f(pred[i * C + c]) - target[(n * C + c) * V + v];
      acc += fabsf(d);
      if (dpred) dpred[i * C + c] = f2bf(d > 0.f ? inv_numel : (d < 0.f ? -inv_numel : 0.f));
    }
  }
  float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) atomicAdd(loss_sum, s * inv_numel);
}

// AutoencoderKL.sampling (AEKL:786-787) + AutoEncoder.get_kl_loss (T-AE:68-72) on channels-last bf16 latents:
//   z = mu + eps * sigma;   kl = 0.5 * sum(mu^2 + sigma^2 - log(sigma^2) - 1) / B;   *loss += kl_weight * kl
// eps is fp32 NCDHW (torch.randn_like layout), n = N * V voxels, C latent channels.
__global__ void k_reparam_kl_fwd(const bf16* __restrict__ mu, const bf16* __restrict__ sigma, const float* __restrict__ eps,
                                 bf16* __restrict__ z, float* __restrict__ loss, int C, int64_t V, int64_t total, float klw_over_b) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t n = i / V, v = i - n * V;
    for (int c = 0; c < C; ++c) {
      const float m = bf2f(mu[i * C + c]), sg = bf2f(sigma[i * C + c]);
      z[i * C + c] = f2bf(m + eps[(n * C + c) * V + v] * sg);
      acc += 0.5f * (m * m + sg * sg - logf(sg * sg) - 1.f);
    }
  }
  float s = block_sum_256(acc, red);
  if (threadIdx.x == 0 && loss) atomicAdd(loss, s * klw_over_b);
}
// dmu = dz + klw/B * mu;   dsigma = dz * eps + klw/B * (sigma - 1/sigma)
__global__ void k_reparam_kl_bwd(const bf16* __restrict__ mu, const bf16* __restrict__ sigma, const float* __restrict__ eps,
                                 const bf16* __restrict__ dz, bf16* __restrict__ dmu, bf16* __restrict__ dsigma, int C, int64_t V,
                                 int64_t total, float klw_over_b) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t n = i / V, v = i - n * V;
    for (int c = 0; c < C; ++c) {
      const float m = bf2f(mu[i * C + c]), sg = bf2f(sigma[i * C + c]), g = bf2f(dz[i * C + c]);
      dmu[i * C + c] = f2bf(g + klw_over_b * m);
      dsigma[i * C + c] = f2bf(g * eps[(n * C + c) * V + v] + klw_over_b * (sg - 1.f / sg));
    }
  }
}

// ---------------------------------------------------------------- class embedding (nn.Embedding rows added to the time embedding,
// UNet:1837-1839, 1975-1980): emb[b][:] += W[labels[b]][:];  backward: dW[labels[b]][:] += d_emb[b][:] (labels may repeat: atomics)
__global__ void k_embedding_add(float* __restrict__ emb, const float* __restrict__ w, const int64_t* __restrict__ labels, int B, int dim) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * dim) return;
  const int b = i / dim, j = i - b * dim;
  emb[i] += w[labels[b] * dim + j];
}
__global__ void k_embedding_bwd(const float* __restrict__ d_emb, const int64_t* __restrict__ labels, float* __restrict__ dw, int B, int dim) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * dim) return;
  const int b = i / dim, j = i - b * dim;
  atomicAdd(dw + labels[b] * dim + j, d_emb[i]);
}

// condition dropout of classifier-free guidance (not part of the reference): the labels the embedding reads, with the null class in
// place of a dropped sample's label -- forward and backward both take `out`, so dropped samples train the null row
__global__ void k_select_labels(const int64_t* __restrict__ labels, const uint8_t* __restrict__ drop, int64_t null_class,
                                int64_t* __restrict__ out, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) out[b] = drop[b] ? null_class : labels[b];
}
// ... and the fp32 -> bf16 cast of the cross-attention context [N][row] that writes zero rows for dropped samples
__global__ void k_cast_bf16_drop(const float* __restrict__ s, bf16* __restrict__ d, const uint8_t* __restrict__ drop, int64_t row, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    d[i] = f2bf(drop[i / row] ? 0.f : s[i]);
}

// ---------------------------------------------------------------- sinusoidal timestep embedding (UNet:461-485)
__global__ void k_timestep_embedding(const int64_t* __restrict__ t, float* __restrict__ out, int B, int dim, float neg_log_period) {
  int half = dim / 2;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * dim) return;
  int b = i / dim, j = i - b * dim;
  float v = 0.f;
  if (j < 2 * half) {
    int k = j < half ? j : j - half;
    // freq rounded once from fp64 (== torch's CPU fp32 exp to within an ulp); at t ~ 1000 an ulp of freq is 1e-4 rad
    float freq = (float)exp((double)(neg_log_period * (float)k) / (double)half);
    float arg = (float)t[b] * freq;
    v = j < half ? cosf(arg) : sinf(arg);
  }
  out[i] = v;  // odd dim: last column zero-padded
}

// small fp32 vectors (time embedding MLP): y = silu(x) / dx = dy * silu'(x)
__global__ void k_silu_f32(const float* x, float* y, int64_t n) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) y[i] = silu_f(x[i]);
}
__global__ void k_silu_bwd_f32(const float* x, const float* dy, float* dx, int64_t n) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) dx[i] = dy[i] * silu_grad_f(x[i]);
}

// ---------------------------------------------------------------- column sums: out[n][c] (+)= sum_v x[n][v][c]
// grid (chunks, N); one block reduces a V-range for all C channels; partial results are added with fp32 atomics
// (C floats per block -> a few thousand atomics per call, far below the atomic rate).
__global__ void k_colsum(const bf16* __restrict__ x, float* __restrict__ out, int out_stride, int C, int64_t V, int64_t vchunk) {
  extern __shared__ float sm[];  // [rows][C]
  int n = blockIdx.y;
  int C8 = C / 8;
  int rows = blockDim.x / C8;  // voxel lanes
  int cg = threadIdx.x % C8, r = threadIdx.x / C8;
  int64_t v0 = blockIdx.x * vchunk, v1 = v0 + vchunk < V ? v0 + vchunk : V;
  F8 acc;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc.v[j] = 0.f;
  if (r < rows)
    for (int64_t v = v0 + r; v < v1; v += 4 * rows) {  // 4 independent 16-byte loads in flight per lane
      u32x4 raw[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int64_t vk = v + (int64_t)k * rows;
        u32x4 z = {0u, 0u, 0u, 0u};
        raw[k] = vk < v1 ? *(const u32x4*)(x + ((int64_t)n * V + vk) * C + cg * 8) : z;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        F8 g = unpack8(raw[k]);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc.v[j] += g.v[j];
      }
    }
  if (r < rows)
#pragma unroll
    for (int j = 0; j < 8; ++j) sm[r * C + cg * 8 + j] = acc.v[j];
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < rows; ++k) s += sm[k * C + c];
    atomicAdd(out + (int64_t)n * out_stride + c, s);
  }
}

// ragged channel counts (C = 1, 4, ...; the 1-channel output conv): one pass per channel, block reduce + one atomic
__global__ void __launch_bounds__(256) k_colsum_ragged(const bf16* __restrict__ x, float* __restrict__ out, int out_stride, int C,
                                                       int64_t V, int64_t vchunk) {
  __shared__ float red[4];
  int n = blockIdx.y;
  int64_t v0 = blockIdx.x * vchunk, v1 = v0 + vchunk < V ? v0 + vchunk : V;
  for (int c = 0; c < C; ++c) {
    float acc = 0.f;
    for (int64_t v = v0 + threadIdx.x; v < v1; v += 256) acc += bf2f(x[((int64_t)n * V + v) * C + c]);
    float s = block_sum_256(acc, red);
    if (threadIdx.x == 0) atomicAdd(out + (int64_t)n * out_stride + c, s);
  }
}

// AutoencoderKL.encode tail (AEKL:767-769): sigma = exp(clamp(logvar, -30, 20) / 2), and its backward
// (clamp passes the gradient on the closed interval, like aten::clamp)
__global__ void k_logvar_sigma(const bf16* __restrict__ lv, bf16* __restrict__ sigma, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v = fminf(fmaxf(bf2f(lv[i]), -30.f), 20.f);
    sigma[i] = f2bf(__expf(0.5f * v));
  }
}
__global__ void k_logvar_sigma_bwd(const bf16* __restrict__ dsigma, const bf16* __restrict__ lv, const bf16* __restrict__ sigma,
                                   bf16* __restrict__ dlv, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v = bf2f(lv[i]);
    bool pass = v >= -30.f && v <= 20.f;
    dlv[i] = f2bf(pass ? 0.5f * bf2f(dsigma[i]) * bf2f(sigma[i]) : 0.f);
  }
}

// y[r][c] += x[r][c] over a [rows][cols] block with row pitches ldx / ldy  (fp32; tiny tensors: biases, embeddings)
__global__ void k_add_f32_2d(const float* x, int ldx, float* y, int ldy, int rows, int cols) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  int r = i / cols, c = i - r * cols;
  y[(int64_t)r * ldy + c] += x[(int64_t)r * ldx + c];
}
// out[c] (+)= sum_r in[r][c]
__global__ void k_sum_rows_f32(const float* in, int ld, int rows, int cols, float* out, int accumulate) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  float s = accumulate ? out[c] : 0.f;
  for (int r = 0; r < rows; ++r) s += in[(int64_t)r * ld + c];
  out[c] = s;
}

}  // namespace

extern "C" {

int mi_ncdhw_f32_to_ndhwc_bf16(const float* src, void* dst, int N, int C, int64_t V, hipStream_t st) {
  if (N <= 0 || C <= 0 || V <= 0) return MI_ERR_BAD_ARG;
  int64_t total = (int64_t)N * V;
  hipLaunchKernelGGL(k_ncdhw_to_ndhwc, dim3(grid_for(total)), dim3(kThreads), 0, st, src, (bf16*)dst, C, V, total);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_ndhwc_bf16_to_ncdhw_f32(const void* src, float* dst, int N, int C, int64_t V, hipStream_t st) {
  if (N <= 0 || C <= 0 || V <= 0) return MI_ERR_BAD_ARG;
  int64_t total = (int64_t)N * V;
  hipLaunchKernelGGL(k_ndhwc_to_ncdhw, dim3(grid_for(total)), dim3(kThreads), 0, st, (const bf16*)src, dst, C, V, total);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_add_bf16(const void* a, const void* b, void* out, int64_t n, hipStream_t st) {
  if (n <= 0) return MI_ERR_BAD_ARG;
  if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) != 0) return MI_ERR_BAD_ARG;
  int64_t n8 = n / 8;
  if (n8 > 0) hipLaunchKernelGGL(k_add_bf16, dim3(grid_for(n8)), dim3(kThreads), 0, st, (const u32x4*)a, (const u32x4*)b, (u32x4*)out, n8);
  if (n8 * 8 < n)
    hipLaunchKernelGGL(k_add_bf16_tail, dim3(1), dim3(64), 0, st, (const bf16*)a, (const bf16*)b, (bf16*)out, n8 * 8, n);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_cast_f32_to_bf16(const float* src, void* dst, int64_t n, hipStream_t st) {
  if (n <= 0) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_cast_f32_bf16, dim3(grid_for(n)), dim3(kThreads), 0, st, src, (bf16*)dst, n);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_copy_channels(const void* src, int Cs, int c0s, void* dst, int Cd, int c0d, int nC, int64_t nvox, hipStream_t st) {
  if ((Cs | c0s | Cd | c0d | nC) & 7 || nC <= 0 || nvox <= 0 || c0s + nC > Cs || c0d + nC > Cd) return MI_ERR_BAD_ARG;
  int64_t total = nvox * (nC / 8);
  hipLaunchKernelGGL(k_copy_channels, dim3(grid_for(total)), dim3(kThreads), 0, st, (const bf16*)src, Cs, c0s, (bf16*)dst, Cd, c0d,
                     nC / 8, total);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_upsample_nearest_fwd(const void* x, void* y, int N, int D, int H, int W, int C, int fd, int fh, int fw, hipStream_t st) {
  if (!x || !y || N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || C & 7 || fd < 1 || fh < 1 || fw < 1) return MI_ERR_BAD_ARG;
  int64_t total = (int64_t)N * D * fd * H * fh * W * fw * (C / 8);
  hipLaunchKernelGGL(k_upsample_fwd, dim3(grid_for(total)), dim3(kThreads), 0, st, (const bf16*)x, (bf16*)y, D, H, W, C / 8, fd, fh, fw, total);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_upsample_nearest_bwd(const void* dy, void* dx, int N, int D, int H, int W, int C, int fd, int fh, int fw, hipStream_t st) {
  if (!dy || !dx || N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || C & 7 || fd < 1 || fh < 1 || fw < 1) return MI_ERR_BAD_ARG;
  int64_t total = (int64_t)N * D * H * W * (C / 8);
  hipLaunchKernelGGL(k_upsample_bwd, dim3(grid_for(total)), dim3(kThreads), 0, st, (const bf16*)dy, (bf16*)dx, D, H, W, C / 8, fd, fh, fw, total);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_space_to_depth(const void* in, int in_cs, void* out, int N, int D, int H, int W, int C, int fd, int fh, int fw, hipStream_t st) {
  if (!in || !out || N <= 0 || D <= 0 || H <= 0 || W <= 0 || fd < 1 || fh < 1 || fw < 1) return MI_ERR_BAD_ARG;
  if (in_cs < C || (in_cs & 7)) return MI_ERR_BAD_ARG;
  if (C <= 0 || C & 7) return MI_ERR_BAD_ARG;
  int Dp = (D + fd - 1) / fd, Hp = (H + fh - 1) / fh, Wp = (W + fw - 1) / fw;
  int64_t total = (int64_t)N * Dp * Hp * Wp * fd * fh * fw * (C / 8);
  hipLaunchKernelGGL(k_space_depth, dim3(grid_for(total)), dim3(kThreads), 0, st, (const bf16*)in, (bf16*)out, D, H, W, C / 8, fd, fh, fw, Dp, Hp, Wp, 1, total, in_cs / 8);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_depth_to_space(const void* in, void* out, int N, int D, int H, int W, int C, int fd, int fh, int fw, hipStream_t st) {
  // (D, H, W, C) describe the SPACE-side tensor `out`; `in` is [N, ceil(D/fd), ceil(H/fh), ceil(W/fw), fd*fh*fw*C]
  if (!in || !out || N <= 0 || D <= 0 || H <= 0 || W <= 0 || fd < 1 || fh < 1 || fw < 1) return MI_ERR_BAD_ARG;
  if (C <= 0 || C & 7) return MI_ERR_BAD_ARG;
  int Dp = (D + fd - 1) / fd, Hp = (H + fh - 1) / fh, Wp = (W + fw - 1) / fw;
  int64_t total = (int64_t)N * Dp * Hp * Wp * fd * fh * fw * (C / 8);
  hipLaunchKernelGGL(k_space_depth, dim3(grid_for(total)), dim3(kThreads), 0, st, (const bf16*)in, (bf16*)out, D, H, W, C / 8, fd, fh, fw, Dp, Hp, Wp, 0, total, C / 8);
  MI_CHECK_LAUNCH();
  return 0;
}
static int avgpool_dims(int D, int H, int W, const int k[3], const int s[3], int o[3]) {
  const int in[3] = {D, H, W};
  for (int a = 0; a < 3; ++a) {
    if (k[a] <= 0 || s[a] <= 0 || in[a] < k[a]) return MI_ERR_BAD_ARG;
    o[a] = (in[a] - k[a]) / s[a] + 1;
  }
  return 0;
}
int mi_avgpool_fwd(const void* x, void* y, int N, int D, int H, int W, int C, const int kernel[3], const int stride[3], hipStream_t st) {
  int o[3];
  if (!x || !y || N <= 0 || C <= 0 || (C & 7) || avgpool_dims(D, H, W, kernel, stride, o)) return MI_ERR_BAD_ARG;
  int64_t total = (int64_t)N * o[0] * o[1] * o[2] * (C / 8);
  hipLaunchKernelGGL(k_avgpool_fwd, dim3(grid_for(total)), dim3(kThreads), 0, st, (const bf16*)x, (bf16*)y, D, H, W, C / 8, kernel[0], kernel[1],
                     kernel[2], stride[0], stride[1], stride[2], o[0], o[1], o[2], total);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_avgpool_bwd(const void* dy, void* dx, int N, int D, int H, int W, int C, const int kernel[3], const int stride[3], hipStream_t st) {
  int o[3];
  if (!dy || !dx || N <= 0 || C <= 0 || (C & 7) || avgpool_dims(D, H, W, kernel, stride, o)) return MI_ERR_BAD_ARG;
  int64_t total = (int64_t)N * D * H * W * (C / 8);
  hipLaunchKernelGGL(k_avgpool_bwd, dim3(grid_for(total)), dim3(kThreads), 0, st, (const bf16*)dy, (bf16*)dx, D, H, W, C / 8, kernel[0], kernel[1],
                     kernel[2], stride[0], stride[1], stride[2], o[0], o[1], o[2], total);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_crop_pad(const void* src, int src_is_f16, int C, int D, int H, int W, const int lo[3], float* out, int oD, int oH, int oW,
                float pad_value, int flip_mask, float scale, int clamp01, hipStream_t st) {
  if (!src || !out || !lo || C <= 0 || D <= 0 || H <= 0 || W <= 0 || oD <= 0 || oH <= 0 || oW <= 0) return MI_ERR_BAD_ARG;
  const int64_t total = (int64_t)C * oD * oH * oW;
  if (src_is_f16)
    hipLaunchKernelGGL(k_crop_pad<_Float16>, dim3(grid_for(total)), dim3(kThreads), 0, st, (const _Float16*)src, out, C, D, H, W, lo[0], lo[1], lo[2],
                       oD, oH, oW, pad_value, flip_mask, scale, clamp01, total);
  else
    hipLaunchKernelGGL(k_crop_pad<float>, dim3(grid_for(total)), dim3(kThreads), 0, st, (const float*)src, out, C, D, H, W, lo[0], lo[1], lo[2], oD,
                       oH, oW, pad_value, flip_mask, scale, clamp01, total);
  MI_CHECK_LAUNCH();
  return 0;
}
static int qsample(const float* x0, const float* noise, const float* sqrt_acp, const float* sqrt_1macp, const int64_t* t, const float* cond,
                   int cond_channels, void* out, float* velocity, int N, int C, int64_t V, int num_train_timesteps, const uint8_t* drop,
                   hipStream_t st) {
  int64_t total = (int64_t)N * V;
  if (total <= 0 || C <= 0 || num_train_timesteps <= 0 || !x0 || !noise || !sqrt_acp || !sqrt_1macp || !t || !out) return MI_ERR_BAD_ARG;
  if (cond_channels < 0 || (cond_channels > 0 && !cond)) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_qsample, dim3(grid_for(total)), dim3(kThreads), 0, st, x0, noise, sqrt_acp, sqrt_1macp, t, cond, (bf16*)out, velocity, C,
                     cond ? cond_channels : 0, V, total, num_train_timesteps, drop);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_qsample(const float* x0, const float* noise, const float* sqrt_acp, const float* sqrt_1macp, const int64_t* t, const float* cond,
               int cond_channels, void* out, float* velocity, int N, int C, int64_t V, int num_train_timesteps, hipStream_t st) {
  return qsample(x0, noise, sqrt_acp, sqrt_1macp, t, cond, cond_channels, out, velocity, N, C, V, num_train_timesteps, nullptr, st);
}
int mi_qsample_drop(const float* x0, const float* noise, const float* sqrt_acp, const float* sqrt_1macp, const int64_t* t, const float* cond,
                    int cond_channels, void* out, float* velocity, int N, int C, int64_t V, int num_train_timesteps, const uint8_t* drop,
                    hipStream_t st) {
  if (!drop) return MI_ERR_BAD_ARG;
  return qsample(x0, noise, sqrt_acp, sqrt_1macp, t, cond, cond_channels, out, velocity, N, C, V, num_train_timesteps, drop, st);
}
int mi_diffusion_step(float* x, const void* model_out, const float* noise, const float* table, const int64_t* index, const float* guidance,
                      const float* mask, const float* image, const float* known_noise, const float* known, void* x_cl, int x_cl_cs, int N,
                      int C, int64_t V, int flags, int ddim, hipStream_t st) {
  int64_t total = (int64_t)N * V;
  const int given = (mask != nullptr) + (image != nullptr) + (known_noise != nullptr) + (known != nullptr);  // the known region: all or none
  if (N <= 0 || V <= 0 || C <= 0 || !x || !model_out || !noise || !table || !index || (given != 0 && given != 4) || (x_cl && x_cl_cs < C))
    return MI_ERR_BAD_ARG;
  const dim3 grid(grid_for(total)), block(kThreads);
  const bf16* mo = (const bf16*)model_out;
  bf16* cl = (bf16*)x_cl;
  if (given == 4) {
    auto kern = ddim ? (guidance ? k_diffusion_step_inpaint<true, true> : k_diffusion_step_inpaint<true, false>)
                     : (guidance ? k_diffusion_step_inpaint<false, true> : k_diffusion_step_inpaint<false, false>);
    hipLaunchKernelGGL(kern, grid, block, 0, st, x, mo, noise, table, index, guidance, mask, image, known_noise, known, cl, x_cl_cs, C, V, total,
                       flags);
  } else if (guidance) {
    hipLaunchKernelGGL(ddim ? k_diffusion_step_guided<true> : k_diffusion_step_guided<false>, grid, block, 0, st, x, mo, noise, table, index,
                       guidance, cl, x_cl_cs, C, V, total, flags);
  } else {
    hipLaunchKernelGGL(ddim ? k_diffusion_step<true> : k_diffusion_step<false>, grid, block, 0, st, x, mo, noise, table, index, cl, x_cl_cs, C,
                       V, total, flags);
  }
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_renoise(float* x, const float* noise, float a, float b, void* x_cl, int x_cl_cs, int N, int halves, int C, int64_t V, hipStream_t st) {
  int64_t total = (int64_t)N * V;
  if (N <= 0 || V <= 0 || C <= 0 || !x || !noise || (halves != 1 && halves != 2) || (x_cl && x_cl_cs < C)) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_renoise, dim3(grid_for(total)), dim3(kThreads), 0, st, x, noise, a, b, (bf16*)x_cl, x_cl_cs, halves, C, V, total);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_mse_fwd_bwd(const void* pred, const float* target, void* dpred, float* loss, int N, int C, int64_t V, float grad_scale,
                   hipStream_t st) {
  int64_t total = (int64_t)N * V;
  if (total <= 0) return MI_ERR_BAD_ARG;
  hipError_t e = mi_zero_fill_f32(loss, 1, 1, 1, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_mse, dim3(grid_for(total, 1024)), dim3(kThreads), 0, st, (const bf16*)pred, target, (bf16*)dpred, loss, C, V, total,
                     1.0f / (float)(total * C), grad_scale);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_l1_fwd_bwd(const void* pred, const float* target, void* dpred, float* loss, int N, int C, int64_t V, int accumulate, hipStream_t st) {
  int64_t total = (int64_t)N * V;
  if (total <= 0) return MI_ERR_BAD_ARG;
  if (!accumulate) {
    hipError_t e = mi_zero_fill_f32(loss, 1, 1, 1, st);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k_l1, dim3(grid_for(total, 1024)), dim3(kThreads), 0, st, (const bf16*)pred, target, (bf16*)dpred, loss, C, V, total,
                     1.0f / (float)(total * C));
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_reparam_kl_fwd(const void* mu, const void* sigma, const float* eps, void* z, float* loss, int N, int C, int64_t V, float kl_weight,
                      hipStream_t st) {
  int64_t total = (int64_t)N * V;
  if (total <= 0 || C <= 0) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_reparam_kl_fwd, dim3(grid_for(total, 1024)), dim3(kThreads), 0, st, (const bf16*)mu, (const bf16*)sigma, eps, (bf16*)z, loss,
                     C, V, total, kl_weight / (float)N);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_reparam_kl_bwd(const void* mu, const void* sigma, const float* eps, const void* dz, void* dmu, void* dsigma, int N, int C, int64_t V,
                      float kl_weight, hipStream_t st) {
  int64_t total = (int64_t)N * V;
  if (total <= 0 || C <= 0) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_reparam_kl_bwd, dim3(grid_for(total, 1024)), dim3(kThreads), 0, st, (const bf16*)mu, (const bf16*)sigma, eps,
                     (const bf16*)dz, (bf16*)dmu, (bf16*)dsigma, C, V, total, kl_weight / (float)N);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_embedding_add(float* emb, const float* weight, const int64_t* labels, int B, int dim, hipStream_t st) {
  if (B <= 0 || dim <= 0 || !emb || !weight || !labels) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_embedding_add, dim3(ceil_div((int64_t)B * dim, 256)), dim3(256), 0, st, emb, weight, labels, B, dim);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_embedding_bwd(const float* d_emb, const int64_t* labels, float* dweight, int B, int dim, hipStream_t st) {
  if (B <= 0 || dim <= 0 || !d_emb || !dweight || !labels) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_embedding_bwd, dim3(ceil_div((int64_t)B * dim, 256)), dim3(256), 0, st, d_emb, labels, dweight, B, dim);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_select_labels(const int64_t* labels, const uint8_t* drop, int64_t null_class, int64_t* out, int B, hipStream_t st) {
  if (B <= 0 || null_class < 0 || !labels || !drop || !out) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_select_labels, dim3(ceil_div((int64_t)B, 256)), dim3(256), 0, st, labels, drop, null_class, out, B);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_cast_bf16_drop(const float* src, void* dst, const uint8_t* drop, int N, int64_t row, hipStream_t st) {
  if (N <= 0 || row <= 0 || !src || !dst || !drop) return MI_ERR_BAD_ARG;
  int64_t n = (int64_t)N * row;
  hipLaunchKernelGGL(k_cast_bf16_drop, dim3(grid_for(n)), dim3(kThreads), 0, st, src, (bf16*)dst, drop, row, n);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_timestep_embedding(const int64_t* t, float* out, int B, int dim, float max_period, hipStream_t st) {
  if (B <= 0 || dim <= 0) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_timestep_embedding, dim3(ceil_div((int64_t)B * dim, 256)), dim3(256), 0, st, t, out, B, dim, -logf(max_period));
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_silu_f32(const float* x, float* y, int64_t n, hipStream_t st) {
  if (n <= 0 || !x || !y) return MI_ERR_BAD_ARG;  // n = 0 would launch an empty grid
  hipLaunchKernelGGL(k_silu_f32, dim3(ceil_div(n, 256)), dim3(256), 0, st, x, y, n);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_silu_bwd_f32(const float* x, const float* dy, float* dx, int64_t n, hipStream_t st) {
  if (n <= 0 || !x || !dy || !dx) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_silu_bwd_f32, dim3(ceil_div(n, 256)), dim3(256), 0, st, x, dy, dx, n);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_colsum_bf16(const void* x, float* out, int out_stride, int N, int64_t V, int C, int accumulate, hipStream_t st) {
  if (C <= 0 || C > 8192 || N <= 0 || V <= 0 || out_stride < C) return MI_ERR_BAD_ARG;
  if (!accumulate) {
    hipError_t e = mi_zero_fill_f32(out, out_stride, N, C, st);
    if (e != hipSuccess) return (int)e;
  }
  if (C & 7) {
    if (C > 64) return MI_ERR_UNSUPPORTED;
    int64_t vc = 8192;
    hipLaunchKernelGGL(k_colsum_ragged, dim3(ceil_div(V, vc), N), dim3(256), 0, st, (const bf16*)x, out, out_stride, C, V, vc);
    MI_CHECK_LAUNCH();
    return 0;
  }
  int C8 = C / 8;
  int threads = 256;
  if (C8 > threads) threads = ((C8 + 63) / 64) * 64;
  int rows = threads / C8;
  int64_t vchunk = (V + 511) / 512;  // ~512 blocks whatever the shape (a [4096 x 768] matrix in 2048-row chunks = 2 blocks)
  if (vchunk < 16) vchunk = 16;
  int chunks = ceil_div(V, vchunk);
  hipLaunchKernelGGL(k_colsum, dim3(chunks, N), dim3(threads), sizeof(float) * (size_t)rows * C, st, (const bf16*)x, out, out_stride, C, V, vchunk);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_logvar_to_sigma_fwd(const void* logvar, void* sigma, int64_t n, hipStream_t st) {
  if (n <= 0) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_logvar_sigma, dim3(grid_for(n)), dim3(kThreads), 0, st, (const bf16*)logvar, (bf16*)sigma, n);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_logvar_to_sigma_bwd(const void* dsigma, const void* logvar, const void* sigma, void* dlogvar, int64_t n, hipStream_t st) {
  if (n <= 0) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_logvar_sigma_bwd, dim3(grid_for(n)), dim3(kThreads), 0, st, (const bf16*)dsigma, (const bf16*)logvar,
                     (const bf16*)sigma, (bf16*)dlogvar, n);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_add_f32_2d(const float* x, int ldx, float* y, int ldy, int rows, int cols, hipStream_t st) {
  if (rows <= 0 || cols <= 0 || !x || !y) return MI_ERR_BAD_ARG;
  if (ldy < cols || (ldx != 0 && ldx < cols)) return MI_ERR_BAD_ARG;  // ldx = 0 broadcasts one row; any other pitch below cols overlaps rows
  hipLaunchKernelGGL(k_add_f32_2d, dim3(ceil_div((int64_t)rows * cols, 256)), dim3(256), 0, st, x, ldx, y, ldy, rows, cols);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_zero_f32_2d(float* x, int ld, int rows, int cols, hipStream_t st) {
  if (rows <= 0 || cols <= 0 || ld < cols) return MI_ERR_BAD_ARG;
  hipError_t e = mi_zero_fill_f32(x, ld, rows, cols, st);
  return (int)e;
}
int mi_sum_rows_f32(const float* in, int ld, int rows, int cols, float* out, int accumulate, hipStream_t st) {
  if (rows <= 0 || cols <= 0 || !in || !out || ld < cols) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_sum_rows_f32, dim3(ceil_div(cols, 256)), dim3(256), 0, st, in, ld, rows, cols, out, accumulate);
  MI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
