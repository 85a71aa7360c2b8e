// LPIPS-VGG perceptual loss of the autoencoder's generator step (train_autoencoder.py:416, :601 `PerceptualLoss(**perceptual_params)`;
// third-party `generative` / `lpips` classes: PARITY UNPINNED).  The 13 VGG16 3x3 convs run on the library's 2-D conv plans (forward
// and data gradient only: the network is frozen); this file holds the glue around them:
//   - slice gather with the ImageNet scaling layer (channels-last volume -> [S][A][B][8] bf16, channels 3..7 zero) and its adjoint,
//     the scatter-add of the slice gradients into the volume's gradient;
//   - ReLU fused with the 2x2 / stride-2 max-pool, forward and backward (ties go to the first maximum in scan order, as in torch);
//   - the LPIPS head of one level: channel-normalised features of both branches, squared difference, 1x1 head, mean over pixels and
//     slices, accumulated into a loss scalar together with the gradient w.r.t. the first branch's feature -- one pass.
#include "common.h"
#include "medimgen_hip.h"

namespace {

constexpr int kT = 256;

inline int grid_for(int64_t total) {
  int64_t g = (total + kT - 1) / kT;
  return (int)(g > 256 * 32 ? 256 * 32 : (g < 1 ? 1 : g));
}

// voxel offset (in voxels) of pixel (a, b) of slice `i` of the volume [N][D][H][W] cut across spatial `axis` (0 = D, 1 = H, 2 = W);
// slices are numbered n-major (i = n * L + l, L = extent of the axis), pixel axes are the two remaining spatial axes in order.
__device__ __forceinline__ int64_t slice_voxel(int i, int a, int b, int axis, int D, int H, int W) {
  const int L = axis == 0 ? D : (axis == 1 ? H : W);
  const int n = i / L, l = i - n * L;
  int d, h, w;
  if (axis == 0) { d = l; h = a; w = b; }
  else if (axis == 1) { d = a; h = l; w = b; }
  else { d = a; h = b; w = l; }
  return (((int64_t)n * D + d) * H + h) * W + w;
}

__global__ void __launch_bounds__(kT) k_perc_gather(const bf16* __restrict__ x, int xcs, int C, int N, int D, int H, int W, int axis,
                                                    const int* __restrict__ idx, int S, int A, int B, const float* __restrict__ shift,
                                                    const float* __restrict__ scale, u32x4* __restrict__ out) {
  const int64_t total = (int64_t)S * A * B;
  const int L = axis == 0 ? D : (axis == 1 ? H : W);
  const float s0 = shift[0], s1 = shift[1], s2 = shift[2];
  const float r0 = 1.f / scale[0], r1 = 1.f / scale[1], r2 = 1.f / scale[2];
  for (int64_t p = blockIdx.x * (int64_t)kT + threadIdx.x; p < total; p += (int64_t)gridDim.x * kT) {
    const int s = (int)(p / ((int64_t)A * B));
    const int ab = (int)(p - (int64_t)s * A * B);
    const int a = ab / B, b = ab - a * B;
    const int i = idx[s];
    F8 f;
#pragma unroll
    for (int c = 0; c < 8; ++c) f.v[c] = 0.f;
    if (i >= 0 && i < N * L) {  // (an index outside the axis reads nothing: a zero slice instead of a stray load)
      const bf16* v = x + slice_voxel(i, a, b, axis, D, H, W) * xcs;
      const float v0 = bf2f(v[0]);
      const float v1 = C == 3 ? bf2f(v[1]) : v0, v2 = C == 3 ? bf2f(v[2]) : v0;  // one channel broadcasts to three
      f.v[0] = (v0 - s0) * r0;
      f.v[1] = (v1 - s1) * r1;
      f.v[2] = (v2 - s2) * r2;
    }
    out[p] = pack8(f);
  }
}

__global__ void __launch_bounds__(kT) k_perc_scatter(const u32x4* __restrict__ ds, int axis, const int* __restrict__ idx, int S, int A, int B,
                                                     int N, int D, int H, int W, int C, const float* __restrict__ scale, bf16* __restrict__ dx,
                                                     int dxcs) {
  const int64_t total = (int64_t)S * A * B;
  const int L = axis == 0 ? D : (axis == 1 ? H : W);
  const float r0 = 1.f / scale[0], r1 = 1.f / scale[1], r2 = 1.f / scale[2];
  for (int64_t p = blockIdx.x * (int64_t)kT + threadIdx.x; p < total; p += (int64_t)gridDim.x * kT) {
    const int s = (int)(p / ((int64_t)A * B));
    const int ab = (int)(p - (int64_t)s * A * B);
    const int a = ab / B, b = ab - a * B;
    const int i = idx[s];
    if (i < 0 || i >= N * L) continue;
    const F8 g = unpack8(ds[p]);
    bf16* v = dx + slice_voxel(i, a, b, axis, D, H, W) * dxcs;
    if (C == 3) {
      v[0] = f2bf(bf2f(v[0]) + g.v[0] * r0);
      v[1] = f2bf(bf2f(v[1]) + g.v[1] * r1);
      v[2] = f2bf(bf2f(v[2]) + g.v[2] * r2);
    } else {
      v[0] = f2bf(bf2f(v[0]) + g.v[0] * r0 + g.v[1] * r1 + g.v[2] * r2);
    }
  }
}

__global__ void __launch_bounds__(kT) k_pad_cin(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin, int Cin_pad, int taps) {
  const int64_t total = (int64_t)Cout * Cin_pad * taps;
  for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
    const int t = (int)(i % taps);
    const int64_t r = i / taps;
    const int ci = (int)(r % Cin_pad), co = (int)(r / Cin_pad);
    out[i] = ci < Cin ? w[((int64_t)co * Cin + ci) * taps + t] : 0.f;
  }
}

// One thread per (image, 2x2 window, channel octet); windows cover ceil(H/2) x ceil(W/2) so that an odd last row / column is still
// rectified, the pooled output (floor mode) is written for whole windows only.
__global__ void __launch_bounds__(kT) k_relu_pool_fwd(u32x4* __restrict__ x, u32x4* __restrict__ pooled, int N, int H, int W, int C8) {
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2, Ho = H / 2, Wo = W / 2;
  const int64_t total = (int64_t)N * Hc * Wc * C8;
  for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
    const int c = (int)(i % C8);
    int64_t r = i / C8;
    const int wc = (int)(r % Wc);
    r /= Wc;
    const int hc = (int)(r % Hc);
    const int n = (int)(r / Hc);
    F8 m;
#pragma unroll
    for (int k = 0; k < 8; ++k) m.v[k] = 0.f;  // (every input is rectified: 0 is a lower bound of the maximum)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int h = 2 * hc + dy, w = 2 * wc + dx;
        if (h >= H || w >= W) continue;
        const int64_t o = (((int64_t)n * H + h) * W + w) * C8 + c;
        F8 f = unpack8(x[o]);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          f.v[k] = f.v[k] > 0.f ? f.v[k] : 0.f;
          m.v[k] = fmaxf(m.v[k], f.v[k]);
        }
        x[o] = pack8(f);
      }
    if (pooled && hc < Ho && wc < Wo) pooled[(((int64_t)n * Ho + hc) * Wo + wc) * C8 + c] = pack8(m);
  }
}

__global__ void __launch_bounds__(kT) k_relu_fwd(u32x4* __restrict__ x, int64_t n8) {
  for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < n8; i += (int64_t)gridDim.x * kT) {
    F8 f = unpack8(x[i]);
#pragma unroll
    for (int k = 0; k < 8; ++k) f.v[k] = f.v[k] > 0.f ? f.v[k] : 0.f;
    x[i] = pack8(f);
  }
}

// dx = (dadd + route(dpooled)) * (a > 0); the pooled gradient of a window goes to its FIRST maximum in scan order (row-major), like
// torch's max_pool2d backward.  dx may alias dadd (each thread reads its own elements before writing them).
__global__ void __launch_bounds__(kT) k_relu_pool_bwd(const u32x4* __restrict__ a, const u32x4* __restrict__ dpooled, const u32x4* dadd, u32x4* dx,
                                                      int N, int H, int W, int C8) {
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2, Ho = H / 2, Wo = W / 2;
  const int64_t total = (int64_t)N * Hc * Wc * C8;
  for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
    const int c = (int)(i % C8);
    int64_t r = i / C8;
    const int wc = (int)(r % Wc);
    r /= Wc;
    const int hc = (int)(r % Hc);
    const int n = (int)(r / Hc);
    F8 av[4], g[4];
    int64_t off[4];
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int h = 2 * hc + (q >> 1), w = 2 * wc + (q & 1);
      ok[q] = h < H && w < W;
      off[q] = (((int64_t)n * H + h) * W + w) * C8 + c;
#pragma unroll
      for (int k = 0; k < 8; ++k) av[q].v[k] = g[q].v[k] = 0.f;
      if (ok[q]) {
        av[q] = unpack8(a[off[q]]);
        if (dadd) g[q] = unpack8(dadd[off[q]]);
      }
    }
    if (dpooled && hc < Ho && wc < Wo) {
      const F8 dp = unpack8(dpooled[(((int64_t)n * Ho + hc) * Wo + wc) * C8 + c]);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        int arg = 0;
        float best = av[0].v[k];
#pragma unroll
        for (int q = 1; q < 4; ++q)
          if (av[q].v[k] > best) { best = av[q].v[k]; arg = q; }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q == arg) g[q].v[k] += dp.v[k];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!ok[q]) continue;
#pragma unroll
      for (int k = 0; k < 8; ++k) g[q].v[k] = av[q].v[k] > 0.f ? g[q].v[k] : 0.f;
      dx[off[q]] = pack8(g[q]);
    }
  }
}

// LPIPS head of one level on features f0 (reconstruction branch) and f1 (target branch), [S * P][C] bf16, C = 8 * LANES:
//   n = f / (||f||_2 + eps) per pixel,  value = sum_c w_c (n0_c - n1_c)^2,  *loss += coef * sum over pixels, coef = weight / (S * P)
//   df0 = coef * d(value)/d(f0) = g / r0 - f0 * <g, f0> / (r0^2 ||f0||),  g_c = 2 coef w_c (n0_c - n1_c),  r0 = ||f0|| + eps
// A group of LANES lanes owns one pixel, 8 channels per lane (one 16-byte load per tensor); the per-pixel sums are shuffles inside the
// group.  (||f0|| = 0: the second term is dropped -- torch would give 0 * inf there.)
template <int LANES>
__global__ void __launch_bounds__(kT) k_lpips_head(const u32x4* __restrict__ f0, const u32x4* __restrict__ f1, const float* __restrict__ w,
                                                   int64_t npix, float coef, float eps, float* __restrict__ loss, u32x4* __restrict__ df0) {
  __shared__ float red[4];
  const int lane = threadIdx.x % LANES;
  const int64_t group = (blockIdx.x * (int64_t)kT + threadIdx.x) / LANES, ngroups = (int64_t)gridDim.x * (kT / LANES);
  float wl[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) wl[k] = w[lane * 8 + k];
  float acc = 0.f;
  for (int64_t p = group; p < npix; p += ngroups) {
    const F8 u = unpack8(f0[p * LANES + lane]), v = unpack8(f1[p * LANES + lane]);
    float su = 0.f, sv = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      su += u.v[k] * u.v[k];
      sv += v.v[k] * v.v[k];
    }
#pragma unroll
    for (int off = 1; off < LANES; off <<= 1) {
      su += __shfl_xor(su, off, 64);
      sv += __shfl_xor(sv, off, 64);
    }
    const float nu = sqrtf(su), r0 = nu + eps, r1 = sqrtf(sv) + eps;
    const float i0 = 1.f / r0, i1 = 1.f / r1;
    float g[8], val = 0.f, dot = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float d = u.v[k] * i0 - v.v[k] * i1;
      val += wl[k] * d * d;
      g[k] = 2.f * coef * wl[k] * d;
      dot += g[k] * u.v[k];
    }
    acc += val;
    if (df0) {
#pragma unroll
      for (int off = 1; off < LANES; off <<= 1) dot += __shfl_xor(dot, off, 64);
      const float t = nu > 0.f ? dot * i0 * i0 / nu : 0.f;
      F8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o.v[k] = g[k] * i0 - u.v[k] * t;
      df0[p * LANES + lane] = pack8(o);
    }
  }
  const float s = block_sum_256(acc, red);
  if (threadIdx.x == 0 && loss) atomicAdd(loss, coef * s);
}

}  // namespace

extern "C" {

int mi_perc_gather(const void* x, int x_cstride, int C, int N, int D, int H, int W, int axis, const int* idx, int S, const float* shift,
                   const float* scale, void* out, hipStream_t st) {
  if (!x || !idx || !shift || !scale || !out || (C != 1 && C != 3) || x_cstride < C || N <= 0 || D <= 0 || H <= 0 || W <= 0 || S <= 0 ||
      axis < 0 || axis > 2)
    return MI_ERR_BAD_ARG;
  const int A = axis == 0 ? H : D, B = axis == 2 ? H : W;
  hipLaunchKernelGGL(k_perc_gather, dim3(grid_for((int64_t)S * A * B)), dim3(kT), 0, st, (const bf16*)x, x_cstride, C, N, D, H, W, axis, idx, S, A,
                     B, shift, scale, (u32x4*)out);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_perc_scatter_add(const void* dslices, int axis, const int* idx, int S, int N, int D, int H, int W, int C, const float* scale, void* dx,
                        int dx_cstride, hipStream_t st) {
  if (!dslices || !idx || !scale || !dx || (C != 1 && C != 3) || dx_cstride < C || N <= 0 || D <= 0 || H <= 0 || W <= 0 || S <= 0 || axis < 0 ||
      axis > 2)
    return MI_ERR_BAD_ARG;
  const int A = axis == 0 ? H : D, B = axis == 2 ? H : W;
  hipLaunchKernelGGL(k_perc_scatter, dim3(grid_for((int64_t)S * A * B)), dim3(kT), 0, st, (const u32x4*)dslices, axis, idx, S, A, B, N, D, H, W, C,
                     scale, (bf16*)dx, dx_cstride);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_pad_cin_f32(const float* w, float* out, int Cout, int Cin, int Cin_pad, int taps, hipStream_t st) {
  if (!w || !out || Cout <= 0 || Cin <= 0 || Cin_pad < Cin || taps <= 0) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_pad_cin, dim3(grid_for((int64_t)Cout * Cin_pad * taps)), dim3(kT), 0, st, w, out, Cout, Cin, Cin_pad, taps);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_relu_maxpool2_fwd(void* x, void* pooled, int N, int H, int W, int C, hipStream_t st) {
  if (!x || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7)) return MI_ERR_BAD_ARG;
  if (!pooled) {
    const int64_t n8 = (int64_t)N * H * W * C / 8;
    hipLaunchKernelGGL(k_relu_fwd, dim3(grid_for(n8)), dim3(kT), 0, st, (u32x4*)x, n8);
  } else {
    const int64_t total = (int64_t)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 8);
    hipLaunchKernelGGL(k_relu_pool_fwd, dim3(grid_for(total)), dim3(kT), 0, st, (u32x4*)x, (u32x4*)pooled, N, H, W, C / 8);
  }
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_relu_maxpool2_bwd(const void* a, const void* dpooled, const void* dadd, void* dx, int N, int H, int W, int C, hipStream_t st) {
  if (!a || !dx || (!dpooled && !dadd) || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7)) return MI_ERR_BAD_ARG;
  const int64_t total = (int64_t)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 8);
  hipLaunchKernelGGL(k_relu_pool_bwd, dim3(grid_for(total)), dim3(kT), 0, st, (const u32x4*)a, (const u32x4*)dpooled, (const u32x4*)dadd,
                     (u32x4*)dx, N, H, W, C / 8);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_lpips_head(const void* f0, const void* f1, const float* w, int S, int64_t P, int C, float weight, float eps, float* loss, void* df0,
                  hipStream_t st) {
  if (!f0 || !f1 || !w || S <= 0 || P <= 0 || (!loss && !df0)) return MI_ERR_BAD_ARG;
  const int64_t npix = (int64_t)S * P;
  const float coef = weight / (float)npix;
  const int lanes = C / 8;
  const int64_t g = (npix * lanes + kT - 1) / kT;
  const dim3 grid((int)(g > 4096 ? 4096 : g));
#define MI_HEAD(L)                                                                                                                  \
  hipLaunchKernelGGL(k_lpips_head<L>, grid, dim3(kT), 0, st, (const u32x4*)f0, (const u32x4*)f1, w, npix, coef, eps, loss, (u32x4*)df0)
  switch (C) {
    case 64: MI_HEAD(8); break;
    case 128: MI_HEAD(16); break;
    case 256: MI_HEAD(32); break;
    case 512: MI_HEAD(64); break;
    default: return MI_ERR_UNSUPPORTED;
  }
#undef MI_HEAD
  MI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
