// SSIM / MS-SSIM of the LDM's validation (train_ldm.py:276-277 `MultiScaleSSIMMetric(...)` / `SSIMMetric(...)`, :315-321 the pairwise
// loop; third-party `generative.metrics` classes: PARITY UNPINNED, see metrics.py for the restated formula).
//   - k_ssim_pairs: one workgroup per (pair, channel, output tile of TH x TW x DC).  Per input plane: x / y window -> LDS, the five
//     statistics mean x, mean y, var x, var y, cov xy of the weighted window merged along W then H in LDS, then along D by a KD-deep
//     rolling merge in registers (an accumulator per pending output plane); the merge is the running-mean / running-spread update
//     (ssim_merge), not a filter of raw moments, so flat regions have exactly zero variance at any level.  ssim and cs are evaluated
//     per output voxel and summed.  Only Sigma ssim and Sigma cs of the tile leave the chip (fp64, one pair of values per workgroup).
//     2-D images are D = 1, KD = 1.
//   - k_ssim_pool2: floor 2x average pool of the spatial axes (the MS-SSIM pyramid), fp32.
//   - k_ssim_finalize: per pair, the tile partials of every scale in a fixed order (fp64), relu / power / product, fp32 results.
// The tiling depends on the shape and the kernel only, never on the number of pairs: results are reproducible bit for bit and a pair
// scores the same in any batch.
#include "common.h"
#include "medimgen_hip.h"

namespace {

constexpr int kT = 256;
constexpr int TH = 16, TW = 32;                  // output tile (H x W); every thread owns TH * TW / kT = 2 output columns
constexpr int MAXK = 11;                         // taps per axis
constexpr int RH = TH + MAXK - 1, RW = TW + MAXK - 1;
constexpr int NLD = (RH * RW + kT - 1) / kT;     // window elements per thread and plane
constexpr int NPOS = TH * TW / kT;
constexpr int MAX_SCALES = 8;
constexpr int64_t MAX_BLOCKS = 1 << 22;          // per launch (the dispatch's work-item count is 32-bit)

inline int depth_chunk(int kD) { return kD <= 5 ? 16 : 32; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }

struct PairShape {
  int C, D, H, W, kD, kH, kW, Do, Ho, Wo, DC, nd, nh, nw;
  float c1, c2;
};

__device__ __forceinline__ double block_sum_256_f64(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// One step of the weighted running mean / spread (West's update) of a window, for both images at once: a = (mean x, mean y, var x, var y,
// cov xy) of the taps merged so far, v the same five of the incoming item (a sample: spreads 0).  gn = g / W_total, r = g / W_k,
// c = g W_{k-1} / (W_k W_total) with W_k the sum of the taps up to this one, so a[2..4] end as the window's variances and covariance.
// Unlike E[x^2] - E[x]^2 nothing cancels: in a flat window every difference is exactly 0 and the spreads stay exactly 0, whatever
// the level -- with the raw moments a flat window at level v left v^2 * 1e-7 of rounding in each spread, against c2 = 9e-4 (the zero
// background of two volumes whose tile starts inside the object: 1.4e-4 off in a whole tile's mean).
__device__ __forceinline__ void ssim_merge(float (&a)[5], const float (&v)[5], float gn, float r, float c) {
  const float dx = v[0] - a[0], dy = v[1] - a[1];
  a[0] += r * dx;
  a[1] += r * dy;
  a[2] += gn * v[2] + c * (dx * dx);
  a[3] += gn * v[3] + c * (dy * dy);
  a[4] += gn * v[4] + c * (dx * dy);
}

template <int KD>
__global__ void __launch_bounds__(kT) k_ssim_pairs(const float* __restrict__ xb, const float* __restrict__ yb, const int* __restrict__ pairs,
                                                   PairShape s, const float* __restrict__ taps, double* __restrict__ part, int part_stride,
                                                   int part_off) {
  __shared__ float sx[RH * RW], sy[RH * RW];
  __shared__ float sh[5][RH * TW];
  __shared__ double red[2][4];
  const int tid = threadIdx.x;
  const int tiles = s.C * s.nd * s.nh * s.nw;
  const int pair = blockIdx.x / tiles, tile = blockIdx.x - pair * tiles;
  int r = tile;
  const int tw_ = r % s.nw; r /= s.nw;
  const int th_ = r % s.nh; r /= s.nh;
  const int td_ = r % s.nd;
  const int c = r / s.nd;
  const int h0 = th_ * TH, w0 = tw_ * TW, d0 = td_ * s.DC;
  const int vh = min(TH, s.Ho - h0), vw = min(TW, s.Wo - w0), vd = min(s.DC, s.Do - d0);
  const int rows = vh + s.kH - 1, cols = vw + s.kW - 1, nwin = rows * cols;  // rows <= RH, cols <= RW; h0 + rows <= H, w0 + cols <= W
  const int nplanes = vd + KD - 1;                                            // d0 + nplanes <= D
  const int64_t V = (int64_t)s.D * s.H * s.W;
  const float* x = xb + ((int64_t)pairs[2 * pair] * s.C + c) * V + (int64_t)h0 * s.W + w0;
  const float* y = yb + ((int64_t)pairs[2 * pair + 1] * s.C + c) * V + (int64_t)h0 * s.W + w0;

  // per axis (D, H, W) and tap: the three weights of ssim_merge (the fp32 taps do not sum to exactly 1: W_total is their own sum)
  __shared__ float kc[3][3][MAXK];
  if (tid < 3) {
    const int n = tid == 0 ? KD : (tid == 1 ? s.kH : s.kW);
    const float* g = taps + (tid == 0 ? 0 : (tid == 1 ? KD : KD + s.kH));
    float tot = 0.f, wk = 0.f;
    for (int t = 0; t < n; ++t) tot += g[t];
    for (int t = 0; t < MAXK; ++t) {
      const float gt = t < n ? g[t] : 0.f, prev = wk;
      wk += gt;
      kc[tid][0][t] = gt / tot;
      kc[tid][1][t] = wk > 0.f ? gt / wk : 0.f;
      kc[tid][2][t] = wk > 0.f ? gt * prev / (wk * tot) : 0.f;
    }
  }
  __syncthreads();
  float gd[3][KD];  // slot t of the rolling D filter always takes tap KD - 1 - t
#pragma unroll
  for (int t = 0; t < KD; ++t)
#pragma unroll
    for (int m = 0; m < 3; ++m) gd[m][t] = kc[0][m][KD - 1 - t];

  float px[NLD], py[NLD];
  int loff[NLD], goff[NLD];
#pragma unroll
  for (int k = 0; k < NLD; ++k) {
    const int e = tid + k * kT;
    const int rr = e / cols, cc = e - rr * cols;
    loff[k] = e < nwin ? rr * RW + cc : -1;
    goff[k] = rr * s.W + cc;
  }
  auto load_plane = [&](int p) {
    const float* xp = x + (int64_t)(d0 + p) * s.H * s.W;
    const float* yp = y + (int64_t)(d0 + p) * s.H * s.W;
#pragma unroll
    for (int k = 0; k < NLD; ++k)
      if (loff[k] >= 0) {
        px[k] = xp[goff[k]];
        py[k] = yp[goff[k]];
      }
  };

  // per owned output column: KD pending output planes x 5 statistics
  float acc[NPOS][KD][5];
#pragma unroll
  for (int q = 0; q < NPOS; ++q)
#pragma unroll
    for (int t = 0; t < KD; ++t)
#pragma unroll
      for (int m = 0; m < 5; ++m) acc[q][t][m] = 0.f;
  float sum_ss = 0.f, sum_cs = 0.f;

  load_plane(0);
  for (int p = 0; p < nplanes; ++p) {
#pragma unroll
    for (int k = 0; k < NLD; ++k)
      if (loff[k] >= 0) {
        sx[loff[k]] = px[k];
        sy[loff[k]] = py[k];
      }
    __syncthreads();
    if (p + 1 < nplanes) load_plane(p + 1);  // in flight while this plane is filtered
    // W pass: rows x vw outputs of the five statistics
    for (int e = tid; e < rows * TW; e += kT) {
      const int rr = e / TW, j = e - rr * TW;
      if (j >= vw) continue;
      const float* ax = sx + rr * RW + j;
      const float* ay = sy + rr * RW + j;
      float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < MAXK; ++t)
        if (t < s.kW) {
          const float smp[5] = {ax[t], ay[t], 0.f, 0.f, 0.f};
          ssim_merge(m, smp, kc[2][0][t], kc[2][1][t], kc[2][2][t]);
        }
      const int o = rr * TW + j;
#pragma unroll
      for (int q = 0; q < 5; ++q) sh[q][o] = m[q];
    }
    __syncthreads();
    // H pass, then the rolling D filter
#pragma unroll
    for (int q = 0; q < NPOS; ++q) {
      const int pos = tid + q * kT;
      const int i = pos / TW, j = pos - i * TW;
      const bool valid = i < vh && j < vw;
      float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      if (valid) {
#pragma unroll
        for (int t = 0; t < MAXK; ++t)
          if (t < s.kH) {
            const int o = (i + t) * TW + j;
            const float row[5] = {sh[0][o], sh[1][o], sh[2][o], sh[3][o], sh[4][o]};
            ssim_merge(v, row, kc[1][0][t], kc[1][1][t], kc[1][2][t]);
          }
      }
#pragma unroll
      for (int t = 0; t < KD; ++t) ssim_merge(acc[q][t], v, gd[0][t], gd[1][t], gd[2][t]);
      if (valid && p >= KD - 1) {  // acc[q][0] is output plane d0 + p - (KD - 1): complete
        const float mx = acc[q][0][0], my = acc[q][0][1], vx = acc[q][0][2], vy = acc[q][0][3], cxy = acc[q][0][4];
        const float cs = (2.f * cxy + s.c2) / (vx + vy + s.c2);
        const float ss = ((2.f * mx * my + s.c1) / (mx * mx + my * my + s.c1)) * cs;
        sum_ss += ss;
        sum_cs += cs;
      }
#pragma unroll
      for (int t = 0; t + 1 < KD; ++t)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[q][t][m] = acc[q][t + 1][m];
#pragma unroll
      for (int m = 0; m < 5; ++m) acc[q][KD - 1][m] = 0.f;
    }
  }
  const double tss = block_sum_256_f64((double)sum_ss, red[0]);
  const double tcs = block_sum_256_f64((double)sum_cs, red[1]);
  if (tid == 0) {
    double* o = part + ((int64_t)pair * part_stride + part_off + tile) * 2;
    o[0] = tss;
    o[1] = tcs;
  }
}

__global__ void __launch_bounds__(kT) k_ssim_pool2(const float* __restrict__ x, float* __restrict__ y, int64_t NC, int D, int H, int W,
                                                   int pool_d) {
  const int Do = pool_d ? D / 2 : D, Ho = H / 2, Wo = W / 2;
  const int64_t total = NC * Do * Ho * Wo;
  for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
    const int w = (int)(i % Wo);
    int64_t r = i / Wo;
    const int h = (int)(r % Ho);
    r /= Ho;
    const int d = (int)(r % Do);
    const int64_t nc = r / Do;
    const int di = pool_d ? 2 * d : d;
    const float* p = x + ((nc * D + di) * H + 2 * h) * (int64_t)W + 2 * w;
    float sum = (p[0] + p[1]) + (p[W] + p[W + 1]);
    if (pool_d) {
      const float* q = p + (int64_t)H * W;
      sum += (q[0] + q[1]) + (q[W] + q[W + 1]);
    }
    y[i] = sum * (pool_d ? 0.125f : 0.25f);
  }
}

struct FinArgs {
  int S;
  int tiles[MAX_SCALES];
  double count[MAX_SCALES];
  double w[MAX_SCALES];
};

__global__ void __launch_bounds__(kT) k_ssim_finalize(const double* __restrict__ part, int P, int part_stride, FinArgs a, float* __restrict__ ms_out,
                                                      float* __restrict__ ssim_out) {
  const int pair = blockIdx.x * kT + threadIdx.x;
  if (pair >= P) return;
  const double* row = part + (int64_t)pair * part_stride * 2;
  double prod = 1.0;
  int off = 0;
  for (int sc = 0; sc < a.S; ++sc) {
    double ss = 0.0, cs = 0.0;
    for (int t = 0; t < a.tiles[sc]; ++t) {
      ss += row[(off + t) * 2];
      cs += row[(off + t) * 2 + 1];
    }
    off += a.tiles[sc];
    ss /= a.count[sc];
    cs /= a.count[sc];
    if (sc == 0 && ssim_out) ssim_out[pair] = (float)ss;
    double m = sc == a.S - 1 ? ss : cs;
    m = m < 0.0 ? 0.0 : m;  // relu (NaN stays NaN)
    prod *= pow(m, a.w[sc]);
  }
  if (ms_out) ms_out[pair] = (float)prod;
}

template <int KD>
void launch_pairs(int64_t blocks, const float* xb, const float* yb, const int* pairs, const PairShape& s, const float* taps, double* part,
                  int part_stride, int part_off, hipStream_t st) {
  hipLaunchKernelGGL(k_ssim_pairs<KD>, dim3((unsigned)blocks), dim3(kT), 0, st, xb, yb, pairs, s, taps, part, part_stride, part_off);
}

}  // namespace

extern "C" {

int mi_ssim_tiles(int D, int H, int W, int kD, int kH, int kW) {
  if (D <= 0 || H <= 0 || W <= 0 || kD <= 0 || kH <= 0 || kW <= 0 || kD > MAXK || kH > MAXK || kW > MAXK || D < kD || H < kH || W < kW)
    return 0;
  return cdiv(D - kD + 1, depth_chunk(kD)) * cdiv(H - kH + 1, TH) * cdiv(W - kW + 1, TW);
}

int mi_ssim_pairs(const float* xb, const float* yb, const int* pairs, int P, int C, int D, int H, int W, const float* taps, int kD, int kH,
                  int kW, float c1, float c2, double* partials, int part_stride, int part_off, hipStream_t st) {
  if (!xb || !yb || !pairs || !taps || !partials || P <= 0 || C <= 0) return MI_ERR_BAD_ARG;
  if (kD > MAXK || kH > MAXK || kW > MAXK) return MI_ERR_UNSUPPORTED;
  const int per_c = mi_ssim_tiles(D, H, W, kD, kH, kW);
  if (per_c <= 0) return MI_ERR_BAD_ARG;
  const int tiles = C * per_c;
  if (part_off < 0 || part_off + tiles > part_stride) return MI_ERR_BAD_ARG;
  PairShape s;
  s.C = C;
  s.D = D;
  s.H = H;
  s.W = W;
  s.kD = kD;
  s.kH = kH;
  s.kW = kW;
  s.Do = D - kD + 1;
  s.Ho = H - kH + 1;
  s.Wo = W - kW + 1;
  s.DC = depth_chunk(kD);
  s.nd = cdiv(s.Do, s.DC);
  s.nh = cdiv(s.Ho, TH);
  s.nw = cdiv(s.Wo, TW);
  s.c1 = c1;
  s.c2 = c2;
  const int chunk = (int)(MAX_BLOCKS / tiles > 0 ? MAX_BLOCKS / tiles : 1);
  for (int p0 = 0; p0 < P; p0 += chunk) {
    const int np = P - p0 < chunk ? P - p0 : chunk;
    const int64_t blocks = (int64_t)np * tiles;
    const int* pp = pairs + 2 * (int64_t)p0;
    double* pt = partials + (int64_t)p0 * part_stride * 2;
#define MI_SSIM_KD(K) \
  case K: launch_pairs<K>(blocks, xb, yb, pp, s, taps, pt, part_stride, part_off, st); break;
    switch (kD) {
      MI_SSIM_KD(1) MI_SSIM_KD(2) MI_SSIM_KD(3) MI_SSIM_KD(4) MI_SSIM_KD(5) MI_SSIM_KD(6) MI_SSIM_KD(7) MI_SSIM_KD(8) MI_SSIM_KD(9)
      MI_SSIM_KD(10) MI_SSIM_KD(11)
      default: return MI_ERR_UNSUPPORTED;
    }
#undef MI_SSIM_KD
    MI_CHECK_LAUNCH();
  }
  return 0;
}

int mi_ssim_pool2(const float* x, float* y, int64_t NC, int D, int H, int W, int pool_d, hipStream_t st) {
  if (!x || !y || NC <= 0 || D <= 0 || H < 2 || W < 2 || (pool_d && D < 2)) return MI_ERR_BAD_ARG;
  const int64_t total = NC * (pool_d ? D / 2 : D) * (H / 2) * (W / 2);
  int64_t g = (total + kT - 1) / kT;
  g = g > 8192 ? 8192 : g;
  hipLaunchKernelGGL(k_ssim_pool2, dim3((unsigned)g), dim3(kT), 0, st, x, y, NC, D, H, W, pool_d);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_ssim_finalize(const double* partials, int P, int part_stride, int S, const int* host_tiles, const double* host_counts,
                     const double* host_weights, float* ms_out, float* ssim_out, hipStream_t st) {
  if (!partials || P <= 0 || S <= 0 || S > MAX_SCALES || !host_tiles || !host_counts || (!ms_out && !ssim_out) || (ms_out && !host_weights))
    return MI_ERR_BAD_ARG;
  FinArgs a;
  a.S = S;
  int total = 0;
  for (int i = 0; i < MAX_SCALES; ++i) {
    a.tiles[i] = i < S ? host_tiles[i] : 0;
    a.count[i] = i < S ? host_counts[i] : 1.0;
    a.w[i] = i < S && host_weights ? host_weights[i] : 0.0;
    if (i < S && (a.tiles[i] <= 0 || !(a.count[i] > 0.0))) return MI_ERR_BAD_ARG;
    total += a.tiles[i];
  }
  if (total > part_stride) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_ssim_finalize, dim3(cdiv(P, kT)), dim3(kT), 0, st, partials, P, part_stride, a, ms_out, ssim_out);
  MI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
