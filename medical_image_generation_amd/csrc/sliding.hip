// Sliding-window inference: the voxel passes around a patch-trained network that is run over a whole case (sliding.py; the semantics
// of monai.inferers.SlidingWindowInferer as restated there: PARITY UNPINNED).  fp32 NCDHW, the public layout of the drop-in modules.
//
//   mi_sw_gather      tiles[b] = the window of row b cut out of the image, out-of-image voxels filled by the padding mode
//   mi_sw_accumulate  acc[n, :, window] += imp * pred[b] (and wsum[window] += imp for the rows of image 0), one launch per row in
//                     stream order: windows of one batch overlap, and the sum over windows must not depend on the batch size
//   mi_sw_finish      out = acc / wsum inside the crop
// (further down: mi_sw_gather_cl / mi_sw_accumulate_cl / mi_sw_diffusion_step, the same passes around a U-Net inside a sampling step)
//
// The extents of the image / the accumulator and the window origins are read from a DEVICE table (row 0 = N, D, H, W; rows 1..B =
// n, z0, y0, x0): they are no launch constants, so one captured graph serves cases of every extent.  The kernels therefore guard
// themselves -- a row that names no image, or a window that leaves the accumulator, is a filler -- and the host checks the same
// things when it is given the host copy of the table.
//
// All three are streaming kernels: an item is four consecutive voxels along W, moved with 16-byte accesses where the window origin,
// the row pitch and the pointers allow it, and voxel by voxel where they do not (an odd x0 or W, a window edge inside the item).
#include "common.h"
#include "diffusion_update.h"
#include "medimgen_hip.h"

#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGrid = 1 << 16;

inline int grid_for(int64_t work) {
  int64_t g = (work + kThreads - 1) / kThreads;
  return (int)(g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g));
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// source index of padded coordinate i on an axis of n samples, -1: outside (constant mode).  Reflect is the whole-sample mirror
// without edge repeat, periodic, so any i is resolved inside [0, n).
__device__ __forceinline__ int resolve(int i, int n, int mode) {
  if (i >= 0 && i < n) return i;
  if (mode == MI_SW_PAD_CONSTANT) return -1;
  if (mode == MI_SW_PAD_REPLICATE || n == 1) return i < 0 ? 0 : n - 1;
  const int period = 2 * (n - 1);
  int m = i % period;
  if (m < 0) m += period;
  return m < n ? m : period - m;
}

struct Geom {
  int N, D, H, W;
};
__device__ __forceinline__ Geom load_geom(const int* __restrict__ table) { return {table[0], table[1], table[2], table[3]}; }
// N * C * D * H * W <= elems, without overflow
__device__ __forceinline__ bool geom_fits(const Geom& g, int C, int64_t elems) {
  if (g.N <= 0 || g.D <= 0 || g.H <= 0 || g.W <= 0) return false;
  int64_t v = (int64_t)g.D * g.H;        // < 2^62
  if (v > elems / g.W) return false;
  v *= g.W;
  if (v > elems / C) return false;
  v *= C;
  return v <= elems / g.N;
}

// ---- gather: one item = V voxels along W of one (b, c, z, y) line of the tiles
template <int V>
__global__ void __launch_bounds__(kThreads) k_sw_gather(const float* __restrict__ image, int64_t image_elems, int C, const int* __restrict__ table,
                                                        int B, int rd, int rh, int rw, int mode, float cval, float* __restrict__ tiles) {
  const Geom g = load_geom(table);
  const bool ok = geom_fits(g, C, image_elems);
  const int xw = rw / V;
  const int64_t items = (int64_t)B * C * rd * rh * xw;
  const bool rows4 = V == 4 && (g.W & 3) == 0;  // every image line starts 16-byte aligned (the host checked the base pointer)
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i / xw;
    const int x = (int)(i - r * xw) * V;
    const int y = (int)(r % rh);
    r /= rh;
    const int z = (int)(r % rd);
    r /= rd;
    const int c = (int)(r % C), b = (int)(r / C);
    const int* row = table + 4 * (1 + b);
    const int n = row[0];
    float v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = 0.f;
    if (ok && n >= 0 && n < g.N) {
      const int sz = resolve(row[1] + z, g.D, mode), sy = resolve(row[2] + y, g.H, mode);
      if (sz < 0 || sy < 0) {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = cval;
      } else {
        const float* line = image + ((((int64_t)n * C + c) * g.D + sz) * g.H + sy) * g.W;
        const int x0 = row[3] + x;
        if (V == 4 && rows4 && (x0 & 3) == 0 && x0 >= 0 && x0 + 4 <= g.W) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(line + x0);
#pragma unroll
          for (int k = 0; k < V; ++k) v[k] = q[k];
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const int sx = resolve(x0 + k, g.W, mode);
            v[k] = sx < 0 ? cval : line[sx];
          }
        }
      }
    }
    float* dst = tiles + i * V;
    if (V == 4) {
      f32x4 q;
#pragma unroll
      for (int k = 0; k < V; ++k) q[k] = v[k];
      *reinterpret_cast<f32x4*>(dst) = q;
    } else {
      dst[0] = v[0];
    }
  }
}

// ---- accumulate: the window of ONE row (launches follow each other in row order); one item = V voxels along W of one (c, z, y)
// line of the window; channel 0 of a row of image 0 also carries the weight sum.  fmaf: one rounding per term.
template <int V>
__global__ void __launch_bounds__(kThreads) k_sw_accumulate(const float* __restrict__ pred, const float* __restrict__ imp,
                                                            const int* __restrict__ table, int b, int Co, int td, int th, int tw,
                                                            float* __restrict__ acc, float* __restrict__ wsum, int64_t acc_elems) {
  const Geom g = load_geom(table);
  if (!geom_fits(g, Co, acc_elems)) return;
  const int* row = table + 4 * (1 + b);
  const int n = row[0], z0 = row[1], y0 = row[2], x0 = row[3];
  if (n < 0 || n >= g.N || z0 < 0 || y0 < 0 || x0 < 0 || z0 > g.D - td || y0 > g.H - th || x0 > g.W - tw) return;  // filler
  const int xw = tw / V;
  const int64_t items = (int64_t)Co * td * th * xw;
  const bool wide = V == 4 && ((x0 | g.W) & 3) == 0;
  const float* p = pred + (int64_t)b * Co * td * th * tw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i / xw;
    const int x = (int)(i - r * xw) * V;
    const int y = (int)(r % th);
    r /= th;
    const int z = (int)(r % td), c = (int)(r / td);
    const int64_t t_off = ((int64_t)z * th + y) * tw + x;            // inside imp (and, per channel, pred)
    const int64_t v_off = (((int64_t)(z0 + z)) * g.H + y0 + y) * g.W + x0 + x;  // inside one channel of the accumulator
    float* a = acc + ((int64_t)n * Co + c) * g.D * g.H * g.W + v_off;
    const bool weight = n == 0 && c == 0;
    if (V == 4 && wide) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(imp + t_off);
      const f32x4 q = *reinterpret_cast<const f32x4*>(p + i * V);
      f32x4 s = *reinterpret_cast<f32x4*>(a);
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = fmaf(w[k], q[k], s[k]);
      *reinterpret_cast<f32x4*>(a) = s;
      if (weight) {
        f32x4 u = *reinterpret_cast<f32x4*>(wsum + v_off);
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] += w[k];
        *reinterpret_cast<f32x4*>(wsum + v_off) = u;
      }
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float w = imp[t_off + k];
        a[k] = fmaf(w, p[i * V + k], a[k]);
        if (weight) wsum[v_off + k] += w;
      }
    }
  }
}

// ---- finish: out[n, c, v] = acc[n, c, v + pad] / wsum[v + pad], IEEE division
template <int V>
__global__ void __launch_bounds__(kThreads) k_sw_finish(const float* __restrict__ acc, const float* __restrict__ wsum, float* __restrict__ out,
                                                        int64_t NC, int D, int H, int W, int pd, int ph, int pw, int fd, int fh, int fw) {
  const int xw = fw / V;
  const int64_t items = NC * fd * fh * xw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i / xw;
    const int x = (int)(i - r * xw) * V;
    const int y = (int)(r % fh);
    r /= fh;
    const int z = (int)(r % fd);
    const int64_t nc = r / fd;
    const int64_t v_off = ((int64_t)(pd + z) * H + ph + y) * W + pw + x;
    const float* a = acc + nc * D * H * W + v_off;
    if (V == 4) {
      const f32x4 s = *reinterpret_cast<const f32x4*>(a), u = *reinterpret_cast<const f32x4*>(wsum + v_off);
      f32x4 q;
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = __fdiv_rn(s[k], u[k]);
      *reinterpret_cast<f32x4*>(out + i * V) = q;
    } else {
      out[i] = __fdiv_rn(a[0], wsum[v_off]);
    }
  }
}

// ================================================================ tiled diffusion sampling (inferer.py, `window_inferer=`)
// The voxel passes of one reverse-diffusion step whose model runs on windows of the training extent (MultiDiffusion, Bar-Tal et al.
// 2023; not part of the reference: PARITY UNPINNED).  The sample x and the accumulator are fp32 NCDHW, the model's input and output are
// NDHWC bf16 window batches; windows lie inside the case (no padding), anything else is a filler.
//   mi_sw_gather_cl       model input of a window batch, straight from x (and the concat condition)
//   mi_sw_accumulate_cl   acc[n, :, window] += imp * (guided) model output, one launch per row in stream order
//   mi_sw_diffusion_step  m = acc / wsum, the scheduler's update of x, acc = 0
// An item is four consecutive voxels along W: the fp32 side moves 16 bytes per access where origin, pitch and pointers allow; the
// bf16 side is the channel vector of each voxel (C + Cc <= a dozen, a runtime count), element by element as k_ncdhw_to_ndhwc does.

// a row's window lies inside the case
__device__ __forceinline__ bool window_inside(const Geom& g, const int* row, int rd, int rh, int rw) {
  return row[0] >= 0 && row[0] < g.N && row[1] >= 0 && row[2] >= 0 && row[3] >= 0 && row[1] <= g.D - rd && row[2] <= g.H - rh &&
         row[3] <= g.W - rw;
}

// ---- gather_cl: one item = V voxels along W of one (b, z, y) line of the window batch, every channel
template <int V>
__global__ void __launch_bounds__(kThreads) k_sw_gather_cl(const float* __restrict__ x, int64_t x_elems, int C, const float* __restrict__ cond,
                                                           int64_t cond_elems, int Cc, const int* __restrict__ table, int B, int halves, int rd,
                                                           int rh, int rw, bf16* __restrict__ out) {
  const Geom g = load_geom(table);
  const bool ok = geom_fits(g, C, x_elems) && (Cc == 0 || geom_fits(g, Cc, cond_elems));
  const int Ct = C + Cc, xw = rw / V;
  const int64_t items = (int64_t)B * rd * rh * xw;
  const int64_t half = items * V * Ct;                        // elements of one half of the model's batch
  const int64_t vol = ok ? (int64_t)g.D * g.H * g.W : 0;
  const bool rows4 = V == 4 && (g.W & 3) == 0;                // every line starts 16-byte aligned (the host checked the base pointers)
  const bf16 zero = f2bf(0.f);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i / xw;
    const int xx = (int)(i - r * xw) * V;
    const int y = (int)(r % rh);
    r /= rh;
    const int z = (int)(r % rd), b = (int)(r / rd);
    const int* row = table + 4 * (1 + b);
    const bool valid = ok && window_inside(g, row, rd, rh, rw);
    const int64_t src = valid ? ((int64_t)(row[1] + z) * g.H + row[2] + y) * g.W + row[3] + xx : 0;
    const bool wide = V == 4 && rows4 && ((row[3] + xx) & 3) == 0;
    bf16* dst = out + i * V * Ct;  // (b, z, y, xx) is voxel i * V of the batch
    for (int c = 0; c < Ct; ++c) {
      float v[V];
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = 0.f;
      if (valid) {
        const float* line = (c < C ? x + ((int64_t)row[0] * C + c) * vol : cond + ((int64_t)row[0] * Cc + (c - C)) * vol) + src;
        if (V == 4 && wide) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(line);
#pragma unroll
          for (int k = 0; k < V; ++k) v[k] = q[k];
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k) v[k] = line[k];
        }
      }
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const bf16 h = f2bf(v[k]);
        dst[k * Ct + c] = h;
        if (halves == 2) dst[half + k * Ct + c] = c < C ? h : zero;  // the null half: the sample again, zero condition channels
      }
    }
  }
}

// ---- accumulate_cl: the window of ONE row; one item = V voxels along W of one (z, y) line of the window, every channel; a row of
// image 0 also carries the weight sum when one is asked for.  pred NULL: the weight sum alone.  fmaf: one rounding per term.
template <int V, bool GUIDED>
__global__ void __launch_bounds__(kThreads) k_sw_accumulate_cl(const bf16* __restrict__ pred, const float* __restrict__ guidance,
                                                               const float* __restrict__ imp, const int* __restrict__ table, int b, int B, int Co,
                                                               int td, int th, int tw, float* __restrict__ acc, float* __restrict__ wsum,
                                                               int64_t acc_elems) {
  const Geom g = load_geom(table);
  if (!geom_fits(g, Co, acc_elems)) return;
  const int* row = table + 4 * (1 + b);
  if (!window_inside(g, row, td, th, tw)) return;  // filler: its predictions are not read
  const int n = row[0], z0 = row[1], y0 = row[2], x0 = row[3];
  const int xw = tw / V;
  const int64_t items = (int64_t)td * th * xw, vol = (int64_t)g.D * g.H * g.W, tvox = (int64_t)td * th * tw;
  const bool wide = V == 4 && ((x0 | g.W) & 3) == 0;
  const bf16* p = pred ? pred + (int64_t)b * tvox * Co : nullptr;
  const bf16* pu = GUIDED ? pred + (int64_t)(B + b) * tvox * Co : nullptr;  // the same window under the null condition
  const float wg = GUIDED ? guidance[0] : 0.f;
  const bool weight = wsum != nullptr && n == 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i / xw;
    const int xx = (int)(i - r * xw) * V;
    const int y = (int)(r % th), z = (int)(r / th);
    const int64_t t_off = i * V;                                                      // inside imp and, per voxel, pred
    const int64_t v_off = ((int64_t)(z0 + z) * g.H + y0 + y) * g.W + x0 + xx;          // inside one channel of the accumulator
    float w[V];
    if (V == 4) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(imp + t_off);
#pragma unroll
      for (int k = 0; k < V; ++k) w[k] = q[k];
    } else {
      w[0] = imp[t_off];
    }
    if (p) {
      for (int c = 0; c < Co; ++c) {
        float q[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
          q[k] = bf2f(p[(t_off + k) * Co + c]);
          if (GUIDED) q[k] = cfg_combine(q[k], bf2f(pu[(t_off + k) * Co + c]), wg);
        }
        float* a = acc + ((int64_t)n * Co + c) * vol + v_off;
        if (V == 4 && wide) {
          f32x4 s = *reinterpret_cast<f32x4*>(a);
#pragma unroll
          for (int k = 0; k < 4; ++k) s[k] = fmaf(w[k], q[k], s[k]);
          *reinterpret_cast<f32x4*>(a) = s;
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k) a[k] = fmaf(w[k], q[k], a[k]);
        }
      }
    }
    if (weight) {
      if (V == 4 && wide) {
        f32x4 u = *reinterpret_cast<f32x4*>(wsum + v_off);
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] += w[k];
        *reinterpret_cast<f32x4*>(wsum + v_off) = u;
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) wsum[v_off + k] += w[k];
      }
    }
  }
}

// ---- diffusion_step: one item = V consecutive elements of x (one (n, c) line when V == 4: the host asks for vol % 4 == 0);
// m = acc / wsum (IEEE division), then ddpm_update / ddim_update exactly as mi_diffusion_step applies them, acc = 0 for the next step
template <int V, bool DDIM>
__global__ void __launch_bounds__(kThreads) k_sw_diffusion_step(float* __restrict__ x, float* __restrict__ acc, const float* __restrict__ wsum,
                                                                const float* __restrict__ z, const float* __restrict__ table,
                                                                const int64_t* __restrict__ index, int64_t vol, int64_t items, int flags) {
  const float* k = table + index[0] * 5;
  const float k0 = k[0], k1 = k[1], k2 = k[2], k3 = k[3], k4 = k[4];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = i * V, v = s % vol;
    float a[V], u[V], xt[V], zl[V];
    if (V == 4) {
      const f32x4 qa = *reinterpret_cast<const f32x4*>(acc + s), qu = *reinterpret_cast<const f32x4*>(wsum + v),
                  qx = *reinterpret_cast<const f32x4*>(x + s);
      f32x4 qz = {0.f, 0.f, 0.f, 0.f};
      if (k4 != 0.f) qz = *reinterpret_cast<const f32x4*>(z + s);  // as the update itself: z is read only where its factor is not 0
#pragma unroll
      for (int j = 0; j < V; ++j) a[j] = qa[j], u[j] = qu[j], xt[j] = qx[j], zl[j] = qz[j];
    } else {
      a[0] = acc[s], u[0] = wsum[v], xt[0] = x[s], zl[0] = k4 != 0.f ? z[s] : 0.f;
    }
    float xn[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float m = __fdiv_rn(a[j], u[j]);
      xn[j] = DDIM ? ddim_update(xt[j], m, zl, j, k0, k1, k2, k3, k4, flags) : ddpm_update(xt[j], m, zl, j, k0, k1, k2, k3, k4, flags);
    }
    if (V == 4) {
      f32x4 q;
#pragma unroll
      for (int j = 0; j < V; ++j) q[j] = xn[j];
      *reinterpret_cast<f32x4*>(x + s) = q;
      *reinterpret_cast<f32x4*>(acc + s) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      x[s] = xn[0];
      acc[s] = 0.f;
    }
  }
}

// N * C * D * H * W <= elems on the host
inline bool host_fits(const int* g, int C, int64_t elems) {
  if (g[0] <= 0 || g[1] <= 0 || g[2] <= 0 || g[3] <= 0) return false;
  int64_t v = (int64_t)g[1] * g[2];
  if (v > elems / g[3]) return false;
  v *= g[3];
  if (v > elems / C) return false;
  v *= C;
  return v <= elems / g[0];
}
// every row of the host table is a filler (n < 0) or a window of extent t that lies inside the table's case
inline bool host_windows_inside(const int* host_table, int B, int td, int th, int tw) {
  const int ext[3] = {host_table[1], host_table[2], host_table[3]}, t[3] = {td, th, tw};
  for (int b = 0; b < B; ++b) {
    const int* row = host_table + 4 * (1 + b);
    if (row[0] < 0) continue;
    if (row[0] >= host_table[0]) return false;
    for (int a = 0; a < 3; ++a)
      if (row[1 + a] < 0 || row[1 + a] > ext[a] - t[a]) return false;
  }
  return true;
}

}  // namespace

extern "C" {

int mi_sw_gather(const float* image, int64_t image_elems, int C, const int* table, const int* host_table, int B, int rd, int rh, int rw, int mode,
                 float cval, float* tiles, hipStream_t st) {
  if (!image || !table || !tiles || image_elems <= 0 || C <= 0 || B <= 0 || rd <= 0 || rh <= 0 || rw <= 0) return MI_ERR_BAD_ARG;
  if (mode != MI_SW_PAD_CONSTANT && mode != MI_SW_PAD_REFLECT && mode != MI_SW_PAD_REPLICATE) return MI_ERR_BAD_ARG;
  if ((int64_t)B * C > INT64_MAX / rd / rh / rw) return MI_ERR_BAD_ARG;
  if (host_table) {
    if (!host_fits(host_table, C, image_elems)) return MI_ERR_BAD_ARG;
    const int ext[3] = {host_table[1], host_table[2], host_table[3]}, roi[3] = {rd, rh, rw};
    for (int b = 0; b < B; ++b) {
      const int* row = host_table + 4 * (1 + b);
      if (row[0] < 0) continue;  // filler
      if (row[0] >= host_table[0]) return MI_ERR_BAD_ARG;
      for (int a = 0; a < 3; ++a) {
        const int64_t o = row[1 + a], before = o < 0 ? -o : 0, after = o + roi[a] > ext[a] ? o + roi[a] - ext[a] : 0;
        if (mode == MI_SW_PAD_REFLECT && (before >= ext[a] || after >= ext[a])) return MI_ERR_BAD_ARG;
        if (o > INT_MAX - roi[a]) return MI_ERR_BAD_ARG;
      }
    }
  }
  const bool wide = (rw & 3) == 0 && aligned16(image) && aligned16(tiles);
  const int64_t items = (int64_t)B * C * rd * rh * (wide ? rw / 4 : rw);
  if (wide)
    hipLaunchKernelGGL(k_sw_gather<4>, dim3(grid_for(items)), dim3(kThreads), 0, st, image, image_elems, C, table, B, rd, rh, rw, mode, cval, tiles);
  else
    hipLaunchKernelGGL(k_sw_gather<1>, dim3(grid_for(items)), dim3(kThreads), 0, st, image, image_elems, C, table, B, rd, rh, rw, mode, cval, tiles);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_sw_accumulate(const float* pred, const float* imp, const int* table, const int* host_table, int B, int Co, int td, int th, int tw,
                     float* acc, float* wsum, int64_t acc_elems, hipStream_t st) {
  if (!pred || !imp || !table || !acc || !wsum || acc_elems <= 0 || B <= 0 || Co <= 0 || td <= 0 || th <= 0 || tw <= 0) return MI_ERR_BAD_ARG;
  if ((int64_t)B * Co > INT64_MAX / td / th / tw) return MI_ERR_BAD_ARG;
  if (host_table) {
    if (!host_fits(host_table, Co, acc_elems)) return MI_ERR_BAD_ARG;
    const int ext[3] = {host_table[1], host_table[2], host_table[3]}, t[3] = {td, th, tw};
    for (int b = 0; b < B; ++b) {
      const int* row = host_table + 4 * (1 + b);
      if (row[0] < 0) continue;  // filler
      if (row[0] >= host_table[0]) return MI_ERR_BAD_ARG;
      for (int a = 0; a < 3; ++a)
        if (row[1 + a] < 0 || row[1 + a] > ext[a] - t[a]) return MI_ERR_BAD_ARG;  // the window leaves the accumulator
    }
  }
  const bool wide = (tw & 3) == 0 && aligned16(pred) && aligned16(imp) && aligned16(acc) && aligned16(wsum);
  const int grid = grid_for((int64_t)Co * td * th * (wide ? tw / 4 : tw));
  for (int b = 0; b < B; ++b) {
    if (wide)
      hipLaunchKernelGGL(k_sw_accumulate<4>, dim3(grid), dim3(kThreads), 0, st, pred, imp, table, b, Co, td, th, tw, acc, wsum, acc_elems);
    else
      hipLaunchKernelGGL(k_sw_accumulate<1>, dim3(grid), dim3(kThreads), 0, st, pred, imp, table, b, Co, td, th, tw, acc, wsum, acc_elems);
    MI_CHECK_LAUNCH();
  }
  return 0;
}

int mi_sw_finish(const float* acc, const float* wsum, float* out, int N, int Co, int D, int H, int W, int pd, int ph, int pw, int fd, int fh, int fw,
                 hipStream_t st) {
  if (!acc || !wsum || !out || N <= 0 || Co <= 0 || D <= 0 || H <= 0 || W <= 0 || fd <= 0 || fh <= 0 || fw <= 0) return MI_ERR_BAD_ARG;
  if (pd < 0 || ph < 0 || pw < 0 || pd > D - fd || ph > H - fh || pw > W - fw) return MI_ERR_BAD_ARG;
  if ((int64_t)N * Co > INT64_MAX / D / H / W) return MI_ERR_BAD_ARG;
  const bool wide = ((fw | W | pw) & 3) == 0 && aligned16(acc) && aligned16(wsum) && aligned16(out);
  const int64_t NC = (int64_t)N * Co, items = NC * fd * fh * (wide ? fw / 4 : fw);
  if (wide)
    hipLaunchKernelGGL(k_sw_finish<4>, dim3(grid_for(items)), dim3(kThreads), 0, st, acc, wsum, out, NC, D, H, W, pd, ph, pw, fd, fh, fw);
  else
    hipLaunchKernelGGL(k_sw_finish<1>, dim3(grid_for(items)), dim3(kThreads), 0, st, acc, wsum, out, NC, D, H, W, pd, ph, pw, fd, fh, fw);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_sw_gather_cl(const float* x, int64_t x_elems, int C, const float* cond, int64_t cond_elems, int Cc, const int* table, const int* host_table,
                    int B, int guided, int rd, int rh, int rw, void* out, hipStream_t st) {
  if (!x || !table || !out || x_elems <= 0 || C <= 0 || Cc < 0 || B <= 0 || rd <= 0 || rh <= 0 || rw <= 0) return MI_ERR_BAD_ARG;
  if ((Cc > 0) != (cond != nullptr) || (Cc > 0 && cond_elems <= 0) || C > INT_MAX - Cc) return MI_ERR_BAD_ARG;
  if (2 * (int64_t)B * (C + Cc) > INT64_MAX / rd / rh / rw) return MI_ERR_BAD_ARG;
  if (host_table) {
    if (!host_fits(host_table, C, x_elems) || (Cc && !host_fits(host_table, Cc, cond_elems))) return MI_ERR_BAD_ARG;
    if (!host_windows_inside(host_table, B, rd, rh, rw)) return MI_ERR_BAD_ARG;
  }
  const bool wide = (rw & 3) == 0 && aligned16(x) && aligned16(cond);
  const int64_t items = (int64_t)B * rd * rh * (wide ? rw / 4 : rw);
  const int halves = guided ? 2 : 1;
  if (wide)
    hipLaunchKernelGGL(k_sw_gather_cl<4>, dim3(grid_for(items)), dim3(kThreads), 0, st, x, x_elems, C, cond, cond_elems, Cc, table, B, halves, rd,
                       rh, rw, (bf16*)out);
  else
    hipLaunchKernelGGL(k_sw_gather_cl<1>, dim3(grid_for(items)), dim3(kThreads), 0, st, x, x_elems, C, cond, cond_elems, Cc, table, B, halves, rd,
                       rh, rw, (bf16*)out);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_sw_accumulate_cl(const void* pred, const float* guidance, const float* imp, const int* table, const int* host_table, int B, int Co, int td,
                        int th, int tw, float* acc, float* wsum, int64_t acc_elems, hipStream_t st) {
  if (!imp || !table || !acc || acc_elems <= 0 || B <= 0 || Co <= 0 || td <= 0 || th <= 0 || tw <= 0) return MI_ERR_BAD_ARG;
  if ((!pred && !wsum) || (!pred && guidance)) return MI_ERR_BAD_ARG;  // nothing to do; no prediction to guide
  if (2 * (int64_t)B * Co > INT64_MAX / td / th / tw) return MI_ERR_BAD_ARG;
  if (host_table && (!host_fits(host_table, Co, acc_elems) || !host_windows_inside(host_table, B, td, th, tw))) return MI_ERR_BAD_ARG;
  const bool wide = (tw & 3) == 0 && aligned16(imp) && aligned16(acc) && aligned16(wsum);
  const int grid = grid_for((int64_t)td * th * (wide ? tw / 4 : tw));
  const bf16* p = (const bf16*)pred;
  auto kern = wide ? (guidance ? k_sw_accumulate_cl<4, true> : k_sw_accumulate_cl<4, false>)
                   : (guidance ? k_sw_accumulate_cl<1, true> : k_sw_accumulate_cl<1, false>);
  for (int b = 0; b < B; ++b) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), 0, st, p, guidance, imp, table, b, B, Co, td, th, tw, acc, wsum, acc_elems);
    MI_CHECK_LAUNCH();
  }
  return 0;
}

int mi_sw_diffusion_step(float* x, float* acc, const float* wsum, const float* noise, const float* table, const int64_t* index, int N, int C,
                         int64_t V, int flags, int ddim, hipStream_t st) {
  if (!x || !acc || !wsum || !noise || !table || !index || N <= 0 || C <= 0 || V <= 0) return MI_ERR_BAD_ARG;
  if ((int64_t)N * C > INT64_MAX / V) return MI_ERR_BAD_ARG;
  const int64_t total = (int64_t)N * C * V;
  const bool wide = (V & 3) == 0 && aligned16(x) && aligned16(acc) && aligned16(wsum) && aligned16(noise);
  const int64_t items = wide ? total / 4 : total;
  const dim3 grid(grid_for(items)), block(kThreads);
  auto kern = wide ? (ddim ? k_sw_diffusion_step<4, true> : k_sw_diffusion_step<4, false>)
                   : (ddim ? k_sw_diffusion_step<1, true> : k_sw_diffusion_step<1, false>);
  hipLaunchKernelGGL(kern, grid, block, 0, st, x, acc, wsum, noise, table, index, V, items, flags);
  MI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
