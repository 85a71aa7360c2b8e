// Case preprocessing on the device: the reference's planner stage that turns a raw case into a training case
// (medimgen/configuration.py: resample_image_label 1105-1167, crop_image_label 1048-1071, normalize_zscore_then_minmax 1204-1221,
// process_patient 1383-1430).  The reference runs it through scipy.ndimage.zoom in fp64 on the host; here every voxel pass is a
// kernel over fp32 buffers that are already resident:
//
//   mi_pp_prefilter3       cubic B-spline prefilter along one axis of a contiguous [A][n][B] view (gain 6, pole sqrt(3) - 2, whole-
//                          sample mirror), out of place
//   mi_pp_resample_axis    out[a][o][b] = sum_k w[o][k] * src[a][idx[o][k]][b]: the per-output taps are built on the host in fp64
//                          (order 0: one tap, a pure gather with scipy's index choice; order 1: two; order 3: four on the
//                          prefiltered coefficients, mirrored indices resolved on the host)
//   mi_pp_resample_labels  separable order-1 / order-0 scores of every `label == value` indicator, argmax, uint8 -- no one-hot volume
//   mi_pp_nonzero_box      per-axis min / max index of x != 0 over all channels -> six ints on the device
//   mi_pp_box_stats        per channel sum, sum of squares (fp64 fold, as validation.hip), min, max inside the box
//   mi_pp_finish_image     crop + (x, y, z, c) -> (c, z, y, x) + normalise, tiled through LDS; mi_pp_finish_label: the same for uint8
//
// All of it is memory-bound.  Layout decides the kernels: with B > 1 lanes run across B (coalesced) and each lane marches its own
// line; with B == 1 (lines contiguous) a wave stages 64 lines x 64 samples through LDS, so global traffic is 256-byte rows and the
// recursion walks LDS columns (row pitch 65: conflict-free), carrying its state from chunk to chunk in registers.
#include "common.h"
#include "medimgen_hip.h"

#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr float kPole = -0.26794919243112270647f;                  // sqrt(3) - 2
constexpr float kAnti = kPole / (kPole * kPole - 1.0f);            // z / (z^2 - 1)
constexpr int kTile = 64;                                          // lines per wave and samples per chunk of the row kernel
constexpr int kRowThreads = 128;                                   // two waves: 2 x 64 x 65 floats of LDS
constexpr int kStatBlocks = 256;                                   // partials per channel of mi_pp_box_stats

inline int grid_for(int64_t work, int cap) {
  int64_t g = (work + kThreads - 1) / kThreads;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---- prefilter, B > 1: one lane per (a, b) column, stride B between samples.  Forward: c[0] = 6 * sum_k w0[k] x[k] (the mirror sum,
// exact for n <= n_init, truncated where |z|^k is far below fp32 resolution otherwise), c[i] = 6 x[i] + z c[i-1]; backward in place
// (this thread reads what it wrote): c[n-1] = z / (z^2 - 1) * (c[n-1] + z c[n-2]), c[i] = z (c[i+1] - c[i]).
__global__ void k_prefilter_cols(const float* __restrict__ x, float* __restrict__ c, int64_t cols, int n, int64_t B, const float* __restrict__ w0,
                                 int n_init) {
  const int64_t col = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (col >= cols) return;
  const int64_t a = col / B, base = a * n * B + (col - a * B);
  const float* xs = x + base;
  float* cs = c + base;
  float s = 0.f;
  for (int k = 0; k < n_init; ++k) s = fmaf(w0[k], xs[k * B], s);
  float prev = 6.0f * s, prev2 = 0.f;
  cs[0] = prev;
  int i = 1;
  for (; i + 4 <= n; i += 4) {  // the four loads do not depend on the recursion
    const float v0 = xs[i * B], v1 = xs[(i + 1) * B], v2 = xs[(i + 2) * B], v3 = xs[(i + 3) * B];
    const float c0 = fmaf(kPole, prev, 6.0f * v0), c1 = fmaf(kPole, c0, 6.0f * v1), c2 = fmaf(kPole, c1, 6.0f * v2),
                c3 = fmaf(kPole, c2, 6.0f * v3);
    cs[i * B] = c0, cs[(i + 1) * B] = c1, cs[(i + 2) * B] = c2, cs[(i + 3) * B] = c3;
    prev2 = c2, prev = c3;
  }
  for (; i < n; ++i) {
    prev2 = prev;
    prev = fmaf(kPole, prev, 6.0f * xs[i * B]);
    cs[i * B] = prev;
  }
  float next = kAnti * fmaf(kPole, prev2, prev);
  cs[(int64_t)(n - 1) * B] = next;
  i = n - 2;
  for (; i >= 3; i -= 4) {
    const float v0 = cs[i * B], v1 = cs[(i - 1) * B], v2 = cs[(i - 2) * B], v3 = cs[(i - 3) * B];
    const float c0 = kPole * (next - v0), c1 = kPole * (c0 - v1), c2 = kPole * (c1 - v2), c3 = kPole * (c2 - v3);
    cs[i * B] = c0, cs[(i - 1) * B] = c1, cs[(i - 2) * B] = c2, cs[(i - 3) * B] = c3;
    next = c3;
  }
  for (; i >= 0; --i) {
    next = kPole * (next - cs[i * B]);
    cs[i * B] = next;
  }
}

// ---- prefilter, B == 1: lines are contiguous.  A wave owns 64 lines; per chunk of 64 samples it loads 64 rows of 256 bytes into its
// LDS tile, lane l marches line l through the tile, and the tile goes back as 256-byte rows.  The same lane stores and later reloads
// every address of c, so the backward sweep needs no fence.  n_init <= 64: the mirror sum reads the first chunk only.
__global__ void __launch_bounds__(kRowThreads) k_prefilter_rows(const float* __restrict__ x, float* __restrict__ c, int64_t lines, int n,
                                                             const float* __restrict__ w0, int n_init) {
  __shared__ float tiles[kRowThreads / kTile][kTile][kTile + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float(*tile)[kTile + 1] = tiles[wave];
  const int64_t line0 = ((int64_t)blockIdx.x * (kRowThreads / kTile) + wave) * kTile;
  const int rows = (int)(lines - line0 < kTile ? (lines - line0 < 0 ? 0 : lines - line0) : kTile);
  const int chunks = (n + kTile - 1) / kTile;
  float prev = 0.f, prev2 = 0.f;
  for (int ch = 0; ch < chunks; ++ch) {
    const int j0 = ch * kTile, len = n - j0 < kTile ? n - j0 : kTile;
    if (lane < len)
      for (int r = 0; r < rows; ++r) tile[r][lane] = x[(line0 + r) * n + j0 + lane];
    __syncthreads();
    if (lane < rows) {
      int j = 0;
      if (ch == 0) {
        float s = 0.f;
        for (int k = 0; k < n_init; ++k) s = fmaf(w0[k], tile[lane][k], s);
        prev = 6.0f * s;
        tile[lane][0] = prev;
        j = 1;
      }
      for (; j < len; ++j) {
        prev2 = prev;
        prev = fmaf(kPole, prev, 6.0f * tile[lane][j]);
        tile[lane][j] = prev;
      }
    }
    __syncthreads();
    if (lane < len)
      for (int r = 0; r < rows; ++r) c[(line0 + r) * n + j0 + lane] = tile[r][lane];
    __syncthreads();
  }
  float next = 0.f;
  for (int ch = chunks - 1; ch >= 0; --ch) {
    const int j0 = ch * kTile, len = n - j0 < kTile ? n - j0 : kTile;
    if (lane < len)
      for (int r = 0; r < rows; ++r) tile[r][lane] = c[(line0 + r) * n + j0 + lane];
    __syncthreads();
    if (lane < rows) {
      int j = len - 1;
      if (ch == chunks - 1) {  // prev, prev2 = the forward sweep's c[n-1], c[n-2]
        next = kAnti * fmaf(kPole, prev2, prev);
        tile[lane][j] = next;
        --j;
      }
      for (; j >= 0; --j) {
        next = kPole * (next - tile[lane][j]);
        tile[lane][j] = next;
      }
    }
    __syncthreads();
    if (lane < len)
      for (int r = 0; r < rows; ++r) c[(line0 + r) * n + j0 + lane] = tile[r][lane];
    __syncthreads();
  }
}

// ---- interpolation: one output element per thread-step, b fastest (B == 1: o fastest, neighbouring lanes read neighbouring samples)
template <int NT>
__global__ void k_resample_taps(const float* __restrict__ src, float* __restrict__ dst, int64_t total, int n, int n_out, int64_t B,
                                const int* __restrict__ idx, const float* __restrict__ w) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ao = i / B, b = i - ao * B, a = ao / n_out;
    const int o = (int)(ao - a * n_out);
    const float* s = src + a * n * B + b;
    float v;
    if (NT == 1) {
      v = s[idx[o * 4] * B];
    } else {
      v = w[o * 4] * s[idx[o * 4] * B];
#pragma unroll
      for (int k = 1; k < NT; ++k) v = fmaf(w[o * 4 + k], s[idx[o * 4 + k] * B], v);
    }
    dst[i] = v;
  }
}

// ---- labels: per output voxel the trilinear (or nearest along a low-resolution axis: second weight 0) score of every value's
// indicator, from the eight corner labels; argmax with ties to the lowest index (values ascending), as np.argmax
__global__ void k_resample_labels(const float* __restrict__ lab, uint8_t* __restrict__ out, const float* __restrict__ values, int nv, int Y,
                                  int Z, int Xo, int Yo, int Zo, const int* __restrict__ ix, const float* __restrict__ wx,
                                  const int* __restrict__ iy, const float* __restrict__ wy, const int* __restrict__ iz,
                                  const float* __restrict__ wz) {
  __shared__ float vals[32];
  if ((int)threadIdx.x < nv) vals[threadIdx.x] = values[threadIdx.x];
  __syncthreads();
  const int64_t total = (int64_t)Xo * Yo * Zo;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t xy = i / Zo;
    const int oz = (int)(i - xy * Zo), ox = (int)(xy / Yo), oy = (int)(xy - (int64_t)ox * Yo);
    float l[8], w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int kx = k >> 2, ky = (k >> 1) & 1, kz = k & 1;
      l[k] = lab[((int64_t)ix[ox * 2 + kx] * Y + iy[oy * 2 + ky]) * Z + iz[oz * 2 + kz]];
      w[k] = (wx[ox * 2 + kx] * wy[oy * 2 + ky]) * wz[oz * 2 + kz];
    }
    float best = -1.f;
    int arg = 0;
    for (int v = 0; v < nv; ++v) {
      const float val = vals[v];
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) s += l[k] == val ? w[k] : 0.f;
      if (s > best) best = s, arg = v;
    }
    out[i] = (uint8_t)vals[arg];
  }
}

// ---- non-zero box
__global__ void k_box_init(int* __restrict__ box) {
  if (threadIdx.x < 6) box[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : -1;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}
// per-thread extents over a grid-stride sweep, wave butterfly, one atomic per wave and bound
__global__ void k_nonzero_box(const float* __restrict__ x, int64_t total, int Y, int Z, int C, int* __restrict__ box) {
  int lo0 = INT_MAX, lo1 = INT_MAX, lo2 = INT_MAX, hi0 = -1, hi1 = -1, hi2 = -1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (x[i] != 0.f) {
      const int64_t vox = i / C, xy = vox / Z;
      const int z = (int)(vox - xy * Z), px = (int)(xy / Y), py = (int)(xy - (int64_t)px * Y);
      lo0 = min(lo0, px), hi0 = max(hi0, px);
      lo1 = min(lo1, py), hi1 = max(hi1, py);
      lo2 = min(lo2, z), hi2 = max(hi2, z);
    }
  }
  lo0 = wave_min_i(lo0), lo1 = wave_min_i(lo1), lo2 = wave_min_i(lo2);
  hi0 = wave_max_i(hi0), hi1 = wave_max_i(hi1), hi2 = wave_max_i(hi2);
  if ((threadIdx.x & 63) == 0 && hi0 >= 0) {
    atomicMin(box + 0, lo0), atomicMin(box + 1, lo1), atomicMin(box + 2, lo2);
    atomicMax(box + 3, hi0), atomicMax(box + 4, hi1), atomicMax(box + 5, hi2);
  }
}

// ---- channel statistics inside the box: blockIdx.y = channel; every term enters its thread's fp64 partial exactly
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__global__ void __launch_bounds__(kThreads) k_box_stats(const float* __restrict__ x, int Y, int Z, int C, int x0, int y0, int z0, int ny, int nz,
                                                        int64_t nvox, double* __restrict__ partials) {
  __shared__ double red[4][4];
  const int c = blockIdx.y;
  double s = 0.0, q = 0.0;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t xy = i / nz;
    const int z = (int)(i - xy * nz), px = (int)(xy / ny), py = (int)(xy - (int64_t)px * ny);
    const float v = x[((((int64_t)(x0 + px) * Y) + y0 + py) * Z + z0 + z) * C + c];
    s += (double)v;
    q += (double)v * (double)v;
    lo = fminf(lo, v), hi = fmaxf(hi, v);
  }
  s = wave_sum_f64(s), q = wave_sum_f64(q);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lo = fminf(lo, __shfl_xor(lo, off, 64)), hi = fmaxf(hi, __shfl_xor(hi, off, 64));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave][0] = s, red[wave][1] = q, red[wave][2] = (double)lo, red[wave][3] = (double)hi;
  __syncthreads();
  if (threadIdx.x == 0) {
    double* p = partials + ((int64_t)c * gridDim.x + blockIdx.x) * 4;
    p[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    p[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    p[2] = fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]));
    p[3] = fmax(fmax(red[0][3], red[1][3]), fmax(red[2][3], red[3][3]));
  }
}
// fold the partials of channel blockIdx.x in a fixed order -> stats[c] = {sum, sum of squares, min, max}
__global__ void __launch_bounds__(kThreads) k_box_stats_fold(const double* __restrict__ partials, int nparts, double* __restrict__ stats) {
  __shared__ double red[kThreads][4];
  const double* p = partials + (int64_t)blockIdx.x * nparts * 4;
  double s = 0.0, q = 0.0, lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < nparts; i += kThreads) s += p[i * 4], q += p[i * 4 + 1], lo = fmin(lo, p[i * 4 + 2]), hi = fmax(hi, p[i * 4 + 3]);
  red[threadIdx.x][0] = s, red[threadIdx.x][1] = q, red[threadIdx.x][2] = lo, red[threadIdx.x][3] = hi;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[threadIdx.x][0] += red[threadIdx.x + o][0];
      red[threadIdx.x][1] += red[threadIdx.x + o][1];
      red[threadIdx.x][2] = fmin(red[threadIdx.x][2], red[threadIdx.x + o][2]);
      red[threadIdx.x][3] = fmax(red[threadIdx.x][3], red[threadIdx.x + o][3]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) stats[blockIdx.x * 4 + threadIdx.x] = red[0][threadIdx.x];
}

// ---- finishing pass: in (x, y, z, c) inside the box -> out (c, z, y, x).  A 32 x 32 (x, z) tile per (y, c): rows of z in, rows of x
// out, through LDS with pitch 33.  NORM: out = (v - lo[c]) * inv[c], which is normalize_zscore_then_minmax with the mean and the
// standard deviation cancelled ((z - z_min) / (z_max - z_min) = (v - min) / (max - min)).
template <typename T, bool NORM>
__global__ void __launch_bounds__(kThreads) k_finish(const T* __restrict__ in, T* __restrict__ out, int Y, int Z, int C, int x0, int y0, int z0,
                                                     int nx, int ny, int nz, const float* __restrict__ lo_inv) {
  __shared__ T tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int xb = blockIdx.x * 32, zb = blockIdx.y * 32;
  for (int yc = blockIdx.z; yc < ny * C; yc += gridDim.z) {
    const int y = yc / C, c = yc - y * C;
    for (int r = ty; r < 32; r += 8) {
      const int px = xb + r, pz = zb + tx;
      if (px < nx && pz < nz) tile[r][tx] = in[((((int64_t)(x0 + px) * Y) + y0 + y) * Z + z0 + pz) * C + c];
    }
    __syncthreads();
    float lo = 0.f, inv = 1.f;
    if (NORM) lo = lo_inv[c * 2], inv = lo_inv[c * 2 + 1];
    for (int r = ty; r < 32; r += 8) {
      const int pz = zb + r, px = xb + tx;
      if (px < nx && pz < nz) {
        T v = tile[tx][r];
        if (NORM) v = (T)fminf(((float)v - lo) * inv, 1.0f);  // lo is the exact minimum; the rounded 1 / (max - min) may overshoot 1 by an ulp
        out[(((int64_t)c * nz + pz) * ny + y) * nx + px] = v;
      }
    }
    __syncthreads();
  }
}

inline bool box_ok(int X, int Y, int Z, int x0, int y0, int z0, int nx, int ny, int nz) {
  return X > 0 && Y > 0 && Z > 0 && x0 >= 0 && y0 >= 0 && z0 >= 0 && nx > 0 && ny > 0 && nz > 0 && x0 <= X - nx && y0 <= Y - ny && z0 <= Z - nz;
}
template <typename T, bool NORM>
int finish_launch(const T* in, T* out, int X, int Y, int Z, int C, int x0, int y0, int z0, int nx, int ny, int nz, const float* lo_inv,
                  hipStream_t st) {
  if (!in || !out || C <= 0 || (NORM && !lo_inv) || !box_ok(X, Y, Z, x0, y0, z0, nx, ny, nz)) return MI_ERR_BAD_ARG;
  const int64_t gy = (nz + 31) / 32, gz = (int64_t)ny * C;
  if (gy > 65535) return MI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((k_finish<T, NORM>), dim3((nx + 31) / 32, (int)gy, (int)(gz > 65535 ? 65535 : gz)), dim3(kThreads), 0, st, in, out, Y, Z, C,
                     x0, y0, z0, nx, ny, nz, lo_inv);
  MI_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

int mi_pp_prefilter3(const float* x, float* c, int64_t A, int n, int64_t B, const float* init_w, int n_init, hipStream_t st) {
  if (!x || !c || x == c || !init_w || A <= 0 || n < 2 || B <= 0 || n_init < 1 || n_init > n || n_init > kTile) return MI_ERR_BAD_ARG;
  if (A > INT64_MAX / n / B) return MI_ERR_BAD_ARG;
  if (B == 1) {
    const int64_t blocks = (A + kRowThreads - 1) / kRowThreads;  // one line per thread
    if (blocks > INT_MAX) return MI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_prefilter_rows, dim3((int)blocks), dim3(kRowThreads), 0, st, x, c, A, n, init_w, n_init);
  } else {
    const int64_t cols = A * B, blocks = (cols + kThreads - 1) / kThreads;
    if (blocks > INT_MAX) return MI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_prefilter_cols, dim3((int)blocks), dim3(kThreads), 0, st, x, c, cols, n, B, init_w, n_init);
  }
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_pp_resample_axis(const float* src, float* dst, int64_t A, int n, int n_out, int64_t B, const int* tap_idx, const float* tap_w, int ntaps,
                        hipStream_t st) {
  if (!src || !dst || src == dst || !tap_idx || !tap_w || A <= 0 || n <= 0 || n_out <= 0 || B <= 0) return MI_ERR_BAD_ARG;
  if (ntaps != 1 && ntaps != 2 && ntaps != 4) return MI_ERR_BAD_ARG;
  const int nmax = n > n_out ? n : n_out;
  if (A > INT64_MAX / nmax / B) return MI_ERR_BAD_ARG;
  const int64_t total = A * n_out * B;
  const int grid = grid_for(total, 1 << 16);
#define MI_PP_TAPS(nt) \
  hipLaunchKernelGGL(k_resample_taps<nt>, dim3(grid), dim3(kThreads), 0, st, src, dst, total, n, n_out, B, tap_idx, tap_w)
  if (ntaps == 1) MI_PP_TAPS(1);
  else if (ntaps == 2) MI_PP_TAPS(2);
  else MI_PP_TAPS(4);
#undef MI_PP_TAPS
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_pp_resample_labels(const float* label, uint8_t* out, const float* values, int nvalues, int X, int Y, int Z, int Xo, int Yo, int Zo,
                          const int* ix, const float* wx, const int* iy, const float* wy, const int* iz, const float* wz, hipStream_t st) {
  if (!label || !out || !values || !ix || !wx || !iy || !wy || !iz || !wz) return MI_ERR_BAD_ARG;
  if (X <= 0 || Y <= 0 || Z <= 0 || Xo <= 0 || Yo <= 0 || Zo <= 0 || nvalues < 1) return MI_ERR_BAD_ARG;
  if (nvalues > 32) return MI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_resample_labels, dim3(grid_for((int64_t)Xo * Yo * Zo, 1 << 16)), dim3(kThreads), 0, st, label, out, values, nvalues, Y, Z,
                     Xo, Yo, Zo, ix, wx, iy, wy, iz, wz);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_pp_nonzero_box(const float* x, int X, int Y, int Z, int C, int* box, hipStream_t st) {
  if (!x || !box || X <= 0 || Y <= 0 || Z <= 0 || C <= 0) return MI_ERR_BAD_ARG;
  const int64_t total = (int64_t)X * Y * Z * C;
  hipLaunchKernelGGL(k_box_init, dim3(1), dim3(64), 0, st, box);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_nonzero_box, dim3(grid_for(total, 4096)), dim3(kThreads), 0, st, x, total, Y, Z, C, box);
  MI_CHECK_LAUNCH();
  return 0;
}

int64_t mi_pp_stats_workspace_bytes(int C) { return C > 0 ? (int64_t)sizeof(double) * 4 * kStatBlocks * C : 0; }

int mi_pp_box_stats(const float* x, int X, int Y, int Z, int C, int x0, int y0, int z0, int nx, int ny, int nz, double* stats, double* workspace,
                    hipStream_t st) {
  if (!x || !stats || !workspace || C <= 0 || C > 65535 || ((uintptr_t)stats & 7) || ((uintptr_t)workspace & 7)) return MI_ERR_BAD_ARG;
  if (!box_ok(X, Y, Z, x0, y0, z0, nx, ny, nz)) return MI_ERR_BAD_ARG;
  const int64_t nvox = (int64_t)nx * ny * nz;
  const int grid = grid_for(nvox, kStatBlocks);
  hipLaunchKernelGGL(k_box_stats, dim3(grid, C), dim3(kThreads), 0, st, x, Y, Z, C, x0, y0, z0, ny, nz, nvox, workspace);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_box_stats_fold, dim3(C), dim3(kThreads), 0, st, workspace, grid, stats);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_pp_finish_image(const float* x, float* out, int X, int Y, int Z, int C, int x0, int y0, int z0, int nx, int ny, int nz, const float* lo_inv,
                       hipStream_t st) {
  return finish_launch<float, true>(x, out, X, Y, Z, C, x0, y0, z0, nx, ny, nz, lo_inv, st);
}

int mi_pp_finish_label(const uint8_t* label, uint8_t* out, int X, int Y, int Z, int x0, int y0, int z0, int nx, int ny, int nz, hipStream_t st) {
  return finish_launch<uint8_t, false>(label, out, X, Y, Z, 1, x0, y0, z0, nx, ny, nz, nullptr, st);
}

}  // extern "C"
