// Forward-only loss reductions of the validation loops (train_ldm.LDM.validate_epoch, T-LDM:193-239;
// train_autoencoder.AutoEncoder.validate_one_epoch, T-AE:438-467; adapt_kl_loss_weight, T-AE:295-328): the value mi_mse_fwd_bwd /
// mi_l1_fwd_bwd / mi_reparam_kl_fwd put in *loss, without a gradient tensor or z, and the epoch's running mean kept on the device.
//
// All three are streaming reductions (HBM-bound): 16-byte loads on both operands, grid-stride loop, fp32 sums over chains of 8
// elements folded into an fp64 per-thread partial, fp64 wave butterfly, ONE fp64 partial per workgroup stored into the meter block,
// and a second one-workgroup launch that folds the partials in a fixed order and updates {last, sum, count}.  No float atomics: the
// value does not depend on the order workgroups arrive in, so a replayed graph is bit-reproducible.  The kernel boundary between the
// two launches is the cross-workgroup hand-off (no fences, no flags).
#include "common.h"
#include "medimgen_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = MI_METER_PARTIALS;

inline int blocks_for(int64_t work) {
  int64_t g = (work + kThreads - 1) / kThreads;
  return (int)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// this workgroup's partial -> partials[blockIdx.x]; blockDim.x == 256, `red` = 4 doubles of LDS
__device__ __forceinline__ void store_block_partial(double v, double* red, double* __restrict__ partials) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// pred NDHWC bf16, target NCDHW fp32; V % 8 == 0 and both bases 16-byte aligned: one item = 8 consecutive voxels of one sample =
// C 16-byte loads of pred and, per channel, two 16-byte loads of target.  L1: sum |d|, else sum d^2.
template <int C, bool L1>
__global__ void k_eval_vec(const u32x4* __restrict__ pred, const float* __restrict__ target, double* __restrict__ partials, int64_t V,
                           int64_t items) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t vox = i * 8, n = vox / V, v = vox - n * V;
    float p[8 * C];  // [voxel j][channel c]
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const F8 f = unpack8(pred[i * C + k]);
#pragma unroll
      for (int j = 0; j < 8; ++j) p[8 * k + j] = f.v[j];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const f32x4* t = (const f32x4*)(target + (n * C + c) * V + v);
      const f32x4 t0 = t[0], t1 = t[1];
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = p[j * C + c] - (j < 4 ? t0[j & 3] : t1[j & 3]);
        s += L1 ? fabsf(d) : d * d;
      }
      acc += (double)s;
    }
  }
  store_block_partial(acc, red, partials);
}
// any C, V and alignment: one voxel per thread-step, like k_mse / k_l1
template <bool L1>
__global__ void k_eval_scalar(const bf16* __restrict__ pred, const float* __restrict__ target, double* __restrict__ partials, int C, int64_t V,
                              int64_t total) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / V, v = i - n * V;
    for (int c = 0; c < C; ++c) {
      const float d = bf2f(pred[i * C + c]) - target[(n * C + c) * V + v];
      acc += (double)(L1 ? fabsf(d) : d * d);
    }
  }
  store_block_partial(acc, red, partials);
}

// 0.5 * (mu^2 + sigma^2 - log(sigma^2) - 1) per element (T-AE:68-72), in fp64 at fp32 cost: the square of a bf16 is exact in fp32,
// and log(sigma^2) = 2 * ((e - 127) ln 2 + log(1 + k / 128)) for sigma = 2^(e-127) (1 + k/128) -- a bf16 has 7 mantissa bits, so the
// logarithm is one lookup in a 128-entry fp64 table (built per workgroup) and one fma.  The terms cancel near mu = 0, sigma = 1,
// which is where a trained encoder puts them; fp32 logf there leaves ~1e-7 absolute per term.
__device__ __forceinline__ double kl_term(float m, float s, const double* tab) {
  const uint32_t b = __float_as_uint(s) & 0x7fffffffu;
  const int e = (int)(b >> 23), k = (int)(b >> 16) & 0x7f;
  const double lg = (e == 0 || e == 255) ? log((double)__uint_as_float(b))  // zero / subnormal / inf / nan: the library's answer
                                         : (double)(e - 127) * 0.6931471805599453 + tab[k];
  return 0.5 * ((double)(m * m) + (double)(s * s) - 2.0 * lg - 1.0);
}
// mu, sigma: bf16, same (channels-last) layout, so the sum runs over the flat buffers: n8 16-byte items, then the scalar tail
__global__ void k_kl_eval(const bf16* __restrict__ mu, const bf16* __restrict__ sigma, double* __restrict__ partials, int64_t n8, int64_t total) {
  __shared__ double red[4];
  __shared__ double tab[128];
  if (threadIdx.x < 128) tab[threadIdx.x] = log(1.0 + (double)threadIdx.x / 128.0);
  __syncthreads();
  double acc = 0.0;
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
  const u32x4* mu8 = (const u32x4*)mu;
  const u32x4* sg8 = (const u32x4*)sigma;
  for (int64_t i = gid; i < n8; i += gstride) {
    const F8 m = unpack8(mu8[i]), s = unpack8(sg8[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += kl_term(m.v[j], s.v[j], tab);
  }
  for (int64_t i = n8 * 8 + gid; i < total; i += gstride) acc += kl_term(bf2f(mu[i]), bf2f(sigma[i]), tab);
  store_block_partial(acc, red, partials);
}

// fold the workgroup partials in a fixed order; last = sum * scale, sum += last, count += 1
__global__ void k_meter_finalize(double* __restrict__ acc, int nparts, double scale) {
  __shared__ double red[kThreads];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) s += acc[MI_METER_HEADER + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double loss = red[0] * scale;
    acc[0] = loss;
    acc[1] += loss;
    acc[2] += 1.0;
  }
}
__global__ void k_meter_reset(double* __restrict__ acc) {
  if (threadIdx.x < MI_METER_HEADER) acc[threadIdx.x] = 0.0;
}

template <bool L1>
int eval_launch(const void* pred, const float* target, double* acc, int N, int C, int64_t V, hipStream_t st) {
  if (!pred || !target || !acc || N <= 0 || C <= 0 || V <= 0 || ((uintptr_t)acc & 7)) return MI_ERR_BAD_ARG;
  const int64_t total = (int64_t)N * V;
  double* partials = acc + MI_METER_HEADER;
  int grid;
  const bool vec = V % 8 == 0 && aligned16(pred) && aligned16(target) && (C <= 4 || C == 8);
  if (vec) {
    const int64_t items = total / 8;
    grid = blocks_for(items);
    const u32x4* p = (const u32x4*)pred;
#define MI_EVAL_CASE(c) \
  case c: hipLaunchKernelGGL((k_eval_vec<c, L1>), dim3(grid), dim3(kThreads), 0, st, p, target, partials, V, items); break;
    switch (C) {
      MI_EVAL_CASE(1)
      MI_EVAL_CASE(2)
      MI_EVAL_CASE(3)
      MI_EVAL_CASE(4)
      MI_EVAL_CASE(8)
    }
#undef MI_EVAL_CASE
  } else {
    grid = blocks_for(total);
    hipLaunchKernelGGL(k_eval_scalar<L1>, dim3(grid), dim3(kThreads), 0, st, (const bf16*)pred, target, partials, C, V, total);
  }
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_meter_finalize, dim3(1), dim3(kThreads), 0, st, acc, grid, 1.0 / ((double)total * C));
  MI_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

int64_t mi_meter_bytes(void) { return (int64_t)sizeof(double) * (MI_METER_HEADER + MI_METER_PARTIALS); }

int mi_meter_reset(double* acc, hipStream_t st) {
  if (!acc || ((uintptr_t)acc & 7)) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_meter_reset, dim3(1), dim3(64), 0, st, acc);
  MI_CHECK_LAUNCH();
  return 0;
}
int mi_mse_eval(const void* pred, const float* target, double* acc, int N, int C, int64_t V, hipStream_t st) {
  return eval_launch<false>(pred, target, acc, N, C, V, st);
}
int mi_l1_eval(const void* pred, const float* target, double* acc, int N, int C, int64_t V, hipStream_t st) {
  return eval_launch<true>(pred, target, acc, N, C, V, st);
}
int mi_kl_eval(const void* mu, const void* sigma, double* acc, int N, int C, int64_t V, hipStream_t st) {
  if (!mu || !sigma || !acc || N <= 0 || C <= 0 || V <= 0 || ((uintptr_t)acc & 7)) return MI_ERR_BAD_ARG;
  const int64_t total = (int64_t)N * V * C;
  const int64_t n8 = (aligned16(mu) && aligned16(sigma)) ? total / 8 : 0;
  const int grid = blocks_for(n8 > 0 ? n8 : total);
  hipLaunchKernelGGL(k_kl_eval, dim3(grid), dim3(kThreads), 0, st, (const bf16*)mu, (const bf16*)sigma, acc + MI_METER_HEADER, n8, total);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_meter_finalize, dim3(1), dim3(kThreads), 0, st, acc, grid, 1.0 / (double)N);
  MI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
