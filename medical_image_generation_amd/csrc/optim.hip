// Fused optimizer over the flat fp32 parameter arena: global grad-norm (clip_grad_norm_, T-LDM:177) + Adam / AdamW
// (torch.optim defaults, T-LDM:121, T-AE:470, T-DDPM:383) in two launches instead of ~8 elementwise ops x 332 tensors.
// HBM-bound: 4 arrays read + 3 written, 16-byte accesses.  Step count and clip norm live in device memory so the
// whole train step can be captured in a hipGraph and replayed.
#include "common.h"
#include "medimgen_hip.h"

namespace {

__global__ void __launch_bounds__(256) k_sumsq(const f32x4* __restrict__ x, int64_t n4, const float* __restrict__ tail, int ntail,
                                               float* __restrict__ out) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 v = x[i];
    acc += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) acc += tail[threadIdx.x] * tail[threadIdx.x];
  float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) atomicAdd(out, s);
}

struct AdamArgs {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  float lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale;
  int decoupled;
  const float* sumsq;  // may be null: no clipping
  const float* step;   // device scalar holding the 1-based step count (already incremented)
};

__global__ void __launch_bounds__(256) k_adam(AdamArgs a) {
  const float t = *a.step;
  const float bc1 = 1.f - powf(a.beta1, t), bc2 = 1.f - powf(a.beta2, t);
  const float step_size = a.lr / bc1, inv_sqrt_bc2 = rsqrtf(bc2);
  // grad_scale: the gradient buffer holds grad_scale^-1 times the gradient (a SUM all-reduce over `world` ranks with
  // grad_scale = 1/world is the data-parallel mean); the norm of the true gradient is grad_scale * sqrt(sumsq)
  float clip = a.grad_scale;
  if (a.sumsq) {  // torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to 1
    float c = a.max_norm / (a.grad_scale * sqrtf(*a.sumsq) + 1e-6f);
    clip = (c < 1.f ? c : 1.f) * a.grad_scale;
  }
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
    float p = a.p[i], g = a.g[i] * clip, m = a.m[i], v = a.v[i];
    if (a.decoupled)
      p *= 1.f - a.lr * a.weight_decay;
    else
      g += a.weight_decay * p;
    m = a.beta1 * m + (1.f - a.beta1) * g;
    v = a.beta2 * v + (1.f - a.beta2) * g * g;
    p -= step_size * m / (sqrtf(v) * inv_sqrt_bc2 + a.eps);
    a.p[i] = p;
    a.m[i] = m;
    a.v[i] = v;
  }
}

// k_adam with the hyperparameters read from a device block {lr, beta1, beta2, eps, weight_decay, max_norm} (uniform scalar loads,
// once per thread), so a captured graph follows a learning-rate schedule or a loaded checkpoint.  The loop body is k_adam's statement
// for statement: the compiler then forms the same fused multiply-adds and the results are bit-identical for the same fp32 values
// (an f32x4 restatement contracted differently and was not).
// EMA: the same launch also moves a shadow of the parameters, e += (1 - d) * (p - e) on the final p (the lerp form keeps its accuracy
// for d near 1).  d = hp[6], or min(hp[6], (1 + t) / (10 + t)) when hp[7] != 0 (warm-up on the incremented step count t): uniform per
// launch, read from the device block like lr, so a captured graph follows a changed decay.  One body for both instantiations, and
// the shadow statements come after the three stores: p / m / v of EMA = true are bit-identical to EMA = false.
struct AdamDevArgs {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  const float* hp;
  float grad_scale;
  int decoupled;
  const float* sumsq;
  const float* step;
  float* ema;  // EMA = true only
};

template <bool EMA>
__global__ void __launch_bounds__(256) k_adam_dev(AdamDevArgs a) {
  const float lr = a.hp[0], beta1 = a.hp[1], beta2 = a.hp[2], eps = a.hp[3], weight_decay = a.hp[4];
  const float t = *a.step;
  const float bc1 = 1.f - powf(beta1, t), bc2 = 1.f - powf(beta2, t);
  const float step_size = lr / bc1, inv_sqrt_bc2 = rsqrtf(bc2);
  float clip = a.grad_scale;
  if (a.sumsq) {
    float c = a.hp[5] / (a.grad_scale * sqrtf(*a.sumsq) + 1e-6f);
    clip = (c < 1.f ? c : 1.f) * a.grad_scale;
  }
  float one_minus_d = 0.f;
  if constexpr (EMA) {
    float d = a.hp[6];
    if (a.hp[7] != 0.f) {
      const float w = (1.f + t) / (10.f + t);
      d = w < d ? w : d;
    }
    one_minus_d = 1.f - d;
  }
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
    float p = a.p[i], g = a.g[i] * clip, m = a.m[i], v = a.v[i];
    if (a.decoupled)
      p *= 1.f - lr * weight_decay;
    else
      g += weight_decay * p;
    m = beta1 * m + (1.f - beta1) * g;
    v = beta2 * v + (1.f - beta2) * g * g;
    p -= step_size * m / (sqrtf(v) * inv_sqrt_bc2 + eps);
    a.p[i] = p;
    a.m[i] = m;
    a.v[i] = v;
    if constexpr (EMA) {
      float e = a.ema[i];
      e += one_minus_d * (p - e);
      a.ema[i] = e;
    }
  }
}

__global__ void k_step_inc(float* step) { *step += 1.f; }
__global__ void __launch_bounds__(256) k_scale(float* __restrict__ x, float alpha, int64_t n) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] *= alpha;
}
// y += alpha * x (gradient accumulation over micro-batches: T-LDM:173-180 sums the micro-step gradients)
__global__ void __launch_bounds__(256) k_axpy(f32x4* __restrict__ y, const f32x4* __restrict__ x, float alpha, int64_t n4, float* __restrict__ yt,
                                              const float* __restrict__ xt, int ntail) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 a = y[i], b = x[i];
    a[0] += alpha * b[0]; a[1] += alpha * b[1]; a[2] += alpha * b[2]; a[3] += alpha * b[3];
    y[i] = a;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) yt[threadIdx.x] += alpha * xt[threadIdx.x];
}
// a <-> b (the trainer's parameters and their moving average trade places around validation / sampling)
__global__ void __launch_bounds__(256) k_swap(f32x4* a, f32x4* b, int64_t n4, float* at, float* bt, int ntail) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) {
    float x = at[threadIdx.x], y = bt[threadIdx.x];
    at[threadIdx.x] = y;
    bt[threadIdx.x] = x;
  }
}

}  // namespace

extern "C" {

int mi_sumsq_f32(const float* x, int64_t n, float* out, int accumulate, hipStream_t st) {
  if (n <= 0 || ((uintptr_t)x & 15)) return MI_ERR_BAD_ARG;
  if (!accumulate) {
    hipError_t e = mi_zero_fill_f32(out, 1, 1, 1, st);
    if (e != hipSuccess) return (int)e;
  }
  int64_t n4 = n / 4;
  int grid = (int)((n4 + 255) / 256);
  grid = grid < 1 ? 1 : (grid > 2048 ? 2048 : grid);
  hipLaunchKernelGGL(k_sumsq, dim3(grid), dim3(256), 0, st, (const f32x4*)x, n4, x + n4 * 4, (int)(n - n4 * 4), out);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int decoupled_weight_decay, const float* grad_sumsq, float max_norm, float grad_scale,
                 float* step_counter, hipStream_t st) {
  if (n <= 0 || !step_counter || !(grad_scale > 0.f)) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, st, step_counter);
  AdamArgs a{param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale, decoupled_weight_decay,
             grad_sumsq, step_counter};
  int grid = (int)((n + 255) / 256);
  grid = grid > 4096 ? 4096 : grid;
  hipLaunchKernelGGL(k_adam, dim3(grid), dim3(256), 0, st, a);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* hparams, int decoupled_weight_decay,
                     const float* grad_sumsq, float grad_scale, float* step_counter, hipStream_t st) {
  if (n <= 0 || !param || !grad || !exp_avg || !exp_avg_sq || !hparams || !step_counter || !(grad_scale > 0.f)) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, st, step_counter);
  AdamDevArgs a{param, grad, exp_avg, exp_avg_sq, n, hparams, grad_scale, decoupled_weight_decay, grad_sumsq, step_counter, nullptr};
  int grid = (int)((n + 255) / 256);
  grid = grid > 4096 ? 4096 : grid;
  hipLaunchKernelGGL(k_adam_dev<false>, dim3(grid), dim3(256), 0, st, a);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_adam_ema_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, const float* hparams,
                         int decoupled_weight_decay, const float* grad_sumsq, float grad_scale, float* step_counter, hipStream_t st) {
  if (n <= 0 || !param || !grad || !exp_avg || !exp_avg_sq || !ema || !hparams || !step_counter || !(grad_scale > 0.f)) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, st, step_counter);
  AdamDevArgs a{param, grad, exp_avg, exp_avg_sq, n, hparams, grad_scale, decoupled_weight_decay, grad_sumsq, step_counter, ema};
  int grid = (int)((n + 255) / 256);
  grid = grid > 4096 ? 4096 : grid;
  hipLaunchKernelGGL(k_adam_dev<true>, dim3(grid), dim3(256), 0, st, a);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_swap_f32(float* a, float* b, int64_t n, hipStream_t st) {
  if (n <= 0 || !a || !b || ((uintptr_t)a & 15) || ((uintptr_t)b & 15)) return MI_ERR_BAD_ARG;
  int64_t n4 = n / 4;
  int grid = (int)((n4 + 255) / 256);
  grid = grid < 1 ? 1 : (grid > 4096 ? 4096 : grid);
  hipLaunchKernelGGL(k_swap, dim3(grid), dim3(256), 0, st, (f32x4*)a, (f32x4*)b, n4, a + n4 * 4, b + n4 * 4, (int)(n - n4 * 4));
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_scale_f32(float* x, float alpha, int64_t n, hipStream_t st) {
  if (n <= 0 || !x) return MI_ERR_BAD_ARG;
  int grid = (int)((n + 255) / 256);
  hipLaunchKernelGGL(k_scale, dim3(grid > 4096 ? 4096 : grid), dim3(256), 0, st, x, alpha, n);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_axpy_f32(float* y, const float* x, float alpha, int64_t n, hipStream_t st) {
  if (n <= 0 || !y || !x || ((uintptr_t)x & 15) || ((uintptr_t)y & 15)) return MI_ERR_BAD_ARG;
  int64_t n4 = n / 4;
  int grid = (int)((n4 + 255) / 256);
  grid = grid < 1 ? 1 : (grid > 4096 ? 4096 : grid);
  hipLaunchKernelGGL(k_axpy, dim3(grid), dim3(256), 0, st, (f32x4*)y, (const f32x4*)x, alpha, n4, y + n4 * 4, x + n4 * 4, (int)(n - n4 * 4));
  MI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
