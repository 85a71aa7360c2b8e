// Vector quantiser of the VQ-VAE (generative.networks.layers.vector_quantizer.EMAQuantizer, restated in tests/vqvae_ref.py: PARITY
// UNPINNED): nearest-code search, straight-through gather + commitment loss, its backward, and the EMA codebook update.
//
// Tokens are the encoder's output as it stands: channels-last bf16 [T][pitch], D channels used.  Codebook and EMA state are fp32.
// All arithmetic is fp32 (bf16 products would flip near-ties: a token's two best codes are often closer than one bf16 rounding of the
// dot product), sums that run over many terms are folded in fp64.  No float atomics anywhere: every output is a pure function of the
// inputs, so two runs, and eager against hipGraph replay, agree bit for bit.
//
// mi_vq_assign is an fp32 register-tiled NT GEMM (64 tokens x 64 codes per workgroup pass, 4 x 4 per thread, D in chunks of 32 through
// LDS read with 16-byte accesses) whose epilogue keeps a running (min, index) per token instead of storing the product.  LDS use is
// 17 KiB per workgroup, so the CU's occupancy is bounded by registers, not LDS.
//
// mi_vq_ema_update needs dw_k = sum of the tokens assigned to code k in a fixed order.  It sorts token ids by code with a STABLE
// counting sort (per-chunk histograms with integer LDS atomics -> exclusive scan over chunks and codes -> scatter where a token's rank
// inside its 256-token batch is counted, not raced for), then one workgroup per code adds its tokens in ascending token order.
#include "common.h"
#include "medimgen_hip.h"

namespace {

constexpr int kTT = 64, kKT = 64, kDC = 32, kPad = 4;  // assign: tokens / codes per workgroup pass, D chunk, LDS row padding (floats)
constexpr int kThreads = 256;
constexpr int kMaxK = 8192, kMaxD = 256;
constexpr int kScanThreads = 1024;

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int ema_chunks(int64_t T) {
  const int64_t c = (T + MI_VQ_EMA_CHUNK - 1) / MI_VQ_EMA_CHUNK;
  return (int)(c < 1 ? 1 : (c > MI_VQ_EMA_MAX_CHUNKS ? MI_VQ_EMA_MAX_CHUNKS : c));
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int clamp_code(int k, int K) { return k < 0 ? 0 : (k >= K ? K - 1 : k); }

// ---- nearest code ---------------------------------------------------------------------------------------------------------------
// thread (tx, ty) = (tid % 16, tid / 16): tokens t0 + 4 ty + i, codes k0 + 4 tx + j.  dist = |e|^2 - 2 x.e with |e|^2 accumulated beside
// the dot products from the same LDS values, so two identical code rows give identical bits and the lower index wins.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_vq_assign(const bf16* __restrict__ x, int64_t xcs, const float* __restrict__ cb,
                                                        int* __restrict__ idx, int64_t T, int D, int K) {
  __shared__ __attribute__((aligned(16))) float xs[kDC][kTT + kPad];
  __shared__ __attribute__((aligned(16))) float es[kDC][kKT + kPad];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t t0 = blockIdx.x * (int64_t)kTT;
  float best[4];
  int bidx[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) best[i] = __builtin_inff(), bidx[i] = 0;

  for (int k0 = 0; k0 < K; k0 += kKT) {
    float acc[4][4], en[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      en[i] = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    }
    for (int d0 = 0; d0 < D; d0 += kDC) {
      __syncthreads();  // the previous chunk has been consumed
      if (VEC) {        // 64 tokens x 4 groups of 8 channels: one 16-byte load per thread
        const int r = tid >> 2, d = d0 + (tid & 3) * 8;
        const int64_t t = t0 + r;
        F8 f;
#pragma unroll
        for (int j = 0; j < 8; ++j) f.v[j] = 0.f;
        if (t < T && d < D) f = unpack8(*(const u32x4*)(x + t * xcs + d));  // D % 8 == 0: the group lies inside the row
#pragma unroll
        for (int j = 0; j < 8; ++j) xs[(tid & 3) * 8 + j][r] = f.v[j];
      } else {
        for (int e = tid; e < kTT * kDC; e += kThreads) {
          const int r = e / kDC, c = e % kDC, d = d0 + c;
          const int64_t t = t0 + r;
          xs[c][r] = (t < T && d < D) ? bf2f(x[t * xcs + d]) : 0.f;
        }
      }
      for (int e = tid; e < kKT * kDC; e += kThreads) {
        const int r = e / kDC, c = e % kDC, k = k0 + r, d = d0 + c;
        es[c][r] = (k < K && d < D) ? cb[(int64_t)k * D + d] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int c = 0; c < kDC; ++c) {
        const f32x4 xv = *(const f32x4*)&xs[c][ty * 4];
        const f32x4 ev = *(const f32x4*)&es[c][tx * 4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(xv[i], ev[j], acc[i][j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) en[j] = fmaf(ev[j], ev[j], en[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // ascending k within the thread and across tiles: `<` keeps the lowest index of a tie
      const int k = k0 + tx * 4 + j;
      if (k < K) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float dist = fmaf(-2.f, acc[i][j], en[j]);
          if (dist < best[i]) best[i] = dist, bidx[i] = k;
        }
      }
    }
  }
  // the 16 tx lanes of a token are adjacent lanes of one wave: (min, lowest index) butterfly
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best[i], off, 64);
      const int oi = __shfl_xor(bidx[i], off, 64);
      if (ov < best[i] || (ov == best[i] && oi < bidx[i])) best[i] = ov, bidx[i] = oi;
    }
    const int64_t t = t0 + ty * 4 + i;
    if (tx == 0 && t < T) idx[t] = bidx[i];
  }
}

// ---- straight-through gather + commitment loss ----------------------------------------------------------------------------------
// one item = one element (VEC: 8 channels of one token).  x == nullptr: zq = bf16(q) alone (decoding stored indices).
template <bool VEC>
__global__ void k_vq_gather(const bf16* __restrict__ x, int64_t xcs, const float* __restrict__ cb, const int* __restrict__ idx,
                            bf16* __restrict__ zq, int64_t zcs, float* __restrict__ diff, double* __restrict__ partials, int64_t T, int D,
                            int K) {
  __shared__ double red[4];
  constexpr int W = VEC ? 8 : 1;
  const int per = D / W;
  const int64_t items = T * per;
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i / per;
    const int d = (int)(i - t * per) * W;
    const float* q = cb + (int64_t)clamp_code(idx[t], K) * D + d;
    if (VEC) {
      const f32x4 q0 = ((const f32x4*)q)[0], q1 = ((const f32x4*)q)[1];
      F8 o;
      if (x) {
        const F8 xv = unpack8(*(const u32x4*)(x + t * xcs + d));
        f32x4 d0, d1;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float df = (j < 4 ? q0[j & 3] : q1[j & 3]) - xv.v[j];
          o.v[j] = xv.v[j] + df;
          if (j < 4) d0[j & 3] = df; else d1[j & 3] = df;
          s = fmaf(df, df, s);
        }
        ((f32x4*)(diff + t * D + d))[0] = d0;
        ((f32x4*)(diff + t * D + d))[1] = d1;
        acc += (double)s;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] = j < 4 ? q0[j & 3] : q1[j & 3];
      }
      *(u32x4*)(zq + t * zcs + d) = pack8(o);
    } else {
      if (x) {
        const float xv = bf2f(x[t * xcs + d]), df = q[0] - xv;
        zq[t * zcs + d] = f2bf(xv + df);
        diff[t * D + d] = df;
        acc += (double)(df * df);
      } else {
        zq[t * zcs + d] = f2bf(q[0]);
      }
    }
  }
  if (!x) return;  // uniform over the grid
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void k_vq_loss_finalize(const double* __restrict__ partials, int nparts, double scale, float* __restrict__ loss) {
  __shared__ double red[kThreads];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) s += partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(red[0] * scale);
}

// dx = dq + c (x - q), c = weight[0] * scale with the weight from device memory
__global__ void k_vq_bwd(const bf16* __restrict__ dq, int64_t dqcs, const float* __restrict__ diff, const float* __restrict__ weight,
                         float scale, bf16* __restrict__ dx, int64_t dxcs, int64_t T, int D) {
  const float cc = *weight * scale;
  const int64_t total = T * D;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i / D;
    const int d = (int)(i - t * D);
    dx[t * dxcs + d] = f2bf(fmaf(cc, -diff[i], bf2f(dq[t * dqcs + d])));
  }
}

// ---- EMA codebook update ---------------------------------------------------------------------------------------------------------
// cnt[c][k] = tokens of chunk c assigned to k (integer LDS atomics: order-free)
__global__ __launch_bounds__(kThreads) void k_vq_hist(const int* __restrict__ idx, int64_t T, int K, int64_t chunk_len,
                                                      int* __restrict__ cnt) {
  __shared__ int h[kMaxK];
  for (int k = threadIdx.x; k < K; k += kThreads) h[k] = 0;
  __syncthreads();
  const int64_t lo = blockIdx.x * chunk_len, hi = (lo + chunk_len < T) ? lo + chunk_len : T;
  for (int64_t t = lo + threadIdx.x; t < hi; t += kThreads) atomicAdd(&h[clamp_code(idx[t], K)], 1);
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += kThreads) cnt[(int64_t)blockIdx.x * K + k] = h[k];
}
// one workgroup: cnt -> exclusive over chunks, count[k], base[k] (exclusive over codes), the new ema_cluster_size, n = its sum (fp64,
// fixed-order tree) and the perplexity of this batch's assignment
__global__ __launch_bounds__(kScanThreads) void k_vq_scan(int* __restrict__ cnt, int chunks, int K, int64_t T, int* __restrict__ count,
                                                           int* __restrict__ base, float* __restrict__ ema_cs, float decay,
                                                           double* __restrict__ nsum, float* __restrict__ perplexity) {
  __shared__ int tot[kMaxK];
  __shared__ int tsum[kScanThreads];
  __shared__ double red_n[kScanThreads], red_e[kScanThreads];
  const int tid = threadIdx.x;
  double ln = 0.0, le = 0.0;
  for (int k = tid; k < K; k += kScanThreads) {
    int run = 0;
    for (int c = 0; c < chunks; ++c) {
      const int v = cnt[(int64_t)c * K + k];
      cnt[(int64_t)c * K + k] = run;
      run += v;
    }
    tot[k] = run;
    count[k] = run;
    const float cs = ema_cs[k] * decay + (1.f - decay) * (float)run;
    ema_cs[k] = cs;
    ln += (double)cs;
    const float p = (float)run / (float)T;
    le += (double)(p * logf(p + 1e-10f));
  }
  __syncthreads();
  constexpr int kPer = kMaxK / kScanThreads;  // 8 consecutive codes per thread
  int s = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) s += (tid * kPer + j < K) ? tot[tid * kPer + j] : 0;
  tsum[tid] = s;
  red_n[tid] = ln;
  red_e[tid] = le;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {
    const int v = tid >= off ? tsum[tid - off] : 0;
    __syncthreads();
    tsum[tid] += v;
    __syncthreads();
  }
  int excl = tsum[tid] - s;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int k = tid * kPer + j;
    if (k < K) {
      base[k] = excl;
      excl += tot[k];
    }
  }
  for (int o = kScanThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red_n[tid] += red_n[tid + o], red_e[tid] += red_e[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    *nsum = red_n[0];
    *perplexity = expf(-(float)red_e[0]);
  }
}
// perm[base[k] + (tokens of k before t)] = t: tokens of one code in ascending order.  A chunk walks its tokens in batches of 256; inside
// a batch a token's rank is the number of lower threads with the same code, the LDS cursors advance by integer atomics afterwards.
__global__ __launch_bounds__(kThreads) void k_vq_scatter(const int* __restrict__ idx, int64_t T, int K, int64_t chunk_len,
                                                         const int* __restrict__ cnt, const int* __restrict__ base, int* __restrict__ perm) {
  __shared__ int cur[kMaxK];
  __shared__ int sidx[kThreads];
  const int tid = threadIdx.x;
  for (int k = tid; k < K; k += kThreads) cur[k] = base[k] + cnt[(int64_t)blockIdx.x * K + k];
  const int64_t lo = blockIdx.x * chunk_len, hi = (lo + chunk_len < T) ? lo + chunk_len : T;
  for (int64_t b = lo; b < hi; b += kThreads) {  // uniform trip count
    const int64_t t = b + tid;
    const int my = t < hi ? clamp_code(idx[t], K) : -1;
    sidx[tid] = my;
    __syncthreads();
    if (my >= 0) {
      int rank = 0;
      for (int j = 0; j < tid; ++j) rank += sidx[j] == my;
      const int64_t pos = (int64_t)cur[my] + rank;
      if (pos < T) perm[pos] = (int)t;  // always true for consistent counts; the guard keeps a racing writer of idx from faulting
    }
    __syncthreads();
    if (my >= 0) atomicAdd(&cur[my], 1);
    __syncthreads();
  }
}
// one workgroup per code: dw in ascending token order (S = 256 / D interleaved slices per channel, fp64, folded in slice order), then
// ema_w = decay ema_w + (1 - decay) dw, w = (cs + eps) / (n + K eps) n, embedding = ema_w / w
__global__ __launch_bounds__(kThreads) void k_vq_ema_reduce(const bf16* __restrict__ x, int64_t xcs, const int* __restrict__ perm,
                                                            const int* __restrict__ base, const int* __restrict__ count, int64_t T, int D,
                                                            int K, float* __restrict__ ema_w, float* __restrict__ emb,
                                                            const float* __restrict__ ema_cs, const double* __restrict__ nsum, float decay,
                                                            float eps) {
  __shared__ double part[kThreads];
  const int k = blockIdx.x, tid = threadIdx.x, S = kThreads / D;
  const int d = tid % D, s = tid / D;
  const int n_k = count[k], b = base[k];
  if (s < S) {
    double acc = 0.0;
    for (int j = s; j < n_k; j += S) {
      const int64_t t = perm[b + j];
      if (t >= 0 && t < T) acc += (double)bf2f(x[t * xcs + d]);
    }
    part[tid] = acc;
  }
  __syncthreads();
  if (tid < D) {
    double dw = 0.0;
    for (int q = 0; q < S; ++q) dw += part[q * D + tid];
    const float n = (float)*nsum;
    const float w = (ema_cs[k] + eps) / (n + (float)K * eps) * n;
    const int64_t o = (int64_t)k * D + tid;
    const float ew = ema_w[o] * decay + (1.f - decay) * (float)dw;
    ema_w[o] = ew;
    emb[o] = ew / w;
  }
}

// ---- small channels-last helpers of the VQ-VAE's im2col / GEMM convs ------------------------------------------------------------
// y[v][c] = act(x[v][c] + bias[c]) for c < C
__global__ void k_bias_act(const bf16* __restrict__ x, int64_t xcs, const float* __restrict__ bias, bf16* __restrict__ y, int64_t ycs,
                           int64_t nvox, int C, int relu) {
  const int64_t total = nvox * C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / C;
    const int c = (int)(i - v * C);
    float u = bf2f(x[v * xcs + c]) + bias[c];
    if (relu) u = u > 0.f ? u : 0.f;
    y[v * ycs + c] = f2bf(u);
  }
}
// y[v][c] = c < C ? x[v][c] : 0 for c < Cp
__global__ void k_pad_channels(const bf16* __restrict__ x, int64_t xcs, int C, bf16* __restrict__ y, int Cp, int64_t nvox) {
  const int64_t total = nvox * Cp;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / Cp;
    const int c = (int)(i - v * Cp);
    y[i] = c < C ? x[v * xcs + c] : f2bf(0.f);
  }
}
// y[i] += alpha[0] * x[i], alpha from device memory
__global__ void k_axpy_dev(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ alpha, int64_t n) {
  const float a = *alpha;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = fmaf(a, x[i], y[i]);
}

// ---- fixed-order reductions of the VQ train step (the float-atomic forms mi_l1_fwd_bwd / mi_sumsq_f32 add their workgroup sums in
// arrival order: equal up to rounding, not bit for bit) ----------------------------------------------------------------------------
__device__ __forceinline__ void store_block_partial(double v, double* red, double* __restrict__ partials) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// pred NDHWC bf16, target NCDHW fp32: dpred = sign(pred - target) / numel (the values mi_l1_fwd_bwd writes), sum |d| into partials
__global__ void k_l1_det(const bf16* __restrict__ pred, const float* __restrict__ target, bf16* __restrict__ dpred,
                         double* __restrict__ partials, int C, int64_t V, int64_t total, float inv_numel) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / V, v = i - n * V;
    for (int c = 0; c < C; ++c) {
      const float d = bf2f(pred[i * C + c]) - target[(n * C + c) * V + v];
      acc += (double)fabsf(d);
      dpred[i * C + c] = f2bf(d > 0.f ? inv_numel : (d < 0.f ? -inv_numel : 0.f));
    }
  }
  store_block_partial(acc, red, partials);
}
__global__ void k_sumsq_det(const float* __restrict__ x, int64_t n, double* __restrict__ partials) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) acc += (double)(x[i] * x[i]);
  store_block_partial(acc, red, partials);
}

// x[i] = ab[0] * x[i] + ab[1], both scalars from device memory
__global__ void k_affine_dev(float* __restrict__ x, const float* __restrict__ ab, int64_t n) {
  const float a = ab[0], b = ab[1];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] = fmaf(a, x[i], b);
}
// column sums of x [rows][cs] bf16 in a fixed order: workgroup b sums its row chunk per channel (256 / C interleaved row slices per
// channel, fp64, folded in slice order) into part[b][C]; k_colsum_fold adds the chunks in order and accumulates into out
__global__ __launch_bounds__(kThreads) void k_colsum_part(const bf16* __restrict__ x, int64_t cs, int64_t rows, int C, int64_t chunk,
                                                          double* __restrict__ part) {
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < rows ? lo + chunk : rows;
  for (int c0 = 0; c0 < C; c0 += kThreads) {
    const int cw = C - c0 < kThreads ? C - c0 : kThreads, S = kThreads / cw;
    const int c = tid % cw, s = tid / cw;
    double acc = 0.0;
    if (s < S)
      for (int64_t r = lo + s; r < hi; r += S) acc += (double)bf2f(x[r * cs + c0 + c]);
    __syncthreads();  // red of the previous channel block has been read
    red[tid] = acc;
    __syncthreads();
    if (tid < cw) {
      double t = 0.0;
      for (int q = 0; q < S; ++q) t += red[q * cw + tid];
      part[(int64_t)blockIdx.x * C + c0 + tid] = t;
    }
  }
}
__global__ void k_colsum_fold(const double* __restrict__ part, int chunks, int C, float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double t = 0.0;
  for (int b = 0; b < chunks; ++b) t += part[(int64_t)b * C + c];
  out[c] += (float)t;
}

inline int grid_for(int64_t work) {
  const int64_t g = (work + kThreads - 1) / kThreads;
  return (int)(g < 1 ? 1 : (g > MI_VQ_PARTIALS ? MI_VQ_PARTIALS : g));
}
inline int check_shape(int64_t T, int D, int K) {
  if (T <= 0 || D <= 0 || K <= 0 || T > (int64_t)1 << 30) return MI_ERR_BAD_ARG;
  if (D > kMaxD || K > kMaxK) return MI_ERR_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" {

int mi_vq_assign(const void* x, int x_cstride, const float* codebook, int* idx, int64_t T, int D, int K, hipStream_t st) {
  if (!x || !codebook || !idx || x_cstride < D) return MI_ERR_BAD_ARG;
  if (const int rc = check_shape(T, D, K)) return rc;
  const int grid = (int)((T + kTT - 1) / kTT);
  const bool vec = D % 8 == 0 && x_cstride % 8 == 0 && aligned16(x);
  if (vec)
    hipLaunchKernelGGL(k_vq_assign<true>, dim3(grid), dim3(kThreads), 0, st, (const bf16*)x, (int64_t)x_cstride, codebook, idx, T, D, K);
  else
    hipLaunchKernelGGL(k_vq_assign<false>, dim3(grid), dim3(kThreads), 0, st, (const bf16*)x, (int64_t)x_cstride, codebook, idx, T, D, K);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_vq_gather_loss(const void* x, int x_cstride, const float* codebook, const int* idx, void* zq, int zq_cstride, float* diff,
                      float* loss, double* partials, int64_t T, int D, int K, float commitment_cost, hipStream_t st) {
  if (!codebook || !idx || !zq || zq_cstride < D) return MI_ERR_BAD_ARG;
  if (x && (!diff || !loss || !partials || x_cstride < D || ((uintptr_t)partials & 7))) return MI_ERR_BAD_ARG;
  if (const int rc = check_shape(T, D, K)) return rc;
  const bool vec = D % 8 == 0 && zq_cstride % 8 == 0 && aligned16(zq) && aligned16(codebook) &&
                   (!x || (x_cstride % 8 == 0 && aligned16(x) && aligned16(diff)));
  const int grid = grid_for(vec ? T * (D / 8) : T * D);
  if (vec)
    hipLaunchKernelGGL(k_vq_gather<true>, dim3(grid), dim3(kThreads), 0, st, (const bf16*)x, (int64_t)x_cstride, codebook, idx, (bf16*)zq,
                       (int64_t)zq_cstride, diff, partials, T, D, K);
  else
    hipLaunchKernelGGL(k_vq_gather<false>, dim3(grid), dim3(kThreads), 0, st, (const bf16*)x, (int64_t)x_cstride, codebook, idx, (bf16*)zq,
                       (int64_t)zq_cstride, diff, partials, T, D, K);
  MI_CHECK_LAUNCH();
  if (x) {
    hipLaunchKernelGGL(k_vq_loss_finalize, dim3(1), dim3(kThreads), 0, st, partials, grid, (double)commitment_cost / ((double)T * D), loss);
    MI_CHECK_LAUNCH();
  }
  return 0;
}

int mi_vq_bwd(const void* dq, int dq_cstride, const float* diff, const float* weight, float scale, void* dx, int dx_cstride, int64_t T,
              int D, hipStream_t st) {
  if (!dq || !diff || !weight || !dx || dq_cstride < D || dx_cstride < D) return MI_ERR_BAD_ARG;
  if (const int rc = check_shape(T, D, 1)) return rc;
  hipLaunchKernelGGL(k_vq_bwd, dim3(grid_for(T * D)), dim3(kThreads), 0, st, (const bf16*)dq, (int64_t)dq_cstride, diff, weight, scale,
                     (bf16*)dx, (int64_t)dx_cstride, T, D);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_vq_ema_update(const void* x, int x_cstride, const int* idx, int64_t T, int D, int K, float* embedding, float* ema_cluster_size,
                     float* ema_w, float decay, float eps, float* perplexity, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  if (!x || !idx || !embedding || !ema_cluster_size || !ema_w || !perplexity || !workspace || x_cstride < D || ((uintptr_t)workspace & 7))
    return MI_ERR_BAD_ARG;
  if (const int rc = check_shape(T, D, K)) return rc;
  const int chunks = ema_chunks(T);
  if (workspace_bytes < 8 + 4 * ((int64_t)chunks * K + 2 * (int64_t)K + T)) return MI_ERR_BAD_ARG;
  const int64_t chunk_len = (T + chunks - 1) / chunks;
  double* nsum = (double*)workspace;
  int* cnt = (int*)(nsum + 1);
  int* count = cnt + (int64_t)chunks * K;
  int* base = count + K;
  int* perm = base + K;
  hipLaunchKernelGGL(k_vq_hist, dim3(chunks), dim3(kThreads), 0, st, idx, T, K, chunk_len, cnt);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_vq_scan, dim3(1), dim3(kScanThreads), 0, st, cnt, chunks, K, T, count, base, ema_cluster_size, decay, nsum,
                     perplexity);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_vq_scatter, dim3(chunks), dim3(kThreads), 0, st, idx, T, K, chunk_len, (const int*)cnt, (const int*)base, perm);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_vq_ema_reduce, dim3(K), dim3(kThreads), 0, st, (const bf16*)x, (int64_t)x_cstride, (const int*)perm,
                     (const int*)base, (const int*)count, T, D, K, ema_w, embedding, (const float*)ema_cluster_size, (const double*)nsum,
                     decay, eps);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_axpy_dev_f32(float* y, const float* x, const float* alpha, int64_t n, hipStream_t st) {
  if (!y || !x || !alpha || n <= 0) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_axpy_dev, dim3(grid_for(n)), dim3(kThreads), 0, st, y, x, alpha, n);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_l1_fwd_bwd_det(const void* pred, const float* target, void* dpred, float* loss, double* partials, int N, int C, int64_t V,
                      hipStream_t st) {
  if (!pred || !target || !dpred || !loss || !partials || N <= 0 || C <= 0 || V <= 0 || ((uintptr_t)partials & 7)) return MI_ERR_BAD_ARG;
  const int64_t total = (int64_t)N * V;
  const int grid = grid_for(total);
  hipLaunchKernelGGL(k_l1_det, dim3(grid), dim3(kThreads), 0, st, (const bf16*)pred, target, (bf16*)dpred, partials, C, V, total,
                     1.f / (float)(total * C));
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_vq_loss_finalize, dim3(1), dim3(kThreads), 0, st, (const double*)partials, grid, 1.0 / ((double)total * C), loss);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_sumsq_det_f32(const float* x, int64_t n, float* out, double* partials, hipStream_t st) {
  if (!x || !out || !partials || n <= 0 || ((uintptr_t)partials & 7)) return MI_ERR_BAD_ARG;
  const int grid = grid_for(n);
  hipLaunchKernelGGL(k_sumsq_det, dim3(grid), dim3(kThreads), 0, st, x, n, partials);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_vq_loss_finalize, dim3(1), dim3(kThreads), 0, st, (const double*)partials, grid, 1.0, out);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_affine_dev_f32(float* x, const float* ab, int64_t n, hipStream_t st) {
  if (!x || !ab || n <= 0) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_affine_dev, dim3(grid_for(n)), dim3(kThreads), 0, st, x, ab, n);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_colsum_det_bf16(const void* x, int x_cstride, int64_t rows, int C, float* out, double* workspace, hipStream_t st) {
  if (!x || !out || !workspace || rows <= 0 || C <= 0 || x_cstride < C || ((uintptr_t)workspace & 7)) return MI_ERR_BAD_ARG;
  int64_t chunks = (rows + MI_VQ_COLSUM_ROWS - 1) / MI_VQ_COLSUM_ROWS;
  if (chunks > MI_VQ_COLSUM_MAX_CHUNKS) chunks = MI_VQ_COLSUM_MAX_CHUNKS;
  const int64_t chunk = (rows + chunks - 1) / chunks;
  hipLaunchKernelGGL(k_colsum_part, dim3((int)chunks), dim3(kThreads), 0, st, (const bf16*)x, (int64_t)x_cstride, rows, C, chunk, workspace);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_colsum_fold, dim3((C + kThreads - 1) / kThreads), dim3(kThreads), 0, st, (const double*)workspace, (int)chunks, C, out);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_bias_act_bf16(const void* x, int x_cstride, const float* bias, void* y, int y_cstride, int64_t nvox, int C, int relu, hipStream_t st) {
  if (!x || !bias || !y || nvox <= 0 || C <= 0 || x_cstride < C || y_cstride < C) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_bias_act, dim3(grid_for(nvox * C)), dim3(kThreads), 0, st, (const bf16*)x, (int64_t)x_cstride, bias, (bf16*)y,
                     (int64_t)y_cstride, nvox, C, relu);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_fit_channels_bf16(const void* x, int x_cstride, int C, void* y, int Cy, int64_t nvox, hipStream_t st) {
  if (!x || !y || nvox <= 0 || C <= 0 || Cy <= 0 || x_cstride < (C < Cy ? C : Cy)) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_pad_channels, dim3(grid_for(nvox * Cy)), dim3(kThreads), 0, st, (const bf16*)x, (int64_t)x_cstride, C, (bf16*)y,
                     Cy, nvox);
  MI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
