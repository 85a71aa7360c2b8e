// 2-D k4 p1 convolutions (stride 2 / 1) of the PatchDiscriminator on dense NHWC bf16 -- the planner's `'2D'` discriminator_params
// (configuration.py:966-967), train_autoencoder.py:371-397, 416-423.  Unlike the 3-D lowering of disc.hip there is no patch matrix:
//
//   MFMA path (Cin % 16 == 0, Cout % 32 == 0: the three middle layers).  The NT GEMM of gemm.hip (32x32x16 bf16 MFMA, 80-byte LDS rows,
//   register prefetch of the next K tile) with the A operand gathered in place: only the address and predicate of the 16-byte piece
//   differ (conv2d_k4_index.h holds that arithmetic, host-callable).
//     forward        y[(n, oh, ow)][co]  = sum_k x_gathered[(n, oh, ow)][k] * Wf[co][k],           k = (th, tw, ci)
//     data gradient  dx[(n, ih, iw)][ci] = sum_k dy_gathered[(n, ih, iw)][k] * Wd[ci][k],          k = (th, tw, co); stride 2: one GEMM
//                    per parity class of (ih, iw) over its 4 taps, written to its strided pixels -- a gather, no scatter, no atomics
//     weight gradient dW[co][k] = sum_pixels dy[pixel][co] * x_gathered[pixel][k]: both operands are pixel-major, so they are staged as
//                    [pixel][32 channels] LDS images and read through ds_read_b64_tr_b16 (as k_wgrad1x1 does); the pixel axis is split
//                    into ranges whose fp32 slabs a second kernel folds in a fixed order into the torch-layout gradient (+=): bit-stable.
//   Edge path (the image layer, Cin < 8, and the logits layer, Cout = 1; any channel counts): plain VALU direct kernels.  Weights are
//   rounded to bf16 on the fly (what the MFMA path's pack does), the bias stays fp32.
#include "common.h"
#include "conv2d_k4_index.h"
#include "medimgen_hip.h"

namespace {

constexpr int kT = 256;
constexpr int BK = 32, PITCH = 40;  // as gemm.hip

inline int grid_for(int64_t total) {
  int64_t g = (total + kT - 1) / kT;
  return (int)(g > 256 * 32 ? 256 * 32 : (g < 1 ? 1 : g));
}
__device__ __forceinline__ float wbf(float w) { return bf2f(f2bf(w)); }

// ------------------------------------------------------------------------------------------------ weight packs
// torch weight [Cout][Cin][4][4] fp32 -> wf [Cout][16 Cin] bf16 (forward / the K order of the weight gradient) and
// wd [classes][Cin][T T Cout] bf16 (data gradient: 1 class of 16 taps at stride 1, 4 parity classes of 4 taps at stride 2)
__global__ void __launch_bounds__(kT) k_c2d_pack(const float* __restrict__ w, bf16* __restrict__ wf, bf16* __restrict__ wd, int Cin, int Cout, int s) {
  const int64_t total = (int64_t)16 * Cin * Cout;
  const int ncls = s == 2 ? 4 : 1;
  for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
    {
      const int k = (int)(i % (16 * Cin)), co = (int)(i / (16 * Cin));
      const int tap = k / Cin, ci = k - tap * Cin;
      wf[i] = f2bf(w[((int64_t)co * Cin + ci) * 16 + tap]);
    }
    if (wd) {
      const int kd = 16 / ncls * Cout;
      const int k = (int)(i % kd);
      int64_t r = i / kd;
      const int ci = (int)(r % Cin), cls = (int)(r / Cin);
      const C2dGeom g = c2d_dgrad_geom(4, 4, Cin, Cout, s, cls);
      int tap, co;
      c2d_tap(g, k, &tap, &co);
      wd[i] = f2bf(w[((int64_t)co * Cin + ci) * 16 + tap]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ gathered NT GEMM (forward, data gradient)
struct C2dGemmArgs {
  const bf16* src;  // gathered tensor
  const bf16* B;    // [classes][N][K]
  bf16* dst;
  C2dGeom g[4];
  int64_t M[4];     // rows per class
  int64_t sB;
  int N, K;
};

template <int WT>
__global__ void __launch_bounds__(256) k_c2d_gemm(C2dGemmArgs p) {
  constexpr int BM = 64 * WT, BN = 64 * WT;
  __shared__ __attribute__((aligned(16))) bf16 lds[2][2][BM * PITCH];  // [buf][A|B][row][PITCH]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const int cls = blockIdx.z;
  const C2dGeom g = p.g[cls];
  const int64_t M = p.M[cls];
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  if (m0 >= M) return;  // (the parity classes of odd extents differ in rows; uniform per workgroup)
  const bf16* B = p.B + cls * p.sB;
  const int n0 = blockIdx.y * BN;

  int prow[WT], pk[WT], rn[WT], ra[WT], rb[WT];
  bool rok[WT];
#pragma unroll
  for (int i = 0; i < WT; ++i) {
    const int pc = tid + 256 * i;
    prow[i] = pc >> 2;
    pk[i] = (pc & 3) * 8;
    const int64_t m = m0 + prow[i];
    rok[i] = m < M;
    c2d_row(g, rok[i] ? m : 0, &rn[i], &ra[i], &rb[i]);
  }
  u32x4 fa_[WT], fb_[WT];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < WT; ++i) {
      const u32x4 zero = {0u, 0u, 0u, 0u};
      const int k = k0 + pk[i];
      const int bn = n0 + prow[i];
      int64_t off = 0;
      // explicit row AND column predicate: a pixel outside the image is a zero, never an address
      const bool ok = rok[i] && k < p.K && c2d_src_at(g, rn[i], ra[i], rb[i], k, &off);
      fa_[i] = ok ? *(const u32x4*)(p.src + off) : zero;
      fb_[i] = (bn < p.N && k < p.K) ? *(const u32x4*)(B + (int64_t)bn * p.K + k) : zero;
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < WT; ++i) {
      *(u32x4*)(&lds[buf][0][prow[i] * PITCH + pk[i]]) = fa_[i];
      *(u32x4*)(&lds[buf][1][prow[i] * PITCH + pk[i]]) = fb_[i];
    }
  };

  f32x16 acc[WT][WT];
#pragma unroll
  for (int a = 0; a < WT; ++a)
#pragma unroll
    for (int b = 0; b < WT; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  const int nk = (p.K + BK - 1) / BK;
  gload(0);
  lstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * BK);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fa[WT], fb[WT];
#pragma unroll
      for (int i = 0; i < WT; ++i) {
        fa[i] = *(const bf16x8*)(&lds[buf][0][(wm * 32 * WT + i * 32 + r) * PITCH + ks * 16 + h * 8]);
        fb[i] = *(const bf16x8*)(&lds[buf][1][(wn * 32 * WT + i * 32 + r) * PITCH + ks * 16 + h * 8]);
      }
#pragma unroll
      for (int a = 0; a < WT; ++a)
#pragma unroll
        for (int b = 0; b < WT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    if (kt + 1 < nk) lstore(buf ^ 1);
    __syncthreads();
  }

  // epilogue. D map (32x32x16): col = lane & 31 -> n, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) -> m -> its pixel of dst
#pragma unroll
  for (int a = 0; a < WT; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t m = m0 + wm * 32 * WT + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (m >= M) continue;
      const int64_t doff = c2d_dst(g, m);
#pragma unroll
      for (int b = 0; b < WT; ++b) {
        const int n = n0 + wn * 32 * WT + b * 32 + r;
        if (n < p.N) p.dst[doff + n] = f2bf(acc[a][b][e]);
      }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// 64 (co) x 64 (k) tile of dW per workgroup and pixel range; 64 pixels per step = 4 MFMA k-steps of 16.  LDS images: per operand two
// 32-channel chunks of [64 pixels][64 bytes]; ds_read_b64_tr_b16 delivers 4 pixels x 16 channels channel-per-lane = the MFMA k axis.
struct C2dWgradArgs {
  const bf16* x;
  const bf16* dy;  // [P][Cout]
  float* slab;     // [splits][Cout][K]
  C2dGeom g;       // the forward map
  int64_t P, per_split;  // per_split % 64 == 0
  int Cout, K;
};

__device__ __forceinline__ void tr_read8(u32x2& dst, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(dst) : "v"(addr) : "memory");
}

__global__ void __launch_bounds__(256) k_c2d_wgrad(C2dWgradArgs p) {
  constexpr int IMG = 64 * 64;  // bytes of one chunk image
  __shared__ __attribute__((aligned(16))) char lds[2][2][2 * IMG];  // [buf][dy|x][chunk image]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int k0 = blockIdx.x * 64, co0 = blockIdx.y * 64;
  const int64_t pbeg = (int64_t)blockIdx.z * p.per_split;
  const int64_t pend = pbeg + p.per_split < p.P ? pbeg + p.per_split : p.P;
  const int nit = pend > pbeg ? (int)((pend - pbeg + 63) >> 6) : 0;
  typedef __attribute__((address_space(3))) char lds_char;
  const unsigned l0 = (unsigned)(size_t)(lds_char*)&lds[0][0][0];

  // loader: piece = 8 channels of one pixel; 64 pixels x 8 pieces per operand, 2 per thread
  int ppix[2], pq[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int pc = tid + 256 * i;
    ppix[i] = pc >> 3;
    pq[i] = pc & 7;
  }
  u32x4 ry[2], rx[2];
  auto gload = [&](int it) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const u32x4 zero = {0u, 0u, 0u, 0u};
      const int64_t gp = pbeg + (int64_t)it * 64 + ppix[i];
      const int co = co0 + pq[i] * 8, k = k0 + pq[i] * 8;
      const bool rowok = gp < pend;
      ry[i] = (rowok && co + 8 <= p.Cout) ? *(const u32x4*)(p.dy + gp * p.Cout + co) : zero;
      int64_t off = 0;
      const bool ok = rowok && k + 8 <= p.K && c2d_src(p.g, rowok ? gp : 0, k < p.K ? k : 0, &off);
      rx[i] = ok ? *(const u32x4*)(p.x + off) : zero;
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = (pq[i] >> 2) * IMG + ppix[i] * 64 + (pq[i] & 3) * 16;
      *(u32x4*)(&lds[buf][0][o]) = ry[i];
      *(u32x4*)(&lds[buf][1][o]) = rx[i];
    }
  };
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  // transposed-read lane roles: 16-lane group gq -> channel half (gq & 1), pixel half (gq >> 1); lane 4q+p of it -> pixel q, channels 4p
  const int gq = lane >> 4, qv = (lane >> 2) & 3, pp = lane & 3;
  const unsigned lane_off = ((gq >> 1) * 8 + qv) * 64 + ((gq & 1) * 16 + pp * 4) * 2;

  if (nit > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();
  for (int it = 0; it < nit; ++it) {
    const int buf = it & 1;
    if (it + 1 < nit) gload(it + 1);
    const unsigned ya = l0 + (unsigned)((buf * 2 + 0) * 2 * IMG + wm * IMG) + lane_off;
    const unsigned xa = l0 + (unsigned)((buf * 2 + 1) * 2 * IMG + wn * IMG) + lane_off;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      u32x2 fa[2], fb[2];
      tr_read8(fa[0], ya + ks * 16 * 64);
      tr_read8(fa[1], ya + ks * 16 * 64 + 4 * 64);
      tr_read8(fb[0], xa + ks * 16 * 64);
      tr_read8(fb[1], xa + ks * 16 * 64 + 4 * 64);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      asm volatile("" : "+v"(fa[0]), "+v"(fa[1]), "+v"(fb[0]), "+v"(fb[1]));
      __builtin_amdgcn_sched_barrier(0);
      const u32x4 va = {fa[0][0], fa[0][1], fa[1][0], fa[1][1]};
      const u32x4 vb = {fb[0][0], fb[0][1], fb[1][0], fb[1][1]};
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, va), __builtin_bit_cast(bf16x8, vb), acc, 0, 0, 0);
    }
    if (it + 1 < nit) lstore(buf ^ 1);
    __syncthreads();
  }
  // D: col = lane & 31 -> k, row -> co.  Every (split, co, k) is written by exactly one workgroup (zeros for an empty range).
  const int k = k0 + wn * 32 + (lane & 31);
  if (k < p.K) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int co = co0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
      if (co < p.Cout) p.slab[((int64_t)blockIdx.z * p.Cout + co) * p.K + k] = acc[e];
    }
  }
}

// dw [Cout][Cin][16] (+ db [Cout]) += sum over splits, in split order.  perm: slab rows are [Cout][(tap, ci)] (MFMA path); otherwise
// they are already in torch order, followed by the Cout bias sums when db is given (edge path).
__global__ void __launch_bounds__(kT) k_c2d_fold(const float* __restrict__ slab, int splits, int64_t row, float* __restrict__ dw, float* __restrict__ db,
                                                 int Cin, int Cout, int perm) {
  const int64_t nw = (int64_t)Cout * Cin * 16;
  for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < row; i += (int64_t)gridDim.x * kT) {
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += slab[z * row + i];
    if (i >= nw) {
      db[i - nw] += s;
    } else if (perm) {
      const int ci = (int)(i % Cin);
      int64_t r = i / Cin;
      const int tap = (int)(r % 16), co = (int)(r / 16);
      dw[((int64_t)co * Cin + ci) * 16 + tap] += s;
    } else {
      dw[i] += s;
    }
  }
}

// ------------------------------------------------------------------------------------------------ edge path (VALU, any channel counts)
// The edge layers' weights are small: each workgroup keeps them in LDS, rounded to bf16, as [(tap, ci)][co] -- lanes that differ in co
// (image layer) or in ci (logits layer) read neighbouring words instead of torch-layout words 64 bytes apart.  Above kWL words the
// kernels read the torch tensor directly.
constexpr int kWL = 12288;
__device__ __forceinline__ bool stage_weights(const float* __restrict__ w, float* wl, int Cin, int Cout) {
  const int nw = Cout * Cin * 16;
  if (nw > kWL) return false;
  for (int i = threadIdx.x; i < nw; i += kT) {
    const int tap = i & 15, ci = (i >> 4) % Cin, co = (i >> 4) / Cin;
    wl[(tap * Cin + ci) * Cout + co] = wbf(w[i]);
  }
  __syncthreads();
  return true;
}

// L lanes per output element stride over k = (tap, ci): 1 for the image layer (K = 16 Cin is tiny), 64 for the logits layer (Cout = 1)
template <int L>
__global__ void __launch_bounds__(kT) k_c2d_edge_fwd(const bf16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     bf16* __restrict__ y, int H, int W, int Cin, int Cout, int s, int Ho, int Wo, int64_t total) {
  __shared__ float wl[kWL];
  const bool staged = stage_weights(w, wl, Cin, Cout);
  const int64_t gid = blockIdx.x * (int64_t)kT + threadIdx.x;
  const int lane = (int)(gid % L);
  for (int64_t o = gid / L; o < total; o += (int64_t)gridDim.x * kT / L) {  // (L == 64: o is uniform over the wave)
    const int co = (int)(o % Cout);
    int64_t r = o / Cout;
    const int ow = (int)(r % Wo); r /= Wo;
    const int oh = (int)(r % Ho);
    const int n = (int)(r / Ho);
    float acc = 0.f;
    if (L == 1) {  // all 16 taps of a channel in flight at once: predicated loads, no branch
      for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll
        for (int tap = 0; tap < 16; ++tap) {
          const int ih = oh * s - 1 + (tap >> 2), iw = ow * s - 1 + (tap & 3);
          const bool in = (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
          const float xv = in ? bf2f(x[(((int64_t)n * H + ih) * W + iw) * Cin + ci]) : 0.f;
          acc += xv * (staged ? wl[(tap * Cin + ci) * Cout + co] : wbf(w[((int64_t)co * Cin + ci) * 16 + tap]));
        }
      }
    }
    for (int k = lane; L != 1 && k < 16 * Cin; k += L) {
      const int tap = k / Cin, ci = k - tap * Cin;
      const int ih = oh * s - 1 + (tap >> 2), iw = ow * s - 1 + (tap & 3);
      if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
        acc += bf2f(x[(((int64_t)n * H + ih) * W + iw) * Cin + ci]) * (staged ? wl[k * Cout + co] : wbf(w[((int64_t)co * Cin + ci) * 16 + tap]));
    }
    if (L == 64) acc = wave_sum(acc);
    if (lane == 0) y[o] = f2bf(acc + (bias ? bias[co] : 0.f));
  }
}

// one thread per (input pixel, ci): the (oh, ow, th, tw) that read the pixel, all co -- a gather
__global__ void __launch_bounds__(kT) k_c2d_edge_dgrad(const bf16* __restrict__ dy, const float* __restrict__ w, bf16* __restrict__ dx, int H, int W,
                                                       int Cin, int Cout, int s, int Ho, int Wo, int64_t total) {
  __shared__ float wl[kWL];
  const bool staged = stage_weights(w, wl, Cin, Cout);
  for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
    const int ci = (int)(i % Cin);
    int64_t r = i / Cin;
    const int iw = (int)(r % W); r /= W;
    const int ih = (int)(r % H);
    const int n = (int)(r / H);
    float acc = 0.f;
    for (int th = 0; th < 4; ++th) {
      const int nh = ih + 1 - th;
      if (nh < 0 || nh % s) continue;
      const int oh = nh / s;
      if (oh >= Ho) continue;
      for (int tw = 0; tw < 4; ++tw) {
        const int nw = iw + 1 - tw;
        if (nw < 0 || nw % s) continue;
        const int ow = nw / s;
        if (ow >= Wo) continue;
        const bf16* src = dy + (((int64_t)n * Ho + oh) * Wo + ow) * Cout;
        const float* wp = w + (int64_t)ci * 16 + th * 4 + tw;
        if (staged) {
          const float* wq = wl + ((th * 4 + tw) * Cin + ci) * Cout;
          int co = 0;
          if ((Cout & 7) == 0) {  // (then every pixel of dy starts on 16 bytes)
            for (; co < Cout; co += 8) {
              const F8 f = unpack8(*(const u32x4*)(src + co));
#pragma unroll
              for (int j = 0; j < 8; ++j) acc += f.v[j] * wq[co + j];
            }
          }
          for (; co < Cout; ++co) acc += bf2f(src[co]) * wq[co];
        } else {
          for (int co = 0; co < Cout; ++co) acc += bf2f(src[co]) * wbf(wp[(int64_t)co * Cin * 16]);
        }
      }
    }
    dx[i] = f2bf(acc);
  }
}

// blockIdx.x: pixel range, blockIdx.y: 1024 outputs (torch order [co][ci][tap], then the Cout bias sums when with_bias), 4 per thread
__global__ void __launch_bounds__(kT) k_c2d_edge_wgrad(const bf16* __restrict__ x, const bf16* __restrict__ dy, float* __restrict__ slab, int H, int W,
                                                       int Cin, int Cout, int s, int Ho, int Wo, int64_t P, int64_t per_split, int with_bias) {
  const int64_t nw = (int64_t)Cout * Cin * 16, row = nw + (with_bias ? Cout : 0);
  int co[4], ci[4], th[4], tw[4], kind[4];  // kind: 0 none, 1 weight, 2 bias
  int64_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = (int64_t)blockIdx.y * 1024 + j * kT + threadIdx.x;
    kind[j] = o[j] >= row ? 0 : (o[j] >= nw ? 2 : 1);
    co[j] = ci[j] = th[j] = tw[j] = 0;
    if (kind[j] == 2) co[j] = (int)(o[j] - nw);
    if (kind[j] == 1) {
      const int tap = (int)(o[j] % 16);
      th[j] = tap >> 2, tw[j] = tap & 3;
      ci[j] = (int)((o[j] / 16) % Cin);
      co[j] = (int)(o[j] / (16 * (int64_t)Cin));
    }
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t pbeg = (int64_t)blockIdx.x * per_split;
  const int64_t pend = pbeg + per_split < P ? pbeg + per_split : P;
#pragma unroll 4
  for (int pix = (int)pbeg; pix < (int)pend; ++pix) {  // (P <= N H W < 2^31: check_dims)
    const int r = pix / Wo, ow = pix - r * Wo;
    const int n = r / Ho, oh = r - n * Ho;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (kind[j] == 0) continue;
      const float g = bf2f(dy[(int64_t)pix * Cout + co[j]]);
      if (kind[j] == 2) {
        acc[j] += g;
      } else {
        const int ih = oh * s - 1 + th[j], iw = ow * s - 1 + tw[j];
        if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) acc[j] += g * bf2f(x[(((int64_t)n * H + ih) * W + iw) * Cin + ci[j]]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (kind[j]) slab[(int64_t)blockIdx.x * row + o[j]] = acc[j];
}

// ------------------------------------------------------------------------------------------------ host side
inline int check_dims(int N, int H, int W, int Cin, int Cout, int s) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (s != 1 && s != 2)) return MI_ERR_BAD_ARG;
  if (c2d_out_extent(H, s) < 1 || c2d_out_extent(W, s) < 1) return MI_ERR_BAD_ARG;
  if ((int64_t)N * H * W > 2147483647LL) return MI_ERR_UNSUPPORTED;
  return 0;
}
inline int check_mfma(int Cin, int Cout) { return (Cin % 16 || Cout % 32) ? MI_ERR_UNSUPPORTED : 0; }

int launch_gemm(const C2dGemmArgs& a, int ncls, hipStream_t st) {
  int64_t mmax = 0, t128 = 0;
  for (int c = 0; c < ncls; ++c) {
    mmax = a.M[c] > mmax ? a.M[c] : mmax;
    t128 += ceil_div(a.M[c], 128);
  }
  if (t128 * ceil_div(a.N, 128) < 256)  // fewer workgroups than CUs: quarter-size tiles (as mi_gemm_nt_bf16)
    hipLaunchKernelGGL(k_c2d_gemm<1>, dim3(ceil_div(mmax, 64), ceil_div(a.N, 64), ncls), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_c2d_gemm<2>, dim3(ceil_div(mmax, 128), ceil_div(a.N, 128), ncls), dim3(256), 0, st, a);
  MI_CHECK_LAUNCH();
  return 0;
}

inline int mfma_splits(int64_t P, int Cin, int Cout) {
  const int64_t tiles = (int64_t)ceil_div(Cout, 64) * ceil_div(16 * Cin, 64);
  int64_t s = 1024 / tiles, byp = (P + 127) / 128;
  s = s < byp ? s : byp;
  return (int)(s < 1 ? 1 : (s > 64 ? 64 : s));
}
inline int edge_splits(int64_t P) {
  const int64_t s = (P + 127) / 128;
  return (int)(s < 1 ? 1 : (s > 2048 ? 2048 : s));
}

}  // namespace

extern "C" {

int mi_conv2d_k4_pack(const float* w, void* w_fwd, void* w_dgrad, int Cin, int Cout, int stride, hipStream_t st) {
  if (!w || !w_fwd || Cin <= 0 || Cout <= 0 || (stride != 1 && stride != 2)) return MI_ERR_BAD_ARG;
  if (int e = check_mfma(Cin, Cout)) return e;
  hipLaunchKernelGGL(k_c2d_pack, dim3(grid_for((int64_t)16 * Cin * Cout)), dim3(kT), 0, st, w, (bf16*)w_fwd, (bf16*)w_dgrad, Cin, Cout, stride);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_conv2d_k4_fwd(const void* x, const void* w_fwd, void* y, int N, int H, int W, int Cin, int Cout, int stride, hipStream_t st) {
  if (!x || !w_fwd || !y) return MI_ERR_BAD_ARG;
  if (int e = check_dims(N, H, W, Cin, Cout, stride)) return e;
  if (int e = check_mfma(Cin, Cout)) return e;
  C2dGemmArgs a = {};
  a.src = (const bf16*)x, a.B = (const bf16*)w_fwd, a.dst = (bf16*)y;
  a.g[0] = c2d_fwd_geom(H, W, Cin, Cout, stride);
  a.M[0] = c2d_rows(a.g[0], N);
  a.sB = 0, a.N = Cout, a.K = c2d_k(a.g[0]);
  return launch_gemm(a, 1, st);
}

int mi_conv2d_k4_dgrad(const void* dy, const void* w_dgrad, void* dx, int N, int H, int W, int Cin, int Cout, int stride, hipStream_t st) {
  if (!dy || !w_dgrad || !dx) return MI_ERR_BAD_ARG;
  if (int e = check_dims(N, H, W, Cin, Cout, stride)) return e;
  if (int e = check_mfma(Cin, Cout)) return e;
  const int ncls = stride == 2 ? 4 : 1;
  C2dGemmArgs a = {};
  a.src = (const bf16*)dy, a.B = (const bf16*)w_dgrad, a.dst = (bf16*)dx;
  for (int c = 0; c < ncls; ++c) {
    a.g[c] = c2d_dgrad_geom(H, W, Cin, Cout, stride, c);
    a.M[c] = c2d_rows(a.g[c], N);
  }
  a.N = Cin, a.K = c2d_k(a.g[0]);
  a.sB = (int64_t)Cin * a.K;
  return launch_gemm(a, ncls, st);
}

int mi_conv2d_k4_wgrad_splits(int N, int H, int W, int Cin, int Cout, int stride) {
  if (check_dims(N, H, W, Cin, Cout, stride) || check_mfma(Cin, Cout)) return 0;
  return mfma_splits((int64_t)N * c2d_out_extent(H, stride) * c2d_out_extent(W, stride), Cin, Cout);
}

int mi_conv2d_k4_wgrad(const void* x, const void* dy, float* dw, float* workspace, int N, int H, int W, int Cin, int Cout, int stride,
                       hipStream_t st) {
  if (!x || !dy || !dw || !workspace) return MI_ERR_BAD_ARG;
  if (int e = check_dims(N, H, W, Cin, Cout, stride)) return e;
  if (int e = check_mfma(Cin, Cout)) return e;
  C2dWgradArgs a;
  a.x = (const bf16*)x, a.dy = (const bf16*)dy, a.slab = workspace;
  a.g = c2d_fwd_geom(H, W, Cin, Cout, stride);
  a.P = c2d_rows(a.g, N);
  const int splits = mfma_splits(a.P, Cin, Cout);
  a.per_split = ((a.P + splits - 1) / splits + 63) / 64 * 64;
  a.Cout = Cout, a.K = 16 * Cin;
  hipLaunchKernelGGL(k_c2d_wgrad, dim3(ceil_div(a.K, 64), ceil_div(Cout, 64), splits), dim3(256), 0, st, a);
  MI_CHECK_LAUNCH();
  const int64_t row = (int64_t)Cout * a.K;
  hipLaunchKernelGGL(k_c2d_fold, dim3(grid_for(row)), dim3(kT), 0, st, workspace, splits, row, dw, (float*)nullptr, Cin, Cout, 1);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_conv2d_k4_edge_fwd(const void* x, const float* w, const float* bias, void* y, int N, int H, int W, int Cin, int Cout, int stride,
                          hipStream_t st) {
  if (!x || !w || !y) return MI_ERR_BAD_ARG;
  if (int e = check_dims(N, H, W, Cin, Cout, stride)) return e;
  const int Ho = c2d_out_extent(H, stride), Wo = c2d_out_extent(W, stride);
  const int64_t total = (int64_t)N * Ho * Wo * Cout;
  if (16 * Cin <= 128)
    hipLaunchKernelGGL(k_c2d_edge_fwd<1>, dim3(grid_for(total)), dim3(kT), 0, st, (const bf16*)x, w, bias, (bf16*)y, H, W, Cin, Cout, stride, Ho, Wo, total);
  else
    hipLaunchKernelGGL(k_c2d_edge_fwd<64>, dim3(grid_for(total * 64)), dim3(kT), 0, st, (const bf16*)x, w, bias, (bf16*)y, H, W, Cin, Cout, stride, Ho, Wo,
                       total);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_conv2d_k4_edge_dgrad(const void* dy, const float* w, void* dx, int N, int H, int W, int Cin, int Cout, int stride, hipStream_t st) {
  if (!dy || !w || !dx) return MI_ERR_BAD_ARG;
  if (int e = check_dims(N, H, W, Cin, Cout, stride)) return e;
  const int64_t total = (int64_t)N * H * W * Cin;
  hipLaunchKernelGGL(k_c2d_edge_dgrad, dim3(grid_for(total)), dim3(kT), 0, st, (const bf16*)dy, w, (bf16*)dx, H, W, Cin, Cout, stride,
                     c2d_out_extent(H, stride), c2d_out_extent(W, stride), total);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_conv2d_k4_edge_wgrad_splits(int N, int H, int W, int Cin, int Cout, int stride) {
  if (check_dims(N, H, W, Cin, Cout, stride)) return 0;
  return edge_splits((int64_t)N * c2d_out_extent(H, stride) * c2d_out_extent(W, stride));
}

int mi_conv2d_k4_edge_wgrad(const void* x, const void* dy, float* dw, float* dbias, float* workspace, int N, int H, int W, int Cin, int Cout,
                            int stride, hipStream_t st) {
  if (!x || !dy || !dw || !workspace) return MI_ERR_BAD_ARG;
  if (int e = check_dims(N, H, W, Cin, Cout, stride)) return e;
  const int Ho = c2d_out_extent(H, stride), Wo = c2d_out_extent(W, stride);
  const int64_t P = (int64_t)N * Ho * Wo, row = (int64_t)Cout * Cin * 16 + (dbias ? Cout : 0);
  if (row > 1024 * 65535LL) return MI_ERR_UNSUPPORTED;
  const int splits = edge_splits(P);
  const int64_t per = (P + splits - 1) / splits;
  hipLaunchKernelGGL(k_c2d_edge_wgrad, dim3(splits, ceil_div(row, 1024)), dim3(kT), 0, st, (const bf16*)x, (const bf16*)dy, workspace, H, W, Cin, Cout,
                     stride, Ho, Wo, P, per, dbias ? 1 : 0);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_c2d_fold, dim3(grid_for(row)), dim3(kT), 0, st, workspace, splits, row, dw, dbias, Cin, Cout, 0);
  MI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
