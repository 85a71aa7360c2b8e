// Distribution metrics of the LDM's validation (train_ldm.py:32 `FIDMetric, MMDMetric`, :308-310 `fid(synth_features, real_features)`;
// third-party `generative.metrics` classes: PARITY UNPINNED, see metrics.py for the restated formulas) plus KID.  Everything is fp64 on
// the device; the inputs are fp32 rows of two groups (group 0: n rows at z0, group 1: m rows at z1; R = n + m, row pitch K).
//   - k_dm_colmean: per-group column means, one thread per column, rows added in row order.
//   - k_dm_gram: G = Zc Zc^T with Zc the rows minus their group's mean (no mean: the raw rows).  v_mfma_f64_16x16x4_f64 tiles; the A and
//     the B operand of a row tile are the same fragment (lane l holds Zc[16 t + (l & 15)][k0 + (l >> 4)]), and the result lane map is
//     col = l & 15, row = (l >> 4) + 4 * reg (NOT the f32 forms' map).  A workgroup owns a pair of 64-row panels (bi <= bj) and one K
//     chunk: 64-column stages go through LDS (coalesced fp32 loads, centred to fp64 on the way in, the next two stages' loads in flight
//     while this one is multiplied), its four waves split the 16 k-steps of a stage, and their accumulators are added in wave order.
//     Only tile pairs with tj >= ti are computed.  R <= 64 is one panel pair: the grid is the K chunks alone and Z is read from HBM
//     once (the MMD shape: a few images by millions of voxels).  Rows >= R and columns >= K are zero in LDS, never read.
//   - k_dm_gram_reduce: adds the chunk partials of every entry in chunk order and writes both triangles.  No floating-point atomics
//     anywhere: two runs are bit-equal.
//   - one-sided (Hestenes) Jacobi on a column-major r x c' work matrix (c' = c rounded up to even, the pad column zero): round-robin
//     ordering, c' - 1 rounds of c' / 2 disjoint column pairs per sweep.  k_dm_jacobi_round: one workgroup per pair, one launch per round.
//     k_dm_jacobi_sweep_lds: when r * c' <= JACOBI_LDS_DOUBLES (8192 doubles = 64 KiB of LDS) one workgroup holds the matrix, a wave
//     takes a pair, and all rounds of a sweep run in one launch with a barrier between rounds.  A pair rotates only when
//     |gamma| > 2^-50 sqrt(alpha beta) and alpha beta > 0; every rotation bumps an int counter (integer atomicAdd), which the host reads
//     once per sweep.  No kernel waits on another workgroup.
//   - k_dm_jacobi_norms: the column norms (singular values) and their sum; k_dm_finalize: the scalar scores.  Both are one workgroup
//     with a fixed summation order.
#include "common.h"
#include "medimgen_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int kT = 256;
constexpr int PANEL = 64;                    // rows of a panel: 4 MFMA row tiles
constexpr int KS = 64;                       // columns of a stage
constexpr int LDP = KS + 1;                  // LDS row pitch in doubles: the 16 rows of a fragment read fall into 16 different bank pairs
constexpr int PANEL_DOUBLES = PANEL * LDP;
constexpr int JACOBI_LDS_DOUBLES = 8192;     // r * c' at or below this: the single-workgroup sweep
constexpr int JACOBI_LDS_THREADS = 512;
constexpr int MAX_SWEEPS = 60;

// sum over the 256 threads, the same value in every thread; the order is fixed: per-thread value, xor butterfly, waves 0..3
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ------------------------------------------------------------------------------------------------------------------ column means
__global__ void __launch_bounds__(kT) k_dm_colmean(const float* __restrict__ z0, const float* __restrict__ z1, int n, int m, int64_t K,
                                                   double* __restrict__ mean) {
  const int64_t k = blockIdx.x * (int64_t)kT + threadIdx.x;
  if (k >= K) return;
  const int g = blockIdx.y;
  const float* z = g ? z1 : z0;
  const int rows = g ? m : n;
  double s = 0.0;
  for (int r = 0; r < rows; ++r) s += (double)z[(int64_t)r * K + k];
  mean[(int64_t)g * K + k] = s / (double)rows;
}

// ------------------------------------------------------------------------------------------------------------------ Gram matrix
struct GramPlan {
  int nmac, mpairs, nts, chunks;
  int64_t KC;
};

inline GramPlan gram_plan(int R, int64_t K) {
  GramPlan p;
  p.nmac = (R + PANEL - 1) / PANEL;
  p.mpairs = p.nmac * (p.nmac + 1) / 2;
  const int nt = (R + 15) / 16;
  p.nts = nt < 4 ? nt : 4;
  int64_t want;
  if (p.nmac == 1) {  // one panel pair: the K chunks are the whole grid
    want = (K + 2047) / 2048;
    want = want > 512 ? 512 : want;  // two workgroups per CU are resident; the chunk partials are added one after the other
  } else {  // enough workgroups to fill the chip, chunks of 512 columns at least
    want = (512 + p.mpairs - 1) / p.mpairs;
    const int64_t most = (K + 511) / 512;
    want = want > most ? most : want;
  }
  want = want < 1 ? 1 : want;
  p.KC = ((K + want - 1) / want + KS - 1) / KS * KS;
  p.chunks = (int)((K + p.KC - 1) / p.KC);
  return p;
}

// macro pair index -> (bi, bj), bi <= bj, rows of pairs (0,0) (0,1) .. (0,nmac-1) (1,1) ..
__device__ __forceinline__ void macro_pair(int mp, int nmac, int& bi, int& bj) {
  bi = 0;
  while (mp >= nmac - bi) {
    mp -= nmac - bi;
    ++bi;
  }
  bj = bi + mp;
}

struct GramArgs {
  const float* z0;
  const float* z1;
  const double* mean;  // [2][K] or NULL
  double* ws;          // [mpairs][chunks][nts * nts][256]
  int R, n, nmac, nts, chunks;
  int64_t K, KC;
};

// SINGLE: the one-panel grid (R <= 64): the only pair is the diagonal one, known at compile time (no second panel, no lower tiles)
template <bool SINGLE>
__global__ void __launch_bounds__(kT) k_dm_gram(GramArgs a) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.x, mp = blockIdx.y;
  int bi, bj;
  macro_pair(mp, a.nmac, bi, bj);
  const bool diag = SINGLE || bi == bj;
  double* sA = smem;
  double* sB = diag ? smem : smem + PANEL_DOUBLES;
  const int rowA = bi * PANEL, rowB = bj * PANEL;
  const int ntA = (min(PANEL, a.R - rowA) + 15) / 16, ntB = (min(PANEL, a.R - rowB) + 15) / 16;
  const int64_t kbeg = chunk * a.KC, kend = min(a.K, kbeg + a.KC);
  const int nstage = (int)((kend - kbeg + KS - 1) / KS);
  const int kk = tid & (KS - 1), r0 = tid >> 6;  // this thread stages column kk of rows r0, r0 + 4, ..

  // a stage's loads in registers: two stages are in flight while a third is multiplied (one 64-column stage is 8 KiB per 32 rows: a
  // single one in flight per workgroup leaves the pass waiting on memory latency)
  struct Stage {
    float a[16], b[16];
    double m0, m1;
    bool kok;
  };
  auto load_stage = [&](int s, Stage& g) {
    const int64_t k = kbeg + (int64_t)s * KS + kk;
    g.kok = k < kend;
    g.m0 = g.kok && a.mean ? a.mean[k] : 0.0;
    g.m1 = g.kok && a.mean ? a.mean[a.K + k] : 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int ra = rowA + r0 + 4 * j, rb = rowB + r0 + 4 * j;
      g.a[j] = 0.f;
      g.b[j] = 0.f;
      if (g.kok && j < 4 * ntA && ra < a.R) g.a[j] = ra < a.n ? a.z0[(int64_t)ra * a.K + k] : a.z1[(int64_t)(ra - a.n) * a.K + k];
      if (g.kok && !diag && j < 4 * ntB && rb < a.R) g.b[j] = rb < a.n ? a.z0[(int64_t)rb * a.K + k] : a.z1[(int64_t)(rb - a.n) * a.K + k];
    }
  };
  auto centred = [&](const Stage& g, float v, int row) { return g.kok && row < a.R ? (double)v - (row < a.n ? g.m0 : g.m1) : 0.0; };

  f64x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  // stage s: registers -> LDS (centred, zero outside R x K), refill the registers with stage s + 2, multiply
  auto run_stage = [&](int s, Stage& g) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int rr = r0 + 4 * j;
      if (j < 4 * ntA) sA[rr * LDP + kk] = centred(g, g.a[j], rowA + rr);
      if (!diag && j < 4 * ntB) sB[rr * LDP + kk] = centred(g, g.b[j], rowB + rr);
    }
    __syncthreads();
    if (s + 2 < nstage) load_stage(s + 2, g);
#pragma unroll
    for (int i = 0; i < KS / 16; ++i) {
      const int kcol = (wave + 4 * i) * 4 + (lane >> 4);
      double fa[4], fb[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        fa[t] = t < ntA ? sA[(t * 16 + (lane & 15)) * LDP + kcol] : 0.0;
        fb[t] = t < ntB ? sB[(t * 16 + (lane & 15)) * LDP + kcol] : 0.0;
      }
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
          if (ti < ntA && tj < ntB && (!diag || tj >= ti)) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ti], fb[tj], acc[ti][tj], 0, 0, 0);
    }
    __syncthreads();
  };
  Stage g0, g1;
  load_stage(0, g0);
  if (nstage > 1) load_stage(1, g1);
  for (int s = 0; s < nstage; s += 2) {  // nstage is uniform over the workgroup
    run_stage(s, g0);
    if (s + 1 < nstage) run_stage(s + 1, g1);
  }

  // the four waves' accumulators, added in wave order; entry tid = reg * 64 + lane of the tile
  double* red = smem;  // 4 * 256 doubles, inside the first panel
  double* out = a.ws + ((int64_t)mp * a.chunks + chunk) * (a.nts * a.nts) * kT;
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
      if (ti < ntA && tj < ntB && (!diag || tj >= ti)) {  // uniform over the workgroup
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[ti][tj][r];
        __syncthreads();
        out[(ti * a.nts + tj) * kT + tid] = ((red[tid] + red[kT + tid]) + red[2 * kT + tid]) + red[3 * kT + tid];
        __syncthreads();
      }
}

__global__ void __launch_bounds__(kT) k_dm_gram_reduce(const double* __restrict__ ws, double* __restrict__ G, int R, int nmac, int nts,
                                                       int chunks) {
  const int tid = threadIdx.x, lane = tid & 63, reg = tid >> 6;
  const int slot = blockIdx.x, mp = blockIdx.y;
  const int ti = slot / nts, tj = slot - ti * nts;
  int bi, bj;
  macro_pair(mp, nmac, bi, bj);
  const bool diag = bi == bj;
  if (diag && tj < ti) return;
  const int gi = bi * PANEL + ti * 16 + (lane >> 4) + 4 * reg;  // the f64 MFMA result map
  const int gj = bj * PANEL + tj * 16 + (lane & 15);
  if (gi >= R || gj >= R) return;
  const int64_t stride = (int64_t)nts * nts * kT;
  const double* p = ws + (int64_t)mp * chunks * stride + (int64_t)slot * kT + tid;
  double s = 0.0;
  int c = 0;
  for (; c + 16 <= chunks; c += 16) {  // 16 loads in flight, added in chunk order
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = p[(c + u) * stride];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += v[u];
  }
  for (; c < chunks; ++c) s += p[c * stride];
  G[(int64_t)gi * R + gj] = s;
  if (!(diag && ti == tj)) G[(int64_t)gj * R + gi] = s;  // a diagonal tile holds both of its triangles already
}

// ------------------------------------------------------------------------------------------------------------------ Jacobi
__global__ void __launch_bounds__(kT) k_dm_jacobi_init(const double* __restrict__ G, int R, int n, int m, double* __restrict__ A,
                                                       int* __restrict__ counters) {
  const int r = n >= m ? n : m, c = n >= m ? m : n, cp = c + (c & 1);
  const int64_t total = (int64_t)r * cp;
  for (int64_t e = blockIdx.x * (int64_t)kT + threadIdx.x; e < total; e += (int64_t)gridDim.x * kT) {
    const int j = (int)(e / r), i = (int)(e - (int64_t)j * r);
    double v = 0.0;
    if (j < c) v = n >= m ? G[(int64_t)i * R + n + j] : G[(int64_t)j * R + n + i];  // the n x m block, transposed when m > n
    A[e] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < MAX_SWEEPS) counters[threadIdx.x] = 0;
}

// round-robin (circle method): column c' - 1 stays, the others rotate; the c' / 2 pairs of a round are disjoint
__device__ __forceinline__ void round_pair(int rd, int i, int cp, int& p, int& q) {
  const int N = cp - 1;
  if (i == 0) {
    p = N;
    q = rd;
  } else {
    p = (rd + i) % N;
    q = (rd - i + N) % N;
  }
}

// alpha = |a_p|^2, beta = |a_q|^2, gamma = a_p . a_q -> rotate?  and the rotation's (c, s)
__device__ __forceinline__ bool jacobi_rotation(double alpha, double beta, double gamma, double& cs, double& sn) {
  const double ab = alpha * beta;
  if (!(ab > 0.0) || !(fabs(gamma) > 0x1p-50 * sqrt(ab))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = zeta == 0.0 ? 1.0 : copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  cs = 1.0 / sqrt(1.0 + t * t);
  sn = cs * t;
  return true;
}

__global__ void __launch_bounds__(kT) k_dm_jacobi_round(double* __restrict__ A, int r, int cp, int rd, int* __restrict__ counter) {
  __shared__ double red[3][4];
  int p, q;
  round_pair(rd, blockIdx.x, cp, p, q);
  double* ap = A + (int64_t)p * r;
  double* aq = A + (int64_t)q * r;
  double alpha = 0.0, beta = 0.0, gamma = 0.0;
  for (int i = threadIdx.x; i < r; i += kT) {
    const double x = ap[i], y = aq[i];
    alpha += x * x;
    beta += y * y;
    gamma += x * y;
  }
  alpha = block_sum_f64(alpha, red[0]);
  beta = block_sum_f64(beta, red[1]);
  gamma = block_sum_f64(gamma, red[2]);
  double cs, sn;
  if (!jacobi_rotation(alpha, beta, gamma, cs, sn)) return;  // uniform: every thread holds the same sums
  for (int i = threadIdx.x; i < r; i += kT) {
    const double x = ap[i], y = aq[i];
    ap[i] = cs * x - sn * y;
    aq[i] = sn * x + cs * y;
  }
  if (threadIdx.x == 0) atomicAdd(counter, 1);
}

__global__ void __launch_bounds__(JACOBI_LDS_THREADS) k_dm_jacobi_sweep_lds(double* __restrict__ A, int r, int cp, int* __restrict__ counter) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int total = r * cp;  // <= JACOBI_LDS_DOUBLES
  for (int e = tid; e < total; e += JACOBI_LDS_THREADS) smem[e] = A[e];
  __syncthreads();
  int rotations = 0;
  for (int rd = 0; rd < cp - 1; ++rd) {
    for (int i = wave; i < cp / 2; i += JACOBI_LDS_THREADS / 64) {
      int p, q;
      round_pair(rd, i, cp, p, q);
      double* ap = smem + p * r;
      double* aq = smem + q * r;
      double alpha = 0.0, beta = 0.0, gamma = 0.0;
      for (int k = lane; k < r; k += 64) {
        const double x = ap[k], y = aq[k];
        alpha += x * x;
        beta += y * y;
        gamma += x * y;
      }
      alpha = wave_sum_f64(alpha);
      beta = wave_sum_f64(beta);
      gamma = wave_sum_f64(gamma);
      double cs, sn;
      if (jacobi_rotation(alpha, beta, gamma, cs, sn)) {  // uniform over the wave
        for (int k = lane; k < r; k += 64) {
          const double x = ap[k], y = aq[k];
          ap[k] = cs * x - sn * y;
          aq[k] = sn * x + cs * y;
        }
        ++rotations;
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < total; e += JACOBI_LDS_THREADS) A[e] = smem[e];
  if (lane == 0 && rotations) atomicAdd(counter, rotations);
}

__global__ void __launch_bounds__(kT) k_dm_jacobi_norms(const double* __restrict__ A, int r, int c, double* __restrict__ sv,
                                                        double* __restrict__ nuc) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < c; j += kT / 64) {
    const double* a = A + (int64_t)j * r;
    double s = 0.0;
    for (int i = lane; i < r; i += 64) s += a[i] * a[i];
    s = wave_sum_f64(s);
    if (lane == 0) sv[j] = sqrt(s);
  }
  __syncthreads();  // sv written by this workgroup: visible after the barrier
  double s = 0.0;
  for (int j = threadIdx.x; j < c; j += kT) s += sv[j];
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) *nuc = s;
}

// ------------------------------------------------------------------------------------------------------------------ scores
__device__ __forceinline__ double score_kernel(double g, int degree, double gamma, double coef0) {
  const double k = gamma * g + coef0;
  double v = k;
  for (int d = 1; d < degree; ++d) v *= k;
  return v;
}

// sum over rows [i0, i0 + ni) x columns [j0, j0 + nj) of k(G), the diagonal i - i0 == j - j0 left out when offdiag
__device__ double block_kernel_sum(const double* __restrict__ G, int R, int i0, int ni, int j0, int nj, bool offdiag, bool poly, int degree,
                                   double gamma, double coef0, double* red) {
  const int64_t total = (int64_t)ni * nj;
  double s = 0.0;
  for (int64_t e = threadIdx.x; e < total; e += kT) {
    const int i = (int)(e / nj), j = (int)(e - (int64_t)i * nj);
    if (offdiag && i == j) continue;
    const double g = G[(int64_t)(i0 + i) * R + j0 + j];
    s += poly ? score_kernel(g, degree, gamma, coef0) : g;
  }
  return block_sum_f64(s, red);
}

__global__ void __launch_bounds__(kT) k_dm_finalize(int mode, const double* __restrict__ G, int n, int m, const double* __restrict__ mean, int64_t K,
                                                    const double* __restrict__ nuc, int degree, double gamma, double coef0, double* __restrict__ out) {
  __shared__ double red[4];
  const int R = n + m;
  double t1, t2, t3;
  if (mode == MI_DM_FID) {
    double d = 0.0, tx = 0.0, ty = 0.0;
    for (int64_t k = threadIdx.x; k < K; k += kT) {
      const double v = mean[k] - mean[K + k];
      d += v * v;
    }
    for (int i = threadIdx.x; i < n; i += kT) tx += G[(int64_t)i * R + i];
    for (int i = n + threadIdx.x; i < R; i += kT) ty += G[(int64_t)i * R + i];
    d = block_sum_f64(d, red);
    tx = block_sum_f64(tx, red);
    ty = block_sum_f64(ty, red);
    t1 = d;
    t2 = tx / (double)(n - 1) + ty / (double)(m - 1);
    t3 = 2.0 * *nuc / sqrt((double)(n - 1) * (double)(m - 1));
  } else {
    const bool poly = mode == MI_DM_KID;
    const double sxx = block_kernel_sum(G, R, 0, n, 0, n, true, poly, degree, gamma, coef0, red);
    const double syy = block_kernel_sum(G, R, n, m, n, m, true, poly, degree, gamma, coef0, red);
    const double sxy = block_kernel_sum(G, R, 0, n, n, m, false, poly, degree, gamma, coef0, red);
    t1 = sxx / ((double)n * (double)(n - 1));
    t2 = syy / ((double)m * (double)(m - 1));
    t3 = 2.0 * sxy / ((double)n * (double)m);
  }
  if (threadIdx.x == 0) {
    out[0] = (t1 + t2) - t3;
    out[1] = t1;
    out[2] = t2;
    out[3] = t3;
  }
}

inline bool groups_ok(const void* z0, const void* z1, int n, int m, int64_t K) { return z0 && z1 && n >= 1 && m >= 1 && K >= 1 && (int64_t)n + m < (1 << 30); }

}  // namespace

extern "C" {

int mi_dm_colmean(const float* z0, const float* z1, int n, int m, int64_t K, double* mean, hipStream_t st) {
  if (!groups_ok(z0, z1, n, m, K) || !mean || (K + kT - 1) / kT > 0x7fffffff) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_dm_colmean, dim3((unsigned)((K + kT - 1) / kT), 2), dim3(kT), 0, st, z0, z1, n, m, K, mean);
  MI_CHECK_LAUNCH();
  return 0;
}

int64_t mi_dm_gram_workspace_bytes(int R, int64_t K) {
  if (R < 1 || K < 1) return 0;
  const GramPlan p = gram_plan(R, K);
  return (int64_t)p.mpairs * p.chunks * p.nts * p.nts * kT * (int64_t)sizeof(double);
}

int mi_dm_gram_single_pass(int R) { return R >= 1 && R <= PANEL; }

int mi_dm_gram(const float* z0, const float* z1, int n, int m, int64_t K, const double* mean, double* G, double* workspace, hipStream_t st) {
  if (!groups_ok(z0, z1, n, m, K) || !G || !workspace) return MI_ERR_BAD_ARG;
  const int R = n + m;
  const GramPlan p = gram_plan(R, K);
  if (p.mpairs > 65535) return MI_ERR_UNSUPPORTED;  // grid.y
  GramArgs a;
  a.z0 = z0;
  a.z1 = z1;
  a.mean = mean;
  a.ws = workspace;
  a.R = R;
  a.n = n;
  a.nmac = p.nmac;
  a.nts = p.nts;
  a.chunks = p.chunks;
  a.K = K;
  a.KC = p.KC;
  const size_t lds = (size_t)(p.nmac == 1 ? 1 : 2) * PANEL_DOUBLES * sizeof(double);  // 33 KiB or 65 KiB
  if (p.nmac == 1) {
    hipLaunchKernelGGL(k_dm_gram<true>, dim3(p.chunks, 1), dim3(kT), lds, st, a);
  } else {
    static bool attr_set = false;
    if (!attr_set) {
      hipError_t e = hipFuncSetAttribute((const void*)k_dm_gram<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
      attr_set = true;
    }
    hipLaunchKernelGGL(k_dm_gram<false>, dim3(p.chunks, p.mpairs), dim3(kT), lds, st, a);
  }
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dm_gram_reduce, dim3(p.nts * p.nts, p.mpairs), dim3(kT), 0, st, (const double*)workspace, G, R, p.nmac, p.nts, p.chunks);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_dm_jacobi_max_sweeps(void) { return MAX_SWEEPS; }

int mi_dm_jacobi_single_workgroup(int n, int m) {
  if (n < 1 || m < 1) return 0;
  const int r = n >= m ? n : m, c = n >= m ? m : n, cp = c + (c & 1);
  return (int64_t)r * cp <= JACOBI_LDS_DOUBLES;
}

int mi_dm_jacobi_init(const double* G, int n, int m, double* A, int* counters, hipStream_t st) {
  if (!G || !A || !counters || n < 1 || m < 1) return MI_ERR_BAD_ARG;
  const int r = n >= m ? n : m, c = n >= m ? m : n, cp = c + (c & 1);
  const int64_t total = (int64_t)r * cp;
  int64_t g = (total + kT - 1) / kT;
  g = g > 4096 ? 4096 : g;
  hipLaunchKernelGGL(k_dm_jacobi_init, dim3((unsigned)g), dim3(kT), 0, st, G, n + m, n, m, A, counters);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_dm_jacobi_round(double* A, int r, int cp, int round, int* counter, hipStream_t st) {
  if (!A || !counter || r < 1 || cp < 2 || (cp & 1) || cp > r + 1 || round < 0 || round >= cp - 1) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_dm_jacobi_round, dim3(cp / 2), dim3(kT), 0, st, A, r, cp, round, counter);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_dm_jacobi_sweep(double* A, int r, int cp, int* counter, hipStream_t st) {
  if (!A || !counter || r < 1 || cp < 2 || (cp & 1) || cp > r + 1) return MI_ERR_BAD_ARG;
  if ((int64_t)r * cp <= JACOBI_LDS_DOUBLES) {
    static bool attr_set = false;
    if (!attr_set) {
      hipError_t e = hipFuncSetAttribute((const void*)k_dm_jacobi_sweep_lds, hipFuncAttributeMaxDynamicSharedMemorySize, JACOBI_LDS_DOUBLES * (int)sizeof(double));
      if (e != hipSuccess) return (int)e;
      attr_set = true;
    }
    hipLaunchKernelGGL(k_dm_jacobi_sweep_lds, dim3(1), dim3(JACOBI_LDS_THREADS), (size_t)r * cp * sizeof(double), st, A, r, cp, counter);
    MI_CHECK_LAUNCH();
    return 0;
  }
  for (int rd = 0; rd < cp - 1; ++rd) {
    const int rc = mi_dm_jacobi_round(A, r, cp, rd, counter, st);
    if (rc) return rc;
  }
  return 0;
}

int mi_dm_jacobi_norms(const double* A, int r, int c, double* sv, double* nuc, hipStream_t st) {
  if (!A || !sv || !nuc || r < 1 || c < 1 || c > r) return MI_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_dm_jacobi_norms, dim3(1), dim3(kT), 0, st, A, r, c, sv, nuc);
  MI_CHECK_LAUNCH();
  return 0;
}

int mi_dm_finalize(int mode, const double* G, int n, int m, const double* mean, int64_t K, const double* nuc, int degree, double gamma,
                   double coef0, double* out, hipStream_t st) {
  if (!G || !out || n < 2 || m < 2) return MI_ERR_BAD_ARG;
  if (mode == MI_DM_FID) {
    if (!mean || !nuc || K < 1) return MI_ERR_BAD_ARG;
  } else if (mode == MI_DM_KID) {
    if (degree < 1) return MI_ERR_BAD_ARG;
  } else if (mode != MI_DM_MMD) {
    return MI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(k_dm_finalize, dim3(1), dim3(kT), 0, st, mode, G, n, m, mean, K, nuc, degree, gamma, coef0, out);
  MI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
