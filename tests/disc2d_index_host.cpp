// Host walk of csrc/conv2d_k4_index.h (tests/test_disc2d_cpu.py compiles and runs it): every (row, 16-byte piece) the three MFMA kernels of
// csrc/disc2d.hip gather, for one layer shape.
//   usage: disc2d_index_host N Cin Cout H W stride unfold.bin
// unfold.bin: int32 [N][Cin * 16][Ho * Wo] = F.unfold(ids, 4, padding=1, stride) of ids[n][c][h][w] = 1 + NHWC element offset (0: padding).
//   forward / weight gradient map: each valid address lies inside x and is the element F.unfold puts there; invalid <=> unfold's zero
//   data gradient map: each valid address lies inside dy; the (dy pixel, tap) pairs of the dx pixel a row writes are exactly the pairs
//   of the forward relation (each once, none missing); every dx pixel is written exactly once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv2d_k4_index.h"

#define CHECK(c, ...)                       \
  do {                                      \
    if (!(c)) {                             \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);    \
      std::fprintf(stderr, "\n");           \
      return 1;                             \
    }                                       \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int N = std::atoi(argv[1]), Cin = std::atoi(argv[2]), Cout = std::atoi(argv[3]), H = std::atoi(argv[4]), W = std::atoi(argv[5]),
            s = std::atoi(argv[6]);
  const int Ho = c2d_out_extent(H, s), Wo = c2d_out_extent(W, s);
  CHECK(Ho >= 1 && Wo >= 1, "output extent");
  const int64_t L = (int64_t)Ho * Wo, nx = (int64_t)N * H * W * Cin, ny = (int64_t)N * L * Cout;
  std::vector<int32_t> unf((size_t)N * Cin * 16 * L);
  {
    std::FILE* f = std::fopen(argv[7], "rb");
    CHECK(f, "cannot open %s", argv[7]);
    const size_t got = std::fread(unf.data(), sizeof(int32_t), unf.size(), f);
    std::fclose(f);
    CHECK(got == unf.size(), "short read: %zu of %zu", got, unf.size());
  }

  // ---- forward map (the weight gradient gathers x through the same map)
  const C2dGeom g = c2d_fwd_geom(H, W, Cin, Cout, s);
  CHECK(c2d_rows(g, N) == N * L && c2d_k(g) == 16 * Cin, "forward extents");
  int64_t fwd_pairs = 0;
  for (int64_t m = 0; m < N * L; ++m) {
    const int64_t n = m / L, l = m % L;
    const int64_t d = c2d_dst(g, m);
    CHECK(d == m * Cout && d + Cout <= ny, "forward destination of row %lld", (long long)m);
    for (int k = 0; k < 16 * Cin; k += 8) {
      int64_t off;
      const bool ok = c2d_src(g, m, k, &off);
      int tap, c;
      c2d_tap(g, k, &tap, &c);
      CHECK(tap == k / Cin && c == k % Cin && c + 8 <= Cin, "tap of k %d", k);
      if (ok) CHECK(off >= 0 && off + 8 <= nx && off % 8 == 0, "row %lld k %d: offset %lld outside x", (long long)m, k, (long long)off);
      for (int j = 0; j < 8; ++j) {
        const int32_t want = unf[((size_t)n * Cin * 16 + (size_t)(c + j) * 16 + tap) * L + l];
        CHECK(ok ? want == off + j + 1 : want == 0, "row %lld k %d: gathers %lld, unfold has %d", (long long)m, k + j,
              ok ? (long long)(off + j) : -1LL, want - 1);
      }
      fwd_pairs += ok && c == 0;
    }
  }

  // ---- data gradient maps
  const int ncls = s == 2 ? 4 : 1;
  std::vector<char> seen_pair((size_t)N * L * 16, 0), seen_dst((size_t)N * H * W, 0);
  int64_t dg_pairs = 0, dst_rows = 0;
  for (int cls = 0; cls < ncls; ++cls) {
    const C2dGeom q = c2d_dgrad_geom(H, W, Cin, Cout, s, cls);
    CHECK(c2d_k(q) * ncls == 16 * Cout, "data-gradient K");
    const int64_t M = c2d_rows(q, N);
    for (int64_t m = 0; m < M; ++m) {
      const int64_t d = c2d_dst(q, m);
      CHECK(d >= 0 && d + Cin <= nx && d % Cin == 0, "class %d row %lld: destination outside dx", cls, (long long)m);
      const int64_t dpix = d / Cin;
      CHECK(!seen_dst[dpix], "dx pixel %lld written twice", (long long)dpix);
      seen_dst[dpix] = 1, ++dst_rows;
      const int iw = (int)(dpix % W), ih = (int)(dpix / W % H), n = (int)(dpix / W / H);
      for (int k = 0; k < c2d_k(q); k += 8) {
        int64_t off;
        const bool ok = c2d_src(q, m, k, &off);
        int tap, co;
        c2d_tap(q, k, &tap, &co);
        CHECK(tap >= 0 && tap < 16 && co >= 0 && co + 8 <= Cout, "class %d k %d: tap", cls, k);
        const int th = tap >> 2, tw = tap & 3;
        const int nh = ih + 1 - th, nw = iw + 1 - tw;  // the output pixel that reads (ih, iw) through tap (th, tw), if any
        const bool want = nh >= 0 && nw >= 0 && nh % s == 0 && nw % s == 0 && nh / s < Ho && nw / s < Wo;
        CHECK(ok == want, "class %d row %lld k %d: valid %d, the forward relation says %d", cls, (long long)m, k, (int)ok, (int)want);
        if (!ok) continue;
        CHECK(off >= 0 && off + 8 <= ny && off % 8 == 0, "class %d row %lld k %d: offset outside dy", cls, (long long)m, k);
        const int64_t ypix = off / Cout;
        CHECK(off % Cout == co && ypix == ((int64_t)n * Ho + nh / s) * Wo + nw / s, "class %d row %lld k %d: wrong dy element", cls, (long long)m, k);
        if (co == 0) {
          CHECK(!seen_pair[ypix * 16 + tap], "pair gathered twice");
          seen_pair[ypix * 16 + tap] = 1, ++dg_pairs;
        }
      }
    }
  }
  CHECK(dst_rows == (int64_t)N * H * W, "dx pixels written: %lld of %lld", (long long)dst_rows, (long long)N * H * W);
  CHECK(dg_pairs == fwd_pairs, "data gradient gathers %lld (pixel, tap) pairs, the forward %lld", (long long)dg_pairs, (long long)fwd_pairs);
  std::printf("ok rows %lld pairs %lld\n", (long long)(N * L), (long long)fwd_pairs);
  return 0;
}
