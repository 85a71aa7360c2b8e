// Index arithmetic of the 2-D k4 p1 convolutions (disc2d.hip): every MFMA kernel there is a GEMM whose rows are pixels of a row grid and
// whose K axis is (tap row, tap column, channel) of a tensor that is GATHERED in place -- no patch matrix.  This header is the whole
// (row, k) -> (address, valid) map, host- and device-callable, so that a plain g++ program can walk it (tests/disc2d_index_host.cpp).
//
//   forward / weight gradient : rows (n, oh, ow), gathered tensor x,  K = 16 Cin,  pixel (oh s - 1 + th, ow s - 1 + tw)
//   data gradient, stride 1   : rows (n, ih, iw), gathered tensor dy, K = 16 Cout, pixel (ih + 1 - th, iw + 1 - tw)
//   data gradient, stride 2   : one GEMM per parity class (py, px) of the input pixels (ih, iw) = (2a + py, 2b + px); only the taps with
//                               th = ih + 1 (mod 2) reach them: th = 1 - py + 2 jh, K = 4 Cout, pixel (a + py - jh, b + px - jw)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MI_HD __host__ __device__
#else
#define MI_HD
#endif

struct C2dGeom {
  int RH, RW;         // row grid of one image: GEMM row m = (n * RH + a) * RW + b
  int SH, SW, SC;     // gathered tensor [N][SH][SW][SC]
  int T;              // taps per axis of this GEMM; K = T * T * SC, k = (jh * T + jw) * SC + c
  int sa, h0, w0, d;  // gathered pixel = (a * sa + h0 + d * jh, b * sa + w0 + d * jw)
  int t0h, t0w, ts;   // kernel tap of (jh, jw) = (t0h + ts * jh, t0w + ts * jw)
  int DH, DW, DC;     // written tensor [N][DH][DW][DC]
  int so, py, px;     // written pixel = (a * so + py, b * so + px)
};

MI_HD inline int c2d_out_extent(int in, int s) { return in < 2 ? 0 : (in + 2 - 4) / s + 1; }  // (no window fits below 2)

MI_HD inline C2dGeom c2d_fwd_geom(int H, int W, int Cin, int Cout, int s) {
  C2dGeom g;
  g.RH = c2d_out_extent(H, s), g.RW = c2d_out_extent(W, s);
  g.SH = H, g.SW = W, g.SC = Cin;
  g.T = 4;
  g.sa = s, g.h0 = -1, g.w0 = -1, g.d = 1;
  g.t0h = 0, g.t0w = 0, g.ts = 1;
  g.DH = g.RH, g.DW = g.RW, g.DC = Cout;
  g.so = 1, g.py = 0, g.px = 0;
  return g;
}

// cls: parity class py * 2 + px (stride 2: 0..3; stride 1: 0 only)
MI_HD inline C2dGeom c2d_dgrad_geom(int H, int W, int Cin, int Cout, int s, int cls) {
  C2dGeom g;
  g.SH = c2d_out_extent(H, s), g.SW = c2d_out_extent(W, s), g.SC = Cout;
  g.DH = H, g.DW = W, g.DC = Cin;
  g.sa = 1, g.d = -1;
  if (s == 1) {
    g.RH = H, g.RW = W;
    g.T = 4;
    g.h0 = 1, g.w0 = 1;
    g.t0h = 0, g.t0w = 0, g.ts = 1;
    g.so = 1, g.py = 0, g.px = 0;
  } else {
    g.py = cls >> 1, g.px = cls & 1;
    g.RH = (H - g.py + 1) / 2, g.RW = (W - g.px + 1) / 2;
    g.T = 2;
    g.h0 = g.py, g.w0 = g.px;
    g.t0h = 1 - g.py, g.t0w = 1 - g.px, g.ts = 2;
    g.so = 2;
  }
  return g;
}

MI_HD inline int c2d_k(const C2dGeom& g) { return g.T * g.T * g.SC; }
MI_HD inline int64_t c2d_rows(const C2dGeom& g, int N) { return (int64_t)N * g.RH * g.RW; }

MI_HD inline void c2d_row(const C2dGeom& g, int64_t m, int* n, int* a, int* b) {
  const int per = g.RH * g.RW;
  const int64_t img = m / per;
  const int rem = (int)(m - img * per);
  *n = (int)img;
  *a = rem / g.RW;
  *b = rem - *a * g.RW;
}

// element offset of channel c of the gathered pixel of row (n, a, b) at K index k; false: the pixel lies outside the tensor (a zero)
MI_HD inline bool c2d_src_at(const C2dGeom& g, int n, int a, int b, int k, int64_t* off) {
  const int tap = k / g.SC, c = k - tap * g.SC;
  const int jh = tap / g.T, jw = tap - jh * g.T;
  const int sh = a * g.sa + g.h0 + g.d * jh, sw = b * g.sa + g.w0 + g.d * jw;
  *off = (((int64_t)n * g.SH + sh) * g.SW + sw) * g.SC + c;
  return (unsigned)sh < (unsigned)g.SH && (unsigned)sw < (unsigned)g.SW;
}
MI_HD inline bool c2d_src(const C2dGeom& g, int64_t m, int k, int64_t* off) {
  int n, a, b;
  c2d_row(g, m, &n, &a, &b);
  return c2d_src_at(g, n, a, b, k, off);
}

// element offset of channel 0 of the pixel row (n, a, b) writes
MI_HD inline int64_t c2d_dst_at(const C2dGeom& g, int n, int a, int b) {
  return (((int64_t)n * g.DH + (a * g.so + g.py)) * g.DW + (b * g.so + g.px)) * g.DC;
}
MI_HD inline int64_t c2d_dst(const C2dGeom& g, int64_t m) {
  int n, a, b;
  c2d_row(g, m, &n, &a, &b);
  return c2d_dst_at(g, n, a, b);
}

// kernel tap (th * 4 + tw) that K index k multiplies, and its channel
MI_HD inline void c2d_tap(const C2dGeom& g, int k, int* tap16, int* c) {
  const int tap = k / g.SC;
  const int jh = tap / g.T, jw = tap - jh * g.T;
  *c = k - tap * g.SC;
  *tap16 = (g.t0h + g.ts * jh) * 4 + (g.t0w + g.ts * jw);
}
