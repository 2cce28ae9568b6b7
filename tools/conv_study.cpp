// Development study (host build): how the Jacobi stopping threshold trades sweeps for
// accuracy on 8x8 uint8 tiles, with the wave-uniform termination of the kernels emulated
// (64 consecutive tiles sweep in lock-step until none of them saw cos^2 > T).
//   g++ -O2 -o tools/bin/conv_study tools/conv_study.cpp && tools/bin/conv_study [3 [move2 [waves [seed]]]]
// (argument 3: the sweeps run behind the LQ prelude, lq_prelude_pk - what the kernels do since round 5;
//  argument 4: behind the prelude, the untested sweeps (three at T = 1e-7, the embed's rule; two otherwise) rotate scaled
//  columns (jacobi_rot_scaled_pk), the swap branch taken by a whole wave at a pair where any of its 64 tiles has tau > 0,
//  and the scales are folded back behind them - what the kernels do since round 6; also reported: the share of a
//  sweep's 28 pairs at which the wave wants that branch, and the range of the squared scales;
//  argument 5: as 4, but the columns stay scaled to the end, as in the sigma-only iteration since round 8 - every sweep
//  rotates scaled columns, nothing is folded back except once ahead of the 7th sweep's norms (JAC_SIGMA_FOLD_AT), and the
//  final norms are those of the scaled columns times their scales;
//  move2 > 0: a sweep is the last one only if, besides cos^2 <= T, no rotation of it moved the squared norms by w with
//  w^2 > move2 n2[0] max(n2[p], n2[q]) - the second stopping test of jacobi_rot_pk, JAC_MOVE2)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include <algorithm>
#include "../digital-watermarking-for-image-video-using-dct-svd-singular-value-decomposition_amd/csrc/wm_tile_math.h"
using namespace wm;

// jacobi_rot_pk with the largest cos^2 and the largest norm move w^2 / (n2[0] max(al, be)) it saw reported instead of
// fixed threshold tests
static void rot(v2f (&a)[4][8], float (&n2)[8], int p, int q, float& maxc2, float& maxmv) {
  v2f gv = a[0][p] * a[0][q];
  for (int rp = 1; rp < 4; ++rp) gv = fma2(a[rp][p], a[rp][q], gv);
  const float g = gv[0] + gv[1];
  const float al = n2[p], be = n2[q];
  const float c2 = g * g / fmaxf(al * be, 1e-30f);
  if (c2 > maxc2) maxc2 = c2;
  const float ta = fabsf(be - al) + 1e-18f, ih = frsq(ffma(g + g, g + g, ta * ta)), rx = frsq(ffma(0.5f * ta, ih, 0.5f));
  const float w = fabsf((((g * ih) * rx) * rx) * g), mv = w * w / fmaxf(fmaxf(al, be) * n2[0], 1e-30f);
  if (mv > maxmv) maxmv = mv;
  bool dummy = false;
  jacobi_rot_pk<0>(a, n2, p, q, dummy);
}

// the same around jacobi_rot_scaled_pk
static void rot_scaled(v2f (&a)[4][8], float (&n2)[8], float (&w2)[8], int p, int q, float& maxc2, float& maxmv, bool wave_swaps, bool rcp) {
  v2f gv = a[0][p] * a[0][q];
  for (int rp = 1; rp < 4; ++rp) gv = fma2(a[rp][p], a[rp][q], gv);
  const float gt = gv[0] + gv[1], gg = (gt * (w2[p] * w2[q])) * gt;
  const float al = n2[p], be = n2[q];
  const float c2 = gg / fmaxf(al * be, 1e-30f);
  if (c2 > maxc2) maxc2 = c2;
  const float ta = fabsf(be - al) + 1e-18f, ih = frsq(ffma(gg, 4.0f, ta * ta)), rx = frsq(ffma(0.5f * ta, ih, 0.5f));
  const float w = ((gg * ih) * rx) * rx, mv = w * w / fmaxf(fmaxf(al, be) * n2[0], 1e-30f);
  if (mv > maxmv) maxmv = mv;
  bool dummy = false;
  if (rcp) jacobi_rot_scaled_pk<false, true>(a, n2, w2, p, q, wave_swaps, dummy);   // the sigma-only iteration's 1 / c^2
  else jacobi_rot_scaled_pk(a, n2, w2, p, q, wave_swaps);
}

static void svd_f64(const double (&x)[8][8], double (&s)[8]) {
  double a[8][8];
  for (int r = 0; r < 8; ++r) for (int c = 0; c < 8; ++c) a[r][c] = x[r][c];
  for (int sw = 0; sw < 30; ++sw)
    for (int p = 0; p < 7; ++p)
      for (int q = p + 1; q < 8; ++q) {
        double al = 0, be = 0, g = 0;
        for (int r = 0; r < 8; ++r) { al += a[r][p] * a[r][p]; be += a[r][q] * a[r][q]; g += a[r][p] * a[r][q]; }
        if (fabs(g) < 1e-300) continue;
        const double z = (be - al) / (2 * g), t = (z >= 0 ? 1 : -1) / (fabs(z) + sqrt(1 + z * z));
        const double c = 1 / sqrt(1 + t * t), s_ = c * t;
        for (int r = 0; r < 8; ++r) { const double X = a[r][p], Y = a[r][q]; a[r][p] = c * X - s_ * Y; a[r][q] = s_ * X + c * Y; }
      }
  for (int c = 0; c < 8; ++c) { double n = 0; for (int r = 0; r < 8; ++r) n += a[r][c] * a[r][c]; s[c] = sqrt(n); }
  std::sort(s, s + 8, [](double u, double v) { return u > v; });
}

int main(int argc, char** argv) {
  const float MOVE2 = argc > 2 ? (float)atof(argv[2]) : 0.0f;
  const int NW = argc > 3 ? atoi(argv[3]) : 400;   // waves of 64 tiles
  const int MODE = argc > 1 ? atoi(argv[1]) : 0;
  // quantised: a smooth tile after a JPEG-like round trip (8x8 DCT, luminance table at quality 50, rounded back to 8 bits);
  // posterised: the natural tile at 16 grey levels.  Both are rich in repeated rows, rank-deficient tiles and
  // near-degenerate pairs - what compressed or banded content feeds the kernels.
  const char* kinds[] = {"noise", "natural", "quantised", "posterised"};
  static const int QT[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  double Cm[8][8];
  for (int u = 0; u < 8; ++u) for (int x = 0; x < 8; ++x) Cm[u][x] = (u ? 0.5 : sqrt(0.125)) * cos((2 * x + 1) * u * M_PI / 16);
  const float thr[] = {1e-7f, 1e-6f, 1e-5f, 1e-4f, 3e-4f, 1e-3f, 1e-2f};
  for (int kind = 0; kind < 4; ++kind) {
    srand(argc > 4 ? atoi(argv[4]) : 1234);
    std::vector<uint8_t> px((size_t)NW * 64 * 64);
    for (int t = 0; t < NW * 64; ++t) {
      const double b0 = 20 + rand() % 200, gx = (rand() % 200 - 100) / 25.0, gy = (rand() % 200 - 100) / 25.0, cxy = (rand() % 200 - 100) / 400.0;
      for (int r = 0; r < 8; ++r) for (int c = 0; c < 8; ++c) {
        double v;
        if (kind == 0) v = rand() % 256;
        else { double n = 0; for (int k = 0; k < 4; ++k) n += (rand() % 1000) / 1000.0 - 0.5; v = b0 + gx * c + gy * r + cxy * r * c + 3.5 * n; }
        if (kind == 3) v = 16 * floor(v / 16) + 8;
        px[(size_t)t * 64 + r * 8 + c] = (uint8_t)fmin(fmax(v, 0.0), 255.0);
      }
      if (kind == 2) {
        uint8_t* P = &px[(size_t)t * 64];
        double X[8][8], D[8][8];
        for (int u = 0; u < 8; ++u) for (int v = 0; v < 8; ++v) {
          double d = 0;
          for (int r = 0; r < 8; ++r) for (int c = 0; c < 8; ++c) d += Cm[u][r] * Cm[v][c] * (P[r * 8 + c] - 128.0);
          D[u][v] = QT[u * 8 + v] * nearbyint(d / QT[u * 8 + v]);
        }
        for (int r = 0; r < 8; ++r) for (int c = 0; c < 8; ++c) {
          double d = 0;
          for (int u = 0; u < 8; ++u) for (int v = 0; v < 8; ++v) d += Cm[u][r] * Cm[v][c] * D[u][v];
          X[r][c] = d + 128.0;
        }
        for (int r = 0; r < 8; ++r) for (int c = 0; c < 8; ++c) P[r * 8 + c] = (uint8_t)fmin(fmax(nearbyint(X[r][c]), 0.0), 255.0);
      }
    }
    for (float T : thr) {
      double sum_sweeps = 0, max_err = 0, sum_err = 0, max_cos = 0, sum_tile_sweeps = 0; long nerr = 0, above = 0;
      int hist[16] = {0};
      long swap_pairs[12] = {0}, sweeps_run[12] = {0}; float w2min = 1.0f, w2max = 1.0f;
      for (int w = 0; w < NW; ++w) {
        static v2f a[64][4][8]; static float n2[64][8]; static float w2[64][8];
        int tile_done[64];
        for (int l = 0; l < 64; ++l) {
          for (int rp = 0; rp < 4; ++rp) for (int c = 0; c < 8; ++c) {
            v2f v = {(float)px[((size_t)w * 64 + l) * 64 + (2 * rp) * 8 + c], (float)px[((size_t)w * 64 + l) * 64 + (2 * rp + 1) * 8 + c]};
            a[l][rp][c] = v;
          }
          if (MODE >= 3 && MODE <= 5) lq_prelude_pk(a[l]);   // B0 = X Q: row-pivoted Householder LQ from the right
          col_norms2_pk(a[l], n2[l]); tile_done[l] = 0;
          for (int c = 0; c < 8; ++c) w2[l][c] = 1.0f;
          if (argc > 1 && atoi(argv[1]) == 1) {      // experiment: columns sorted by norm (descending) before the first sweep
            int ord[8]; for (int c = 0; c < 8; ++c) ord[c] = c;
            std::sort(ord, ord + 8, [&](int u, int v) { return n2[l][u] > n2[l][v]; });
            v2f b[4][8]; float m2[8];
            for (int c = 0; c < 8; ++c) { for (int rp = 0; rp < 4; ++rp) b[rp][c] = a[l][rp][ord[c]]; m2[c] = n2[l][ord[c]]; }
            for (int c = 0; c < 8; ++c) { for (int rp = 0; rp < 4; ++rp) a[l][rp][c] = b[rp][c]; n2[l][c] = m2[c]; }
          }
          if (argc > 1 && atoi(argv[1]) == 2) {      // experiment: the ROWS' mean removed first?  (no: changes the matrix) - transpose instead
            v2f b[4][8];
            float t_[8][8];
            for (int rp = 0; rp < 4; ++rp) for (int c = 0; c < 8; ++c) { t_[2 * rp][c] = a[l][rp][c][0]; t_[2 * rp + 1][c] = a[l][rp][c][1]; }
            for (int rp = 0; rp < 4; ++rp) for (int c = 0; c < 8; ++c) { v2f v = {t_[c][2 * rp], t_[c][2 * rp + 1]}; b[rp][c] = v; }
            for (int rp = 0; rp < 4; ++rp) for (int c = 0; c < 8; ++c) a[l][rp][c] = b[rp][c];
            col_norms2_pk(a[l], n2[l]);
          }
        }
        int sweep = 0; bool more = true;
        while (more && sweep < 12) {
          more = false;
          float ms[64], mvs[64];
          const bool scaled = (MODE == 4 && sweep < (T <= 1e-7f ? 3 : 2)) || MODE == 5;
          for (int l = 0; l < 64; ++l) {
            if ((MODE == 4 && !scaled) || (MODE == 5 && sweep == JAC_SIGMA_FOLD_AT)) {   // (the first time: the scales go back into B; afterwards w2 == 1)
              for (int c = 0; c < 8; ++c) { w2min = fminf(w2min, w2[l][c]); w2max = fmaxf(w2max, w2[l][c]); }
              fold_scales_pk(a[l], w2[l]);
              for (int c = 0; c < 8; ++c) w2[l][c] = 1.0f;
            }
            if (sweep >= 2 && (sweep & 1) == 0) col_norms2_scaled_pk(a[l], w2[l], n2[l]);   // (w2 == 1 unless MODE 4)
            ms[l] = mvs[l] = 0;
            if (!scaled)
              for (int p = 0; p < 7; ++p) for (int q = p + 1; q < 8; ++q) rot(a[l], n2[l], p, q, ms[l], mvs[l]);
          }
          if (MODE >= 4) {                           // pair by pair across the wave: the swap branch is the wave's
            ++sweeps_run[sweep];
            for (int p = 0; p < 7; ++p) for (int q = p + 1; q < 8; ++q) {
              bool any = false;
              for (int l = 0; l < 64; ++l) any = any || (n2[l][q] - n2[l][p] > 0.0f);
              swap_pairs[sweep] += any;
              if (scaled) for (int l = 0; l < 64; ++l) rot_scaled(a[l], n2[l], w2[l], p, q, ms[l], mvs[l], any, MODE == 5);
            }
          }
          for (int l = 0; l < 64; ++l) {
            const float m = ms[l], mv = mvs[l];
            bool bad = m > T || (MOVE2 > 0 && mv > MOVE2);
            if (sweep + 1 >= JAC_DEFI_FROM && !(n2[l][7] > SIGMA_RATIO_MIN2 * n2[l][0])) bad = false;   // the rank-deficient exit of jacobi_cols_pk
            if (sweep >= 2 && bad) more = true;
            if (!bad && !tile_done[l]) tile_done[l] = sweep + 1;
            if (bad) tile_done[l] = 0;
          }
          if (sweep < 2) more = true;
          ++sweep;
        }
        sum_sweeps += sweep; hist[sweep]++;
        for (int l = 0; l < 64; ++l) {
          sum_tile_sweeps += tile_done[l] ? std::max(tile_done[l], 3) : sweep;
          col_norms2_scaled_pk(a[l], w2[l], n2[l]);  // (w2 == 1 unless MODE 5)
          fold_scales_pk(a[l], w2[l]);               // (for the final cosines below)
          double x[8][8], s[8];
          for (int r = 0; r < 8; ++r) for (int c = 0; c < 8; ++c) x[r][c] = px[((size_t)w * 64 + l) * 64 + r * 8 + c];
          svd_f64(x, s);
          for (int i = 0; i < 8; ++i) { const double e = fabs(sqrt((double)n2[l][i]) - s[i]) / s[0]; max_err = std::max(max_err, e); sum_err += e; ++nerr; above += e > 2e-6; }
          for (int p = 0; p < 7; ++p) for (int q = p + 1; q < 8; ++q) {
            double g = 0; for (int rp = 0; rp < 4; ++rp) g += (double)a[l][rp][p][0] * a[l][rp][q][0] + (double)a[l][rp][p][1] * a[l][rp][q][1];
            max_cos = std::max(max_cos, fabs(g) / sqrt((double)n2[l][p] * n2[l][q] + 1e-300));
          }
        }
      }
      printf("%-8s T=%.0e  wave sweeps avg %.3f [3:%d 4:%d 5:%d 6:%d 7+:%d]  per-tile avg %.3f  sigma err/s1 max %.2e mean %.2e above 2e-6: %ld  final max cos %.2e\n",
             kinds[kind], T, sum_sweeps / NW, hist[3], hist[4], hist[5], hist[6], hist[7] + hist[8] + hist[9] + hist[10] + hist[11] + hist[12],
             sum_tile_sweeps / (NW * 64.0), max_err, sum_err / nerr, above, max_cos);
      if (MODE >= 4) {
        printf("%-8s T=%.0e  pairs of 28 in the swap branch, sweep 1..6:", kinds[kind], T);
        for (int k = 0; k < 6; ++k) printf(" %.2f", sweeps_run[k] ? (double)swap_pairs[k] / sweeps_run[k] : 0.0);
        printf("  squared scales in [%.2e, %.2e]\n", w2min, w2max);
      }
    }
  }
  return 0;
}
