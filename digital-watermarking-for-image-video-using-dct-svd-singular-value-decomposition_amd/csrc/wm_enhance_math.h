// Per-element arithmetic of the extract post-processing chain (app_dct_svd_single.py:223-227, 275-277, 88-110):
//   fastNlMeansDenoising(wy, None, 7, 7, 21)           -> nlm_* (weight table, distance shift, final division)
//   fastNlMeansDenoisingColored(out, None, 3, 3, 7, 21) -> lab_* (COLOR_LBGR2Lab / Lab2LBGR, 8-bit) + nlm_*
//   createCLAHE(2.0, (8, 8)).apply                      -> clahe_*
//   GaussianBlur(e, (0, 0), 1.0) + addWeighted          -> blur_tap / unsharp_px
// OpenCV 4.x's algorithms as documented and restated in tests/enhance_oracle.py; parity with OpenCV itself is not
// pinned.  Everything is integer except the CLAHE interpolation, the addWeighted blend and
// the Lab -> BGR direction, which are f32 with no fused operations on both sides.
//
// The header is host/device: hipcc compiles it into the gfx950 kernels (wm_enhance.hip); the CPU suite compiles the
// same functions with g++ (tests/enhance_harness.cpp).  The host-only table builders run once per call on the host.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define WME_HD __host__ __device__ __forceinline__
#else
#define WME_HD inline
#endif

namespace wme {

constexpr int NLM_TEMPLATE = 7;
constexpr int NLM_SEARCH = 21;
constexpr int NLM_BORDER = NLM_SEARCH / 2 + NLM_TEMPLATE / 2;   // 13: copyMakeBorder of the denoiser
constexpr int NLM_MAX_LUT = 2048;                                 // longest non-zero weight prefix a kernel keeps in LDS
constexpr int CLAHE_BINS = 256;
constexpr int LAB_SHIFT = 12, LAB_SHIFT2 = 15, LAB_CBRT_N = 3072;  // RGB2Lab_b: xyz / lab shifts, 256 * 3/2 * 2^3 entries

// BORDER_REFLECT_101 (borderInterpolate): repeated reflection, so that a border wider than the image still lands inside
WME_HD int reflect101(int p, int len) {
  if (len == 1) return 0;
  while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

WME_HD uint32_t sat_u8(float v) {   // saturate_cast<uchar>(float): cvRound (half to even), then clamp
  const float r = rintf(v);
  return r <= 0.0f ? 0u : (r >= 255.0f ? 255u : (uint32_t)r);
}

// ---- NL-means --------------------------------------------------------------------------------------------------
// fixed_point_mult: INT_MAX / (search^2 * 255)
inline int nlm_fpm(int search) { return (int)(2147483647 / ((int64_t)search * search * 255)); }
// almost_template_window_size_sq_bin_shift: log2 of the next power of two >= template^2
inline int nlm_shift(int tmpl) {
  int s = 0;
  while ((1 << s) < tmpl * tmpl) ++s;
  return s;
}
// Weight by shifted distance ad = ssd >> shift:  cvRound(fpm * exp(-(ad * 2^shift / template^2) / (h^2 * channels))),
// zero below 0.001 * fpm.  The table is non-increasing, so it is kept as its non-zero prefix w[0 .. n) plus w[n] = 0;
// returns n, or -1 when the prefix does not fit in cap - 1 entries.
inline int nlm_weights(float h, int channels, int tmpl, int search, int* w, int cap) {
  const int fpm = nlm_fpm(search);
  const int shift = nlm_shift(tmpl);
  const double mult = (double)(1 << shift) / (double)(tmpl * tmpl);
  const float h2 = h * h;
  const int max_dist = 255 * 255 * channels;
  const int n_all = (int)(max_dist / mult + 1);
  int n = 0;
  for (; n < n_all; ++n) {
    const double dist = n * mult;
    const double wv = exp(-dist / ((double)h2 * channels));
    int weight = (int)nearbyint(fpm * wv);
    if (weight < 0.001 * fpm) weight = 0;
    if (weight == 0) break;
    if (n >= cap - 1) return -1;
    w[n] = weight;
  }
  w[n] = 0;
  return n;
}
// (est + wsum / 2) / wsum in unsigned 32-bit: est <= 441 * fpm * 255 < 2^31 by the choice of fpm
WME_HD uint32_t nlm_divide(uint32_t est, uint32_t wsum) { return (est + wsum / 2) / wsum; }

// ---- CLAHE -----------------------------------------------------------------------------------------------------
// Size the LUTs are computed over: when either side is not a multiple of the grid, BOTH sides are padded (bottom /
// right, reflect-101) by tiles - size % tiles, so a side that was divisible still gets a whole extra tile row of 8.
WME_HD void clahe_padded(int H, int W, int tiles_x, int tiles_y, int& Hp, int& Wp) {
  if (W % tiles_x == 0 && H % tiles_y == 0) { Hp = H; Wp = W; return; }
  Hp = H + tiles_y - H % tiles_y;
  Wp = W + tiles_x - W % tiles_x;
}
// clip_limit * total / 256, at least 1; saturates at INT_MAX instead of an undefined cast: a count
// at or above the tile's pixel count clips nothing, so a huge clip equals clip <= 0
WME_HD int clahe_clip_count(double clip_limit, int tile_total) {
  if (!(clip_limit > 0.0)) return 0;
  const double c = clip_limit * tile_total / CLAHE_BINS;
  if (c >= 2147483647.0) return 2147483647;
  return c > 1.0 ? (int)c : 1;
}
// clip at `clip`, spread the excess: excess / 256 to every bin, then one more to bins 0, step, 2 step, ... for the
// residual (step = max(256 / residual, 1)).  clip == 0: no clipping.
WME_HD void clahe_clip_hist(int* hist, int clip) {
  if (clip <= 0) return;
  int clipped = 0;
  for (int i = 0; i < CLAHE_BINS; ++i)
    if (hist[i] > clip) { clipped += hist[i] - clip; hist[i] = clip; }
  const int batch = clipped / CLAHE_BINS;
  int residual = clipped - batch * CLAHE_BINS;
  for (int i = 0; i < CLAHE_BINS; ++i) hist[i] += batch;
  if (residual != 0) {
    const int step = (CLAHE_BINS / residual) > 1 ? CLAHE_BINS / residual : 1;
    for (int i = 0; i < CLAHE_BINS && residual > 0; i += step, --residual) hist[i]++;
  }
}
// lutScale = (float)(255.0 / tileSizeTotal), the division in double as in CLAHE_Impl::apply
inline float clahe_lut_scale(int tile_total) { return (float)(255.0 / (double)tile_total); }
WME_HD uint32_t clahe_lut_value(int cumsum, float scale) { return sat_u8((float)cumsum * scale); }

// one axis of the bilinear interpolation: pixel coordinate -> the two tiles and their weights
WME_HD void clahe_axis(int p, float inv_t, int tiles, int& t1, int& t2, float& a, float& a1) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float tf = (float)p * inv_t - 0.5f;
  const float fl = floorf(tf);
  int i1 = (int)fl;
  int i2 = i1 + 1;
  a = tf - fl;
  a1 = 1.0f - a;
  t1 = i1 < 0 ? 0 : i1;
  t2 = i2 > tiles - 1 ? tiles - 1 : i2;
}
WME_HD uint32_t clahe_blend(uint32_t l11, uint32_t l12, uint32_t l21, uint32_t l22, float xa1, float xa, float ya1, float ya) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float top = (float)l11 * xa1 + (float)l12 * xa;
  const float bot = (float)l21 * xa1 + (float)l22 * xa;
  const float res = top * ya1 + bot * ya;
  return sat_u8(res);
}

// ---- unsharp: GaussianBlur(sigma 1) on 8-bit, 7 taps of 8 fractional bits, then addWeighted ------------------------
WME_HD int blur_tap(int k) {   // k = 0 .. 6: [1, 14, 62, 102, 62, 14, 1] / 256
  return k == 3 ? 102 : (k == 2 || k == 4) ? 62 : (k == 1 || k == 5) ? 14 : 1;
}
// blur = (sum_r tap_r * rowsum_r + 2^15) >> 16, rowsum = sum_c tap_c * p (exact in 16 bits)
WME_HD uint32_t blur_round(uint32_t acc) { return (acc + 32768u) >> 16; }
// addWeighted(e, 1 + a, blur, -a, 0) in f32: (e * alpha + blur * beta) + 0, no fused operations
WME_HD uint32_t unsharp_px(uint32_t e, uint32_t blur, float alpha, float beta) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float t = (float)e * alpha;
  const float u = (float)blur * beta;
  return sat_u8(t + u + 0.0f);
}
inline void unsharp_weights(float amount, float& alpha, float& beta) {
  alpha = (float)(1.0 + (double)amount);
  beta = (float)(-(double)amount);
}

// ---- Lab, 8-bit, linear RGB (COLOR_LBGR2Lab / COLOR_Lab2LBGR), D65 -----------------------------------------------
// forward: RGB2Lab_b's integer path.  Host tables: the cube-root table (2^15 fixed point) and the XYZ rows scaled by
// 2^12 / white point, laid out for B, G, R input bytes.
inline void lab_tables(uint16_t* cbrt_tab, int* coeffs) {
  for (int i = 0; i < LAB_CBRT_N; ++i) {
    const float x = (float)i * (1.0f / (255.0f * 8.0f));
    const double f = x < 0.008856f ? (double)(x * 7.787f) + 0.13793103448275862 : (double)(float)cbrt((double)x);
    const double v = nearbyint(32768.0 * f);
    cbrt_tab[i] = (uint16_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
  }
  static const double m[9] = {0.412453, 0.357580, 0.180423, 0.212671, 0.715160, 0.072169, 0.019334, 0.119193, 0.950227};
  static const double wp[3] = {0.950456, 1.0, 1.088754};
  for (int i = 0; i < 3; ++i) {
    coeffs[i * 3 + 2] = (int)nearbyint(4096.0 * m[i * 3] / wp[i]);       // R
    coeffs[i * 3 + 1] = (int)nearbyint(4096.0 * m[i * 3 + 1] / wp[i]);   // G
    coeffs[i * 3 + 0] = (int)nearbyint(4096.0 * m[i * 3 + 2] / wp[i]);   // B
  }
}
WME_HD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
WME_HD void bgr_to_lab_px(uint32_t b, uint32_t g, uint32_t r, const uint16_t* tab, const int* C, uint32_t& L, uint32_t& A,
                          uint32_t& B) {
  const int s0 = (int)b * 8, s1 = (int)g * 8, s2 = (int)r * 8;   // linear gamma table: i << 3
  const int fX = tab[descale(s0 * C[0] + s1 * C[1] + s2 * C[2], LAB_SHIFT)];
  const int fY = tab[descale(s0 * C[3] + s1 * C[4] + s2 * C[5], LAB_SHIFT)];
  const int fZ = tab[descale(s0 * C[6] + s1 * C[7] + s2 * C[8], LAB_SHIFT)];
  const int Lscale = (116 * 255 + 50) / 100;
  const int Lshift = -((16 * 255 * (1 << LAB_SHIFT2) + 50) / 100);
  const int l = descale(Lscale * fY + Lshift, LAB_SHIFT2);
  const int a = descale(500 * (fX - fY) + 128 * (1 << LAB_SHIFT2), LAB_SHIFT2);
  const int bb = descale(200 * (fY - fZ) + 128 * (1 << LAB_SHIFT2), LAB_SHIFT2);
  L = (uint32_t)(l < 0 ? 0 : (l > 255 ? 255 : l));
  A = (uint32_t)(a < 0 ? 0 : (a > 255 ? 255 : a));
  B = (uint32_t)(bb < 0 ? 0 : (bb > 255 ? 255 : bb));
}
// inverse: Lab2RGB_f on L * 100/255, a - 128, b - 128, then saturate_cast<uchar>(v * 255).  C: the XYZ -> RGB rows times
// the white point, in f32, rows ordered B, G, R.
inline void lab_inv_coeffs(float* C) {
  static const float m[9] = {3.240479f, -1.53715f, -0.498535f, -0.969256f, 1.875991f, 0.041556f, 0.055648f, -0.204043f, 1.057311f};
  static const float wp[3] = {0.950456f, 1.0f, 1.088754f};
  for (int i = 0; i < 3; ++i) {
    C[i + 6] = m[i] * wp[i];          // R row
    C[i + 3] = m[i + 3] * wp[i];      // G row
    C[i + 0] = m[i + 6] * wp[i];      // B row
  }
}
WME_HD float lab_clip01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
WME_HD void lab_to_bgr_px(uint32_t L8, uint32_t A8, uint32_t B8, const float* C, uint32_t& b, uint32_t& g, uint32_t& r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float li = (float)L8 * (100.0f / 255.0f);
  const float ai = (float)((int)A8 - 128), bi = (float)((int)B8 - 128);
  const float lthresh = 0.008856f * 903.3f;
  const float fthresh = 7.787f * 0.008856f + 16.0f / 116.0f;
  float y, fy;
  if (li <= lthresh) {
    y = li / 903.3f;
    fy = 7.787f * y + 16.0f / 116.0f;
  } else {
    fy = (li + 16.0f) / 116.0f;
    y = fy * fy * fy;
  }
  float fx = ai / 500.0f + fy, fz = fy - bi / 200.0f;
  fx = fx <= fthresh ? (fx - 16.0f / 116.0f) / 7.787f : fx * fx * fx;
  fz = fz <= fthresh ? (fz - 16.0f / 116.0f) / 7.787f : fz * fz * fz;
  const float bo = lab_clip01(C[0] * fx + C[1] * y + C[2] * fz);
  const float go = lab_clip01(C[3] * fx + C[4] * y + C[5] * fz);
  const float ro = lab_clip01(C[6] * fx + C[7] * y + C[8] * fz);
  b = sat_u8(bo * 255.0f);
  g = sat_u8(go * 255.0f);
  r = sat_u8(ro * 255.0f);
}

}  // namespace wme
