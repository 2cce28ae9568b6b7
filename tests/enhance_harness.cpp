// CPU build of the extract post-processing arithmetic in csrc/wm_enhance_math.h, for tests only: the CPU suite
// drives the very functions the gfx950 kernels are made of (tests/test_enhance_math_cpu.py) and holds them against
// tests/enhance_oracle.py.  Straight per-pixel loops, no tiling; nothing in the product loads this file.
//
//   g++ -O2 -shared -fPIC -ffp-contract=off -o <tmp>/libwm_enhance_harness.so tests/enhance_harness.cpp
#include <stdlib.h>
#include <string.h>
#include "../digital-watermarking-for-image-video-using-dct-svd-singular-value-decomposition_amd/csrc/wm_enhance_math.h"

using namespace wme;

extern "C" {

int eh_nlm_weights(float h, int channels, int* w, int cap) {
  return nlm_weights(h, channels, NLM_TEMPLATE, NLM_SEARCH, w, cap);
}

// fastNlMeansDenoising straight from the definition, per pixel: 441 offsets x 49 template taps
int eh_nlmeans(const uint8_t* src, uint8_t* dst, int H, int W, int ch, float h) {
  static int w[NLM_MAX_LUT];
  const int n_nz = nlm_weights(h, ch, NLM_TEMPLATE, NLM_SEARCH, w, NLM_MAX_LUT);
  if (n_nz < 0) return -1;
  const int shift = nlm_shift(NLM_TEMPLATE), sr = NLM_SEARCH / 2, tr = NLM_TEMPLATE / 2;
  auto px = [&](int y, int x, int c) { return (int)src[((size_t)reflect101(y, H) * W + reflect101(x, W)) * ch + c]; };
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      uint32_t est[2] = {0, 0}, wsum = 0;
      for (int dy = -sr; dy <= sr; ++dy)
        for (int dx = -sr; dx <= sr; ++dx) {
          uint32_t ssd = 0;
          for (int ty = -tr; ty <= tr; ++ty)
            for (int tx = -tr; tx <= tr; ++tx)
              for (int c = 0; c < ch; ++c) {
                const int e = px(y + ty, x + tx, c) - px(y + dy + ty, x + dx + tx, c);
                ssd += (uint32_t)(e * e);
              }
          uint32_t ad = ssd >> shift;
          if (ad > (uint32_t)n_nz) ad = (uint32_t)n_nz;
          const uint32_t wt = (uint32_t)w[ad];
          wsum += wt;
          for (int c = 0; c < ch; ++c) est[c] += wt * (uint32_t)px(y + dy, x + dx, c);
        }
      for (int c = 0; c < ch; ++c) dst[((size_t)y * W + x) * ch + c] = (uint8_t)nlm_divide(est[c], wsum);
    }
  return n_nz;
}

// luts: tiles_y * tiles_x * 256 bytes (out)
int eh_clahe(const uint8_t* src, uint8_t* dst, int H, int W, float clip_limit, int tiles_x, int tiles_y, uint8_t* luts) {
  int Hp, Wp;
  clahe_padded(H, W, tiles_x, tiles_y, Hp, Wp);
  const int tw = Wp / tiles_x, th = Hp / tiles_y, total = tw * th;
  const int clip = clahe_clip_count((double)clip_limit, total);
  const float scale = clahe_lut_scale(total);
  for (int ty = 0; ty < tiles_y; ++ty)
    for (int tx = 0; tx < tiles_x; ++tx) {
      int hist[CLAHE_BINS] = {0};
      for (int r = 0; r < th; ++r)
        for (int c = 0; c < tw; ++c)
          hist[src[(size_t)reflect101(ty * th + r, H) * W + reflect101(tx * tw + c, W)]]++;
      clahe_clip_hist(hist, clip);
      int sum = 0;
      for (int i = 0; i < CLAHE_BINS; ++i) {
        sum += hist[i];
        luts[((size_t)ty * tiles_x + tx) * CLAHE_BINS + i] = (uint8_t)clahe_lut_value(sum, scale);
      }
    }
  const float inv_tw = 1.0f / (float)tw, inv_th = 1.0f / (float)th;
  for (int y = 0; y < H; ++y) {
    int ty1, ty2;
    float ya, ya1;
    clahe_axis(y, inv_th, tiles_y, ty1, ty2, ya, ya1);
    for (int x = 0; x < W; ++x) {
      int tx1, tx2;
      float xa, xa1;
      clahe_axis(x, inv_tw, tiles_x, tx1, tx2, xa, xa1);
      const int v = src[(size_t)y * W + x];
      const uint8_t* l1 = luts + (size_t)ty1 * tiles_x * CLAHE_BINS;
      const uint8_t* l2 = luts + (size_t)ty2 * tiles_x * CLAHE_BINS;
      dst[(size_t)y * W + x] = (uint8_t)clahe_blend(l1[tx1 * CLAHE_BINS + v], l1[tx2 * CLAHE_BINS + v],
                                                    l2[tx1 * CLAHE_BINS + v], l2[tx2 * CLAHE_BINS + v], xa1, xa, ya1, ya);
    }
  }
  return clip;
}

int eh_unsharp(const uint8_t* src, uint8_t* dst, int H, int W, int ch, float amount) {
  float alpha, beta;
  unsharp_weights(amount, alpha, beta);
  for (int c = 0; c < ch; ++c)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        uint32_t acc = 0;
        for (int r = 0; r < 7; ++r) {
          uint32_t row = 0;
          for (int k = 0; k < 7; ++k)
            row += (uint32_t)blur_tap(k) * src[((size_t)reflect101(y - 3 + r, H) * W + reflect101(x - 3 + k, W)) * ch + c];
          acc += (uint32_t)blur_tap(r) * row;
        }
        const size_t o = ((size_t)y * W + x) * ch + c;
        dst[o] = (uint8_t)unsharp_px(src[o], blur_round(acc), alpha, beta);
      }
  return 0;
}

void eh_lab_tables(uint16_t* tab, int* coeffs) { lab_tables(tab, coeffs); }

void eh_bgr_to_lab(const uint8_t* bgr, uint8_t* lab, size_t n) {
  static uint16_t tab[LAB_CBRT_N];
  int C[9];
  lab_tables(tab, C);
  for (size_t i = 0; i < n; ++i) {
    uint32_t L, A, B;
    bgr_to_lab_px(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2], tab, C, L, A, B);
    lab[3 * i] = (uint8_t)L; lab[3 * i + 1] = (uint8_t)A; lab[3 * i + 2] = (uint8_t)B;
  }
}

void eh_lab_to_bgr(const uint8_t* lab, uint8_t* bgr, size_t n) {
  float C[9];
  lab_inv_coeffs(C);
  for (size_t i = 0; i < n; ++i) {
    uint32_t b, g, r;
    lab_to_bgr_px(lab[3 * i], lab[3 * i + 1], lab[3 * i + 2], C, b, g, r);
    bgr[3 * i] = (uint8_t)b; bgr[3 * i + 1] = (uint8_t)g; bgr[3 * i + 2] = (uint8_t)r;
  }
}

}  // extern "C"
