// Stand-alone CPU program over the texture-masked helpers of csrc/wm_tile_math.h (mask_gain, mask_keep, mask_carried,
// mask_sigma_w) - the very functions the gfx950 kernels call, compiled with g++.  Test infrastructure, never a product path.
//
//   mask_harness edges          the rule's edge cases, checked here; exit status 0 = all hold
//   mask_harness run IN OUT     IN:  int32 n, int32 K, float32 lo, hi, cut, then n x 8 float32 cover singular values
//                               OUT: n float32 g, n float32 carried (0 / 1), n x 8 float32 keep, n x 8 float32 G o ones
// tests/test_mask.py builds it twice (plain, and with -fsanitize=address,undefined) and holds OUT against NumPy.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../digital-watermarking-for-image-video-using-dct-svd-singular-value-decomposition_amd/csrc/wm_tile_math.h"

namespace {

int n_bad = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) { fprintf(stderr, "edges: line %d: %s\n", __LINE__, #cond); ++n_bad; } \
  } while (0)

void set(float (&sc)[8], float s1, float s2, float rest = 0.0f) {
  sc[0] = s1; sc[1] = s2;
  for (int i = 2; i < 8; ++i) sc[i] = rest;
}

int edges() {
  float sc[8], keep[8];
  // all-zero sc: r = 0 -> g = 0, also for lo = 0; only the leading value is kept
  set(sc, 0.0f, 0.0f);
  EXPECT(wm::mask_gain(sc, 8.0f, 64.0f) == 0.0f);
  EXPECT(wm::mask_gain(sc, 0.0f, 64.0f) == 0.0f);
  EXPECT(!wm::mask_keep(sc, 8.0f, 64.0f, 0.25f, 8, keep));
  EXPECT(keep[0] == 1.0f);
  for (int i = 1; i < 8; ++i) EXPECT(keep[i] == 0.0f);
  // r == lo -> 0 exactly, r == hi -> 1 exactly (r from one value: the square root is exact)
  set(sc, 500.0f, 8.0f);
  EXPECT(wm::mask_gain(sc, 8.0f, 64.0f) == 0.0f);
  set(sc, 500.0f, 64.0f);
  EXPECT(wm::mask_gain(sc, 8.0f, 64.0f) == 1.0f);
  EXPECT(wm::mask_keep(sc, 8.0f, 64.0f, 1.0f, 8, keep));          // cut = 1 carries g == 1
  for (int i = 0; i < 8; ++i) EXPECT(keep[i] == 1.0f);
  // above hi: clamped
  set(sc, 900.0f, 300.0f, 100.0f);
  EXPECT(wm::mask_gain(sc, 8.0f, 64.0f) == 1.0f);
  // lo = 0 with a tiny hi: every tile with any texture passes at full strength (the pass-through setting)
  set(sc, 500.0f, 1e-3f);
  EXPECT(wm::mask_gain(sc, 0.0f, 1e-6f) == 1.0f);
  // a very large hi: finite, in [0, 1), nothing carried at cut = 0.25
  set(sc, 900.0f, 300.0f, 100.0f);
  {
    const float g = wm::mask_gain(sc, 8.0f, 3.0e38f);
    EXPECT(isfinite(g) && g >= 0.0f && g < 1e-30f);
    EXPECT(!wm::mask_carried(g, 0.25f));
  }
  // midway, carried: keep = (1, 1/g, .., 1/g) with IEEE division; K < 8 cuts the tail, K = 0 keeps nothing
  set(sc, 500.0f, 36.0f);                                              // g = 28 / 56 = 0.5
  EXPECT(wm::mask_gain(sc, 8.0f, 64.0f) == 0.5f);
  EXPECT(wm::mask_keep(sc, 8.0f, 64.0f, 0.25f, 8, keep));
  EXPECT(keep[0] == 1.0f);
  for (int i = 1; i < 8; ++i) EXPECT(keep[i] == 2.0f);
  EXPECT(wm::mask_keep(sc, 8.0f, 64.0f, 0.25f, 3, keep));
  EXPECT(keep[0] == 1.0f && keep[1] == 2.0f && keep[2] == 2.0f);
  for (int i = 3; i < 8; ++i) EXPECT(keep[i] == 0.0f);
  wm::mask_keep(sc, 8.0f, 64.0f, 0.25f, 0, keep);
  for (int i = 0; i < 8; ++i) EXPECT(keep[i] == 0.0f);
  // below the cut: the leading value alone
  EXPECT(!wm::mask_keep(sc, 8.0f, 64.0f, 0.75f, 8, keep));
  EXPECT(keep[0] == 1.0f && keep[1] == 0.0f && keep[7] == 0.0f);
  // G o sigma_w leaves the leading value alone
  {
    float sw[8] = {8, 7, 6, 5, 4, 3, 2, 1};
    wm::mask_sigma_w(0.5f, sw);
    EXPECT(sw[0] == 8.0f && sw[1] == 3.5f && sw[7] == 0.5f);
  }
  return n_bad ? 1 : 0;
}

int run(const char* in_path, const char* out_path) {
  FILE* f = fopen(in_path, "rb");
  if (!f) { perror(in_path); return 2; }
  int32_t head[2];
  float par[3];
  if (fread(head, 4, 2, f) != 2 || fread(par, 4, 3, f) != 3 || head[0] < 0 || head[0] > (1 << 24)) { fclose(f); return 2; }
  const size_t n = (size_t)head[0];
  const int K = head[1];
  std::vector<float> sc(n * 8), g(n), carried(n), keep(n * 8), eff(n * 8);
  if (fread(sc.data(), 4, n * 8, f) != n * 8) { fclose(f); return 2; }
  fclose(f);
  for (size_t t = 0; t < n; ++t) {
    float s[8], k[8], ones[8];
    memcpy(s, &sc[t * 8], sizeof(s));
    for (int i = 0; i < 8; ++i) ones[i] = 1.0f;
    g[t] = wm::mask_gain(s, par[0], par[1]);
    carried[t] = wm::mask_keep(s, par[0], par[1], par[2], K, k) ? 1.0f : 0.0f;
    wm::mask_sigma_w(g[t], ones);
    memcpy(&keep[t * 8], k, sizeof(k));
    memcpy(&eff[t * 8], ones, sizeof(ones));
  }
  f = fopen(out_path, "wb");
  if (!f) { perror(out_path); return 2; }
  const bool ok = fwrite(g.data(), 4, n, f) == n && fwrite(carried.data(), 4, n, f) == n &&
                  fwrite(keep.data(), 4, n * 8, f) == n * 8 && fwrite(eff.data(), 4, n * 8, f) == n * 8;
  return fclose(f) == 0 && ok ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "edges")) return edges();
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: %s edges | run IN OUT\n", argv[0]);
  return 2;
}
