// Stand-alone CPU program over the channel code's scalar decoder of csrc/wm_tile_math.h (k7_decode_scalar: the per-state
// arithmetic k_payload_viterbi runs, compiled with g++).  Test infrastructure, never a product path.
//
//   payload_code_harness edges         fixed points of the per-state helpers, checked here; exit status 0 = all hold
//   payload_code_harness run IN OUT    IN:  int32 n_codewords, then per codeword: int32 n_info, 2 (n_info + 6) int32 L
//                                      OUT: per codeword: n_info uint8 info bits, int32 final metric, (n_info + 6) uint64
//                                           decision words
// tests/test_payload_code.py builds it twice (plain, and with -fsanitize=address,undefined) and holds OUT against NumPy.
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

int edges() {
  EXPECT(wm::k7_clamp(INT32_MAX) == 1024 && wm::k7_clamp(INT32_MIN) == -1024 && wm::k7_clamp(1024) == 1024);
  EXPECT(wm::k7_clamp(-1025) == -1024 && wm::k7_clamp(0) == 0 && wm::k7_clamp(-7) == -7);
  EXPECT(wm::k7_parity(0u) == 0 && wm::k7_parity(0171u) == 1 && wm::k7_parity(0133u) == 1 && wm::k7_parity(3u) == 0);
  // both generators hold bits 0 and 6: the b = 1 branch into a state has the opposite sign on both outputs
  for (int s = 0; s < 64; ++s) {
    EXPECT(wm::k7_sign(s | 64, wm::K7_G0) == -wm::k7_sign(s, wm::K7_G0));
    EXPECT(wm::k7_sign(s | 64, wm::K7_G1) == -wm::k7_sign(s, wm::K7_G1));
  }
  EXPECT(wm::k7_branch(1, -1, 5, 3) == 2 && wm::k7_branch(-1, -1, 5, 3) == -8);
  int b;
  EXPECT(wm::k7_acs(10, 10, 0, b) == 10 && b == 0);                      // a tie goes to b = 0
  EXPECT(wm::k7_acs(10, 11, 0, b) == 11 && b == 1);
  EXPECT(wm::k7_acs(0, 0, -1, b) == 1 && b == 1);
  EXPECT(wm::k7_acs(wm::K7_PM_FLOOR - (1 << 29) + 2048, wm::K7_PM_FLOOR - (1 << 29) + 2048, -2048, b) ==
         wm::K7_PM_FLOOR - (1 << 29) + 4096);                             // the range's low end does not wrap
  EXPECT(wm::k7_back(0, 1ull) == 32 && wm::k7_back(63, 1ull << 63) == 63 && wm::k7_back(63, 0ull) == 31);
  return n_bad ? 1 : 0;
}

int run(const char* in_path, const char* out_path) {
  FILE* f = fopen(in_path, "rb");
  if (!f) { perror(in_path); return 2; }
  FILE* o = fopen(out_path, "wb");
  if (!o) { perror(out_path); fclose(f); return 2; }
  int32_t n_cw;
  bool ok = fread(&n_cw, 4, 1, f) == 1 && n_cw >= 0 && n_cw <= 4096;
  for (int c = 0; ok && c < n_cw; ++c) {
    int32_t n_info;
    ok = fread(&n_info, 4, 1, f) == 1 && n_info >= 1 && n_info <= wm::K7_MAX_STEPS - wm::K7_TAIL;
    if (!ok) break;
    const size_t n_steps = (size_t)n_info + wm::K7_TAIL;
    std::vector<int32_t> llr(2 * n_steps);
    std::vector<uint8_t> info((size_t)n_info);
    std::vector<uint64_t> dec(n_steps);
    ok = fread(llr.data(), 4, llr.size(), f) == llr.size();
    if (!ok) break;
    const int32_t metric = wm::k7_decode_scalar(llr.data(), n_info, info.data(), dec.data());
    ok = fwrite(info.data(), 1, info.size(), o) == info.size() && fwrite(&metric, 4, 1, o) == 1 &&
         fwrite(dec.data(), 8, dec.size(), o) == dec.size();
  }
  fclose(f);
  return fclose(o) == 0 && ok ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "edges")) return edges();
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: %s edges | run IN OUT\n", argv[0]);
  return 2;
}
