// What a translation unit of libwmhip.so needs to run a sigma pass over 8x8 tiles: load a tile, run the sigma-only Jacobi
// stream, hand the eight values to an epilogue.  Included by wmhip.hip (the tile-mode watermark) and wm_payload.hip (the
// blind payload), and the only device code the two share.  Everything here has internal linkage (an unnamed namespace):
// each unit compiles its own instantiations of k_sigma_pass, and a kernel keeps its (anonymous namespace):: name.
#pragma once
#include <hip/hip_runtime.h>

#include "wm_internal.h"
#include "wm_tile_math.h"

using namespace wmi;

namespace {

// The iteration every tile kernel spends its time in (B = X V by one-sided Jacobi) is a generated,
// hand-scheduled gfx950 stream with pinned registers (tools/gen_jacobi_asm.py); -DWM_NO_ASM_JACOBI
// builds the C++ form of wm_tile_math.h instead (A/B, and what the CPU harness tests).
#if !defined(WM_NO_ASM_JACOBI)
#if !__has_include("wm_jacobi_sigma_gfx950.inc")
#error "wm_jacobi_sigma_gfx950.inc is generated: run `python tools/gen_jacobi_asm.py --write` (build() does) before compiling"
#endif
#include "wm_jacobi_sigma_gfx950.inc"
#endif

// singular values of a raw tile (sigma-only kernels: K2, extract, detect); < 0: sweep bound hit
__device__ __forceinline__ int sigma_tile_dev(const wm::RawTile& raw, float (&s)[8]) {
#if !defined(WM_NO_ASM_JACOBI)
  float n2[8];
  // sigma only, behind the LQ prelude (B0 = X Q, wm_tile_math.h: about one sweep fewer): test from the 3rd sweep on, a
  // sweep being the last one if it saw no pair above cos^2 = JAC_CONV2_SIGMA and no rotation that moved a squared value
  // by more than sqrt(JAC_MOVE2) s_1 s_p (the stream's own test; wm_tile_math.h) - four noise waves in five end there,
  // the rest after the 4th (tools/conv_study.cpp 3); from the same sweep on a pair that is below cos^2 = 1e-8 in every tile of the wave is
  // left alone (a third of the 3rd sweep's pair visits and 98 % of the 4th's, tools/skip_study.cpp lq).  The threshold
  // is set by the near-degenerate pairs: a residual cosine c between two equal singular values moves them by c s_i / 2,
  // so 1e-8 bounds the error at 5e-5 s_i; 1e-6 measured 4.7e-4 s_1 on one tile of a 4K noise frame
  // (profiles/r02m_sigma_skip.log), 1e-7 and 1e-8 leave every value where the full sweeps leave it.
  constexpr float SIGMA_SKIP2 = 1e-8f;
  constexpr int SIGMA_SKIP_FROM = 2;
  // Only the norms leave the iteration here, so this is the stream whose columns stay scaled to the end (no fold of the
  // scales into B, scaled rotations in the tested sweeps too): wm_jacobi_sigma_gfx950.inc.
  const unsigned long long more = jacobi_sigma_gfx950(raw.lo, raw.hi, n2, wm::JAC_CONV2_SIGMA, SIGMA_SKIP2, 3, SIGMA_SKIP_FROM);
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = wm::fsqrt(n2[i]);
  return more ? -1 : 1;
#else
  return wm::sigma_tile_pk(raw, s);
#endif
}

// ---------------------------------------------------------------------------
// tile I/O (per lane)
// ---------------------------------------------------------------------------
// The one byte path: a little-endian word of 4 pixels, and the 8 pixels of a tile row as a pair of them.  ALIGNED
// (pointers and strides multiples of 8) moves whole words; otherwise the word is put together from / taken apart into
// single bytes, which the compiler is free to merge into unaligned word accesses where the target allows them.
// (The loads are here; the stores, which only the watermark side uses, are in wmhip.hip.)
template <bool ALIGNED>
__device__ __forceinline__ uint32_t load_px4(const uint8_t* __restrict__ q) {
  if (ALIGNED) return *reinterpret_cast<const uint32_t*>(q);
  return q[0] | (q[1] << 8) | (q[2] << 16) | ((uint32_t)q[3] << 24);
}
template <bool ALIGNED>
__device__ __forceinline__ void load_px8(const uint8_t* __restrict__ q, uint32_t& lo, uint32_t& hi) {
  if (ALIGNED) { const uint2 w = *reinterpret_cast<const uint2*>(q); lo = w.x; hi = w.y; }
  else { lo = load_px4<false>(q); hi = load_px4<false>(q + 4); }
}

template <bool ALIGNED>
__device__ __forceinline__ void load_raw(const uint8_t* __restrict__ p, const size_t stride, wm::RawTile& t) {
#pragma unroll
  for (int r = 0; r < 8; ++r) load_px8<ALIGNED>(p + r * stride, t.lo[r], t.hi[r]);
}

template <bool VEC>
__device__ __forceinline__ void store_row8_f32(float* __restrict__ p, const float (&row)[8]) {
  if (VEC) {
    *reinterpret_cast<float4*>(p) = make_float4(row[0], row[1], row[2], row[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(row[4], row[5], row[6], row[7]);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = row[i];
  }
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, WAVE);
  return x;
}

struct Geom {
  int nbx;          // tiles per tile-row
  int n_tiles;      // tiles per plane
  int W;            // plane width (dense float outputs use W as row stride)
  size_t HW;        // H * W
  size_t row_stride;
  size_t plane_stride;
};

// Where tile (ty, tx) of `plane` starts.  In a strided uint8 / float plane batch: `base` is the batch's pointer, or
// (size_t)0 for the element offset itself (the embed kernels address host and stego with one offset) ...
#define STRIDED_TILE(base, g, plane, ty, tx) \
  ((base) + (plane) * (g).plane_stride + (size_t)(ty) * 8 * (g).row_stride + (size_t)(tx) * 8)
// ... and in a dense [plane][H][W] float output (row stride g.W).
#define DENSE_TILE(out, g, plane, ty, tx) ((out) + (plane) * (g).HW + (size_t)(ty) * 8 * (g).W + (size_t)(tx) * 8)
// (Macros: a function's body is optimised on its own before it is inlined, which folds the tile row's * 8 into one stride
// where a kernel shares it between both addresses, and the extract and embed kernels then compile to other code.)

__device__ __forceinline__ bool tile_coords(const Geom& g, int& t, int& ty, int& tx) {
  t = blockIdx.x * WAVE + threadIdx.x;
  if (t >= g.n_tiles) return false;
  ty = t / g.nbx;
  tx = t - ty * g.nbx;
  return true;
}

// ---------------------------------------------------------------------------
// K2  sigma pass: a tile's singular values, and an epilogue that needs nothing else of the tile
// ---------------------------------------------------------------------------
// epi(raw, s, plane, t, ti), ti = plane * n_tiles + t: a small trivially copyable struct, passed by value
template <bool ALIGNED, typename Epi>
__global__ __launch_bounds__(WAVE, 3) void k_sigma_pass(const uint8_t* __restrict__ planes, const Geom g,
                                                    int* __restrict__ status, const Epi epi) {
  int t, ty, tx;
  if (!tile_coords(g, t, ty, tx)) return;
  const size_t plane = blockIdx.y;
  wm::RawTile raw;
  float s[8];
  load_raw<ALIGNED>(STRIDED_TILE(planes, g, plane, ty, tx), g.row_stride, raw);
  if (sigma_tile_dev(raw, s) < 0) atomicOr(status, 1);
  epi(raw, s, plane, t, plane * g.n_tiles + t);
}

// ---------------------------------------------------------------------------
// host-side launch helpers
// ---------------------------------------------------------------------------
Geom make_geom(int H, int W, int row_stride, size_t plane_stride) {
  Geom g;
  g.nbx = W / 8;
  g.n_tiles = (H / 8) * (W / 8);
  g.W = W;
  g.HW = (size_t)H * (size_t)W;
  g.row_stride = (size_t)row_stride;
  g.plane_stride = plane_stride;
  return g;
}

inline bool u8_aligned(const void* a, const void* b, int row_stride, size_t plane_stride) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)row_stride | (uintptr_t)plane_stride) & 7u) == 0;
}

inline dim3 tile_grid(const Geom& g, int n_planes) {
  return dim3((unsigned)((g.n_tiles + WAVE - 1) / WAVE), (unsigned)n_planes, 1);
}

// The launch of every sigma pass, behind the caller's check_plane_args and rule check: nothing to do without a tile; `bad`
// is the caller's verdict on the pointers of its epilogue (the message, or nullptr), which only counts where there is a tile.
template <typename Epi>
int sigma_pass(wm_ctx* ctx, const uint8_t* planes, int n_planes, int H, int W, int row_stride, size_t plane_stride,
               const char* bad, const Epi& epi) {
  const Geom g = make_geom(H, W, row_stride, plane_stride);
  if (n_planes == 0 || g.n_tiles == 0) return WM_OK;
  if (bad) return set_err(WM_ERR_BADARG, "%s", bad);
  const dim3 grid = tile_grid(g, n_planes), block(WAVE);
  with_bools([&](auto A) {
    hipLaunchKernelGGL((k_sigma_pass<A.value, Epi>), grid, block, 0, ctx->stream, planes, g, ctx->d_status, epi);
  }, u8_aligned(planes, planes, row_stride, plane_stride));
  WM_HIP(hipGetLastError());
  return WM_OK;
}

}  // namespace
