// libwmhip.so - the blind payload (include/wmhip.h): sigma_1 quantisation and its keyed dither, the phase, offset and keyed
// searches, the clip search, the frame scores and the channel code's Viterbi decoder - kernels and C ABI.  A translation unit of its own over
// wm_tile_pass.h (the sigma pass it shares with the tile-mode watermark of wmhip.hip) and wm_internal.h: every kernel here
// is compiled in this unit only, and none of wmhip.hip's is compiled here.
//
//   hipcc -O3 --offload-arch=gfx950 -shared -fPIC -o libwmhip.so wmhip.hip wm_payload.hip ...      (see wmhip.hip)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wm_internal.h"
#include "wm_tile_math.h"
#include "wm_tile_pass.h"

using namespace wmi;

namespace {

// ---------------------------------------------------------------------------
// Blind payload (wm_tile_math.h, payload_target / payload_metric): one bit per tile in the parity of sigma_1
// ---------------------------------------------------------------------------
// Sigma pass on the cover tile: the rule's sigma_w row (target - s_1, 0, .., 0) to a dense [plane][tile][8] array that the
// unchanged embed launches are fed with a per-plane stride, alpha = 1 and K = 1.  tile_bit[n_tiles] is shared by the planes.
// `black` (optional, [plane][tile]): 1 for a tile whose 64 pixels are 0 - see k_embed_black.
struct EpiPayloadSigmaW {
  const uint8_t* __restrict__ tile_bit;
  float* __restrict__ sw_eff;
  uint8_t* __restrict__ black;
  float delta;
  __device__ __forceinline__ void operator()(const wm::RawTile& raw, const float (&s)[8], size_t, const int t,
                                             const size_t ti) const {
    float sw[8];
    wm::payload_sigma_w(s, tile_bit[t] & 1, delta, sw);
    store_row8_f32<true>(sw_eff + ti * 8, sw);
    if (black) black[ti] = (wm::raw_is_constant(raw) && raw.lo[0] == 0u) ? 1 : 0;
  }
};

// The same on the keyed lattice (wm_tile_math.h, payload_dither): tile t of a plane reads its 16-bit dither word from
// tile_dither[plane * dither_plane_stride + t] - stride 0 for a table shared by the planes, n_tiles or more for one table
// per plane, as sigma_w_plane_stride - 2 bytes beside the tile's 64.  A struct of its own: the dither-free kernel keeps its
// arguments and its registers.
struct EpiPayloadSigmaWDither {
  const uint8_t* __restrict__ tile_bit;
  const uint16_t* __restrict__ tile_dither;
  float* __restrict__ sw_eff;
  uint8_t* __restrict__ black;
  size_t dither_plane_stride;
  float delta;
  __device__ __forceinline__ void operator()(const wm::RawTile& raw, const float (&s)[8], const size_t plane, const int t,
                                             const size_t ti) const {
    float sw[8];
    const float d = wm::payload_dither(tile_dither[plane * dither_plane_stride + (size_t)t], delta);
    wm::payload_sigma_w(s, tile_bit[t] & 1, delta, d, sw);
    store_row8_f32<true>(sw_eff + ti * 8, sw);
    if (black) black[ti] = (wm::raw_is_constant(raw) && raw.lo[0] == 0u) ? 1 : 0;
  }
};

// Sigma pass on the stego tile: the decoder's soft value of its sigma_1 to metric[plane][tile], 4 bytes a tile where
// EpiSigma stores 32
struct EpiPayloadMetric {
  float* __restrict__ metric;
  float inv_2delta;
  __device__ __forceinline__ void operator()(const wm::RawTile&, const float (&s)[8], size_t, int, const size_t ti) const {
    metric[ti] = wm::payload_metric(s[0], inv_2delta);
  }
};

// The metric on the keyed lattice: the tile's dither word as in EpiPayloadSigmaWDither
struct EpiPayloadMetricDither {
  float* __restrict__ metric;
  const uint16_t* __restrict__ tile_dither;
  size_t dither_plane_stride;
  float delta, inv_2delta;
  __device__ __forceinline__ void operator()(const wm::RawTile&, const float (&s)[8], const size_t plane, const int t,
                                             const size_t ti) const {
    const float d = wm::payload_dither(tile_dither[plane * dither_plane_stride + (size_t)t], delta);
    metric[ti] = wm::payload_metric(s[0], inv_2delta, d);
  }
};

// soft[j] = sum of metric[p][order[i]], i in [offs[j], offs[j + 1]), over all planes: one wave per bit, no atomics.  order /
// offs are the CSR inverse of the tile-to-bit map (a bit's tiles in ascending tile index).  A lane adds its strided share in
// float64 - planes ascending, then i ascending - and the 64 shares are added by the fixed tree of wave_sum: the same inputs
// give the same bits.  (The terms are float32 values of magnitude <= 1, so the float64 sums carry no visible rounding.)
__global__ __launch_bounds__(WAVE) void k_payload_reduce(const float* __restrict__ metric, const int* __restrict__ order,
                                                     const int* __restrict__ offs, double* __restrict__ soft,
                                                     const int n_tiles, const int n_planes) {
  const int j = blockIdx.x;
  const int lo = max(offs[j], 0), hi = min(offs[j + 1], n_tiles);     // (order has n_tiles entries: device offsets are not trusted)
  double acc = 0.0;
  for (int p = 0; p < n_planes; ++p) {
    const float* __restrict__ m = metric + (size_t)p * n_tiles;
#pragma unroll 4
    for (int i = lo + (int)threadIdx.x; i < hi; i += WAVE) {
      const int t = order[i];
      if ((unsigned)t < (unsigned)n_tiles) acc += (double)m[t];   // (an entry outside the grid is never followed)
    }
  }
  acc = wave_sum(acc);
  if (threadIdx.x == 0) soft[j] = acc;
}

// ---------------------------------------------------------------------------
// Crop resynchronisation of the blind payload (include/wmhip.h): where the embed's tile grid lies in a cropped stego
// ---------------------------------------------------------------------------
// Phase scan: the sigma pass over the 8x8 windows of all 64 grid phases of an h x w plane in one launch - grid (waves of the
// largest grid, 64 phases, planes).  Phase p = 8 py + px has the windows that start at (py + 8 r, px + 8 c), r < ny_p =
// (h - py) / 8, c < nx_p = (w - px) / 8; a wave owns 64 consecutive windows of its phase's grid, one per lane, as k_sigma_pass
// lays a plane out.  Windows start at any byte, so the tile is loaded by the byte path.  What becomes of a window's sigma_1 is
// the epilogue's: epi(slot, i, live, s_1), slot = plane * 64 + phase, i = slot * pitch + t the window's element of a
// [plane][phase][t] array, `pitch` = (h / 8) (w / 8) per phase, each phase's own grid row-major at the start of its slot.  Every
// lane of the wave calls it; the lanes behind the last window of a wave redo that window with live = false.
struct PhaseGeom {
  int h, w, pitch;
  size_t row_stride, plane_stride;
};

__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, WAVE);
  return x;
}
__device__ __forceinline__ long long wave_sum(long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, WAVE);
  return x;
}

// The dither-free search: the vote (wm_tile_math.h, payload_vote) to votes[i] (votes may be NULL); sum |vote| of the wave is
// added to sums[plane][phase] by one integer atomic (integer addition is associative: the sums do not depend on the order the
// waves arrive in).  A lane that is not live votes 0, so the wave's sum needs no masking.
struct EpiPhaseVotes {
  int32_t* __restrict__ votes;
  unsigned long long* __restrict__ sums;
  float inv_2delta;
  __device__ __forceinline__ void operator()(const size_t slot, const size_t i, const bool live, const float s1) const {
    const int v = live ? wm::payload_vote(wm::payload_metric(s1, inv_2delta)) : 0;
    if (votes && live) votes[i] = v;
    const int a = wave_sum(v < 0 ? -v : v);
    if (threadIdx.x == 0) atomicAdd(sums + slot, (unsigned long long)a);
  }
};

// The keyed search: sigma_1 itself to s1[i], for k_payload_keyed_scan below.  No delta and no key: the scan is keyless.
struct EpiPhaseSigma1 {
  float* __restrict__ s1;
  __device__ __forceinline__ void operator()(size_t, const size_t i, const bool live, const float s) const {
    if (live) s1[i] = s;
  }
};

template <typename Epi>
__global__ __launch_bounds__(WAVE, 3) void k_payload_phase_scan(const uint8_t* __restrict__ planes, const PhaseGeom g,
                                                            int* __restrict__ status, const Epi epi) {
  const int phase = blockIdx.y, py = phase >> 3, px = phase & 7;
  const int nx = (g.w - px) / 8, n = ((g.h - py) / 8) * nx;
  if ((int)(blockIdx.x * WAVE) >= n) return;                             // (the whole wave: phases differ in their tile counts)
  const int t = blockIdx.x * WAVE + threadIdx.x;
  const bool live = t < n;
  const int tc = live ? t : n - 1;
  const int r = tc / nx, c = tc - r * nx;
  const size_t plane = blockIdx.z;
  wm::RawTile raw;
  float s[8];
  load_raw<false>(planes + plane * g.plane_stride + (size_t)(py + 8 * r) * g.row_stride + (size_t)(px + 8 * c), g.row_stride, raw);
  if (sigma_tile_dev(raw, s) < 0) atomicOr(status, 1);
  const size_t slot = plane * 64 + phase;
  epi(slot, slot * (size_t)g.pitch + t, live, s[0]);
}

// Offset scan: one workgroup per placement (ty, tx) = (blockIdx.y, blockIdx.x) of the ny x nx vote grid V inside the
// nby x nbx tile-to-bit map T.  hist[n_bits] (int32, LDS) takes V[r][c] at T[ty + r][tx + c] by LDS integer atomics - an entry
// of T outside 0 .. n_bits - 1 is skipped, as k_payload_reduce skips an order entry outside the grid - and the first wave adds
// |hist[j]| up to the placement's int64 score.  Integers throughout: the same inputs give the same bits in any order.
constexpr int OFFSET_SCAN_THREADS = 256;
constexpr int OFFSET_SCAN_MAX_BITS = 16384;          // 64 KiB of LDS: two workgroups a CU

__global__ __launch_bounds__(OFFSET_SCAN_THREADS) void k_payload_offset_scan(const int32_t* __restrict__ V, const int32_t* __restrict__ T,
                                                                         long long* __restrict__ scores, const int ny, const int nx,
                                                                         const int nbx, const int n_bits) {
  extern __shared__ int hist[];
  for (int j = threadIdx.x; j < n_bits; j += OFFSET_SCAN_THREADS) hist[j] = 0;
  __syncthreads();
  const int32_t* __restrict__ Tw = T + (size_t)blockIdx.y * nbx + blockIdx.x;
  const int n = ny * nx;
  for (int i = threadIdx.x; i < n; i += OFFSET_SCAN_THREADS) {
    const int r = i / nx, c = i - r * nx;
    const int j = Tw[(size_t)r * nbx + c];
    if ((unsigned)j < (unsigned)n_bits) atomicAdd(&hist[j], V[i]);
  }
  __syncthreads();
  if (threadIdx.x >= WAVE) return;
  long long acc = 0;
  for (int j = threadIdx.x; j < n_bits; j += WAVE) {
    const long long x = hist[j];
    acc += x < 0 ? -x : x;
  }
  acc = wave_sum(acc);
  if (threadIdx.x == 0) scores[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// Keyed scan (include/wmhip.h, "keyed crop resynchronisation"): every grid phase and every placement of a dithered payload's
// crop in one launch - grid (64-placement strips across, placements down, 64 phases), sized for the phase with the fewest
// windows (7, 7), which has the most placements.  A wave owns 64 consecutive tx of one (phase, ty) and a lane one placement;
// the lane walks its phase's ny_p x nx_p windows and reads window (r, c) on the lattice of tile (ty + r, tx + c) of the
// embed's grid: d from that tile's dither word U[ty + r][tx + c], the metric of s1[phase][r][c] - d, its vote, and |vote|
// added up - per window row in int32 (nx_p <= 65535 windows of at most 2^15 stay below 2^31), the rows in int64.  s1[r][c] is
// the same for the whole wave (a uniform load); the 64 lanes' dither words of a step are consecutive in the table and slide by
// one word per step, and a lane's own next 8 are 16 consecutive bytes, which the compiler loads at once: the table comes
// through the L1, every line many times over, without LDS staging.  Integers past the metric and one writer per score: the
// same inputs give the same bits.  The lanes behind the last placement of a strip redo that placement and store nothing.
struct KeyedGeom {
  int h, w, nby, nbx, pitch;       // pitch = (h / 8) (w / 8): floats per phase of s1
  size_t spitch;                   // scores per phase (wmhip.h)
};

// |vote| of one window on one tile's lattice.  |vote(m)| = vote(|m|): m * 2^15 is exact and rintf is odd (ties to even on both
// sides), so the sign costs nothing.
__device__ __forceinline__ int keyed_abs_vote(const float s1, const uint16_t u, const float delta, const float inv_2delta) {
  return wm::payload_vote(fabsf(wm::payload_metric(s1, inv_2delta, wm::payload_dither(u, delta))));
}

// this wave's phase and placement row: false where the phase has no window or fewer placements than the grid was sized for
__device__ __forceinline__ bool keyed_wave(const KeyedGeom& g, const int phase, const int ty, const int tx0, int& ny, int& nx,
                                           int& n_tx) {
  ny = (g.h - (phase >> 3)) / 8, nx = (g.w - (phase & 7)) / 8;
  if (ny <= 0 || nx <= 0) return false;                                  // a phase without a window writes nothing
  n_tx = g.nbx - nx + 1;
  return ty <= g.nby - ny && tx0 < n_tx;                                 // (the whole wave: phases differ in their placements)
}

// one placement's windows, the lane's own: sp the phase's sigma_1 grid, up the table at the placement's first tile
__device__ __forceinline__ long long keyed_placement_sum(const float* __restrict__ sp, const uint16_t* __restrict__ up, const int ny,
                                                         const int nx, const int nbx, const float delta, const float inv_2delta) {
  constexpr int STEP = 8;          // windows a lane loads before it computes: 8 loads in flight, not one wait per window
  long long acc = 0;
  for (int r = 0; r < ny; ++r, sp += nx, up += nbx) {
    int row = 0, c = 0;
    for (; c + STEP <= nx; c += STEP) {
      float s[STEP];
      uint16_t u[STEP];
#pragma unroll
      for (int k = 0; k < STEP; ++k) s[k] = sp[c + k], u[k] = up[c + k];
#pragma unroll
      for (int k = 0; k < STEP; ++k) row += keyed_abs_vote(s[k], u[k], delta, inv_2delta);
    }
    for (; c < nx; ++c) row += keyed_abs_vote(sp[c], up[c], delta, inv_2delta);
    acc += row;
  }
  return acc;
}

__global__ __launch_bounds__(WAVE) void k_payload_keyed_scan(const float* __restrict__ s1, const uint16_t* __restrict__ U,
                                                         long long* __restrict__ scores, const KeyedGeom g, const float delta,
                                                         const float inv_2delta) {
  const int phase = blockIdx.z, ty = blockIdx.y, tx0 = blockIdx.x * WAVE;
  int ny, nx, n_tx;
  if (!keyed_wave(g, phase, ty, tx0, ny, nx, n_tx)) return;
  const int tx = min(tx0 + (int)threadIdx.x, n_tx - 1);
  const long long acc = keyed_placement_sum(s1 + (size_t)phase * g.pitch, U + (size_t)ty * g.nbx + tx, ny, nx, g.nbx, delta, inv_2delta);
  if (tx0 + (int)threadIdx.x < n_tx) scores[(size_t)phase * g.spitch + (size_t)ty * n_tx + tx] = acc;
}

// The same scores with the lanes over the windows, for a crop with few placements across (only rows cut away, say), where the
// mapping above leaves most of a wave without a placement: a wave owns ONE placement (phase, ty, tx) = blockIdx (z, y, x), lane
// l adds the windows c = l, l + 64, .. of every row, and the 64 shares are added by wave_sum.  Integer sums: the two mappings
// give the same bits, whichever keyed_launch picks.
// lane l's share of one placement's windows: c = l, l + 64, .. of every row
__device__ __forceinline__ long long keyed_windows_share(const float* __restrict__ sp, const uint16_t* __restrict__ up, const int ny,
                                                         const int nx, const int nbx, const float delta, const float inv_2delta) {
  long long acc = 0;
  for (int r = 0; r < ny; ++r, sp += nx, up += nbx) {
    int row = 0;
    for (int c = threadIdx.x; c < nx; c += WAVE) row += keyed_abs_vote(sp[c], up[c], delta, inv_2delta);
    acc += row;
  }
  return acc;
}

__global__ __launch_bounds__(WAVE) void k_payload_keyed_scan_windows(const float* __restrict__ s1, const uint16_t* __restrict__ U,
                                                                 long long* __restrict__ scores, const KeyedGeom g,
                                                                 const float delta, const float inv_2delta) {
  const int phase = blockIdx.z, ty = blockIdx.y, tx = blockIdx.x;
  int ny, nx, n_tx;
  if (!keyed_wave(g, phase, ty, tx, ny, nx, n_tx)) return;
  const long long acc = wave_sum(keyed_windows_share(s1 + (size_t)phase * g.pitch, U + (size_t)ty * g.nbx + tx, ny, nx, g.nbx, delta,
                                                     inv_2delta));
  if (threadIdx.x == 0) scores[(size_t)phase * g.spitch + (size_t)ty * n_tx + tx] = acc;
}

// Clip search (include/wmhip.h, "clip resynchronisation"): the keyed scan over several anchors' scans and many candidates, with
// only (the largest score, its first place) per (candidate, phase) leaving the device.  Grid z = 64 candidate + phase; lanes
// and waves own placements as in the two kernels above (one selection rule for both forms: keyed_launch).  Candidate g reads anchor
// a under table table_of[g][a]; an entry outside 0 .. n_tables - 1 skips the anchor (the load and the test are the wave's, not
// the lane's).  A placement's sum stays in registers across the anchors - int32 per window row, int64 across rows and anchors -
// and nothing is written per anchor.  Reduction: key = score * 2^24 + (2^24 - 1 - index), index = ty n_tx + tx; the index is
// unique within (candidate, phase), so the largest key is the largest score at its FIRST index whatever order the waves arrive
// in: a wave-level max, then one 64-bit integer atomic max per wave into best[g][p][0], which the entry point preset to -1.
// score < 2^39 (the entry point's bound on windows x anchors) and index < 2^24 (its bound on placements) keep the key below
// 2^63.  k_payload_keyed_best_unpack then rewrites every key >= 0 in place as (score, index).
constexpr long long KEYED_INDEX_MASK = (1ll << 24) - 1;

__device__ __forceinline__ long long keyed_key(const long long score, const int index) {
  return (score << 24) | (KEYED_INDEX_MASK - index);
}

__device__ __forceinline__ long long wave_max(long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = max(x, (long long)__shfl_down(x, o, WAVE));
  return x;
}

struct KeyedBestArgs {
  const float* __restrict__ s1;          // [n_anchor][64][pitch]
  const uint16_t* __restrict__ tables;   // [n_tables][nby nbx]
  const int32_t* __restrict__ table_of;  // [candidates of this launch][n_anchor]
  long long* __restrict__ best;          // [candidates of this launch][64][2]
  int n_anchor, n_tables;
};

__global__ __launch_bounds__(WAVE) void k_payload_keyed_best(const KeyedBestArgs a, const KeyedGeom g, const float delta,
                                                         const float inv_2delta) {
  const int phase = blockIdx.z & 63, cand = blockIdx.z >> 6, ty = blockIdx.y, tx0 = blockIdx.x * WAVE;
  int ny, nx, n_tx;
  if (!keyed_wave(g, phase, ty, tx0, ny, nx, n_tx)) return;
  const int tx = min(tx0 + (int)threadIdx.x, n_tx - 1);
  const int32_t* __restrict__ tof = a.table_of + (size_t)cand * a.n_anchor;
  const size_t tsize = (size_t)g.nby * g.nbx, at = (size_t)ty * g.nbx + tx;
  long long acc = 0;
  bool any = false;
  for (int i = 0; i < a.n_anchor; ++i) {
    const int t = tof[i];
    if ((unsigned)t >= (unsigned)a.n_tables) continue;                    // (the whole wave)
    any = true;
    acc += keyed_placement_sum(a.s1 + ((size_t)i * 64 + phase) * g.pitch, a.tables + t * tsize + at, ny, nx, g.nbx, delta, inv_2delta);
  }
  if (!any) return;                                                      // a candidate without a marked anchor keeps (-1, -1)
  const long long key = wave_max(tx0 + (int)threadIdx.x < n_tx ? keyed_key(acc, ty * n_tx + tx) : -1ll);
  if (threadIdx.x == 0) atomicMax(a.best + 2 * ((size_t)cand * 64 + phase), key);
}

__global__ __launch_bounds__(WAVE) void k_payload_keyed_best_windows(const KeyedBestArgs a, const KeyedGeom g, const float delta,
                                                                 const float inv_2delta) {
  const int phase = blockIdx.z & 63, cand = blockIdx.z >> 6, ty = blockIdx.y, tx = blockIdx.x;
  int ny, nx, n_tx;
  if (!keyed_wave(g, phase, ty, tx, ny, nx, n_tx)) return;
  const int32_t* __restrict__ tof = a.table_of + (size_t)cand * a.n_anchor;
  const size_t tsize = (size_t)g.nby * g.nbx, at = (size_t)ty * g.nbx + tx;
  long long acc = 0;
  bool any = false;
  for (int i = 0; i < a.n_anchor; ++i) {
    const int t = tof[i];
    if ((unsigned)t >= (unsigned)a.n_tables) continue;
    any = true;
    acc += keyed_windows_share(a.s1 + ((size_t)i * 64 + phase) * g.pitch, a.tables + t * tsize + at, ny, nx, g.nbx, delta, inv_2delta);
  }
  if (!any) return;
  acc = wave_sum(acc);
  if (threadIdx.x == 0) atomicMax(a.best + 2 * ((size_t)cand * 64 + phase), keyed_key(acc, ty * n_tx + tx));
}

__global__ __launch_bounds__(256) void k_payload_keyed_best_unpack(long long* __restrict__ best, const size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long key = best[2 * i];
  if (key < 0) return;
  best[2 * i] = key >> 24;
  best[2 * i + 1] = KEYED_INDEX_MASK - (key & KEYED_INDEX_MASK);
}

// Frame scores (include/wmhip.h, "frame resynchronisation"): every clip frame against every table at ONE grid phase and ONE
// placement - scores[f][k] = sum over the ny x nx windows of keyed_abs_vote(s1[f][r][c], tables[k][ty + r][tx + c]).  A product
// over a (vote, +) semiring, blocked like one: grid (window chunks, table blocks, frame blocks); a wave owns FRAME_CHUNK
// consecutive windows of the row-major window list, a block of FRAME_FB frames and a block of FRAME_TB tables.  Lane l takes
// the windows i = chunk + l, l + 64, ..: it loads its window's sigma_1 of the 8 frames (registers) and the window's word of
// the 8 tables - consecutive lanes read consecutive words of a table row, 128 bytes a wave - forms each word's dither once
// (the 8 calls of keyed_abs_vote share it after inlining) and adds the 64 votes to 64 int32 accumulators: 48 bytes loaded
// per 64 evaluations.  A lane sees FRAME_CHUNK / 64 = 8 windows of at most 2^15 a chunk, so an accumulator stays below 2^18
// and the wave's sum below 2^24.  At the end of the chunk every accumulator is added over the wave and leaves by one 64-bit
// integer atomic add into scores, which the entry point zeroed: integer addition is associative, so the same inputs give
// the same bits whatever order the waves arrive in.  Grid y and z are capped at FRAME_GRID_CAP blocks; the kernel strides
// over the rest.  A frame behind n_frames or a table behind n_tables is read as the last one (no divergence) and stores
// nothing; a lane behind the last window adds nothing.  The compiler keeps the 16 frame and table bases and the epilogue's
// 64 store masks in scalar registers and parks 26 of them in the lanes of one vector register (v_writelane / v_readlane, outside
// the window loop; nothing goes to memory).  The epilogue holds a score row's address in vector registers for that: with all 64
// addresses scalar it parked 42.  Tried and not taken: the 64 sums gathered into the lanes and stored by one vector atomic
// (through readfirstlane 150 parked, through a butterfly sum 122 and 165 VGPRs), the atomics under one lane-0 branch (167 VGPRs).
constexpr int FRAME_FB = 8;              // frames a lane holds in registers
constexpr int FRAME_TB = 8;              // tables it walks against them
#ifndef WM_FRAME_CHUNK
#define WM_FRAME_CHUNK 512
#endif
constexpr int FRAME_CHUNK = WM_FRAME_CHUNK;   // windows of a wave's chunk (512): 64 frames x 64 tables are 4 096 waves at 1080p and 1 024,
                                            // one a SIMD, at a half-size crop of it (-DWM_FRAME_CHUNK=..: a build to measure another against)
constexpr int FRAME_GRID_CAP = 1024;     // table blocks (grid y) and frame blocks (grid z) of a launch

struct FrameScoreGeom {
  int n_frames, n_tables, n_win, nx, nbx;
  size_t wstride, fstride;               // floats between the windows of a frame and between frames
  size_t tsize, at;                      // words of a table; the placement's first word, ty nbx + tx
};

__global__ __launch_bounds__(WAVE) void k_payload_frame_scores(const float* __restrict__ s1, const uint16_t* __restrict__ tables,
                                                           unsigned long long* __restrict__ scores, const FrameScoreGeom g,
                                                           const float delta, const float inv_2delta) {
  const int i0 = blockIdx.x * FRAME_CHUNK, i1 = min(i0 + FRAME_CHUNK, g.n_win);
  for (int f0 = blockIdx.z * FRAME_FB; f0 < g.n_frames; f0 += gridDim.z * FRAME_FB)
    for (int t0 = blockIdx.y * FRAME_TB; t0 < g.n_tables; t0 += gridDim.y * FRAME_TB) {
      int acc[FRAME_FB][FRAME_TB] = {};
      for (int i = i0 + (int)threadIdx.x; i < i1; i += WAVE) {
        const int r = i / g.nx, c = i - r * g.nx;
        const size_t si = (size_t)i * g.wstride, ui = g.at + (size_t)r * g.nbx + c;
        float s[FRAME_FB];
        uint16_t u[FRAME_TB];
#pragma unroll
        for (int k = 0; k < FRAME_FB; ++k) s[k] = s1[(size_t)min(f0 + k, g.n_frames - 1) * g.fstride + si];
#pragma unroll
        for (int t = 0; t < FRAME_TB; ++t) u[t] = tables[(size_t)min(t0 + t, g.n_tables - 1) * g.tsize + ui];
#pragma unroll
        for (int t = 0; t < FRAME_TB; ++t)
#pragma unroll
          for (int k = 0; k < FRAME_FB; ++k) acc[k][t] += keyed_abs_vote(s[k], u[t], delta, inv_2delta);
      }
#pragma unroll
      for (int k = 0; k < FRAME_FB; ++k) {
        unsigned long long* row = scores + (size_t)(f0 + k) * g.n_tables + t0;
        asm volatile("" : "+v"(row));                                      // the row's address in vector registers: table t is an immediate offset
#pragma unroll
        for (int t = 0; t < FRAME_TB; ++t) {
          const int sum = wave_sum(acc[k][t]);
          if (threadIdx.x == 0 && f0 + k < g.n_frames && t0 + t < g.n_tables) atomicAdd(row + t, (unsigned long long)sum);
        }
      }
    }
}

// The channel code's decoder (wmhip.h, "channel code"; the per-state arithmetic is wm_tile_math.h's): one wave per codeword,
// lane = state, the path metric in one register, no LDS, no atomics.  Steps go in chunks of 64: lane i loads and clamps the
// pair of step t0 + i (the pairs are wave-uniform per step and handed out by a uniform-index lane read), keeps the decision
// word of step t0 + i, and the chunk's words leave as one 512-byte store.  A step is two cross-lane reads of pm (the
// predecessors' lanes are fixed, so their byte addresses are computed once), one add, one subtract, a compare-select and a
// ballot.  The traceback runs in the same launch: it depends on the state only, so the chunk's 64 words are loaded at once
// (lane i = step t0 + i) and walked with uniform-index lane reads - no dependent global load - and lane i's info bit leaves
// as one byte of a coalesced store.  The words are written and read back by the same wave; the barrier in between orders them.
__global__ __launch_bounds__(WAVE) void k_payload_viterbi(const int32_t* __restrict__ llr, const int n_info, const size_t llr_stride,
                                                      uint8_t* __restrict__ info_bits, int32_t* __restrict__ final_metric,
                                                      unsigned long long* decisions) {
  const int lane = threadIdx.x, n_steps = n_info + wm::K7_TAIL;
  const int32_t* __restrict__ L = llr + (size_t)blockIdx.x * llr_stride;
  unsigned long long* D = decisions + (size_t)blockIdx.x * (size_t)n_steps;
  const int32_t g0 = wm::k7_sign(lane, wm::K7_G0), g1 = wm::k7_sign(lane, wm::K7_G1);
  const int from0 = (lane >> 1) << 2, from1 = ((lane >> 1) | 32) << 2;       // ds_bpermute takes the source lane's byte address
  int32_t pm = lane ? wm::K7_PM_FLOOR : 0;
  for (int t0 = 0; t0 < n_steps; t0 += WAVE) {
    const int n = min(WAVE, n_steps - t0);
    int32_t la = 0, lb = 0;
    if (lane < n) {
      la = wm::k7_clamp(L[2 * (size_t)(t0 + lane)]);
      lb = wm::k7_clamp(L[2 * (size_t)(t0 + lane) + 1]);
    }
    unsigned long long word = 0;
    for (int i = 0; i < n; ++i) {                                          // (i is uniform: the lane reads are v_readlane)
      const int32_t bm = wm::k7_branch(g0, g1, __builtin_amdgcn_readlane(la, i), __builtin_amdgcn_readlane(lb, i));
      const int32_t p0 = __builtin_amdgcn_ds_bpermute(from0, pm), p1 = __builtin_amdgcn_ds_bpermute(from1, pm);
      int b;
      pm = wm::k7_acs(p0, p1, bm, b);
      const unsigned long long d = __ballot(b);
      if (lane == i) word = d;
    }
    if (lane < n) D[t0 + lane] = word;
  }
  if (final_metric && lane == 0) final_metric[blockIdx.x] = pm;            // state 0: the tail leads every path there
  __syncthreads();                                                         // the wave's own stores, before it loads them
  int s = 0;
  for (int t0 = (n_steps - 1) / WAVE * WAVE; t0 >= 0; t0 -= WAVE) {
    const int n = min(WAVE, n_steps - t0);
    const unsigned long long word = lane < n ? D[t0 + lane] : 0ull;
    const int lo = (int)(unsigned)word, hi = (int)(unsigned)(word >> 32);
    int u = 0;
    for (int i = n - 1; i >= 0; --i) {
      if (lane == i) u = s & 1;
      const unsigned long long d = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(lo, i) |
                                   ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, i) << 32);
      s = wm::k7_back(s, d);
    }
    if (t0 + lane < n_info) info_bits[(size_t)blockIdx.x * (size_t)n_info + (size_t)(t0 + lane)] = (uint8_t)u;
  }
}

// Angle scores (include/wmhip.h, "rotation resynchronisation"): per candidate rotation the sum of payload_vote(|m|) over the
// tiles of the restored H x W plane whose whole footprint lies inside the h x w source, and their number.  Grid (2048-tile
// strips, candidates); a lane owns 8 tiles, 256 apart, and for each: the rule's validity test at the tile's four corner pixels (the map is affine, so
// the interior follows), its vote, then wave_sum and one integer atomic per wave into scores[a] / counts[a], which the entry
// point zeroed.  Integer sums: the same inputs give the same bits in any order.  valid (may be NULL): the test's outcome,
// one byte a tile.
struct AngleGeom {
  int h, w, H, W, nbx, n_tiles;
};

__device__ __forceinline__ bool angle_corner_ok(const AngleGeom& g, const int C, const int S, const int y, const int x) {
  const unsigned X2 = (unsigned)(2 * x + 1 - g.W), Y2 = (unsigned)(2 * y + 1 - g.H);
  const int U = (int)((unsigned)C * X2 - (unsigned)S * Y2 + ((unsigned)(g.w - 1) << 16));
  const int V = (int)((unsigned)S * X2 + (unsigned)C * Y2 + ((unsigned)(g.h - 1) << 16));
  const int x0 = U >> 17, y0 = V >> 17;
  return x0 >= 1 && x0 + 2 <= g.w - 1 && y0 >= 1 && y0 + 2 <= g.h - 1;
}

constexpr int ANGLE_THREADS = 256;
constexpr int ANGLE_TRIPS = 8;       // tiles a lane takes, 256 apart: 2048 tiles a workgroup, so few waves meet at a candidate's sums

__global__ __launch_bounds__(ANGLE_THREADS) void k_payload_angle_scores(const float* __restrict__ metric, const int32_t* __restrict__ cand,
                                                                    unsigned long long* __restrict__ scores, int* __restrict__ counts,
                                                                    uint8_t* __restrict__ valid, const AngleGeom g) {
  const int a = blockIdx.y;
  const int C = cand[2 * a], S = cand[2 * a + 1];
  int v = 0, n = 0;                  // (8 votes of at most 2^15 stay far below 2^31)
#pragma unroll 2
  for (int k = 0; k < ANGLE_TRIPS; ++k) {
    const int t = (blockIdx.x * ANGLE_TRIPS + k) * ANGLE_THREADS + threadIdx.x;
    if (t >= g.n_tiles) break;
    const int r = t / g.nbx, c = t - r * g.nbx;
    const bool ok = angle_corner_ok(g, C, S, 8 * r, 8 * c) && angle_corner_ok(g, C, S, 8 * r, 8 * c + 7) &&
                    angle_corner_ok(g, C, S, 8 * r + 7, 8 * c) && angle_corner_ok(g, C, S, 8 * r + 7, 8 * c + 7);
    const size_t i = (size_t)a * g.n_tiles + t;
    if (ok) v += wm::payload_vote(fabsf(metric[i])), n += 1;
    if (valid) valid[i] = ok ? 1 : 0;
  }
  const long long vs = wave_sum((long long)v);
  n = wave_sum(n);
  if ((threadIdx.x & (WAVE - 1)) == 0 && n) {
    atomicAdd(scores + a, (unsigned long long)vs);
    atomicAdd(counts + a, n);
  }
}

// ---------------------------------------------------------------------------
// host-side argument checking / launch helpers
// ---------------------------------------------------------------------------
// the payload rule's step (include/wmhip.h): 8 <= delta <= 512, finite
int check_delta(const float delta) {
  if (!(isfinite(delta) && wm::payload_delta_ok(delta))) return set_err(WM_ERR_BADARG, "payload needs a finite delta in 8..512");
  return WM_OK;
}

// The launch of both phase scans, behind the caller's check_plane_args and rule check: nothing to do without a plane or a
// whole tile; `bad` as in sigma_pass; `sums`: the scan's [plane][phase] sums to clear first, or nullptr where it has none.
template <typename Epi>
int phase_scan(wm_ctx* ctx, const uint8_t* stego, int n_planes, int h, int w, int row_stride, size_t plane_stride, const char* bad,
               int64_t* sums, const Epi& epi) {
  const size_t pitch = (size_t)(h / 8) * (size_t)(w / 8);
  if (n_planes == 0 || pitch == 0) return WM_OK;
  if (pitch > (size_t)INT32_MAX) return set_err(WM_ERR_BADARG, "more than 2^31 - 1 tiles a plane");
  if (bad) return set_err(WM_ERR_BADARG, "%s", bad);
  if (sums) WM_HIP(hipMemsetAsync(sums, 0, (size_t)n_planes * 64 * sizeof(int64_t), ctx->stream));
  const PhaseGeom g{h, w, (int)pitch, (size_t)row_stride, plane_stride};
  const dim3 grid((unsigned)((pitch + WAVE - 1) / WAVE), 64, (unsigned)n_planes);
  hipLaunchKernelGGL(k_payload_phase_scan<Epi>, grid, dim3(WAVE), 0, ctx->stream, stego, g, ctx->d_status, epi);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

// The lane mapping and the grid (sized for phase (7, 7); z = 64 candidates + phase) of a keyed launch, for both forms: `head`
// is what the form's two kernels take in front of (g, delta, 1 / (2 delta)).  A lane per placement fills n_tx of every 64
// lanes, a lane per window of a row nx of every 64: the second mapping where it fills at least twice as many (the first
// reads s1 once a wave and the table in 16-byte pieces, so it is the cheaper one per window).
template <typename Kernel, typename... Head>
int keyed_launch(wm_ctx* ctx, Kernel per_placement, Kernel per_window, const KeyedGeom& g, int n_cand, float delta, Head... head) {
  const long long n_tx = g.nbx - g.w / 8 + 1, nx = g.w / 8, n_tx_max = g.nbx - (g.w - 7) / 8 + 1;
  const bool windows = nx * ((n_tx + WAVE - 1) / WAVE) >= 2 * n_tx * ((nx + WAVE - 1) / WAVE);
  const dim3 grid((unsigned)(windows ? n_tx_max : (n_tx_max + WAVE - 1) / WAVE), (unsigned)(g.nby - (g.h - 7) / 8 + 1), (unsigned)(64 * n_cand));
  hipLaunchKernelGGL(windows ? per_window : per_placement, grid, dim3(WAVE), 0, ctx->stream, head..., g, delta, 1.0f / (2.0f * delta));
  WM_HIP(hipGetLastError());
  return WM_OK;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

// ---- blind payload: sigma pass + target, sigma pass + metric -----------------------
// The keyed dither of a payload call (include/wmhip.h): `on` false for the dither-free entry points, else the table of 16-bit
// words and its plane stride.  bad_dither: the message where the table cannot serve n_tiles tiles a plane, else nullptr -
// it only counts where there is a tile (sigma_pass).
struct Dither {
  bool on;
  const uint16_t* table;
  size_t plane_stride;
};
constexpr Dither NO_DITHER{false, nullptr, 0};

static const char* bad_dither(const Dither& dz, int H, int W) {
  if (!dz.on) return nullptr;
  if (!dz.table || ((uintptr_t)dz.table & 1u)) return "tile_dither is NULL or not 2-byte aligned";
  if (dz.plane_stride != 0 && dz.plane_stride < (size_t)(H / 8) * (size_t)(W / 8))
    return "dither_plane_stride must be 0 (shared) or at least n_tiles";
  return nullptr;
}

static int payload_sigma_w_dev(wm_ctx* ctx, const uint8_t* planes, const uint8_t* tile_bit, const Dither& dz, float* sigma_w_eff,
                               uint8_t* black, int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta) {
  WM_TRY(check_plane_args(ctx, planes, n_planes, H, W, row_stride, plane_stride));
  WM_TRY(check_delta(delta));
  const char* bad = !tile_bit ? "tile_bit is NULL"
                    : (!sigma_w_eff || ((uintptr_t)sigma_w_eff & 15u)) ? "sigma_w_eff is NULL or not 16-byte aligned"
                    : bad_dither(dz, H, W);
  if (dz.on)
    return sigma_pass(ctx, planes, n_planes, H, W, row_stride, plane_stride, bad,
                      EpiPayloadSigmaWDither{tile_bit, dz.table, sigma_w_eff, black, dz.plane_stride, delta});
  return sigma_pass(ctx, planes, n_planes, H, W, row_stride, plane_stride, bad, EpiPayloadSigmaW{tile_bit, sigma_w_eff, black, delta});
}

static int payload_metric_dev(wm_ctx* ctx, const uint8_t* stego, const Dither& dz, float* metric, int n_planes, int H, int W,
                              int row_stride, size_t plane_stride, float delta) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  WM_TRY(check_delta(delta));
  const char* bad = (!metric || ((uintptr_t)metric & 3u)) ? "metric is NULL or not 4-byte aligned" : bad_dither(dz, H, W);
  const float inv_2delta = 1.0f / (2.0f * delta);
  if (dz.on)
    return sigma_pass(ctx, stego, n_planes, H, W, row_stride, plane_stride, bad,
                      EpiPayloadMetricDither{metric, dz.table, dz.plane_stride, delta, inv_2delta});
  return sigma_pass(ctx, stego, n_planes, H, W, row_stride, plane_stride, bad, EpiPayloadMetric{metric, inv_2delta});
}

int wm_payload_sigma_w_tiles_u8_dev(wm_ctx* ctx, const uint8_t* planes, const uint8_t* tile_bit, float* sigma_w_eff,
                                    int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta) {
  return payload_sigma_w_dev(ctx, planes, tile_bit, NO_DITHER, sigma_w_eff, nullptr, n_planes, H, W, row_stride, plane_stride, delta);
}

int wm_payload_sigma_w_tiles_dither_u8_dev(wm_ctx* ctx, const uint8_t* planes, const uint8_t* tile_bit, const uint16_t* tile_dither,
                                           float* sigma_w_eff, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                           size_t dither_plane_stride, float delta) {
  return payload_sigma_w_dev(ctx, planes, tile_bit, Dither{true, tile_dither, dither_plane_stride}, sigma_w_eff, nullptr, n_planes,
                             H, W, row_stride, plane_stride, delta);
}

int wm_payload_metric_tiles_u8_dev(wm_ctx* ctx, const uint8_t* stego, float* metric, int n_planes, int H, int W,
                                   int row_stride, size_t plane_stride, float delta) {
  return payload_metric_dev(ctx, stego, NO_DITHER, metric, n_planes, H, W, row_stride, plane_stride, delta);
}

int wm_payload_metric_tiles_dither_u8_dev(wm_ctx* ctx, const uint8_t* stego, const uint16_t* tile_dither, float* metric,
                                          int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                          size_t dither_plane_stride, float delta) {
  return payload_metric_dev(ctx, stego, Dither{true, tile_dither, dither_plane_stride}, metric, n_planes, H, W, row_stride,
                            plane_stride, delta);
}

// ---- K1 fed with a sigma_w derived from the cover (embed_derived_dev, wmhip.hip): the payload embed ----------
static int embed_payload_dev(wm_ctx* ctx, const uint8_t* host, const uint8_t* tile_bit, const Dither& dz, uint8_t* stego,
                            float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                            float delta) {
  WM_TRY(check_plane_args(ctx, host, n_planes, H, W, row_stride, plane_stride));
  WM_TRY(check_delta(delta));
  const char* missing = (!tile_bit || !sigma_c) ? "tile_bit / sigma_c is NULL" : bad_dither(dz, H, W);
  return embed_derived_dev(ctx, host, stego, sigma_c, yw, n_planes, H, W, row_stride, plane_stride, 1.0f, 1, missing,
                           [&](float* eff, uint8_t* black) {
    return payload_sigma_w_dev(ctx, host, tile_bit, dz, eff, black, n_planes, H, W, row_stride, plane_stride, delta);
  });
}

int wm_embed_tiles_payload_u8_dev(wm_ctx* ctx, const uint8_t* host, const uint8_t* tile_bit, uint8_t* stego, float* sigma_c,
                                  float* yw, int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta) {
  return embed_payload_dev(ctx, host, tile_bit, NO_DITHER, stego, sigma_c, yw, n_planes, H, W, row_stride, plane_stride, delta);
}

int wm_embed_tiles_payload_dither_u8_dev(wm_ctx* ctx, const uint8_t* host, const uint8_t* tile_bit, const uint16_t* tile_dither,
                                         uint8_t* stego, float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                                         size_t plane_stride, size_t dither_plane_stride, float delta) {
  return embed_payload_dev(ctx, host, tile_bit, Dither{true, tile_dither, dither_plane_stride}, stego, sigma_c, yw, n_planes, H, W,
                           row_stride, plane_stride, delta);
}

// the metric into the context's grow-only workspace, then one wave per bit over it
static int payload_soft_dev(wm_ctx* ctx, const uint8_t* stego, const Dither& dz, const int32_t* order, const int32_t* offs,
                            int n_bits, double* soft, int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  WM_TRY(check_delta(delta));
  const size_t nt = (size_t)(H / 8) * (size_t)(W / 8);
  if (n_planes == 0 || H == 0 || W == 0) return WM_OK;
  if (n_bits < 1 || (size_t)n_bits > nt) return set_err(WM_ERR_BADARG, "n_bits must be in 1..n_tiles");
  if (!order || !offs || !soft || (((uintptr_t)order | (uintptr_t)offs) & 3u) || ((uintptr_t)soft & 7u))
    return set_err(WM_ERR_BADARG, "order / offs / soft is NULL or misaligned");
  if (const char* bad = bad_dither(dz, H, W)) return set_err(WM_ERR_BADARG, "%s", bad);      // (before the workspace grows)
  float* metric = nullptr;
  WM_TRY(staged(ctx, &ctx->sigma_ws, &ctx->sigma_ws_bytes, "payload metric", [&](Carve& cv) {
    metric = cv.take<float>((size_t)n_planes * nt);
  }));
  WM_TRY(payload_metric_dev(ctx, stego, dz, metric, n_planes, H, W, row_stride, plane_stride, delta));
  hipLaunchKernelGGL(k_payload_reduce, dim3((unsigned)n_bits), dim3(WAVE), 0, ctx->stream, (const float*)metric,
                     (const int*)order, (const int*)offs, soft, (int)nt, n_planes);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

int wm_payload_soft_tiles_u8_dev(wm_ctx* ctx, const uint8_t* stego, const int32_t* order, const int32_t* offs, int n_bits,
                                 double* soft, int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta) {
  return payload_soft_dev(ctx, stego, NO_DITHER, order, offs, n_bits, soft, n_planes, H, W, row_stride, plane_stride, delta);
}

int wm_payload_soft_tiles_dither_u8_dev(wm_ctx* ctx, const uint8_t* stego, const uint16_t* tile_dither, const int32_t* order,
                                        const int32_t* offs, int n_bits, double* soft, int n_planes, int H, int W, int row_stride,
                                        size_t plane_stride, size_t dither_plane_stride, float delta) {
  return payload_soft_dev(ctx, stego, Dither{true, tile_dither, dither_plane_stride}, order, offs, n_bits, soft, n_planes, H, W,
                          row_stride, plane_stride, delta);
}

// ---- crop resynchronisation: the phase scan and the offset scan -----------------------
int wm_payload_phase_scan_u8_dev(wm_ctx* ctx, const uint8_t* stego, int32_t* votes, int64_t* sums, int n_planes, int h, int w,
                                 int row_stride, size_t plane_stride, float delta) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, h, w, row_stride, plane_stride));
  WM_TRY(check_delta(delta));
  const bool bad = !sums || ((uintptr_t)sums & 7u) || ((uintptr_t)votes & 3u);
  return phase_scan(ctx, stego, n_planes, h, w, row_stride, plane_stride, bad ? "sums is NULL, or sums / votes is misaligned" : nullptr, sums,
                    EpiPhaseVotes{votes, reinterpret_cast<unsigned long long*>(sums), 1.0f / (2.0f * delta)});
}

int wm_payload_offset_scores_dev(wm_ctx* ctx, const int32_t* votes, const int32_t* tile_bit_index, int64_t* scores, int ny, int nx,
                                 int nby, int nbx, int n_bits) {
  WM_TRY(wmi::use_ctx(ctx));
  if (ny < 0 || nx < 0 || nby < 0 || nbx < 0) return set_err(WM_ERR_BADARG, "negative size");
  if (n_bits < 1 || n_bits > OFFSET_SCAN_MAX_BITS) return set_err(WM_ERR_BADARG, "n_bits must be in 1..16384");
  if (ny > nby || nx > nbx) return WM_OK;                                // no placement
  const size_t n_ty = (size_t)(nby - ny) + 1, n_tx = (size_t)(nbx - nx) + 1;
  if ((size_t)nby * (size_t)nbx > (size_t)INT32_MAX || n_ty > 65535) return set_err(WM_ERR_BADARG, "tile grid too large");
  if (!scores || ((uintptr_t)scores & 7u)) return set_err(WM_ERR_BADARG, "scores is NULL or misaligned");
  if (ny == 0 || nx == 0) {                                              // no window: every placement scores 0
    WM_HIP(hipMemsetAsync(scores, 0, n_ty * n_tx * sizeof(int64_t), ctx->stream));
    return WM_OK;
  }
  if (!votes || !tile_bit_index || (((uintptr_t)votes | (uintptr_t)tile_bit_index) & 3u))
    return set_err(WM_ERR_BADARG, "votes / tile_bit_index is NULL or misaligned");
  const size_t lds = (size_t)n_bits * sizeof(int);
  if (lds > 48 * 1024)
    WM_HIP(hipFuncSetAttribute((const void*)k_payload_offset_scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_payload_offset_scan, dim3((unsigned)n_tx, (unsigned)n_ty), dim3(OFFSET_SCAN_THREADS), lds, ctx->stream, votes,
                     tile_bit_index, reinterpret_cast<long long*>(scores), ny, nx, nbx, n_bits);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

// ---- keyed crop resynchronisation: the sigma_1 scan and the keyed scan -----------------
int wm_payload_sigma1_scan_u8_dev(wm_ctx* ctx, const uint8_t* stego, float* s1, int n_planes, int h, int w, int row_stride,
                                  size_t plane_stride) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, h, w, row_stride, plane_stride));
  return phase_scan(ctx, stego, n_planes, h, w, row_stride, plane_stride, !s1 || ((uintptr_t)s1 & 3u) ? "s1 is NULL or misaligned" : nullptr,
                    nullptr, EpiPhaseSigma1{s1});
}

// the sizes of a keyed search, checked; spitch: the scores per phase (wmhip.h)
static int check_keyed_sizes(int h, int w, int nby, int nbx, float delta, size_t& spitch) {
  if (h < 8 || w < 8) return set_err(WM_ERR_BADARG, "a keyed search needs a whole tile (h, w >= 8)");
  if (nby < 0 || nbx < 0 || h / 8 > nby || w / 8 > nbx) return set_err(WM_ERR_BADARG, "the crop has more tiles than the table");
  WM_TRY(check_delta(delta));
  const size_t n_ty = (size_t)(nby - (h - 7) / 8) + 1, n_tx = (size_t)(nbx - (w - 7) / 8) + 1;
  if (nbx > 65535 || n_ty > 65535 || (size_t)nby * (size_t)nbx > (size_t)INT32_MAX || n_ty * n_tx > ((size_t)1 << 24))
    return set_err(WM_ERR_BADARG, "tile grid too large");                // (2^24 placements a phase: the launch grid, either mapping)
  spitch = n_ty * n_tx;
  return WM_OK;
}

int wm_payload_keyed_scores_dev(wm_ctx* ctx, const float* s1, const uint16_t* tile_dither, int64_t* scores, int h, int w, int nby,
                                int nbx, float delta) {
  WM_TRY(wmi::use_ctx(ctx));
  size_t spitch;
  WM_TRY(check_keyed_sizes(h, w, nby, nbx, delta, spitch));
  if (!tile_dither || ((uintptr_t)tile_dither & 1u)) return set_err(WM_ERR_BADARG, "tile_dither is NULL or at an odd address");
  if (!s1 || !scores || ((uintptr_t)s1 & 3u) || ((uintptr_t)scores & 7u)) return set_err(WM_ERR_BADARG, "s1 / scores is NULL or misaligned");
  WM_HIP(hipMemsetAsync(scores, 0, 64 * spitch * sizeof(int64_t), ctx->stream));
  return keyed_launch(ctx, k_payload_keyed_scan, k_payload_keyed_scan_windows, KeyedGeom{h, w, nby, nbx, (h / 8) * (w / 8), spitch}, 1, delta,
                      s1, tile_dither, reinterpret_cast<long long*>(scores));
}

// the sizes of a clip search, checked (both forms, before any launch or copy)
static int check_keyed_best_sizes(int n_anchor, int n_tables, int n_cand, int h, int w, int nby, int nbx, float delta) {
  size_t spitch;
  WM_TRY(check_keyed_sizes(h, w, nby, nbx, delta, spitch));
  if (n_anchor < 1 || n_cand < 1 || n_tables < 1) return set_err(WM_ERR_BADARG, "n_anchor, n_tables and n_cand must be at least 1");
  if ((size_t)(h / 8) * (size_t)(w / 8) * (size_t)n_anchor >= ((size_t)1 << 24))
    return set_err(WM_ERR_BADARG, "(h / 8) (w / 8) n_anchor must stay below 2^24 (a score below 2^39)");
  return WM_OK;
}

int wm_payload_keyed_best_dev(wm_ctx* ctx, const float* s1, int n_anchor, const uint16_t* tables, int n_tables, const int32_t* table_of,
                              int n_cand, int64_t* best, int h, int w, int nby, int nbx, float delta) {
  WM_TRY(wmi::use_ctx(ctx));
  WM_TRY(check_keyed_best_sizes(n_anchor, n_tables, n_cand, h, w, nby, nbx, delta));
  if (!tables || ((uintptr_t)tables & 1u)) return set_err(WM_ERR_BADARG, "tables is NULL or at an odd address");
  if (!s1 || !table_of || !best || (((uintptr_t)s1 | (uintptr_t)table_of) & 3u) || ((uintptr_t)best & 7u))
    return set_err(WM_ERR_BADARG, "s1 / table_of / best is NULL or misaligned");
  long long* const b = reinterpret_cast<long long*>(best);
  WM_HIP(hipMemsetAsync(best, 0xFF, (size_t)n_cand * 64 * 2 * sizeof(int64_t), ctx->stream));      // every entry (-1, -1)
  const KeyedGeom g{h, w, nby, nbx, (h / 8) * (w / 8), 0};
  constexpr int CHUNK = 1023;                                              // grid z = 64 candidates + phase stays within 65535
  for (int c0 = 0; c0 < n_cand; c0 += CHUNK) {
    WM_TRY(keyed_launch(ctx, k_payload_keyed_best, k_payload_keyed_best_windows, g, std::min(CHUNK, n_cand - c0), delta,
                        KeyedBestArgs{s1, tables, table_of + (size_t)c0 * n_anchor, b + (size_t)c0 * 128, n_anchor, n_tables}));
  }
  const size_t n = (size_t)n_cand * 64;
  hipLaunchKernelGGL(k_payload_keyed_best_unpack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, b, n);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

// ---- frame resynchronisation: every clip frame against every table at one phase and place --------
// the sizes and pointers of a frame-score call, checked (both forms, before any launch or copy)
static int check_frame_scores(const float* s1, size_t s1_window_stride, int n_frames, const uint16_t* tables, int n_tables,
                              const int64_t* scores, int ny, int nx, int nby, int nbx, int ty, int tx, float delta) {
  if (n_frames < 1 || n_tables < 1 || ny < 1 || nx < 1) return set_err(WM_ERR_BADARG, "n_frames, n_tables, ny and nx must be at least 1");
  if (n_frames > (1 << 24) || n_tables > (1 << 24)) return set_err(WM_ERR_BADARG, "more than 2^24 frames or tables");
  if (ty < 0 || tx < 0 || nby < 0 || nbx < 0 || (long long)ty + ny > nby || (long long)tx + nx > nbx)
    return set_err(WM_ERR_BADARG, "the window grid at (ty, tx) does not lie inside the table");
  if ((size_t)nby * (size_t)nbx > ((size_t)1 << 30)) return set_err(WM_ERR_BADARG, "tile grid too large");
  if (s1_window_stride == 0) return set_err(WM_ERR_BADARG, "s1_window_stride must be at least 1");
  WM_TRY(check_delta(delta));
  if (!tables || ((uintptr_t)tables & 1u)) return set_err(WM_ERR_BADARG, "tables is NULL or at an odd address");
  if (!s1 || !scores || ((uintptr_t)s1 & 3u) || ((uintptr_t)scores & 7u)) return set_err(WM_ERR_BADARG, "s1 / scores is NULL or misaligned");
  return WM_OK;
}

int wm_payload_frame_scores_dev(wm_ctx* ctx, const float* s1, size_t s1_window_stride, size_t s1_frame_stride, int n_frames,
                                const uint16_t* tables, int n_tables, int64_t* scores, int ny, int nx, int nby, int nbx, int ty, int tx,
                                float delta) {
  WM_TRY(wmi::use_ctx(ctx));
  WM_TRY(check_frame_scores(s1, s1_window_stride, n_frames, tables, n_tables, scores, ny, nx, nby, nbx, ty, tx, delta));
  WM_HIP(hipMemsetAsync(scores, 0, (size_t)n_frames * (size_t)n_tables * sizeof(int64_t), ctx->stream));
  const int n_win = ny * nx;
  const FrameScoreGeom g{n_frames, n_tables, n_win, nx, nbx, s1_window_stride, s1_frame_stride, (size_t)nby * (size_t)nbx,
                         (size_t)ty * (size_t)nbx + (size_t)tx};
  const dim3 grid((unsigned)((n_win - 1) / FRAME_CHUNK + 1), (unsigned)std::min((n_tables - 1) / FRAME_TB + 1, FRAME_GRID_CAP),
                  (unsigned)std::min((n_frames - 1) / FRAME_FB + 1, FRAME_GRID_CAP));
  hipLaunchKernelGGL(k_payload_frame_scores, grid, dim3(WAVE), 0, ctx->stream, s1, tables, reinterpret_cast<unsigned long long*>(scores), g,
                     delta, 1.0f / (2.0f * delta));
  WM_HIP(hipGetLastError());
  return WM_OK;
}

// ---- rotation resynchronisation: the angle scores ---------------------------------
// the sizes and pointers of a score call, checked (both forms, before any launch or copy)
static int check_angle_scores(const float* metric, const int32_t* cand, int n_angles, const int64_t* scores, const int32_t* counts,
                              int h, int w, int H, int W) {
  if (h < 1 || w < 1 || H < 1 || W < 1 || h > 8192 || w > 8192 || H > 8192 || W > 8192)
    return set_err(WM_ERR_BADARG, "a rotation takes sides in 1..8192");
  if (H % 8 || W % 8) return set_err(WM_ERR_BADARG, "the restored plane's H and W must be multiples of 8");
  if (n_angles < 1 || n_angles > 65535) return set_err(WM_ERR_BADARG, "n_angles must be in 1..65535");
  if (!metric || !cand || !scores || !counts) return set_err(WM_ERR_BADARG, "metric / candidates / scores / counts is NULL");
  return WM_OK;
}

int wm_payload_angle_scores_dev(wm_ctx* ctx, const float* metric, const int32_t* cand, int n_angles, int64_t* scores, int32_t* counts,
                                uint8_t* valid, int h, int w, int H, int W) {
  WM_TRY(wmi::use_ctx(ctx));
  WM_TRY(check_angle_scores(metric, cand, n_angles, scores, counts, h, w, H, W));
  if ((((uintptr_t)metric | (uintptr_t)cand | (uintptr_t)counts) & 3u) || ((uintptr_t)scores & 7u))
    return set_err(WM_ERR_BADARG, "metric / candidates / scores / counts is misaligned");
  WM_HIP(hipMemsetAsync(scores, 0, (size_t)n_angles * sizeof(int64_t), ctx->stream));
  WM_HIP(hipMemsetAsync(counts, 0, (size_t)n_angles * sizeof(int32_t), ctx->stream));
  const AngleGeom g{h, w, H, W, W / 8, (H / 8) * (W / 8)};
  hipLaunchKernelGGL(k_payload_angle_scores, dim3((unsigned)((g.n_tiles + ANGLE_THREADS * ANGLE_TRIPS - 1) / (ANGLE_THREADS * ANGLE_TRIPS)), (unsigned)n_angles),
                     dim3(ANGLE_THREADS), 0, ctx->stream, metric, cand, reinterpret_cast<unsigned long long*>(scores), counts, valid, g);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

// ---- channel code: the Viterbi decode -----------------------------------------
// the sizes of a decode, checked (both forms, before any launch or copy)
static int check_k7_sizes(const int32_t* llr, int n_info, int n_codewords, size_t llr_stride, const uint8_t* info_bits) {
  if (n_info < 1) return set_err(WM_ERR_BADARG, "n_info must be at least 1");
  if (n_info > wm::K7_MAX_STEPS - wm::K7_TAIL) return set_err(WM_ERR_BADARG, "n_info + 6 steps exceed 2^18");
  if (n_codewords < 1) return set_err(WM_ERR_BADARG, "n_codewords must be at least 1");
  if (llr_stride < 2 * (size_t)(n_info + wm::K7_TAIL)) return set_err(WM_ERR_BADARG, "llr_stride < 2 (n_info + 6)");
  if (!llr || !info_bits) return set_err(WM_ERR_BADARG, "llr / info_bits is NULL");
  return WM_OK;
}

int wm_payload_decode_k7_dev(wm_ctx* ctx, const int32_t* llr, int n_info, int n_codewords, size_t llr_stride, uint8_t* info_bits,
                             int32_t* final_metric, uint64_t* decisions) {
  WM_TRY(wmi::use_ctx(ctx));
  WM_TRY(check_k7_sizes(llr, n_info, n_codewords, llr_stride, info_bits));
  if (((uintptr_t)llr | (uintptr_t)final_metric) & 3u || ((uintptr_t)decisions & 7u))
    return set_err(WM_ERR_BADARG, "llr / final_metric / decisions is misaligned");
  if (!decisions) {                                                      // the context's own words: 8 (n_info + 6) bytes a codeword
    WM_TRY(wmi::grow(ctx, &ctx->sigma_ws, &ctx->sigma_ws_bytes,
                     (size_t)n_codewords * (size_t)(n_info + wm::K7_TAIL) * sizeof(uint64_t), "decision words"));
    decisions = static_cast<uint64_t*>(ctx->sigma_ws);
  }
  hipLaunchKernelGGL(k_payload_viterbi, dim3((unsigned)n_codewords), dim3(WAVE), 0, ctx->stream, llr, n_info, llr_stride, info_bits,
                     final_metric, reinterpret_cast<unsigned long long*>(decisions));
  WM_HIP(hipGetLastError());
  return WM_OK;
}

// ===========================================================================
// host-pointer wrappers: H2D, kernels, D2H, sync.  Convenience for callers
// without their own device allocator; the throughput path is *_dev.
// ===========================================================================

// ---- blind payload, host pointers ---------------------------------------------
// Each form once, with the call's Dither (here `table` is the caller's HOST array): the dither-free entry point passes
// NO_DITHER, the dithered one its table, which is staged like the other inputs - n_dither() words.
static size_t n_dither(const Dither& dz, size_t nt, int n_planes) {
  return !dz.on || !nt || !n_planes ? 0 : dz.plane_stride ? (size_t)(n_planes - 1) * dz.plane_stride + nt : nt;
}

static int payload_sigma_w_host(wm_ctx* ctx, const uint8_t* planes, const uint8_t* tile_bit, const Dither& dz, float* sigma_w_eff,
                                int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta) {
  WM_TRY(check_plane_args(ctx, planes, n_planes, H, W, row_stride, plane_stride));
  WM_TRY(check_delta(delta));
  const size_t nt = (size_t)(H / 8) * (W / 8);
  if (n_planes == 0 || nt == 0) return WM_OK;
  if (!tile_bit || !sigma_w_eff) return set_err(WM_ERR_BADARG, "tile_bit / sigma_w_eff is NULL");
  if (const char* bad = bad_dither(dz, H, W)) return set_err(WM_ERR_BADARG, "%s", bad);
  uint8_t *d_p, *d_bit; float* d_eff; uint16_t* d_dz;
  return staged_call(ctx, [&](Carve& cv) {
    d_p = cv.in(plane_span(n_planes, H, row_stride, plane_stride, W), planes);
    d_bit = cv.in(nt, tile_bit);
    d_eff = cv.out((size_t)n_planes * nt * 8, sigma_w_eff);
    d_dz = cv.in(n_dither(dz, nt, n_planes), dz.table);
  }, [&] {
    return payload_sigma_w_dev(ctx, d_p, d_bit, Dither{dz.on, d_dz, dz.plane_stride}, d_eff, nullptr, n_planes, H, W, row_stride,
                               plane_stride, delta);
  });
}

int wm_payload_sigma_w_tiles_u8(wm_ctx* ctx, const uint8_t* planes, const uint8_t* tile_bit, float* sigma_w_eff,
                                int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta) {
  return payload_sigma_w_host(ctx, planes, tile_bit, NO_DITHER, sigma_w_eff, n_planes, H, W, row_stride, plane_stride, delta);
}

int wm_payload_sigma_w_tiles_dither_u8(wm_ctx* ctx, const uint8_t* planes, const uint8_t* tile_bit, const uint16_t* tile_dither,
                                       float* sigma_w_eff, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                       size_t dither_plane_stride, float delta) {
  return payload_sigma_w_host(ctx, planes, tile_bit, Dither{true, tile_dither, dither_plane_stride}, sigma_w_eff, n_planes, H, W,
                              row_stride, plane_stride, delta);
}

static int embed_payload_host(wm_ctx* ctx, const uint8_t* host, const uint8_t* tile_bit, const Dither& dz, uint8_t* stego,
                              float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                              float delta) {
  WM_TRY(check_plane_args(ctx, host, n_planes, H, W, row_stride, plane_stride));
  WM_TRY(check_delta(delta));
  if (!stego) return set_err(WM_ERR_BADARG, "stego is NULL");
  if (n_planes == 0 || H == 0 || W == 0) return WM_OK;
  const size_t nt = (size_t)(H / 8) * (W / 8);
  if (nt > 0 && (!tile_bit || !sigma_c)) return set_err(WM_ERR_BADARG, "tile_bit / sigma_c is NULL");
  if (nt > 0)
    if (const char* bad = bad_dither(dz, H, W)) return set_err(WM_ERR_BADARG, "%s", bad);
  uint16_t* d_dz = nullptr;
  return embed_round_trip(ctx, host, tile_bit, nt, stego, sigma_c, yw, n_planes, H, W, row_stride, plane_stride,
                          [&](uint8_t* d_host, uint8_t* d_bit, uint8_t* d_stego, float* d_sc, float* d_yw) {
    return embed_payload_dev(ctx, d_host, d_bit, Dither{dz.on, d_dz, dz.plane_stride}, d_stego, d_sc, d_yw, n_planes, H, W,
                             row_stride, plane_stride, delta);
  }, [&](Carve& cv) { d_dz = cv.in(n_dither(dz, nt, n_planes), dz.table); });
}

int wm_embed_tiles_payload_u8(wm_ctx* ctx, const uint8_t* host, const uint8_t* tile_bit, uint8_t* stego, float* sigma_c,
                              float* yw, int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta) {
  return embed_payload_host(ctx, host, tile_bit, NO_DITHER, stego, sigma_c, yw, n_planes, H, W, row_stride, plane_stride, delta);
}

int wm_embed_tiles_payload_dither_u8(wm_ctx* ctx, const uint8_t* host, const uint8_t* tile_bit, const uint16_t* tile_dither,
                                     uint8_t* stego, float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                                     size_t plane_stride, size_t dither_plane_stride, float delta) {
  return embed_payload_host(ctx, host, tile_bit, Dither{true, tile_dither, dither_plane_stride}, stego, sigma_c, yw, n_planes, H, W,
                            row_stride, plane_stride, delta);
}

static int payload_metric_host(wm_ctx* ctx, const uint8_t* stego, const Dither& dz, float* metric, int n_planes, int H, int W,
                               int row_stride, size_t plane_stride, float delta) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  WM_TRY(check_delta(delta));
  const size_t nt = (size_t)(H / 8) * (W / 8);
  if (n_planes == 0 || nt == 0) return WM_OK;
  if (!metric) return set_err(WM_ERR_BADARG, "metric is NULL");
  if (const char* bad = bad_dither(dz, H, W)) return set_err(WM_ERR_BADARG, "%s", bad);
  uint8_t* d_p; float* d_m; uint16_t* d_dz;
  return staged_call(ctx, [&](Carve& cv) {
    d_p = cv.in(plane_span(n_planes, H, row_stride, plane_stride, W), stego);
    d_m = cv.out((size_t)n_planes * nt, metric);
    d_dz = cv.in(n_dither(dz, nt, n_planes), dz.table);
  }, [&] {
    return payload_metric_dev(ctx, d_p, Dither{dz.on, d_dz, dz.plane_stride}, d_m, n_planes, H, W, row_stride, plane_stride, delta);
  });
}

int wm_payload_metric_tiles_u8(wm_ctx* ctx, const uint8_t* stego, float* metric, int n_planes, int H, int W,
                               int row_stride, size_t plane_stride, float delta) {
  return payload_metric_host(ctx, stego, NO_DITHER, metric, n_planes, H, W, row_stride, plane_stride, delta);
}

int wm_payload_metric_tiles_dither_u8(wm_ctx* ctx, const uint8_t* stego, const uint16_t* tile_dither, float* metric, int n_planes,
                                      int H, int W, int row_stride, size_t plane_stride, size_t dither_plane_stride, float delta) {
  return payload_metric_host(ctx, stego, Dither{true, tile_dither, dither_plane_stride}, metric, n_planes, H, W, row_stride,
                             plane_stride, delta);
}

// The host form sees order / offs and checks them: offs runs from 0 to n_tiles without decreasing, every order entry names
// a tile of the grid (the device form takes both as they are and only refuses to follow an entry outside the grid).
static int payload_soft_host(wm_ctx* ctx, const uint8_t* stego, const Dither& dz, const int32_t* order, const int32_t* offs,
                             int n_bits, double* soft, int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  WM_TRY(check_delta(delta));
  if (n_planes == 0 || H == 0 || W == 0) return WM_OK;
  const size_t nt = (size_t)(H / 8) * (W / 8);
  if (n_bits < 1 || (size_t)n_bits > nt) return set_err(WM_ERR_BADARG, "n_bits must be in 1..n_tiles");
  if (!order || !offs || !soft) return set_err(WM_ERR_BADARG, "order / offs / soft is NULL");
  if (offs[0] != 0 || (size_t)offs[n_bits] != nt) return set_err(WM_ERR_BADARG, "offs must run from 0 to n_tiles");
  for (int j = 0; j < n_bits; ++j)
    if (offs[j + 1] < offs[j]) return set_err(WM_ERR_BADARG, "offs decreases");
  for (size_t i = 0; i < nt; ++i)
    if (order[i] < 0 || (size_t)order[i] >= nt) return set_err(WM_ERR_BADARG, "order names a tile outside the grid");
  if (const char* bad = bad_dither(dz, H, W)) return set_err(WM_ERR_BADARG, "%s", bad);
  uint8_t* d_p; int32_t *d_order, *d_offs; double* d_soft; uint16_t* d_dz;
  return staged_call(ctx, [&](Carve& cv) {
    d_p = cv.in(plane_span(n_planes, H, row_stride, plane_stride, W), stego);
    d_order = cv.in(nt, order);
    d_offs = cv.in((size_t)n_bits + 1, offs);
    d_soft = cv.out((size_t)n_bits, soft);
    d_dz = cv.in(n_dither(dz, nt, n_planes), dz.table);
  }, [&] {
    return payload_soft_dev(ctx, d_p, Dither{dz.on, d_dz, dz.plane_stride}, d_order, d_offs, n_bits, d_soft, n_planes, H, W,
                            row_stride, plane_stride, delta);
  });
}

int wm_payload_soft_tiles_u8(wm_ctx* ctx, const uint8_t* stego, const int32_t* order, const int32_t* offs, int n_bits,
                             double* soft, int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta) {
  return payload_soft_host(ctx, stego, NO_DITHER, order, offs, n_bits, soft, n_planes, H, W, row_stride, plane_stride, delta);
}

int wm_payload_soft_tiles_dither_u8(wm_ctx* ctx, const uint8_t* stego, const uint16_t* tile_dither, const int32_t* order,
                                    const int32_t* offs, int n_bits, double* soft, int n_planes, int H, int W, int row_stride,
                                    size_t plane_stride, size_t dither_plane_stride, float delta) {
  return payload_soft_host(ctx, stego, Dither{true, tile_dither, dither_plane_stride}, order, offs, n_bits, soft, n_planes, H, W,
                           row_stride, plane_stride, delta);
}

// ---- crop resynchronisation, host pointers ------------------------------------
int wm_payload_phase_scan_u8(wm_ctx* ctx, const uint8_t* stego, int32_t* votes, int64_t* sums, int n_planes, int h, int w,
                             int row_stride, size_t plane_stride, float delta) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, h, w, row_stride, plane_stride));
  WM_TRY(check_delta(delta));
  const size_t pitch = (size_t)(h / 8) * (size_t)(w / 8);
  if (n_planes == 0 || pitch == 0) return WM_OK;
  if (!sums) return set_err(WM_ERR_BADARG, "sums is NULL");
  uint8_t* d_p; int32_t* d_votes; int64_t* d_sums;
  return staged_call(ctx, [&](Carve& cv) {
    d_p = cv.in(plane_span(n_planes, h, row_stride, plane_stride, w), stego);
    d_votes = votes ? cv.out((size_t)n_planes * 64 * pitch, votes) : nullptr;
    d_sums = cv.out((size_t)n_planes * 64, sums);
  }, [&] { return wm_payload_phase_scan_u8_dev(ctx, d_p, d_votes, d_sums, n_planes, h, w, row_stride, plane_stride, delta); });
}

int wm_payload_offset_scores(wm_ctx* ctx, const int32_t* votes, const int32_t* tile_bit_index, int64_t* scores, int ny, int nx,
                             int nby, int nbx, int n_bits) {
  WM_TRY(wmi::use_ctx(ctx));
  if (ny < 0 || nx < 0 || nby < 0 || nbx < 0) return set_err(WM_ERR_BADARG, "negative size");
  if (n_bits < 1 || n_bits > OFFSET_SCAN_MAX_BITS) return set_err(WM_ERR_BADARG, "n_bits must be in 1..16384");
  if (ny > nby || nx > nbx) return WM_OK;
  const size_t n_win = (size_t)ny * (size_t)nx, n_place = ((size_t)(nby - ny) + 1) * ((size_t)(nbx - nx) + 1);
  if (!scores || (n_win && (!votes || !tile_bit_index))) return set_err(WM_ERR_BADARG, "votes / tile_bit_index / scores is NULL");
  int32_t *d_v, *d_t; int64_t* d_s;
  return staged_call(ctx, [&](Carve& cv) {
    d_v = cv.in(n_win, votes);
    d_t = cv.in(n_win ? (size_t)nby * (size_t)nbx : 0, tile_bit_index);
    d_s = cv.out(n_place, scores);
  }, [&] { return wm_payload_offset_scores_dev(ctx, d_v, d_t, d_s, ny, nx, nby, nbx, n_bits); }, true);
}

// ---- keyed crop resynchronisation, host pointers --------------------------------
int wm_payload_sigma1_scan_u8(wm_ctx* ctx, const uint8_t* stego, float* s1, int n_planes, int h, int w, int row_stride,
                              size_t plane_stride) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, h, w, row_stride, plane_stride));
  const size_t pitch = (size_t)(h / 8) * (size_t)(w / 8);
  if (n_planes == 0 || pitch == 0) return WM_OK;
  if (!s1) return set_err(WM_ERR_BADARG, "s1 is NULL");
  uint8_t* d_p; float* d_s1;
  return staged_call(ctx, [&](Carve& cv) {
    d_p = cv.in(plane_span(n_planes, h, row_stride, plane_stride, w), stego);
    d_s1 = cv.out((size_t)n_planes * 64 * pitch, s1);
  }, [&] { return wm_payload_sigma1_scan_u8_dev(ctx, d_p, d_s1, n_planes, h, w, row_stride, plane_stride); });
}

int wm_payload_keyed_scores(wm_ctx* ctx, const float* s1, const uint16_t* tile_dither, int64_t* scores, int h, int w, int nby,
                            int nbx, float delta) {
  WM_TRY(wmi::use_ctx(ctx));
  size_t spitch;
  WM_TRY(check_keyed_sizes(h, w, nby, nbx, delta, spitch));
  if (!tile_dither || ((uintptr_t)tile_dither & 1u)) return set_err(WM_ERR_BADARG, "tile_dither is NULL or at an odd address");
  if (!s1 || !scores) return set_err(WM_ERR_BADARG, "s1 / scores is NULL");
  float* d_s1; uint16_t* d_u; int64_t* d_sc;
  return staged_call(ctx, [&](Carve& cv) {
    d_s1 = cv.in((size_t)64 * (size_t)(h / 8) * (size_t)(w / 8), s1);
    d_u = cv.in((size_t)nby * (size_t)nbx, tile_dither);
    d_sc = cv.out(64 * spitch, scores);
  }, [&] { return wm_payload_keyed_scores_dev(ctx, d_s1, d_u, d_sc, h, w, nby, nbx, delta); }, true);
}

int wm_payload_keyed_best(wm_ctx* ctx, const float* s1, int n_anchor, const uint16_t* tables, int n_tables, const int32_t* table_of,
                          int n_cand, int64_t* best, int h, int w, int nby, int nbx, float delta) {
  WM_TRY(wmi::use_ctx(ctx));
  WM_TRY(check_keyed_best_sizes(n_anchor, n_tables, n_cand, h, w, nby, nbx, delta));
  if (!tables || ((uintptr_t)tables & 1u)) return set_err(WM_ERR_BADARG, "tables is NULL or at an odd address");
  if (!s1 || !table_of || !best) return set_err(WM_ERR_BADARG, "s1 / table_of / best is NULL");
  const size_t n_of = (size_t)n_cand * (size_t)n_anchor;
  for (size_t i = 0; i < n_of; ++i)
    if (table_of[i] < -1 || table_of[i] >= n_tables) return set_err(WM_ERR_BADARG, "table_of names a table outside -1 .. n_tables - 1");
  float* d_s1; uint16_t* d_u; int32_t* d_of; int64_t* d_best;
  return staged_call(ctx, [&](Carve& cv) {
    d_s1 = cv.in((size_t)n_anchor * 64 * (size_t)(h / 8) * (size_t)(w / 8), s1);
    d_u = cv.in((size_t)n_tables * (size_t)nby * (size_t)nbx, tables);
    d_of = cv.in(n_of, table_of);
    d_best = cv.out((size_t)n_cand * 128, best);
  }, [&] { return wm_payload_keyed_best_dev(ctx, d_s1, n_anchor, d_u, n_tables, d_of, n_cand, d_best, h, w, nby, nbx, delta); }, true);
}

// ---- frame resynchronisation, host pointers --------------------------------------
int wm_payload_frame_scores(wm_ctx* ctx, const float* s1, size_t s1_window_stride, size_t s1_frame_stride, int n_frames,
                            const uint16_t* tables, int n_tables, int64_t* scores, int ny, int nx, int nby, int nbx, int ty, int tx,
                            float delta) {
  WM_TRY(wmi::use_ctx(ctx));
  WM_TRY(check_frame_scores(s1, s1_window_stride, n_frames, tables, n_tables, scores, ny, nx, nby, nbx, ty, tx, delta));
  const size_t n_s1 = (size_t)(n_frames - 1) * s1_frame_stride + ((size_t)ny * (size_t)nx - 1) * s1_window_stride + 1;
  float* d_s1; uint16_t* d_u; int64_t* d_sc;
  return staged_call(ctx, [&](Carve& cv) {
    d_s1 = cv.in(n_s1, s1);
    d_u = cv.in((size_t)n_tables * (size_t)nby * (size_t)nbx, tables);
    d_sc = cv.out((size_t)n_frames * (size_t)n_tables, scores);
  }, [&] {
    return wm_payload_frame_scores_dev(ctx, d_s1, s1_window_stride, s1_frame_stride, n_frames, d_u, n_tables, d_sc, ny, nx, nby, nbx, ty,
                                       tx, delta);
  }, true);
}

// ---- rotation resynchronisation, host pointers -----------------------------------
int wm_payload_angle_scores(wm_ctx* ctx, const float* metric, const int32_t* cand, int n_angles, int64_t* scores, int32_t* counts,
                            uint8_t* valid, int h, int w, int H, int W) {
  WM_TRY(wmi::use_ctx(ctx));
  WM_TRY(check_angle_scores(metric, cand, n_angles, scores, counts, h, w, H, W));
  const size_t n = (size_t)n_angles * (size_t)(H / 8) * (size_t)(W / 8);
  float* d_m; int32_t *d_c, *d_n; int64_t* d_s; uint8_t* d_v;
  return staged_call(ctx, [&](Carve& cv) {
    d_m = cv.in(n, metric);
    d_c = cv.in((size_t)2 * n_angles, cand);
    d_s = cv.out((size_t)n_angles, scores);
    d_n = cv.out((size_t)n_angles, counts);
    d_v = valid ? cv.out(n, valid) : nullptr;
  }, [&] { return wm_payload_angle_scores_dev(ctx, d_m, d_c, n_angles, d_s, d_n, d_v, h, w, H, W); }, true);
}

// ---- channel code, host pointers ------------------------------------------------
int wm_payload_decode_k7(wm_ctx* ctx, const int32_t* llr, int n_info, int n_codewords, size_t llr_stride, uint8_t* info_bits,
                         int32_t* final_metric, uint64_t* decisions) {
  WM_TRY(wmi::use_ctx(ctx));
  WM_TRY(check_k7_sizes(llr, n_info, n_codewords, llr_stride, info_bits));
  const size_t n_steps = (size_t)n_info + wm::K7_TAIL, n_cw = (size_t)n_codewords;
  int32_t *d_llr, *d_fm; uint8_t* d_info; uint64_t* d_dec;
  return staged_call(ctx, [&](Carve& cv) {
    d_llr = cv.in((n_cw - 1) * llr_stride + 2 * n_steps, llr);
    d_info = cv.out(n_cw * (size_t)n_info, info_bits);
    d_fm = final_metric ? cv.out(n_cw, final_metric) : nullptr;
    d_dec = decisions ? cv.out(n_cw * n_steps, decisions) : cv.take<uint64_t>(n_cw * n_steps);   // (unwanted words: scratch)
  }, [&] { return wm_payload_decode_k7_dev(ctx, d_llr, n_info, n_codewords, llr_stride, d_info, d_fm, d_dec); }, true);
}

}  // extern "C"
