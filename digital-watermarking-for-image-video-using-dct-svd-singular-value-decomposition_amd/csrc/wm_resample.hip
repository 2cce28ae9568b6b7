// The integer resampler of the blind payload's resize resynchronisation (include/wmhip.h, "resize resynchronisation"):
// uint8 planes [h_in][w_in] -> [h_out][w_out] through a separable filter whose taps the host made (resample.py):
//
//     out[i] = clip((sum_t w[i][t] * px[min(first[i] + t, n_in - 1)] + 2^13) >> 14, 0, 255)          per axis
//
// the horizontal pass into a uint8 intermediate [h_in][w_out] the context owns, then the vertical pass.  Pixels are at most
// 255 and weights fit 16 bits, so every product fits 24-bit multiply-adds and |acc| < 2^23: integers only, no float, no
// atomics, no scratch, and the bytes are those of the NumPy restatement (tests/resample_refs.py).
//
//   k_resample_h  a lane takes 4 adjacent output pixels of one source row and stores them as one dword.  Its taps are its
//                 own (first[i], w[i][.] per output column); the lanes of a wave cover 256 adjacent outputs, whose source
//                 windows overlap or abut: byte loads that the L1 serves.  The intermediate's rows are 16-byte multiples on
//                 a 256-byte base, so the dword store needs no tail and no byte path of its own.
//   k_resample_h_lds  the same lanes and the same store with the workgroup's source span and weights staged in LDS first
//                 (below): the form that runs wherever w is 8-byte aligned and T <= 17, k_resample_h being the path for the rest.
//   k_resample_v a lane takes 16 adjacent output columns of one output row.  The row's taps (first[r], w[r][.]) are the
//                 same for the whole workgroup: scalar loads.  Every tap is one 16-byte load of a line of the intermediate
//                 (always aligned, see above) and 16 multiply-adds; the result leaves as one 16-byte store where the
//                 destination's base and strides allow it and the lane's columns are all inside the plane, byte by byte
//                 otherwise.  Taps of weight 0 (the tail of a row of w, an identity pass) are skipped: no load.
//
// No grid is capped: (column blocks, rows, planes), rows and planes at most 65535.  The only strided loops are the LDS
// form's staging loops, 256 elements a trip, which take several trips at any width above 256.
// The device does not trust `first`: an index outside the source clamps to its last sample, as the rule's min() does.
//
// Below them, k_rotate_planes: the integer rotation of the rotation resynchronisation, one pass, described where it stands.
#include "wm_internal.h"

using namespace wmi;

namespace {

constexpr int RS_NT = 256;
constexpr int RS_BITS = 14;
constexpr int RS_MAX_TAPS = 33;
constexpr int RS_H_PX = 4;       // output pixels a lane of the horizontal pass takes
constexpr int RS_V_PX = 16;      // output columns a lane of the vertical pass takes

__device__ __forceinline__ unsigned rs_round(int acc) {
  return (unsigned)min(max((acc + (1 << (RS_BITS - 1))) >> RS_BITS, 0), 255);
}

__global__ __launch_bounds__(RS_NT) void k_resample_h(const uint8_t* __restrict__ src, const int w_in, const int row_stride,
                                                      const size_t plane_stride, uint8_t* __restrict__ mid, const int w_out,
                                                      const int mid_stride, const size_t mid_plane, const int32_t* __restrict__ first,
                                                      const int16_t* __restrict__ w, const int T) {
  const int i0 = (blockIdx.x * RS_NT + threadIdx.x) * RS_H_PX;
  if (i0 >= w_out) return;
  const uint8_t* s = src + (size_t)blockIdx.z * plane_stride + (size_t)blockIdx.y * row_stride;
  const unsigned last = (unsigned)(w_in - 1);
  unsigned packed = 0;
#pragma unroll
  for (int k = 0; k < RS_H_PX; ++k) {
    const int i = i0 + k;
    if (i < w_out) {
      const int f = first[i];
      const int16_t* wi = w + (size_t)i * T;
      int acc = 0;
      for (int t = 0; t < T; ++t) acc = __mul24((int)s[min((unsigned)(f + t), last)], (int)wi[t]) + acc;
      packed |= rs_round(acc) << (8 * k);
    }
  }
  *reinterpret_cast<unsigned*>(mid + (size_t)blockIdx.z * mid_plane + (size_t)blockIdx.y * mid_stride + i0) = packed;
}

// The same pass with the workgroup's source span and its weights staged in LDS: taken where w lies on an 8-byte boundary
// (the context's cached tables and the staged ones do) and T <= RS_LDS_MAX_T; k_resample_h above is the path for the
// rest, as the byte paths of the other kernels are.  A workgroup's 1024
// outputs read source samples first[o0] .. first[o0 + 1023] + T - 1, at most 1023 * 8 + 1 + 33 of them at the largest ratio
// (RS_SEG holds them); the span comes in by coalesced byte loads (any base, any stride), the weights - contiguous in the
// table - by 8-byte loads, T a lane, where the workgroup is full and by 16-bit loads in the last one.  A tap is then two LDS
// reads instead of two vector loads.  An untrusted table can make a lane read LDS that was not staged, never memory outside
// the buffers: every LDS index is clamped to the segment.
constexpr int RS_SEG = 8320;
constexpr int RS_LDS_MAX_T = 17;
constexpr int RS_H_COLS = RS_NT * RS_H_PX;

__global__ __launch_bounds__(RS_NT) void k_resample_h_lds(const uint8_t* __restrict__ src, const int w_in, const int row_stride,
                                                          const size_t plane_stride, uint8_t* __restrict__ mid, const int w_out,
                                                          const int mid_stride, const size_t mid_plane,
                                                          const int32_t* __restrict__ first, const int16_t* __restrict__ w, const int T) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rs_lds[];
  uint8_t* seg = rs_lds;
  int16_t* wl = reinterpret_cast<int16_t*>(rs_lds + RS_SEG);
  const int o0 = blockIdx.x * RS_H_COLS;
  const int n_out = min(RS_H_COLS, w_out - o0);                       // >= 1 by the grid
  const uint8_t* s = src + (size_t)blockIdx.z * plane_stride + (size_t)blockIdx.y * row_stride;
  const unsigned last = (unsigned)(w_in - 1);
  const int s_lo = (int)min((unsigned)max(first[o0], 0), last);
  const int want = min(max(first[o0 + n_out - 1] + T - s_lo, 1), RS_SEG);
  const int span = min(want, w_in - s_lo);
  for (int j = threadIdx.x; j < span; j += RS_NT) seg[j] = s[s_lo + j];
  const int16_t* wb = w + (size_t)o0 * T;
  if (n_out == RS_H_COLS) {                                          // 1024 T weights = 256 T chunks of 8 bytes
    const uint2* w8 = reinterpret_cast<const uint2*>(wb);
    uint2* l8 = reinterpret_cast<uint2*>(wl);
    for (int c = threadIdx.x; c < RS_NT * T; c += RS_NT) l8[c] = w8[c];
  } else {
    for (int j = threadIdx.x; j < n_out * T; j += RS_NT) wl[j] = wb[j];
  }
  __syncthreads();
  const int i0 = o0 + threadIdx.x * RS_H_PX;
  if (i0 >= w_out) return;
  unsigned packed = 0;
#pragma unroll
  for (int k = 0; k < RS_H_PX; ++k) {
    const int i = i0 + k;
    if (i < w_out) {
      const int f = first[i];
      const int16_t* wi = wl + (threadIdx.x * RS_H_PX + k) * T;
      int acc = 0;
      for (int t = 0; t < T; ++t) {
        const unsigned at = min(min((unsigned)(f + t), last) - (unsigned)s_lo, (unsigned)(RS_SEG - 1));
        acc = __mul24((int)seg[at], (int)wi[t]) + acc;
      }
      packed |= rs_round(acc) << (8 * k);
    }
  }
  *reinterpret_cast<unsigned*>(mid + (size_t)blockIdx.z * mid_plane + (size_t)blockIdx.y * mid_stride + i0) = packed;
}

__global__ __launch_bounds__(RS_NT) void k_resample_v(const uint8_t* __restrict__ mid, const int h_in, const int mid_stride,
                                                      const size_t mid_plane, uint8_t* __restrict__ dst, const int w_out,
                                                      const int row_stride, const size_t plane_stride, const int32_t* __restrict__ first,
                                                      const int16_t* __restrict__ w, const int T, const int dst16) {
  const int c0 = (blockIdx.x * RS_NT + threadIdx.x) * RS_V_PX;
  if (c0 >= w_out) return;
  const int r = blockIdx.y;
  const uint8_t* m = mid + (size_t)blockIdx.z * mid_plane + c0;
  const int f = first[r];
  const int16_t* wr = w + (size_t)r * T;
  const unsigned last = (unsigned)(h_in - 1);
  int acc[RS_V_PX];
#pragma unroll
  for (int k = 0; k < RS_V_PX; ++k) acc[k] = 0;
  for (int t = 0; t < T; ++t) {
    const int wt = wr[t];                                    // the same in every lane of the workgroup
    if (wt == 0) continue;
    const uint4 v = *reinterpret_cast<const uint4*>(m + (size_t)min((unsigned)(f + t), last) * mid_stride);
    const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < RS_V_PX; ++k) acc[k] = __mul24((int)((q[k >> 2] >> (8 * (k & 3))) & 255u), wt) + acc[k];
  }
  unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < RS_V_PX; ++k) o[k >> 2] |= rs_round(acc[k]) << (8 * (k & 3));
  uint8_t* d = dst + (size_t)blockIdx.z * plane_stride + (size_t)r * row_stride + c0;
  if (dst16 && c0 + RS_V_PX <= w_out) {
    *reinterpret_cast<uint4*>(d) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
    const int n = min(RS_V_PX, w_out - c0);
#pragma unroll
    for (int k = 0; k < RS_V_PX; ++k)
      if (k < n) d[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
  }
}

inline int pad16(int n) { return (n + 15) & ~15; }

int check_taps(const void* first, const void* w, int T, const char* axis) {
  if (!first || !w) return set_err(WM_ERR_BADARG, "%s tap table is NULL", axis);
  if (T < 1 || T > RS_MAX_TAPS) return set_err(WM_ERR_BADARG, "%s taps: T must be in 1..33", axis);
  if (((uintptr_t)first & 3u) || ((uintptr_t)w & 1u)) return set_err(WM_ERR_BADARG, "%s tap table is misaligned", axis);
  return WM_OK;
}

// what both forms refuse, in one place; *empty: nothing to do
int check_resample(const wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int n_planes, int h_in, int w_in, int src_row_stride,
                   size_t src_plane_stride, int h_out, int w_out, int dst_row_stride, size_t dst_plane_stride, const int32_t* first_x,
                   const int16_t* w_x, int T_x, const int32_t* first_y, const int16_t* w_y, int T_y, bool* empty) {
  WM_TRY(use_ctx(ctx));
  *empty = n_planes == 0;
  if (n_planes < 0 || n_planes > 65535) return set_err(WM_ERR_BADARG, "n_planes must be in 0..65535");
  if (*empty) return WM_OK;
  if (h_in < 1 || w_in < 1 || h_out < 1 || w_out < 1) return set_err(WM_ERR_BADARG, "plane sizes must be positive");
  if (h_in > 65535 || h_out > 65535) return set_err(WM_ERR_BADARG, "more than 65535 rows");
  if ((long long)h_in > 8ll * h_out || (long long)h_out > 8ll * h_in || (long long)w_in > 8ll * w_out || (long long)w_out > 8ll * w_in)
    return set_err(WM_ERR_BADARG, "a resize beyond 8x");
  if (!src || !dst) return set_err(WM_ERR_BADARG, "plane pointer is NULL");
  if (src_row_stride < w_in || dst_row_stride < w_out) return set_err(WM_ERR_BADARG, "row_stride smaller than a row");
  if (n_planes > 1 && (src_plane_stride < plane_span(1, h_in, src_row_stride, 0, w_in) ||
                       dst_plane_stride < plane_span(1, h_out, dst_row_stride, 0, w_out)))
    return set_err(WM_ERR_BADARG, "plane_stride smaller than one plane");
  WM_TRY(check_taps(first_x, w_x, T_x, "horizontal"));
  return check_taps(first_y, w_y, T_y, "vertical");
}

// ---------------------------------------------------------------------------
// Rotation resynchronisation (include/wmhip.h, "rotation resynchronisation"): n_angles candidate rotations of n_planes planes
// ---------------------------------------------------------------------------
// A workgroup makes one 32 x 32 block of one destination plane dst[a][p]; a lane makes 4 adjacent pixels of one row of it.  The
// map is affine, so the block's source footprint is the bounding box of its four corners' 4 x 4 windows: the corners differ
// by 31 (|C| + |S|) 2^-16 < 43.85 pixels on either axis, so x0 takes at most 45 values and the box is at most 48 x 48
// (RT_SEG).  The box comes into LDS by byte loads, a row of it per 64 lanes, its indices clamped to the source there - once,
// so a pixel's 16 taps need no clamp of their own beyond the one that keeps an untrusted candidate inside the segment - and K
// by one 8-byte load a lane.  A tap is an LDS byte and a 24-bit multiply-add; the 4 pixels leave as one dword where the
// destination's base and strides are multiples of 4 and the lane's pixels are all inside the plane, byte by byte otherwise.
// Integers only, no atomics, no scratch.  Grid (column blocks, row blocks, n_angles * n_planes): nothing capped, no strided
// loop but the staging one, which takes 12 trips at any angle.
constexpr int RT_BLOCK = 32;
constexpr int RT_PX = 4;
constexpr int RT_SEG = 48;
constexpr int RT_PHASES = 256;

struct RotGeom {
  int h, w, H, W, n_planes;
  int src_row_stride, dst_row_stride;
  size_t src_plane_stride, dst_plane_stride;
};

// (U, V) of destination pixel (y, x) under candidate (C, S), in 2^-17 source pixels.  Unsigned products: an untrusted
// candidate wraps, it does not overflow.
__device__ __forceinline__ void rot_uv(const RotGeom& g, const int C, const int S, const int y, const int x, int& U, int& V) {
  const unsigned X2 = (unsigned)(2 * x + 1 - g.W), Y2 = (unsigned)(2 * y + 1 - g.H);
  U = (int)((unsigned)C * X2 - (unsigned)S * Y2 + ((unsigned)(g.w - 1) << 16));
  V = (int)((unsigned)S * X2 + (unsigned)C * Y2 + ((unsigned)(g.h - 1) << 16));
}

__global__ __launch_bounds__(RS_NT) void k_rotate_planes(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const RotGeom g,
                                                         const int32_t* __restrict__ cand, const int16_t* __restrict__ K,
                                                         const int dst4) {
  __shared__ __attribute__((aligned(16))) uint8_t seg[RT_SEG * RT_SEG];
  __shared__ __attribute__((aligned(16))) int16_t kl[RT_PHASES * 4];
  const int a = blockIdx.z / g.n_planes, p = blockIdx.z - a * g.n_planes;
  const int C = cand[2 * a], S = cand[2 * a + 1];
  const int bx = blockIdx.x * RT_BLOCK, by = blockIdx.y * RT_BLOCK;
  // the footprint: the least and the largest x0 - 1 / y0 - 1 of the block's corners (the same in every lane)
  int x_lo = INT32_MAX, y_lo = INT32_MAX, x_hi = INT32_MIN, y_hi = INT32_MIN;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    int U, V;
    rot_uv(g, C, S, by + (c >> 1) * (RT_BLOCK - 1), bx + (c & 1) * (RT_BLOCK - 1), U, V);
    x_lo = min(x_lo, (U >> 17) - 1); x_hi = max(x_hi, (U >> 17) - 1);
    y_lo = min(y_lo, (V >> 17) - 1); y_hi = max(y_hi, (V >> 17) - 1);
  }
  const int nc = min(x_hi - x_lo + 4, RT_SEG), nr = min(y_hi - y_lo + 4, RT_SEG);
  const uint8_t* s = src + (size_t)p * g.src_plane_stride;
  {
    const int c = threadIdx.x & 63;
    if (c < nc) {
      const int sx = min(max(x_lo + c, 0), g.w - 1);
      for (int r = threadIdx.x >> 6; r < nr; r += RS_NT / 64)
        seg[r * RT_SEG + c] = s[(size_t)min(max(y_lo + r, 0), g.h - 1) * g.src_row_stride + sx];
    }
  }
  reinterpret_cast<uint2*>(kl)[threadIdx.x] = reinterpret_cast<const uint2*>(K)[threadIdx.x];
  __syncthreads();
  const int y = by + (int)(threadIdx.x >> 3), x4 = bx + (int)(threadIdx.x & 7) * RT_PX;
  if (y >= g.H || x4 >= g.W) return;
  int U, V;
  rot_uv(g, C, S, y, x4, U, V);
  unsigned packed = 0;
#pragma unroll
  for (int k = 0; k < RT_PX; ++k, U = (int)((unsigned)U + 2u * (unsigned)C), V = (int)((unsigned)V + 2u * (unsigned)S)) {
    const int cx = (U >> 17) - 1 - x_lo, cy = (V >> 17) - 1 - y_lo;
    const int16_t* kx = kl + ((U >> 9) & 255) * 4;
    const int16_t* ky = kl + ((V >> 9) & 255) * 4;
    int col[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) col[i] = min(max(cx + i, 0), RT_SEG - 1);
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint8_t* row = seg + min(max(cy + j, 0), RT_SEG - 1) * RT_SEG;
      int r = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) r = __mul24((int)row[col[i]], (int)kx[i]) + r;
      acc = __mul24((r + (1 << 7)) >> 8, (int)ky[j]) + acc;
    }
    packed |= (unsigned)min(max((acc + (1 << 19)) >> 20, 0), 255) << (8 * k);
  }
  uint8_t* d = dst + ((size_t)a * g.n_planes + p) * g.dst_plane_stride + (size_t)y * g.dst_row_stride + x4;
  if (dst4 && x4 + RT_PX <= g.W) {
    *reinterpret_cast<unsigned*>(d) = packed;
  } else {
    const int n = min(RT_PX, g.W - x4);
#pragma unroll
    for (int k = 0; k < RT_PX; ++k)
      if (k < n) d[k] = (uint8_t)(packed >> (8 * k));
  }
}

constexpr int ROT_MAX_SIDE = 8192;

// what both forms refuse, in one place
int check_rotate(const wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int n_planes, int h, int w, int src_row_stride,
                 size_t src_plane_stride, int H, int W, int dst_row_stride, size_t dst_plane_stride, const int32_t* cand, int n_angles,
                 const int16_t* K) {
  WM_TRY(use_ctx(ctx));
  if (h < 1 || w < 1 || H < 1 || W < 1 || h > ROT_MAX_SIDE || w > ROT_MAX_SIDE || H > ROT_MAX_SIDE || W > ROT_MAX_SIDE)
    return set_err(WM_ERR_BADARG, "a rotation takes sides in 1..8192");
  if (n_angles < 1) return set_err(WM_ERR_BADARG, "n_angles must be at least 1");
  if (n_planes < 1 || (long long)n_planes * n_angles > 65535) return set_err(WM_ERR_BADARG, "n_planes must be at least 1 and n_angles * n_planes at most 65535");
  if (!src || !dst || !cand || !K) return set_err(WM_ERR_BADARG, "src / dst / candidates / K is NULL");
  if (src_row_stride < w || dst_row_stride < W) return set_err(WM_ERR_BADARG, "row_stride smaller than a row");
  if ((n_planes > 1 && src_plane_stride < plane_span(1, h, src_row_stride, 0, w)) ||
      ((long long)n_planes * n_angles > 1 && dst_plane_stride < plane_span(1, H, dst_row_stride, 0, W)))
    return set_err(WM_ERR_BADARG, "plane_stride smaller than one plane");
  return WM_OK;
}

}  // namespace

extern "C" {

int wm_rotate_planes_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int n_planes, int h, int w, int src_row_stride,
                            size_t src_plane_stride, int H, int W, int dst_row_stride, size_t dst_plane_stride, const int32_t* cand,
                            int n_angles, const int16_t* K) {
  WM_TRY(check_rotate(ctx, src, dst, n_planes, h, w, src_row_stride, src_plane_stride, H, W, dst_row_stride, dst_plane_stride, cand,
                      n_angles, K));
  if (((uintptr_t)cand & 3u) || ((uintptr_t)K & 7u)) return set_err(WM_ERR_BADARG, "candidates / K is misaligned (4 / 8 bytes)");
  const RotGeom g{h, w, H, W, n_planes, src_row_stride, dst_row_stride, src_plane_stride, dst_plane_stride};
  const int dst4 = (((uintptr_t)dst | (uintptr_t)dst_row_stride | (n_planes * n_angles > 1 ? (uintptr_t)dst_plane_stride : 0)) & 3u) == 0;
  const dim3 grid((unsigned)((W + RT_BLOCK - 1) / RT_BLOCK), (unsigned)((H + RT_BLOCK - 1) / RT_BLOCK), (unsigned)(n_planes * n_angles));
  hipLaunchKernelGGL(k_rotate_planes, grid, dim3(RS_NT), 0, ctx->stream, src, dst, g, cand, K, dst4);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

int wm_rotate_planes_u8(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int n_planes, int h, int w, int src_row_stride,
                        size_t src_plane_stride, int H, int W, int dst_row_stride, size_t dst_plane_stride, const int32_t* cand,
                        int n_angles, const int16_t* K) {
  WM_TRY(check_rotate(ctx, src, dst, n_planes, h, w, src_row_stride, src_plane_stride, H, W, dst_row_stride, dst_plane_stride, cand,
                      n_angles, K));
  // the destination is staged dense (its gaps on the host are neither read nor written) and copied back row by row
  const size_t dense = (size_t)H * W, n_out = (size_t)n_planes * n_angles;
  uint8_t *d_src, *d_dst; int32_t* d_cand; int16_t* d_K;
  WM_TRY(staged_call(ctx, [&](Carve& cv) {
    d_src = cv.in(plane_span(n_planes, h, src_row_stride, src_plane_stride, w), src);
    d_dst = cv.take<uint8_t>(dense * n_out);
    d_cand = cv.in((size_t)2 * n_angles, cand);
    d_K = cv.in((size_t)RT_PHASES * 4, K);
  }, [&] {
    WM_TRY(wm_rotate_planes_u8_dev(ctx, d_src, d_dst, n_planes, h, w, src_row_stride, src_plane_stride, H, W, W, dense, d_cand, n_angles,
                                   d_K));
    for (size_t q = 0; q < n_out; ++q)
      WM_HIP(hipMemcpy2DAsync(dst + q * dst_plane_stride, (size_t)dst_row_stride, d_dst + q * dense, (size_t)W, (size_t)W, (size_t)H,
                              hipMemcpyDeviceToHost, ctx->stream));
    return WM_OK;
  }, true));
  return WM_OK;
}

int wm_resample_planes_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int n_planes, int h_in, int w_in, int src_row_stride,
                              size_t src_plane_stride, int h_out, int w_out, int dst_row_stride, size_t dst_plane_stride,
                              const int32_t* first_x, const int16_t* w_x, int T_x, const int32_t* first_y, const int16_t* w_y,
                              int T_y) {
  bool empty;
  WM_TRY(check_resample(ctx, src, dst, n_planes, h_in, w_in, src_row_stride, src_plane_stride, h_out, w_out, dst_row_stride,
                        dst_plane_stride, first_x, w_x, T_x, first_y, w_y, T_y, &empty));
  if (empty) return WM_OK;
  const int mid_stride = pad16(w_out);
  const size_t mid_plane = (size_t)mid_stride * h_in;
  uint8_t* mid;
  WM_TRY(staged(ctx, &ctx->resample_ws, &ctx->resample_ws_bytes, "resample intermediate",
                [&](Carve& cv) { mid = cv.take<uint8_t>(mid_plane * n_planes); }));
  const int dst16 = (((uintptr_t)dst | (uintptr_t)dst_row_stride | (n_planes > 1 ? (uintptr_t)dst_plane_stride : 0)) & 15u) == 0;
  const unsigned bx_h = (unsigned)((w_out + RS_NT * RS_H_PX - 1) / (RS_NT * RS_H_PX));
  const unsigned bx_v = (unsigned)((w_out + RS_NT * RS_V_PX - 1) / (RS_NT * RS_V_PX));
  if (T_x <= RS_LDS_MAX_T && ((uintptr_t)w_x & 7u) == 0)
    hipLaunchKernelGGL(k_resample_h_lds, dim3(bx_h, h_in, n_planes), dim3(RS_NT), (size_t)RS_SEG + (size_t)RS_NT * 8 * T_x, ctx->stream,
                       src, w_in, src_row_stride, src_plane_stride, mid, w_out, mid_stride, mid_plane, first_x, w_x, T_x);
  else
    hipLaunchKernelGGL(k_resample_h, dim3(bx_h, h_in, n_planes), dim3(RS_NT), 0, ctx->stream, src, w_in, src_row_stride,
                       src_plane_stride, mid, w_out, mid_stride, mid_plane, first_x, w_x, T_x);
  hipLaunchKernelGGL(k_resample_v, dim3(bx_v, h_out, n_planes), dim3(RS_NT), 0, ctx->stream, mid, h_in, mid_stride, mid_plane, dst,
                     w_out, dst_row_stride, dst_plane_stride, first_y, w_y, T_y, dst16);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

int wm_resample_planes_u8(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int n_planes, int h_in, int w_in, int src_row_stride,
                          size_t src_plane_stride, int h_out, int w_out, int dst_row_stride, size_t dst_plane_stride,
                          const int32_t* first_x, const int16_t* w_x, int T_x, const int32_t* first_y, const int16_t* w_y, int T_y) {
  bool empty;
  WM_TRY(check_resample(ctx, src, dst, n_planes, h_in, w_in, src_row_stride, src_plane_stride, h_out, w_out, dst_row_stride,
                        dst_plane_stride, first_x, w_x, T_x, first_y, w_y, T_y, &empty));
  if (empty) return WM_OK;
  // the destination is staged dense (its gaps on the host are neither read nor written) and copied back row by row
  const size_t dense = (size_t)h_out * w_out;
  uint8_t *d_src, *d_dst; int32_t *d_fx, *d_fy; int16_t *d_wx, *d_wy;
  WM_TRY(staged_call(ctx, [&](Carve& cv) {
    d_src = cv.in(plane_span(n_planes, h_in, src_row_stride, src_plane_stride, w_in), src);
    d_dst = cv.take<uint8_t>(dense * n_planes);
    d_fx = cv.in((size_t)w_out, first_x); d_wx = cv.in((size_t)w_out * T_x, w_x);
    d_fy = cv.in((size_t)h_out, first_y); d_wy = cv.in((size_t)h_out * T_y, w_y);
  }, [&] {
    WM_TRY(wm_resample_planes_u8_dev(ctx, d_src, d_dst, n_planes, h_in, w_in, src_row_stride, src_plane_stride, h_out, w_out, w_out,
                                     dense, d_fx, d_wx, T_x, d_fy, d_wy, T_y));
    for (int p = 0; p < n_planes; ++p)
      WM_HIP(hipMemcpy2DAsync(dst + (size_t)p * dst_plane_stride, (size_t)dst_row_stride, d_dst + (size_t)p * dense, (size_t)w_out,
                              (size_t)w_out, (size_t)h_out, hipMemcpyDeviceToHost, ctx->stream));
    return WM_OK;
  }, true));
  return WM_OK;
}

}  // extern "C"
