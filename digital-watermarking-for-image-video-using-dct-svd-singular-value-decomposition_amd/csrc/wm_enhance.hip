// Extract post-processing chain on the GPU (app_dct_svd_single.py:223-227 gray, 275-277 colour, 88-110):
//   k_nlmeans<CH>   fastNlMeansDenoising, 7x7 template, 21x21 search, L2, 1 or 2 interleaved channels   (hot path)
//   k_clahe_hist    createCLAHE(2.0, (8, 8)): per-tile histogram, clip + redistribute, cumulative sum -> LUT set
//   k_clahe_apply   bilinear interpolation of the four neighbouring tiles' LUTs
//   k_unsharp       GaussianBlur(sigma 1, 7 integer taps) + addWeighted, one LDS tile
//   k_lab_fwd / k_lab_inv   COLOR_LBGR2Lab / COLOR_Lab2LBGR, 8-bit
// The arithmetic is in wm_enhance_math.h, shared with the CPU harness; tests/enhance_oracle.py is the specification.
// Everything is exact integer work except the CLAHE interpolation, the blend and Lab -> BGR (f32, no fused operations),
// so the kernels match the oracle bit for bit.
#include <math.h>
#include <string.h>

#include "wm_internal.h"
#include "wm_enhance_math.h"

using namespace wmi;

namespace {

// ---- NL-means ----------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per 64 x 26 output tile.  The (26 + 26) x (64 + 26) bordered window is loaded into LDS
// once (reflect-101 resolved at load), with the weight table's non-zero prefix.  Per search offset:
//   row pass   32 rows x 8 segments of 8 columns: the template-extended region's squared differences, summed 7 wide
//              along the row (sliding) -> rs[32][64] in LDS
//   column     64 columns x 4 groups of 7 output rows: sliding 7-row sum of rs in registers -> ssd, weight lookup,
//              est / wsum accumulated in registers
// Everything exact in 32 bits.
constexpr int NLM_TW = 64, NLM_TH = 26, NLM_THREADS = 256;
constexpr int NLM_B = wme::NLM_BORDER;                      // 13
constexpr int NLM_R = wme::NLM_SEARCH / 2;                  // 10
constexpr int NLM_T = wme::NLM_TEMPLATE / 2;                // 3
constexpr int NLM_WW = NLM_TW + 2 * NLM_B, NLM_WH = NLM_TH + 2 * NLM_B;   // 90 x 52
constexpr int NLM_RH = NLM_TH + 2 * NLM_T;                  // 32 template-extended rows
constexpr int NLM_RP = NLM_TW + 1;                          // row pitch of rs: the row pass writes without bank conflicts
constexpr int NLM_SHIFT = 6;                                // log2(next_pow2(7 * 7))
constexpr int NLM_ROWS = 7;                                 // output rows per thread in the column pass
static_assert(NLM_RH * 8 == NLM_THREADS, "row pass: one 8-column segment per thread");
static_assert(4 * NLM_ROWS >= NLM_TH && 4 * 64 == NLM_THREADS, "column pass: 64 columns x 4 row groups");

template <int CH>
__global__ __launch_bounds__(NLM_THREADS) void k_nlmeans(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                        const int H, const int W, const int* __restrict__ lut,
                                                        const int n_nz) {
  __shared__ uint8_t win[CH][NLM_WH][NLM_WW];
  __shared__ uint32_t rs[NLM_RH * NLM_RP];
  __shared__ int wl[wme::NLM_MAX_LUT];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * NLM_TW, y0 = blockIdx.y * NLM_TH;
  for (int i = tid; i < NLM_WH * NLM_WW; i += NLM_THREADS) {
    const int wy = i / NLM_WW, wx = i - wy * NLM_WW;
    const int gy = wme::reflect101(y0 - NLM_B + wy, H), gx = wme::reflect101(x0 - NLM_B + wx, W);
    const uint8_t* p = src + ((size_t)gy * W + gx) * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) win[c][wy][wx] = p[c];
  }
  for (int i = tid; i <= n_nz; i += NLM_THREADS) wl[i] = lut[i];      // lut[n_nz] == 0
  __syncthreads();

  // row pass: row r of the template-extended region (window row r + NLM_B - NLM_T), columns 8s .. 8s+7
  const int pr = tid >> 3, ps = (tid & 7) * 8;
  // column pass: column cx, output rows g*7 ..
  const int cx = tid & 63, g = tid >> 6;
  const int ry0 = g * NLM_ROWS;
  const int nrows = min(NLM_ROWS, NLM_TH - ry0);            // wave-uniform: 7, 7, 7, 5
  uint32_t est[NLM_ROWS][CH], wsum[NLM_ROWS];
#pragma unroll
  for (int j = 0; j < NLM_ROWS; ++j) {
    wsum[j] = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) est[j][c] = 0;
  }
  for (int dy = -NLM_R; dy <= NLM_R; ++dy) {
    for (int dx = -NLM_R; dx <= NLM_R; ++dx) {
      {
        const int wr = pr + NLM_B - NLM_T;
        const int wc = ps + NLM_B - NLM_T;
        uint32_t d[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) {
          uint32_t s = 0;
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            const int e = (int)win[c][wr][wc + k] - (int)win[c][wr + dy][wc + k + dx];
            s += (uint32_t)(e * e);
          }
          d[k] = s;
        }
        uint32_t acc = d[0] + d[1] + d[2] + d[3] + d[4] + d[5] + d[6];
        uint32_t* out = rs + pr * NLM_RP + ps;
        out[0] = acc;
#pragma unroll
        for (int j = 1; j < 8; ++j) {
          acc += d[j + 6] - d[j - 1];
          out[j] = acc;
        }
      }
      __syncthreads();
      if (nrows > 0) {
        const uint32_t* col = rs + ry0 * NLM_RP + cx;
        uint32_t acc = col[0] + col[NLM_RP] + col[2 * NLM_RP] + col[3 * NLM_RP] + col[4 * NLM_RP] + col[5 * NLM_RP];
        const int pc = cx + NLM_B + dx;
#pragma unroll
        for (int j = 0; j < NLM_ROWS; ++j) {
          if (j < nrows) {
            acc += col[(j + 6) * NLM_RP];
            const uint32_t ad = min(acc >> NLM_SHIFT, (uint32_t)n_nz);
            const uint32_t w = (uint32_t)wl[ad];
            const int prw = ry0 + j + NLM_B + dy;
            wsum[j] += w;
#pragma unroll
            for (int c = 0; c < CH; ++c) est[j][c] += w * (uint32_t)win[c][prw][pc];
            acc -= col[j * NLM_RP];
          }
        }
      }
      __syncthreads();
    }
  }
  const int x = x0 + cx;
  if (x < W) {
#pragma unroll
    for (int j = 0; j < NLM_ROWS; ++j) {
      const int y = y0 + ry0 + j;
      if (j < nrows && y < H) {
#pragma unroll
        for (int c = 0; c < CH; ++c) dst[((size_t)y * W + x) * CH + c] = (uint8_t)wme::nlm_divide(est[j][c], wsum[j]);
      }
    }
  }
}

// ---- CLAHE -------------------------------------------------------------------------------------------------------
// pixels are read / written at p[(y * W + x) * pstride]: pstride 3 is the Y byte of interleaved YCrCb
struct ClaheGeom {
  int H, W, pstride, tiles_x, tiles_y, tw, th, clip;
  float lut_scale, inv_tw, inv_th;
};

__global__ __launch_bounds__(256) void k_clahe_hist(const uint8_t* __restrict__ src, const ClaheGeom g,
                                                   uint8_t* __restrict__ luts) {
  __shared__ int hist[wme::CLAHE_BINS];
  const int tx = blockIdx.x, ty = blockIdx.y;
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int n = g.tw * g.th;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int r = i / g.tw, c = i - r * g.tw;
    const int y = wme::reflect101(ty * g.th + r, g.H), x = wme::reflect101(tx * g.tw + c, g.W);   // padded bottom / right
    atomicAdd(&hist[src[((size_t)y * g.W + x) * g.pstride]], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {       // 256 bins: clip + redistribute and the running sum, in order, on one lane (in LDS)
    wme::clahe_clip_hist(hist, g.clip);
    int sum = 0;
    for (int i = 0; i < wme::CLAHE_BINS; ++i) { sum += hist[i]; hist[i] = sum; }
  }
  __syncthreads();
  luts[((size_t)ty * g.tiles_x + tx) * wme::CLAHE_BINS + threadIdx.x] =
      (uint8_t)wme::clahe_lut_value(hist[threadIdx.x], g.lut_scale);
}

// src may be dst (the colour chain equalises the Y bytes of YCrCb in place): each lane reads its byte, then writes it
__global__ __launch_bounds__(256) void k_clahe_apply(const uint8_t* src, const ClaheGeom g, const uint8_t* __restrict__ luts,
                                                    uint8_t* dst) {
  const int y = blockIdx.y;
  int ty1, ty2;
  float ya, ya1;
  wme::clahe_axis(y, g.inv_th, g.tiles_y, ty1, ty2, ya, ya1);
  const uint8_t* l1 = luts + (size_t)ty1 * g.tiles_x * wme::CLAHE_BINS;
  const uint8_t* l2 = luts + (size_t)ty2 * g.tiles_x * wme::CLAHE_BINS;
  for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < g.W; x += gridDim.x * blockDim.x) {
    int tx1, tx2;
    float xa, xa1;
    wme::clahe_axis(x, g.inv_tw, g.tiles_x, tx1, tx2, xa, xa1);
    const size_t o = ((size_t)y * g.W + x) * g.pstride;
    const int v = src[o];
    const int i1 = tx1 * wme::CLAHE_BINS + v, i2 = tx2 * wme::CLAHE_BINS + v;
    dst[o] = (uint8_t)wme::clahe_blend(l1[i1], l1[i2], l2[i1], l2[i2], xa1, xa, ya1, ya);
  }
}

// ---- unsharp -----------------------------------------------------------------------------------------------------
// 64 x 16 output pixels of one channel per 256-thread workgroup (blockIdx.z = channel of an interleaved image):
// the (16 + 6) x (64 + 6) input tile, its row pass in LDS, then the column pass and the blend per pixel.
constexpr int US_TW = 64, US_TH = 16;
__global__ __launch_bounds__(256) void k_unsharp(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int H,
                                                const int W, const int CH, const float alpha, const float beta) {
  __shared__ uint8_t tile[US_TH + 6][US_TW + 6];
  __shared__ uint32_t rows[US_TH + 6][US_TW];
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * US_TW, y0 = blockIdx.y * US_TH;
  for (int i = threadIdx.x; i < (US_TH + 6) * (US_TW + 6); i += blockDim.x) {
    const int r = i / (US_TW + 6), q = i - r * (US_TW + 6);
    const int gy = wme::reflect101(y0 - 3 + r, H), gx = wme::reflect101(x0 - 3 + q, W);
    tile[r][q] = src[((size_t)gy * W + gx) * CH + c];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (US_TH + 6) * US_TW; i += blockDim.x) {
    const int r = i / US_TW, q = i - r * US_TW;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) s += (uint32_t)wme::blur_tap(k) * tile[r][q + k];
    rows[r][q] = s;
  }
  __syncthreads();
  const int q = threadIdx.x & (US_TW - 1);
  for (int r = threadIdx.x / US_TW; r < US_TH; r += blockDim.x / US_TW) {
    const int y = y0 + r, x = x0 + q;
    if (y < H && x < W) {
      uint32_t s = 0;
#pragma unroll
      for (int k = 0; k < 7; ++k) s += (uint32_t)wme::blur_tap(k) * rows[r + k][q];
      dst[((size_t)y * W + x) * CH + c] = (uint8_t)wme::unsharp_px(tile[r + 3][q + 3], wme::blur_round(s), alpha, beta);
    }
  }
}

// ---- Lab ---------------------------------------------------------------------------------------------------------
// L at l[i * lstep], a / b at ab[i * abstep], ab[i * abstep + 1]: interleaved Lab (steps 3, 3 with ab = l + 1) or the
// split L plane + ab pair the denoiser takes (steps 1, 2)
struct LabFwd { int C[9]; };
struct LabInv { float C[9]; };

__global__ __launch_bounds__(256) void k_lab_fwd(const uint8_t* __restrict__ bgr, const uint16_t* __restrict__ tab,
                                                const LabFwd k, uint8_t* l, const int lstep, uint8_t* ab,
                                                const int abstep, const size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t L, A, B;
    wme::bgr_to_lab_px(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2], tab, k.C, L, A, B);
    l[i * lstep] = (uint8_t)L;
    ab[i * abstep] = (uint8_t)A;
    ab[i * abstep + 1] = (uint8_t)B;
  }
}

__global__ __launch_bounds__(256) void k_lab_inv(const uint8_t* l, const int lstep, const uint8_t* ab, const int abstep,
                                                const LabInv k, uint8_t* bgr, const size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t b, g, r;
    wme::lab_to_bgr_px(l[i * lstep], ab[i * abstep], ab[i * abstep + 1], k.C, b, g, r);
    bgr[3 * i] = (uint8_t)b;
    bgr[3 * i + 1] = (uint8_t)g;
    bgr[3 * i + 2] = (uint8_t)r;
  }
}

inline unsigned grid_for(size_t n, unsigned cap = 256 * 8) {
  const size_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---- device tables -----------------------------------------------------------------------------------------------
constexpr size_t TAB_LUT_BYTES = (size_t)wm_ctx::ENH_SLOTS * wm_ctx::ENH_LUT * sizeof(int);
constexpr size_t TAB_BYTES = TAB_LUT_BYTES + wme::LAB_CBRT_N * sizeof(uint16_t);
constexpr size_t CLAHE_LUT_BYTES = 16 * 16 * wme::CLAHE_BINS;   // tile grids up to 16 x 16
static_assert(wm_ctx::ENH_LUT == wme::NLM_MAX_LUT, "one table size");

int ensure_tab(wm_ctx* ctx) {
  size_t have = ctx->enh_tab ? TAB_BYTES : 0;
  return grow(ctx, &ctx->enh_tab, &have, TAB_BYTES, "enhance tables");
}

// the weight table's non-zero prefix for (h, channels) on the device; built on the host on a miss, kept in one of
// ENH_SLOTS slots (the gray chain's h = 7 and the colour chain's two h = 3 tables stay resident together)
int nlm_table(wm_ctx* ctx, float h, int channels, const int** d_lut, int* n_nz) {
  WM_TRY(ensure_tab(ctx));
  uint32_t hb;
  memcpy(&hb, &h, 4);
  const uint64_t key = (((uint64_t)hb << 8) | (uint64_t)channels) + 1;
  int slot = -1;
  for (int s = 0; s < wm_ctx::ENH_SLOTS; ++s)
    if (ctx->enh_key[s] == key) slot = s;
  if (slot < 0) {
    int tmp[wm_ctx::ENH_LUT];
    const int n = wme::nlm_weights(h, channels, wme::NLM_TEMPLATE, wme::NLM_SEARCH, tmp, wm_ctx::ENH_LUT);
    if (n < 0) return set_err(WM_ERR_BADARG, "h is too large: the NL-means weight table does not fit");
    slot = ctx->enh_next;
    ctx->enh_next = (ctx->enh_next + 1) % wm_ctx::ENH_SLOTS;
    if (ctx->enh_key[slot]) WM_HIP(hipStreamSynchronize(ctx->stream));    // an earlier upload may still read the slot
    memcpy(ctx->enh_host[slot], tmp, (n + 1) * sizeof(int));
    WM_HIP(hipMemcpyAsync((char*)ctx->enh_tab + (size_t)slot * wm_ctx::ENH_LUT * sizeof(int), ctx->enh_host[slot],
                          (n + 1) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ctx->enh_key[slot] = key;
    ctx->enh_n[slot] = n;
  }
  *d_lut = (const int*)((char*)ctx->enh_tab + (size_t)slot * wm_ctx::ENH_LUT * sizeof(int));
  *n_nz = ctx->enh_n[slot];
  return WM_OK;
}

int lab_table(wm_ctx* ctx, const uint16_t** d_tab, LabFwd* fwd, LabInv* inv) {
  WM_TRY(ensure_tab(ctx));
  int C[9];
  uint16_t tab[wme::LAB_CBRT_N];
  wme::lab_tables(tab, C);
  if (!ctx->enh_lab_ready) {          // uploaded once per context from a host copy that is never rewritten
    memcpy(ctx->enh_lab_host, tab, sizeof(tab));
    WM_HIP(hipMemcpyAsync((char*)ctx->enh_tab + TAB_LUT_BYTES, ctx->enh_lab_host, wme::LAB_CBRT_N * sizeof(uint16_t),
                          hipMemcpyHostToDevice, ctx->stream));
    ctx->enh_lab_ready = 1;
  }
  *d_tab = (const uint16_t*)((char*)ctx->enh_tab + TAB_LUT_BYTES);
  if (fwd) memcpy(fwd->C, C, sizeof(C));
  if (inv) wme::lab_inv_coeffs(inv->C);
  return WM_OK;
}

int check_plane(wm_ctx* ctx, const void* src, const void* dst, int H, int W) {
  WM_TRY(use_ctx(ctx));
  if (!src || !dst) return set_err(WM_ERR_BADARG, "NULL argument");
  if (H <= 0 || W <= 0) return set_err(WM_ERR_BADARG, "H and W must be positive");
  return WM_OK;
}

int nlmeans_launch(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, int channels, float h) {
  const int* d_lut;
  int n_nz;
  WM_TRY(nlm_table(ctx, h, channels, &d_lut, &n_nz));
  const dim3 grid((W + NLM_TW - 1) / NLM_TW, (H + NLM_TH - 1) / NLM_TH);
  if (channels == 1)
    hipLaunchKernelGGL((k_nlmeans<1>), grid, dim3(NLM_THREADS), 0, ctx->stream, src, dst, H, W, d_lut, n_nz);
  else
    hipLaunchKernelGGL((k_nlmeans<2>), grid, dim3(NLM_THREADS), 0, ctx->stream, src, dst, H, W, d_lut, n_nz);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

// luts: CLAHE_LUT_BYTES of device memory
int clahe_launch(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, int pstride, float clip_limit, int tiles_x,
                 int tiles_y, uint8_t* luts) {
  ClaheGeom g;
  g.H = H; g.W = W; g.pstride = pstride; g.tiles_x = tiles_x; g.tiles_y = tiles_y;
  int Hp, Wp;
  wme::clahe_padded(H, W, tiles_x, tiles_y, Hp, Wp);
  g.tw = Wp / tiles_x; g.th = Hp / tiles_y;
  const int total = g.tw * g.th;
  g.clip = wme::clahe_clip_count((double)clip_limit, total);
  g.lut_scale = wme::clahe_lut_scale(total);
  g.inv_tw = 1.0f / (float)g.tw;
  g.inv_th = 1.0f / (float)g.th;
  hipLaunchKernelGGL(k_clahe_hist, dim3(tiles_x, tiles_y), dim3(256), 0, ctx->stream, src, g, luts);
  WM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_clahe_apply, dim3((W + 255) / 256 < 8 ? (W + 255) / 256 : 8, H), dim3(256), 0, ctx->stream, src, g,
                     (const uint8_t*)luts, dst);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

int unsharp_launch(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, int channels, float amount) {
  float alpha, beta;
  wme::unsharp_weights(amount, alpha, beta);
  const dim3 grid((W + US_TW - 1) / US_TW, (H + US_TH - 1) / US_TH, channels);
  hipLaunchKernelGGL(k_unsharp, grid, dim3(256), 0, ctx->stream, src, dst, H, W, channels, alpha, beta);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

}  // namespace

extern "C" {

int wm_nlmeans_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, int channels, float h, int template_ws,
                      int search_ws) {
  WM_TRY(check_plane(ctx, src, dst, H, W));
  if (channels != 1 && channels != 2) return set_err(WM_ERR_BADARG, "NL-means takes 1 or 2 channels");
  if (template_ws != wme::NLM_TEMPLATE || search_ws != wme::NLM_SEARCH)
    return set_err(WM_ERR_BADARG, "NL-means supports template 7 with search 21 only");
  if (!(h > 0.0f) || !isfinite(h)) return set_err(WM_ERR_BADARG, "h must be positive");
  const size_t bytes = (size_t)H * W * channels;
  if ((const uint8_t*)src < dst + bytes && dst < (const uint8_t*)src + bytes)
    return set_err(WM_ERR_BADARG, "NL-means cannot run in place");
  return nlmeans_launch(ctx, src, dst, H, W, channels, h);
}

int wm_clahe_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, float clip_limit, int tiles_x,
                    int tiles_y) {
  WM_TRY(check_plane(ctx, src, dst, H, W));
  if (tiles_x < 1 || tiles_y < 1 || tiles_x > 16 || tiles_y > 16) return set_err(WM_ERR_BADARG, "tile grid must be 1..16 per side");
  if (!isfinite(clip_limit)) return set_err(WM_ERR_BADARG, "clip_limit must be finite");
  WM_TRY(grow(ctx, &ctx->enh_ws, &ctx->enh_ws_bytes, CLAHE_LUT_BYTES, "enhance workspace"));
  return clahe_launch(ctx, src, dst, H, W, 1, clip_limit, tiles_x, tiles_y, (uint8_t*)ctx->enh_ws);
}

int wm_unsharp_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, int channels, float amount) {
  WM_TRY(check_plane(ctx, src, dst, H, W));
  if (channels != 1 && channels != 3) return set_err(WM_ERR_BADARG, "unsharp takes 1 or 3 channels");
  if (!isfinite(amount)) return set_err(WM_ERR_BADARG, "amount must be finite");
  const size_t bytes = (size_t)H * W * channels;
  if (src < dst + bytes && dst < src + bytes) return set_err(WM_ERR_BADARG, "unsharp cannot run in place");
  return unsharp_launch(ctx, src, dst, H, W, channels, amount);
}

int wm_bgr_to_lab_u8_dev(wm_ctx* ctx, const uint8_t* bgr, uint8_t* lab, size_t n_px) {
  WM_TRY(use_ctx(ctx));
  if (n_px == 0) return WM_OK;
  if (!bgr || !lab) return set_err(WM_ERR_BADARG, "NULL argument");
  const uint16_t* tab;
  LabFwd f;
  WM_TRY(lab_table(ctx, &tab, &f, nullptr));
  hipLaunchKernelGGL(k_lab_fwd, dim3(grid_for(n_px)), dim3(256), 0, ctx->stream, bgr, tab, f, lab, 3, lab + 1, 3, n_px);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

int wm_lab_to_bgr_u8_dev(wm_ctx* ctx, const uint8_t* lab, uint8_t* bgr, size_t n_px) {
  WM_TRY(use_ctx(ctx));
  if (n_px == 0) return WM_OK;
  if (!bgr || !lab) return set_err(WM_ERR_BADARG, "NULL argument");
  LabInv k;
  wme::lab_inv_coeffs(k.C);
  hipLaunchKernelGGL(k_lab_inv, dim3(grid_for(n_px)), dim3(256), 0, ctx->stream, lab, 3, lab + 1, 3, k, bgr, n_px);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

// channels 1: nlmeans(h 7) -> CLAHE -> unsharp 0.25 (single:223-227, 88-96)
// channels 3: BGR -> Lab, nlmeans(L, h 3), nlmeans(ab, h 3), Lab -> BGR, CLAHE on Y of YCrCb, unsharp 0.15 (single:275-277, 98-110)
// Intermediates live in the context's grow-only enhance workspace; src may equal dst.
int wm_enhance_extract_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, int channels) {
  WM_TRY(check_plane(ctx, src, dst, H, W));
  if (channels != 1 && channels != 3) return set_err(WM_ERR_BADARG, "the chain takes 1 (gray) or 3 (BGR) channels");
  const size_t n = (size_t)H * W;
  // three segments, each an L plane and the ab pair on the next 256-byte line behind it; from its first byte a segment
  // also holds one interleaved BGR / YCrCb image (3 n bytes end no later than the ab pair does)
  uint8_t *luts, *A, *AB, *B, *AB2, *C;
  WM_TRY(staged(ctx, &ctx->enh_ws, &ctx->enh_ws_bytes, "enhance workspace", [&](Carve& cv) {
    luts = cv.take<uint8_t>(CLAHE_LUT_BYTES);
    A = cv.take<uint8_t>(n); AB = cv.take<uint8_t>(2 * n);
    B = cv.take<uint8_t>(n); AB2 = cv.take<uint8_t>(2 * n);
    C = cv.take<uint8_t>(3 * n);
  }));
  if (channels == 1) {
    WM_TRY(nlmeans_launch(ctx, src, A, H, W, 1, 7.0f));
    WM_TRY(clahe_launch(ctx, A, B, H, W, 1, 2.0f, 8, 8, luts));
    return unsharp_launch(ctx, B, dst, H, W, 1, 0.25f);
  }
  const uint16_t* tab;
  LabFwd f;
  LabInv inv;
  WM_TRY(lab_table(ctx, &tab, &f, &inv));
  uint8_t *L = A, *L2 = B;
  hipLaunchKernelGGL(k_lab_fwd, dim3(grid_for(n)), dim3(256), 0, ctx->stream, src, tab, f, L, 1, AB, 2, n);
  WM_HIP(hipGetLastError());
  WM_TRY(nlmeans_launch(ctx, L, L2, H, W, 1, 3.0f));
  WM_TRY(nlmeans_launch(ctx, AB, AB2, H, W, 2, 3.0f));
  hipLaunchKernelGGL(k_lab_inv, dim3(grid_for(n)), dim3(256), 0, ctx->stream, L2, 1, AB2, 2, inv, C, n);
  WM_HIP(hipGetLastError());
  WM_TRY(wm_bgr_to_ycrcb_u8_dev(ctx, C, A, n));
  WM_TRY(clahe_launch(ctx, A, A, H, W, 3, 2.0f, 8, 8, luts));        // Y in place: the LUTs are built before it is rewritten
  WM_TRY(wm_ycrcb_to_bgr_u8_dev(ctx, A, B, n));
  return unsharp_launch(ctx, B, dst, H, W, 3, 0.15f);
}

int wm_enhance_extract_u8(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, int channels) {
  WM_TRY(check_plane(ctx, src, dst, H, W));
  if (channels != 1 && channels != 3) return set_err(WM_ERR_BADARG, "the chain takes 1 (gray) or 3 (BGR) channels");
  const size_t bytes = (size_t)H * W * channels;
  uint8_t *d_src, *d_dst;
  WM_TRY(staged(ctx, &ctx->scratch, &ctx->scratch_bytes, "scratch", [&](Carve& cv) {
    d_src = cv.take<uint8_t>(bytes); d_dst = cv.take<uint8_t>(bytes);
  }));
  WM_HIP(hipMemcpyAsync(d_src, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  WM_TRY(wm_enhance_extract_u8_dev(ctx, d_src, d_dst, H, W, channels));
  WM_HIP(hipMemcpyAsync(dst, d_dst, bytes, hipMemcpyDeviceToHost, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  return WM_OK;
}

}  // extern "C"
