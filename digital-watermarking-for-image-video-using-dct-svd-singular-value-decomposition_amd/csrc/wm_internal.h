// Internal declarations shared by the translation units of libwmhip.so
// (wmhip.hip: tile-mode kernels + context; wm_payload.hip: blind payload; wm_ref.hip: full-frame mode).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <type_traits>

#include "../../include/wmhip.h"

namespace wmi {

constexpr int WAVE = 64;
constexpr int N_EVENTS = 64;

int set_err(int code, const char* fmt, const char* a = "", const char* b = "");

#define WM_HIP(call)                                                                               \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) return wmi::set_err(WM_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

#define WM_TRY(call)              \
  do {                            \
    int rc_ = (call);             \
    if (rc_ != WM_OK) return rc_; \
  } while (0)

}  // namespace wmi

struct wm_ctx {
  int device = 0;
  int n_cu = 256;                 // multiProcessorCount of the device (persistent grids are sized from it)
  hipStream_t stream = nullptr;
  bool owns_stream = false;
  int* d_status = nullptr;        // [0] sticky kernel status, [1] embed literal-fallback count, [2] constant-tile count
  void* scratch = nullptr;        // grow-only device scratch (host-pointer wrappers)
  size_t scratch_bytes = 0;
  void* partials = nullptr;       // grow-only detect partial sums
  size_t partials_bytes = 0;
  void* fb_list = nullptr;        // grow-only list of tiles for the embed fallback
  size_t fb_bytes = 0;
  void* ref_ws = nullptr;         // grow-only workspace of the full-frame mode
  size_t ref_ws_bytes = 0;
  void* ref_ws2 = nullptr;        // second one: null-space completion of rank-deficient planes
  size_t ref_ws2_bytes = 0;
  void* route_tmp = nullptr;      // grow-only staging of the routed unscramble (wm_route.hip): bucket-major bytes + min-max pairs
  size_t route_tmp_bytes = 0;
  void* extract_f32 = nullptr;    // grow-only float estimate + min-max partials of wm_extract_unscrambled_u8_dev
  size_t extract_f32_bytes = 0;
  void* sigma_ws = nullptr;       // grow-only output of a sigma pass inside one call: the masked / payload embed's sigma_w
  size_t sigma_ws_bytes = 0;      // rows (k_sigma_pass -> the embed launches), or the payload decode's per-tile metric
  void* resample_ws = nullptr;    // grow-only intermediate of the resampler (wm_resample.hip): the planes after the horizontal pass
  size_t resample_ws_bytes = 0;
  static constexpr int MAX_PAIR_TABS = 6;   // round-robin tournaments of the block Jacobi, by block count
  void* pair_tab[MAX_PAIR_TABS] = {};
  int pair_tab_nbk[MAX_PAIR_TABS] = {};
  int pair_tab_next = 0;
  void* hier_dev[MAX_PAIR_TABS] = {};       // two-level (super-block) tournament tables of the block Jacobi, by block count: device part
  void* hier_host[MAX_PAIR_TABS] = {};      // ... and the host part (malloc)
  int hier_key[MAX_PAIR_TABS] = {};         // block count * 16 + super-block size the table was built for
  int hier_next = 0;
  void* hier_ws = nullptr;        // grow-only workspace of the two-level scheme (tracked Gram matrices, rotations, partial sums)
  size_t hier_ws_bytes = 0;
  float* dct_mat[2] = {nullptr, nullptr};   // cached DCT-II basis matrices (device), by size
  int dct_n[2] = {0, 0};
  int ref_last_sweeps = 0;        // outer Jacobi sweeps of the last full-frame SVD (diagnostics)
  double ref_last_flops = 0.0;    // matrix-core flops its Gram / rotation products issued (nominal: skipped pairs counted)
  int ref_last_hier = 0;          // 1: it ran the two-level scheme
  float ref_skip_thr = 0.0f;      // residual cosine the last full-frame Jacobi may have left between two rows
  bool hier_attr_set = false;     // the two-level rotation kernels' dynamic-LDS limits are raised on this context's device
  static constexpr int MAX_AUX = 7;   // extra queues of the batched full-frame Jacobi (created on first use)
  hipStream_t aux_stream[MAX_AUX] = {};
  hipEvent_t ev_fork[MAX_AUX] = {}, ev_join[MAX_AUX] = {};
  hipEvent_t ev[wmi::N_EVENTS] = {};
  // extract post-processing chain (wm_enhance.hip)
  void* enh_ws = nullptr;         // grow-only intermediates of wm_enhance_extract_u8_dev / wm_nlmeans / wm_clahe
  size_t enh_ws_bytes = 0;
  void* enh_tab = nullptr;        // device tables: ENH_SLOTS NL-means weight prefixes, then the Lab tables
  static constexpr int ENH_SLOTS = 4;
  static constexpr int ENH_LUT = 2048;   // == wme::NLM_MAX_LUT
  uint64_t enh_key[ENH_SLOTS] = {};      // (h bits, channels) + 1 of the prefix a slot holds, 0 = empty
  int enh_n[ENH_SLOTS] = {};
  int enh_next = 0;
  int enh_lab_ready = 0;
  int enh_host[ENH_SLOTS][ENH_LUT] = {}; // host source of each slot's upload (kept until the slot is reused)
  uint16_t enh_lab_host[3072] = {};     // host source of the Lab cube-root table upload
};

namespace wmi {
// first statement of every entry point that takes a context: NULL check, and make the
// context's device current (a process may hold contexts on several devices; hipMalloc and
// kernel launches follow the calling thread's current device)
inline int use_ctx(const wm_ctx* ctx) {
  if (!ctx) return set_err(WM_ERR_BADARG, "ctx is NULL");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return set_err(WM_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  return WM_OK;
}
// grow-only device buffer (synchronises the stream before freeing the old one)
int grow(wm_ctx* ctx, void** buf, size_t* have, size_t bytes, const char* what);
// wmhip.hip: the checks every entry point over a batch of strided planes starts with (makes the context's device current)
int check_plane_args(const wm_ctx* ctx, const void* p, int n_planes, int H, int W, int row_stride, size_t plane_stride);
// wmhip.hip: the embed fed with a sigma_w derived from the cover - the masked embed, and the payload embed of wm_payload.hip.
// `pass(eff, black)` enqueues the caller's sigma pass (described at the definition)
int embed_derived_dev(wm_ctx* ctx, const uint8_t* host, uint8_t* stego, float* sigma_c, float* yw, int n_planes, int H, int W,
                      int row_stride, size_t plane_stride, float alpha, int K, const char* missing,
                      const std::function<int(float*, uint8_t*)>& pass);
// arrays carved out of such a buffer, each on a 256-byte line.  base == nullptr is the sizing pass: the same takes return
// nullptr and pad256(off) is what the buffer must hold
struct Carve {
  char* base; size_t off;
  template <typename T> T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
  // The copies of a host-pointer entry point, stated with its layout (staged_call): `up` is enqueued on the spot, `down`
  // is kept until the _dev call is enqueued.  Neither does anything on the sizing pass or for 0 elements, so the host
  // pointer of an array without an element may be NULL.  in / out: a take that is uploaded from / downloaded to `host`.
  hipStream_t stream = nullptr;     // set on the pass that copies
  hipError_t err = hipSuccess;      // first failed upload
  struct Down { void* host; const void* dev; size_t bytes; } downs[4] = {};      // (an entry point has at most 3)
  int n_down = 0;
  template <typename T> void up(T* dev, const T* host, size_t n) {
    if (stream && n && err == hipSuccess) err = hipMemcpyAsync(dev, host, n * sizeof(T), hipMemcpyHostToDevice, stream);
  }
  template <typename T> void down(T* host, const T* dev, size_t n) {
    if (stream && n) downs[n_down++] = Down{host, dev, n * sizeof(T)};
  }
  template <typename T> T* in(size_t n, const T* host) { T* p = take<T>(n); up(p, host, n); return p; }
  template <typename T> T* out(size_t n, T* host) { T* p = take<T>(n); down(host, (const T*)p, n); return p; }
};
inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }
// A layout stated once: `lay(Carve&)` sets the caller's pointers.  It runs on a null base for the size, the grow-only buffer
// (*buf, *have) grows to it, and it runs again on the buffer.  Every byte a kernel touches must be part of a take.
template <typename Lay>
int staged(wm_ctx* ctx, void** buf, size_t* have, const char* what, Lay&& lay) {
  Carve cv{nullptr, 0};
  lay(cv);
  WM_TRY(grow(ctx, buf, have, pad256(cv.off), what));
  cv = Carve{(char*)*buf, 0};
  lay(cv);
  return WM_OK;
}
// A host-pointer entry point stated once, behind its argument checks: `lay` is the layout of its arrays in the context's
// scratch buffer together with their copies (Carve::in / out / up / down), `dev` the _dev call between the uploads and
// the downloads.  Ends in wm_check_status, or with sync_only in a plain synchronise of the stream.
template <typename Lay, typename Dev>
int staged_call(wm_ctx* ctx, Lay&& lay, Dev&& dev, bool sync_only = false) {
  Carve cv{nullptr, 0};
  lay(cv);
  WM_TRY(grow(ctx, &ctx->scratch, &ctx->scratch_bytes, pad256(cv.off), "scratch"));
  cv = Carve{(char*)ctx->scratch, 0};
  cv.stream = ctx->stream;
  lay(cv);
  WM_HIP(cv.err);
  WM_TRY(dev());
  for (int i = 0; i < cv.n_down; ++i)
    WM_HIP(hipMemcpyAsync(cv.downs[i].host, cv.downs[i].dev, cv.downs[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (!sync_only) return wm_check_status(ctx);
  WM_HIP(hipStreamSynchronize(ctx->stream));
  return WM_OK;
}
// elements from the first sample of the first plane to the last sample of the last one
inline size_t plane_span(int n_planes, int H, int row_stride, size_t plane_stride, int W) {
  if (n_planes == 0 || H == 0) return 0;
  return (size_t)(n_planes - 1) * plane_stride + (size_t)(H - 1) * row_stride + (size_t)W;
}
// The round trip of the plain, the masked and the payload embed.  `rule` is the per-tile input of the form (sigma_w, or
// the payload's tile bits: n_rule elements), dev(d_host, d_rule, d_stego, d_sc, d_yw) its _dev call.  `more(cv)` stages
// what a form takes beside them (the payload's dither table) behind the shared arrays.
template <typename T, typename Dev, typename More>
int embed_round_trip(wm_ctx* ctx, const uint8_t* host, const T* rule, size_t n_rule, uint8_t* stego, float* sigma_c, float* yw,
                     int n_planes, int H, int W, int row_stride, size_t plane_stride, const Dev& dev, const More& more) {
  const size_t nt = (size_t)(H / 8) * (W / 8);
  const size_t span = plane_span(n_planes, H, row_stride, plane_stride, W);
  uint8_t *d_host, *d_stego; T* d_rule; float *d_sc, *d_yw;
  return staged_call(ctx, [&](Carve& cv) {
    d_host = cv.in(span, host);
    // bytes between rows / planes that belong to the caller must survive the round trip, so stego goes up first; in place,
    // host and stego are ONE device array (k_copy_border and in-place embedding rely on the equal pointers)
    d_stego = cv.take<uint8_t>(span);
    if (stego != host) cv.up(d_stego, stego, span);
    else d_stego = d_host;
    cv.down(stego, d_stego, span);
    d_rule = cv.in(n_rule, rule);
    d_sc = cv.out((size_t)n_planes * nt * 8, sigma_c);
    d_yw = yw ? cv.out((size_t)n_planes * H * W, yw) : nullptr;
    more(cv);
  }, [&] { return dev(d_host, d_rule, d_stego, d_sc, d_yw); });
}
template <typename T, typename Dev>
int embed_round_trip(wm_ctx* ctx, const uint8_t* host, const T* rule, size_t n_rule, uint8_t* stego, float* sigma_c, float* yw,
                     int n_planes, int H, int W, int row_stride, size_t plane_stride, const Dev& dev) {
  return embed_round_trip(ctx, host, rule, n_rule, stego, sigma_c, yw, n_planes, H, W, row_stride, plane_stride, dev, [](Carve&) {});
}
// runtime bools as template arguments: with_bools(f, a, b) calls f(std::bool_constant<a>{}, std::bool_constant<b>{})
template <typename F> void with_bools(F&& f) { f(); }
template <typename F, typename... Bs> void with_bools(F&& f, bool b, Bs... rest) {
  if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// wm_ref.hip: releases the host part of a two-level tournament table (wm_ctx::hier_host)
void hier_host_free(void* tab);
// wm_route.hip: routed unscramble + normalise; mm_ext != NULL: n_part_ext {min, max} pairs per plane already on the device
// (order-preserving uint form), include_zero: the value 0 also takes part in the min / max
int route_unpermute_normalize(wm_ctx* ctx, const float* src, const wm_route* r, uint8_t* dst, size_t n, int n_planes, int do_norm,
                              const unsigned* mm_ext, unsigned n_part_ext, int include_zero);

// ---- min-max normalise + clip + uint8 (single:221-222), shared by wm_pixel.hip and wm_route.hip ----
__device__ __forceinline__ unsigned f2ord(float f) {   // order-preserving float -> uint
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
// block-wide min / max of order-preserving uints (any block size up to 1024); ends in a barrier, every thread
// returns with the block's values
__device__ __forceinline__ void block_minmax(unsigned& lo, unsigned& hi) {
  __shared__ unsigned s_lo[16], s_hi[16];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_down(lo, o, 64)); hi = max(hi, __shfl_down(hi, o, 64)); }
  if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  const int nw = (blockDim.x + 63) >> 6;
  lo = s_lo[0]; hi = s_hi[0];
  for (int w = 1; w < nw; ++w) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
}
// cv2.normalize(x, None, 0, 255, NORM_MINMAX) followed by clip + truncate; do_norm == 0: clip + truncate only
struct NormQ {
  float lo, scale; int do_norm;
  __device__ NormQ(float lo_, float hi_, int dn) : lo(lo_), do_norm(dn) {
    const double range = (double)hi_ - (double)lo_;
    scale = (dn && range > 2.220446049250313e-16) ? (float)(255.0 / range) : 0.0f;
  }
  __device__ __forceinline__ unsigned operator()(float v) const {
    if (do_norm) v = (v - lo) * scale;
    return (unsigned)fminf(fmaxf(v, 0.0f), 255.0f);
  }
};
}  // namespace wmi
