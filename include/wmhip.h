/* wmhip.h - C ABI of the MI355X (gfx950) DCT-SVD watermark hot path.
 *
 * This is the drop-in boundary.  The reference
 * (Thitrongdan202/Digital-Watermarking-...-DCT-SVD) has no FFI seam: its hot
 * path is ~12 inline NumPy/OpenCV statements per branch inside
 * embed/extract/detect of app_dct_svd_single.py.  Each entry point below names
 * the reference statements (file:line, "single" = app_dct_svd_single.py,
 * "core" = dct_svd_core_secure.py) it replaces when those are applied to every
 * 8x8 tile of a plane ("tile-mode").  The binding a
 * maintainer would add on the reference side is a ctypes stub - see
 * INTEGRATION.md.
 *
 * Conventions
 *  - plain C, caller-owned buffers, nothing retained between calls;
 *  - every function returns an int status (WM_OK == 0); wm_last_error() gives
 *    the message for the calling thread;
 *  - a wm_ctx binds one device + one HIP stream; two contexts are independently
 *    usable from two threads;
 *  - *_dev entry points take DEVICE pointers, enqueue on the context's stream
 *    and return without synchronising; the un-suffixed ones take HOST pointers
 *    and do H2D + kernels + D2H + sync themselves;
 *  - planes are row-major uint8 (or float32) with `row_stride` in ELEMENTS
 *    between rows and `plane_stride` in ELEMENTS between planes; tiles are
 *    numbered t = ty * (W/8) + tx; per-tile arrays are tile-major:
 *    sigma[plane][t][8], U[plane][t][8][8] (row, col), Vt[plane][t][8][8].
 *  - rows/columns beyond the last full tile (H % 8, W % 8) are passed through
 *    unchanged by embed and written as 0 by extract/reconstruct.
 */
#ifndef WMHIP_H
#define WMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WM_OK 0
#define WM_ERR_BADARG 1   /* NULL pointer, non-positive size, K outside 0..8 ...      */
#define WM_ERR_HIP 2      /* a HIP runtime call failed; wm_last_error() has the text  */
#define WM_ERR_NOCONV 3   /* Jacobi hit its sweep bound (numpy: LinAlgError)          */
#define WM_ERR_NOMEM 4    /* device or host allocation failed                         */

#define WM_TILE 8
#define WM_ABI_VERSION 1

typedef struct wm_ctx wm_ctx;

/* ---- library / context ------------------------------------------------- */
int wm_abi_version(void);
const char* wm_last_error(void);
int wm_device_count(int* n_out);
/* stream == NULL: the context creates (and owns) a non-blocking stream.
 * Otherwise `stream` is a hipStream_t the caller owns (e.g. torch's current
 * stream handle) and all work is enqueued there. */
int wm_create(int device, void* stream, wm_ctx** ctx_out);
int wm_destroy(wm_ctx* ctx);
int wm_sync(wm_ctx* ctx);
/* Reads-and-clears the sticky kernel status word (synchronises the stream):
 * WM_OK or WM_ERR_NOCONV. */
int wm_check_status(wm_ctx* ctx);

/* device memory + copies for callers that do not bring their own allocator */
int wm_malloc(wm_ctx* ctx, size_t bytes, void** dptr_out);
int wm_free(wm_ctx* ctx, void* dptr);
int wm_memcpy_h2d(wm_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int wm_memcpy_d2h(wm_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int wm_memset(wm_ctx* ctx, void* dst_dev, int value, size_t bytes);
/* Copy kernel between device memory and pinned host memory that is mapped for the device (hipHostMalloc /
 * hipHostRegister; either direction), enqueued on the context's stream without synchronising: the explicit form of the
 * blit copy hipMemcpyAsync falls back to, for frame pipelines that keep one stream per PCIe direction busy.
 * n_workgroups <= 0: 64. */
int wm_copy_mapped_dev(wm_ctx* ctx, void* dst, const void* src, size_t bytes, int n_workgroups);

/* HIP-event timing on the context's stream (slot 0..63) */
int wm_event_record(wm_ctx* ctx, int slot);
int wm_event_elapsed_ms(wm_ctx* ctx, int slot_start, int slot_stop, float* ms_out);

/* ---- K1: fused tile-mode embed ------------------------------------------
 * Replaces, per 8x8 tile:  .astype(float32) (single:24,122) -> dct2
 * (single:32-33,172) -> np.linalg.svd (single:172) -> S_[:K] = Sc[:K] +
 * alpha*Sw[:K] (single:174-175) -> Uc @ diag(S_) @ Vct (single:176) -> idct2
 * (single:177) -> np.clip(.,0,255).astype(uint8) (single:27,145-147).
 *   host     [n_planes] uint8 planes (in)
 *   sigma_w  watermark singular values [.. n_tiles][8]; plane p reads
 *            sigma_w + p * sigma_w_plane_stride (0 => one set shared by all
 *            planes: the "watermark S computed once per video" shape)
 *   stego    [n_planes] uint8 planes (out; may alias host)
 *   sigma_c  [n_planes][n_tiles][8] host singular values "Sc" (out, for meta)
 *   yw       optional [n_planes][H][W] float32 unclipped stego (what gray-mode
 *            SSIM consumes, single:190); NULL to skip
 *   K        number of leading singular values perturbed, 0..8
 *            (reference: K = max(8, int(kfrac*8)) = 8). */
int wm_embed_tiles_u8_dev(wm_ctx* ctx, const uint8_t* host, const float* sigma_w,
                          uint8_t* stego, float* sigma_c, float* yw,
                          int n_planes, int H, int W, int row_stride, size_t plane_stride,
                          size_t sigma_w_plane_stride, float alpha, int K);
int wm_embed_tiles_u8(wm_ctx* ctx, const uint8_t* host, const float* sigma_w,
                      uint8_t* stego, float* sigma_c, float* yw,
                      int n_planes, int H, int W, int row_stride, size_t plane_stride,
                      size_t sigma_w_plane_stride, float alpha, int K);

/* ---- K2: singular values of every tile of a uint8 plane ------------------
 * Replaces  Cw = dct2(Y); _, S_cw, _ = np.linalg.svd(Cw)  (single:205,
 * 234-236, 297, 305-307) per tile.  sigma: [n_planes][n_tiles][8]. */
int wm_sigma_tiles_u8_dev(wm_ctx* ctx, const uint8_t* planes, float* sigma,
                          int n_planes, int H, int W, int row_stride, size_t plane_stride);
int wm_sigma_tiles_u8(wm_ctx* ctx, const uint8_t* planes, float* sigma,
                      int n_planes, int H, int W, int row_stride, size_t plane_stride);

/* ---- K3: full SVD of every tile of a float32 plane (watermark side) ------
 * Replaces  Wm = dct2(wy_s); Uw, Sw, Vwt = np.linalg.svd(Wm)  (single:173,
 * 131-134) per tile.  U, Vt: [n_planes][n_tiles][8][8]; S: [..][8]. */
int wm_svd_tiles_f32_dev(wm_ctx* ctx, const float* planes, float* U, float* S, float* Vt,
                         int n_planes, int H, int W, int row_stride, size_t plane_stride);
int wm_svd_tiles_f32(wm_ctx* ctx, const float* planes, float* U, float* S, float* Vt,
                     int n_planes, int H, int W, int row_stride, size_t plane_stride);

/* ---- K2+K4: fused tile-mode extract --------------------------------------
 * Replaces, per tile:  dct2 + svd of the stego (single:205) ->
 * Sw_hat = (S_cw - Sc) / max(alpha,1e-8); Sw_hat[K:] = 0 (single:212-213) ->
 * Uw @ diag(Sw_hat) @ Vwt (single:214) -> idct2 (single:218).
 *   sigma_c  [n_planes][n_tiles][8]
 *   Uw, Vwt  [..][n_tiles][8][8]; plane p reads tile index p * uv_plane_stride + t,
 *            uv_plane_stride in TILES: n_tiles (per plane) or 0 (shared by all planes)
 *   out      [n_planes][H][W] float32 scrambled-watermark estimate wy_s
 *            (dense, row stride W) - input of _unpermute (single:220). */
int wm_extract_tiles_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c,
                            const float* Uw, const float* Vwt, float* out,
                            int n_planes, int H, int W, int row_stride, size_t plane_stride,
                            size_t uv_plane_stride, float alpha, int K);

/* Per-watermark preparation for wm_extract_tiles_px_u8_dev: the orthonormal DCT moves into
 * the factors, idct2(Uw diag(s) Vwt) = (D^T Uw) diag(s) (Vwt D) per 8x8 tile:
 *   Ux = D^T Uw,  Vxt = Vwt D   (n_tiles matrices of 8x8 each; in place allowed).
 * No reference counterpart: single:214-218 recomputes the product and the IDCT per call. */
int wm_tile_factors_to_pixel_dev(wm_ctx* ctx, const float* Uw, const float* Vwt, float* Ux, float* Vxt,
                                 size_t n_tiles);

/* wm_extract_tiles_u8_dev with the factors already in the pixel domain (above): same
 * result up to float32 rounding, without the per-tile IDCT (frames of a clip share one
 * watermark, so the preparation is paid once). */
int wm_extract_tiles_px_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Ux,
                               const float* Vxt, float* out, int n_planes, int H, int W, int row_stride,
                               size_t plane_stride, size_t uv_plane_stride, float alpha, int K);
int wm_extract_tiles_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c,
                        const float* Uw, const float* Vwt, float* out,
                        int n_planes, int H, int W, int row_stride, size_t plane_stride,
                        size_t uv_plane_stride, float alpha, int K);

/* The same, returning the SUM over the n_planes estimates ([H][W] float32, planes added in
 * ascending order on the device): the frames of a clip carry one watermark and are averaged by
 * the video extract, so one plane instead of n_planes crosses PCIe. */
int wm_extract_tiles_sum_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                            const float* Vwt, float* out_sum, int n_planes, int H, int W, int row_stride,
                            size_t plane_stride, size_t uv_plane_stride, float alpha, int K);

/* ---- K4: Uw diag(sw_hat) Vwt + idct2 per tile (single:214-218) ----------- */
int wm_reconstruct_tiles_dev(wm_ctx* ctx, const float* Uw, const float* sw_hat, const float* Vwt,
                             float* out, int n_planes, int H, int W);
int wm_reconstruct_tiles(wm_ctx* ctx, const float* Uw, const float* sw_hat, const float* Vwt,
                         float* out, int n_planes, int H, int W);

/* ---- K2+K5: fused tile-mode detect ---------------------------------------
 * Replaces  svd of the stego (single:297) -> Sw_hat = (S_cw - Sc)/max(alpha,
 * 1e-8) over ALL singular values (single:300) -> _nc(Sw, Sw_hat)
 * (single:284-289, 301) with the vectors flattened over all tiles.
 *   scores   [n_planes] float64 normalised-correlation score per plane
 *            (device pointer for _dev).  The caller applies  score >= thresh
 *            and the 3-plane mean of colour mode (single:302, 317-318). */
int wm_detect_tiles_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c,
                           const float* sigma_w, double* scores,
                           int n_planes, int H, int W, int row_stride, size_t plane_stride,
                           size_t sigma_w_plane_stride, float alpha);
int wm_detect_tiles_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c,
                       const float* sigma_w, double* scores,
                       int n_planes, int H, int W, int row_stride, size_t plane_stride,
                       size_t sigma_w_plane_stride, float alpha);

/* ---- Tile mode with texture-masked strength ------------------------------
 * The rule ("Texture-masked strength"; part of the meta format).  For a tile with cover singular values
 * s_1 >= .. >= s_8 (float32, as written to sigma_c) and parameters lo, hi, cut:
 *   r = sqrt(s_2^2 + .. + s_8^2);  g = clamp((r - lo) / (hi - lo), 0, 1) in float32;  G = (1, g, g, g, g, g, g, g)
 *   embed    s'_i = s_i + alpha * G_i * sw_i for i < K, along the tile's own singular vectors.  A black tile (64 zeros)
 *            has none: it moves along the flat vector (U = V = I in the DCT domain, what np.linalg.svd returns for a zero
 *            matrix) and becomes the constant alpha * sw_1 / 8 (clipped, truncated; untouched for K = 0).  Its sigma_c is
 *            what the unmasked embed writes.
 *   carried  a tile is carried iff g >= cut
 *   extract  sw_hat_1 = (s~_1 - s_1) / max(alpha, 1e-8) for every tile; sw_hat_i = (s~_i - s_i) / (max(alpha, 1e-8) * g) for
 *            i >= 2 on carried tiles, 0 on the others; then sw_hat_i = 0 for i >= K
 *   detect   _nc (single:284-289) over the i = 1 values of all tiles and the i >= 2 values of carried tiles only
 * Parameters: 0 <= lo < hi, both finite, 0 < cut <= 1; anything else is WM_ERR_BADARG (checked by the _dev entry points,
 * which the host-pointer forms go through).  Rows and columns outside the tile
 * grid pass through as in the unmasked entry points, whose arguments the masked ones share. */

/* The rule's g and G o sigma_w per tile: K2 on the cover planes, then
 *   sigma_w_eff  [n_planes][n_tiles][8]  G o sigma_w (dense, also where sigma_w is shared: sigma_w_plane_stride 0)
 *   gain         [n_planes][n_tiles] g, or NULL to skip.
 * sigma_w and sigma_w_eff may both be NULL when only gain is wanted. */
int wm_mask_sigma_w_tiles_u8_dev(wm_ctx* ctx, const uint8_t* planes, const float* sigma_w, float* sigma_w_eff, float* gain,
                                 int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                 size_t sigma_w_plane_stride, float lo, float hi);
int wm_mask_sigma_w_tiles_u8(wm_ctx* ctx, const uint8_t* planes, const float* sigma_w, float* sigma_w_eff, float* gain,
                             int n_planes, int H, int W, int row_stride, size_t plane_stride,
                             size_t sigma_w_plane_stride, float lo, float hi);

/* The rule's embed: wm_mask_sigma_w_tiles_u8_dev into a buffer the context owns, then wm_embed_tiles_u8_dev with
 * G o sigma_w, then the black tiles redone along the flat vector (wm_embed_tiles_u8_dev itself gives a black tile the
 * vectors of a fixed pattern, as the reference's arbitrary ones; that entry point is unchanged).  sigma_c is the cover's,
 * as in the unmasked embed; stego may alias host. */
int wm_embed_tiles_masked_u8_dev(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego, float* sigma_c,
                                 float* yw, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                 size_t sigma_w_plane_stride, float alpha, int K, float lo, float hi);
int wm_embed_tiles_masked_u8(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego, float* sigma_c,
                             float* yw, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                             size_t sigma_w_plane_stride, float alpha, int K, float lo, float hi);

/* The rule's extract: wm_extract_tiles_u8_dev / _px_u8_dev / wm_extract_tiles_u8 / _sum_u8 with g taken from sigma_c inside
 * the kernel (the whole chain to uint8: wm_extract_unscrambled_masked_u8_dev, below). */
int wm_extract_tiles_masked_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                                   const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                                   size_t plane_stride, size_t uv_plane_stride, float alpha, int K,
                                   float lo, float hi, float cut);
int wm_extract_tiles_px_masked_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Ux,
                                      const float* Vxt, float* out, int n_planes, int H, int W, int row_stride,
                                      size_t plane_stride, size_t uv_plane_stride, float alpha, int K,
                                      float lo, float hi, float cut);
int wm_extract_tiles_masked_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                               const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                               size_t plane_stride, size_t uv_plane_stride, float alpha, int K,
                               float lo, float hi, float cut);
int wm_extract_tiles_sum_masked_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                                   const float* Vwt, float* out_sum, int n_planes, int H, int W, int row_stride,
                                   size_t plane_stride, size_t uv_plane_stride, float alpha, int K,
                                   float lo, float hi, float cut);

/* The rule's detect: wm_detect_tiles_u8[_dev] over the values the rule takes; their number is counted on the device. */
int wm_detect_tiles_masked_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                                  double* scores, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                  size_t sigma_w_plane_stride, float alpha, float lo, float hi, float cut);
int wm_detect_tiles_masked_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                              double* scores, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                              size_t sigma_w_plane_stride, float alpha, float lo, float hi, float cut);

/* ---- Tile mode, blind payload: one bit per tile in the parity of sigma_1 --
 * The rule ("Blind payload"; part of the meta format).  Parameter: delta, float32, finite, 8 <= delta <= 512.
 * The bias c = 4 is a constant (the embed truncates to uint8, which lowers sigma_1 of a tile by 64 * 0.5 / 8 on average).
 * embed   a tile carries bit b; its cover singular values are s_1 >= s_2 >= .. (float32, as K2 writes them):
 *           q = fma(2 delta, rint((s_1 - b delta) / (2 delta)), b delta)    nearest point of {2 k delta + b delta}, float32,
 *                                                                          ties to even as rintf, one fused multiply-add
 *           if q + c > 2040: q -= 2 delta                                  2040 = 8 * 255: never aim above a white tile
 *           up to 3 times: if q < s_2 + delta: q += 2 delta                sigma_1 stays the leading value
 *           sigma_w_eff = (q + c - s_1, 0, 0, 0, 0, 0, 0, 0), then the unchanged embed with alpha = 1, K = 1
 *         A black cover tile (64 zeros) has no leading singular vector; the payload embed gives it the flat one, as
 *         np.linalg.svd does for a zero matrix: the tile becomes the constant (q + c) / 8.
 * decode  with s~_1 the leading singular value of the stego tile:
 *           x = s~_1 * (1 / (2 delta))    one float32 multiply by the float32 reciprocal
 *           f = x - floor(x);  m = 2 |2 f - 1| - 1          +1 on a bit-0 lattice point, -1 on a bit-1 point
 *         soft[j] = sum of m over all planes and all tiles mapped to bit j, in float64 and in a fixed order (no
 *         atomics: two calls give the same bits); the decoded bit is soft[j] < 0.
 * The tile-to-bit map is the caller's (the Python side: tile t carries bit perm[t] % n_bits of a keyed permutation of the
 * tiles); all planes of a call share it.  Tiles pinned by clipping (a 0/255 checkerboard ..) do not take their bit:
 * repetition over tiles and frames is what covers them.  Rows and columns outside the tile grid pass through.
 * WM_ERR_BADARG: delta outside the range or not finite, n_bits < 1 or > n_tiles, NULL pointers, and in the host-pointer
 * form offs[0] != 0, offs[n_bits] != n_tiles, a decreasing offs or an order entry outside the grid.  Empty inputs
 * (no planes, no tiles) return WM_OK without a launch. */

/* K2 on the cover planes, then the rule's sigma_w rows:
 *   tile_bit     [n_tiles] uint8, the bit (0 / 1) each tile carries, shared by the planes
 *   sigma_w_eff  [n_planes][n_tiles][8] float32 (out) */
int wm_payload_sigma_w_tiles_u8_dev(wm_ctx* ctx, const uint8_t* planes, const uint8_t* tile_bit, float* sigma_w_eff,
                                    int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta);
int wm_payload_sigma_w_tiles_u8(wm_ctx* ctx, const uint8_t* planes, const uint8_t* tile_bit, float* sigma_w_eff,
                                int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta);

/* The rule's embed: the pass above into a buffer the context owns, then wm_embed_tiles_u8_dev with a per-plane
 * sigma_w stride, alpha = 1 and K = 1.  sigma_c (the cover's, out) and yw as in wm_embed_tiles_u8_dev; stego may alias host. */
int wm_embed_tiles_payload_u8_dev(wm_ctx* ctx, const uint8_t* host, const uint8_t* tile_bit, uint8_t* stego, float* sigma_c,
                                  float* yw, int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta);
int wm_embed_tiles_payload_u8(wm_ctx* ctx, const uint8_t* host, const uint8_t* tile_bit, uint8_t* stego, float* sigma_c,
                              float* yw, int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta);

/* K2 on the stego planes, then m of every tile:  metric [n_planes][n_tiles] float32 (out) */
int wm_payload_metric_tiles_u8_dev(wm_ctx* ctx, const uint8_t* stego, float* metric, int n_planes, int H, int W,
                                   int row_stride, size_t plane_stride, float delta);
int wm_payload_metric_tiles_u8(wm_ctx* ctx, const uint8_t* stego, float* metric, int n_planes, int H, int W,
                               int row_stride, size_t plane_stride, float delta);

/* The rule's decode: the metric into a buffer the context owns, then one wave per bit.
 *   order  [n_tiles] int32, the tiles grouped by the bit they carry, ascending tile index within a bit
 *   offs   [n_bits + 1] int32, bit j owns order[offs[j] .. offs[j + 1])   (the CSR inverse of the tile-to-bit map)
 *   soft   [n_bits] float64 (out) */
int wm_payload_soft_tiles_u8_dev(wm_ctx* ctx, const uint8_t* stego, const int32_t* order, const int32_t* offs, int n_bits,
                                 double* soft, int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta);
int wm_payload_soft_tiles_u8(wm_ctx* ctx, const uint8_t* stego, const int32_t* order, const int32_t* offs, int n_bits,
                             double* soft, int n_planes, int H, int W, int row_stride, size_t plane_stride, float delta);

/* ---- Blind payload with keyed dither: every tile's lattice shifted by a secret offset --
 * The rule above puts sigma_1 of every marked tile on the public lattice {k delta}; the forms below shift the lattice of
 * each tile by an offset from a 16-bit dither word u that the caller derives from the key (the Python side:
 * payload.dither_table).  Without the table, sigma_1 mod 2 delta of the stego looks uniform; with it nothing is lost.
 *   offset  d = float(u) * (delta * 2^-15)     ONE float32 multiply, rounded on its own (never contracted into the add or
 *                                              the subtraction that follows); delta * 2^-15 is exact; 0 <= d < 2 delta
 *   embed   b' = b delta + d                   one float32 add
 *           q = fma(2 delta, rint((s_1 - b') / (2 delta)), b')
 *           then as above: the step down from 2040, the climb above s_2 + delta, sigma_w_eff = (q + c - s_1, 0, ..), the
 *           unchanged embed with alpha = 1, K = 1, the flat vector for black tiles
 *   decode  x = (s~_1 - d) * (1 / (2 delta));  f and m as above
 * u = 0 gives the dither-free results bit for bit.
 *   tile_dither          uint16, tile t of plane p reads tile_dither[p * dither_plane_stride + t]
 *   dither_plane_stride  0: one [n_tiles] table shared by the planes; >= n_tiles: one table per plane, that many words apart
 *                        (as sigma_w_plane_stride); the host-pointer forms read (n_planes - 1) * stride + n_tiles words
 * The other arguments are those of the dither-free forms.  WM_ERR_BADARG as there, and for a NULL (or odd-addressed) table
 * or a stride that is neither 0 nor >= n_tiles where there is a tile to work on.  Empty inputs return WM_OK without a
 * launch. */
int wm_payload_sigma_w_tiles_dither_u8_dev(wm_ctx* ctx, const uint8_t* planes, const uint8_t* tile_bit, const uint16_t* tile_dither,
                                           float* sigma_w_eff, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                           size_t dither_plane_stride, float delta);
int wm_payload_sigma_w_tiles_dither_u8(wm_ctx* ctx, const uint8_t* planes, const uint8_t* tile_bit, const uint16_t* tile_dither,
                                       float* sigma_w_eff, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                       size_t dither_plane_stride, float delta);
int wm_embed_tiles_payload_dither_u8_dev(wm_ctx* ctx, const uint8_t* host, const uint8_t* tile_bit, const uint16_t* tile_dither,
                                         uint8_t* stego, float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                                         size_t plane_stride, size_t dither_plane_stride, float delta);
int wm_embed_tiles_payload_dither_u8(wm_ctx* ctx, const uint8_t* host, const uint8_t* tile_bit, const uint16_t* tile_dither,
                                     uint8_t* stego, float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                                     size_t plane_stride, size_t dither_plane_stride, float delta);
int wm_payload_metric_tiles_dither_u8_dev(wm_ctx* ctx, const uint8_t* stego, const uint16_t* tile_dither, float* metric,
                                          int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                          size_t dither_plane_stride, float delta);
int wm_payload_metric_tiles_dither_u8(wm_ctx* ctx, const uint8_t* stego, const uint16_t* tile_dither, float* metric, int n_planes,
                                      int H, int W, int row_stride, size_t plane_stride, size_t dither_plane_stride, float delta);
int wm_payload_soft_tiles_dither_u8_dev(wm_ctx* ctx, const uint8_t* stego, const uint16_t* tile_dither, const int32_t* order,
                                        const int32_t* offs, int n_bits, double* soft, int n_planes, int H, int W, int row_stride,
                                        size_t plane_stride, size_t dither_plane_stride, float delta);
int wm_payload_soft_tiles_dither_u8(wm_ctx* ctx, const uint8_t* stego, const uint16_t* tile_dither, const int32_t* order,
                                    const int32_t* offs, int n_bits, double* soft, int n_planes, int H, int W, int row_stride,
                                    size_t plane_stride, size_t dither_plane_stride, float delta);

/* ---- Blind payload, crop resynchronisation: where the embed's tile grid lies in a cropped stego --
 * A crop alters no pixel that survives it: every whole tile left in an h x w crop (h <= H, w <= W, origin anywhere) still
 * sits on its lattice point.  What is lost is where the grid is.  The rule ("Crop resynchronisation"; dither-free
 * payloads only).  All arithmetic past the metric is integer: the device and a NumPy restatement agree to the bit.
 *   1 vote    vote = (int32) rintf(m * 32768.0f), m the metric of the window's sigma_1 as above: -32768 .. 32768
 *   2 phase   for p = 8 py + px, py, px in 0..7: the windows start at (py + 8 r, px + 8 c), r < ny_p = (h - py) / 8,
 *             c < nx_p = (w - px) / 8;  sum_p = sum of |vote| (int64), count_p = ny_p nx_p.  The winner is the phase with the
 *             largest sum_p / count_p, compared exactly (cross-multiplied integers, on the host); ties go to the smallest p;
 *             phases with count 0 do not take part.  Needs no key.
 *   3 offset  on the winner's votes V[ny][nx] and the tile-to-bit map T[nby][nbx] of the ORIGINAL grid (tile t carries bit
 *             T[t]): every placement 0 <= ty <= nby - ny, 0 <= tx <= nbx - nx has hist[j] = sum of V[r][c] over the windows with
 *             T[ty + r][tx + c] == j (int32) and score = sum over j of |hist[j]| (int64).  The winner is the largest score,
 *             ties to the smallest (ty, tx).  ny > nby or nx > nbx: there is no placement.
 *   4 decode  soft[j] = hist[j] / 32768 at the winner (float64, on the host), the bits as above; the crop's origin in the
 *             marked image is (8 ty - py, 8 tx - px).
 * Only the top phase and the top placement are tried; whether they are right is what the frame's length header and CRC say. */

/* Step 1 and the sums of step 2, all 64 phases of every plane in one launch (rows / columns: h, w of the crop):
 *   votes  [n_planes][64][(h / 8) (w / 8)] int32 (out): phase p's own ny_p x nx_p grid, row-major, at the start of its slot,
 *          the rest of the slot untouched; NULL to skip
 *   sums   [n_planes][64] int64 (out): sum_p; zeroed and accumulated by integer atomics, one per wave
 * WM_ERR_BADARG: delta as above, sums NULL.  No plane or no whole tile (h < 8 or w < 8): WM_OK without a launch, nothing
 * written. */
int wm_payload_phase_scan_u8_dev(wm_ctx* ctx, const uint8_t* stego, int32_t* votes, int64_t* sums, int n_planes, int h, int w,
                                 int row_stride, size_t plane_stride, float delta);
int wm_payload_phase_scan_u8(wm_ctx* ctx, const uint8_t* stego, int32_t* votes, int64_t* sums, int n_planes, int h, int w,
                             int row_stride, size_t plane_stride, float delta);

/* Step 3, one workgroup per placement:
 *   votes           [ny][nx] int32, one phase's grid as the phase scan wrote it
 *   tile_bit_index  [nby][nbx] int32; an entry outside 0 .. n_bits - 1 is skipped (the device does not trust the map)
 *   scores          [nby - ny + 1][nbx - nx + 1] int64 (out)
 * hist is int32 and wraps like any int32 sum, on the device as in NumPy (|vote| <= 2^15: no wrap below 2^16 tiles a bit).
 * WM_ERR_BADARG: n_bits < 1 or > 16384 (hist lives in 64 KiB of LDS), negative sizes, NULL pointers.  No placement: WM_OK
 * without a launch, nothing written; no window (ny or nx 0): every score 0, without a launch. */
int wm_payload_offset_scores_dev(wm_ctx* ctx, const int32_t* votes, const int32_t* tile_bit_index, int64_t* scores, int ny, int nx,
                                 int nby, int nbx, int n_bits);
int wm_payload_offset_scores(wm_ctx* ctx, const int32_t* votes, const int32_t* tile_bit_index, int64_t* scores, int ny, int nx,
                             int nby, int nbx, int n_bits);

/* ---- Blind payload, keyed crop resynchronisation: the same for a payload embedded with keyed dither --
 * Keyed dither leaves the keyless phase scan nothing to find: read without the tile's dither word, (sigma_1 - d) mod 2 delta
 * is uniform at every phase.  Read with the RIGHT word a marked tile sits on its lattice point whatever bit it carries, so
 * one keyed score finds phase and placement together.  The rule ("Keyed crop resynchronisation"); all arithmetic
 * past the metric is integer.
 *   1 scan    phases and windows as in step 2 above; s1[p][r][c] = sigma_1 of the window, float32.  Needs no key.
 *   2 scores  U[nby][nbx] is the embed's dither table.  For every phase p with ny_p nx_p > 0 and every placement
 *             0 <= ty <= nby - ny_p, 0 <= tx <= nbx - nx_p:  d = float(U[ty + r][tx + c]) * (delta * 2^-15), m the metric of
 *             s1[p][r][c] on the lattice shifted by d (x = (s1 - d) * (1 / (2 delta))), vote as above, and
 *             score[p][ty][tx] = sum over the windows of |vote| (int64).
 *   3 winner  the largest score[p][ty][tx] / (ny_p nx_p), compared exactly: within a phase the first maximum in row-major
 *             order, across phases cross-multiplied integers (on the host); ties go to the smallest (p, ty, tx).
 *   4 decode  the votes of the winner's s1 grid under U[ty + r][tx + c] (on the host), soft[j] their sums per bit of the
 *             tile-to-bit map's window as in step 4 above; origin = (8 ty - py, 8 tx - px).
 * Only the top candidate is tried; the frame's length header and CRC say whether it was right.  There is no limit on the
 * payload's bits: nothing here scales with them. */

/* Step 1, all 64 phases of every plane in one launch:
 *   s1  [n_planes][64][(h / 8) (w / 8)] float32 (out): phase p's own ny_p x nx_p grid, row-major, at the start of its slot, the
 *       rest of the slot untouched
 * WM_ERR_BADARG: s1 NULL.  No plane or no whole tile: WM_OK without a launch, nothing written. */
int wm_payload_sigma1_scan_u8_dev(wm_ctx* ctx, const uint8_t* stego, float* s1, int n_planes, int h, int w, int row_stride,
                                  size_t plane_stride);
int wm_payload_sigma1_scan_u8(wm_ctx* ctx, const uint8_t* stego, float* s1, int n_planes, int h, int w, int row_stride,
                              size_t plane_stride);

/* Step 2, every phase and placement in one launch:
 *   s1           one plane's scan, [64][(h / 8) (w / 8)] float32
 *   tile_dither  [nby][nbx] uint16, the embed's table
 *   scores       [64][spitch] int64 (out), spitch = (nby - max(h - 7, 0) / 8 + 1) * (nbx - max(w - 7, 0) / 8 + 1): phase p's own
 *                (nby - ny_p + 1) x (nbx - nx_p + 1) grid, row-major, at the start of its slot.  The whole array is zeroed
 *                first; a phase without a window writes nothing.
 * WM_ERR_BADARG: h / 8 > nby or w / 8 > nbx (not a crop of that grid), h or w < 8, tile_dither NULL or at an odd address,
 * delta outside 8..512, s1 or scores NULL, nbx above 65535 or spitch above 2^24.  Two lane mappings (a lane per placement; a
 * lane per window of a row where a crop has few placements across) give the same bits: the sums are integers. */
int wm_payload_keyed_scores_dev(wm_ctx* ctx, const float* s1, const uint16_t* tile_dither, int64_t* scores, int h, int w, int nby,
                                int nbx, float delta);
int wm_payload_keyed_scores(wm_ctx* ctx, const float* s1, const uint16_t* tile_dither, int64_t* scores, int h, int w, int nby,
                            int nbx, float delta);

/* ---- Blind payload, clip resynchronisation: a dithered video's clip, cut in time and cropped in space --
 * Every marked frame of a video has a dither table keyed by its index in the file, so a clip that lost leading frames (or
 * columns) reads every tile on the wrong lattice.  No surviving pixel is damaged: the keyed score above finds grid phase
 * and placement, and summed over several clip frames it finds the first frame as well - and with more windows behind every
 * candidate it resolves crops the single-plane search cannot.  The rule ("Clip resynchronisation"); all
 * arithmetic past the metric is integer.
 *   inputs   the clip is n_c luma frames of h x w; the meta holds shape (H, W), n_frames F, frame_interval fi, delta and
 *            dither = 1.  Clip frame i is file frame t0 + i.  Unknown: t0 in 0 .. F - n_c, the phase p = 8 py + px and the
 *            placement (ty, tx).
 *   1 scan    step 1 above on the first A = min(n_c, anchors fi) clip frames, the anchors.
 *   2 tables  tables[k] = the dither table of file frame k fi, for the marked frames k < ceil(F / fi).  Candidate g = t0
 *             pairs anchor a with table (t0 + a) / fi where (t0 + a) % fi == 0 and with none (-1) otherwise:
 *             table_of[n_cand][A], int32, host work.  The device knows nothing of frame intervals.
 *   3 scores  score[g][p][ty][tx] = sum over the anchors a with table_of[g][a] >= 0 of step 2's score of anchor a's scan
 *             under tables[table_of[g][a]] (int64).  Only best[g][p] = (the largest score of the phase, the row-major index
 *             ty n_tx_p + tx of its FIRST maximum) leaves the device; a phase without a window and a candidate without a
 *             marked anchor give (-1, -1).
 *   4 winner  the largest score / (ny_p nx_p m_g), m_g the candidate's marked anchors, compared by cross-multiplied
 *             integers (on the host); ties go to the smallest (g, p, index); entries of -1 do not take part.
 *   5 decode  every clip frame i with (t0 + i) % fi == 0: the metric of the view [py : py + 8 ny, px : px + 8 nx] under the
 *             rows [ty : ty + ny, tx : tx + nx] of the table of file frame t0 + i, vote = rint(m 32768), the frames' votes
 *             added (int64), soft[j] their sums per bit of the tile-to-bit map's window as in step 4 above;
 *             origin = (8 ty - py, 8 tx - px), first_frame = t0.
 * Only the top candidate is tried; the frame's length header and CRC say whether it was right.
 *
 * Step 3 in one call:
 *   s1        the anchors' scans, [n_anchor][64][(h / 8) (w / 8)] float32 (wm_payload_sigma1_scan_u8 of n_anchor planes)
 *   tables    [n_tables][nby nbx] uint16
 *   table_of  [n_cand][n_anchor] int32, -1 = skip the anchor
 *   best      [n_cand][64][2] int64 (out): (score, index) per candidate and phase
 * WM_ERR_BADARG: everything wm_payload_keyed_scores_dev refuses; n_anchor, n_tables or n_cand < 1; (h / 8) (w / 8) n_anchor
 * >= 2^24 (a score stays below 2^39: the reduction packs score 2^24 + (2^24 - 1 - index) into one int64, and the 2^24
 * placements a phase bound the index); s1, tables, table_of or best NULL or misaligned (the _dev form); a table_of entry
 * < -1 or >= n_tables (the host form, which reads it; the _dev form cannot, and its kernel skips an entry outside
 * 0 .. n_tables - 1 as it skips -1).  The reduction is a wave-level integer max and one 64-bit integer atomic max per wave:
 * the keys of a (candidate, phase) are distinct, so the result does not depend on the order of arrival.  The two lane
 * mappings of wm_payload_keyed_scores_dev, chosen by its rule, give the same bits. */
int wm_payload_keyed_best_dev(wm_ctx* ctx, const float* s1, int n_anchor, const uint16_t* tables, int n_tables, const int32_t* table_of,
                              int n_cand, int64_t* best, int h, int w, int nby, int nbx, float delta);
int wm_payload_keyed_best(wm_ctx* ctx, const float* s1, int n_anchor, const uint16_t* tables, int n_tables, const int32_t* table_of,
                          int n_cand, int64_t* best, int h, int w, int nby, int nbx, float delta);

/* ---- Blind payload, frame resynchronisation: a dithered video with frames dropped, repeated, reordered or mixed in --
 * The clip search pairs clip frame i with file frame t0 + i, so a frame-rate conversion, a splice, a reversed reel or a title
 * card in the middle loses the payload although every surviving pixel still sits on its lattice point.  At a known grid
 * phase and place a marked frame only has to be told apart from the other TABLES, and it names its own by a wide gap; a
 * frame that carries nothing has no table that stands out.  The rule ("Frame resynchronisation"); all arithmetic
 * past the metric is integer.
 *   inputs    the file is n_c luma frames of h x w, every one cropped to the same rectangle, in any order; the meta holds
 *             (H, W), F = n_frames, fi = frame_interval, delta and dither = 1.  K = ceil(F / fi) and tables[k] = the dither
 *             table of file frame k fi.
 *   1 geometry  the first A = min(n_c, anchors fi) frames are tried in file order, each ALONE through the clip search above:
 *             one anchor, candidate g = table g (table_of = arange(K)[:, None]).  The winner of its `best` is step 4 above
 *             with m_g = 1.  The anchor is accepted when its winner leads every other (candidate, phase) entry of `best` by
 *             the bar of step 3: 10 (s_w n_e - s_e n_w) >= 32768 n_w n_e for the winner's (score, windows) = (s_w, n_w) and
 *             every other entry's (s_e, n_e), in exact integers.  The first accepted anchor fixes (py, px), (ty, tx),
 *             ny = (h - py) / 8 and nx = (w - px) / 8 for every frame.  No accepted anchor: the empty result.
 *   2 scores  s1[f][r][c] = sigma_1 of the window at (py + 8 r, px + 8 c) of frame f (wm_sigma_tiles_u8 of the view
 *             [py : py + 8 ny, px : px + 8 nx], element 0 of a tile's 8), and for every table k
 *             score[f][k] = sum over r < ny, c < nx of |vote| of s1[f][r][c] on the lattice of tables[k][ty + r][tx + c]
 *             (step 2 of the keyed search), int64: wm_payload_frame_scores below.
 *   3 assign  n_win = ny nx.  For frame f: k* the FIRST maximum of its row; second = max(the largest score among the other
 *             tables, 16384 n_win) - the floor is the score of a uniform phase, so K = 1 follows the same rule.  The frame is
 *             accepted when 10 (score[f][k*] - second) >= 32768 n_win (a tenth of full scale); frame_map[f] = k* fi if
 *             accepted, else -1.  Several frames may name one table; all of them vote.  Host work.
 *   4 decode  every accepted frame's votes of its s1 under tables[k*][ty : ty + ny, tx : tx + nx], added (int64), then as
 *             step 5 above with the accepted frames as the multiplicity; origin = (8 ty - py, 8 tx - px).  No accepted
 *             frame: the empty result.
 *
 * Step 2 in one call:
 *   s1      frame f's window i = r nx + c at s1[f * s1_frame_stride + i * s1_window_stride] (strides in floats): window
 *           stride 8 reads the output of wm_sigma_tiles_u8_dev in place, 1 a dense grid
 *   tables  [n_tables][nby nbx] uint16
 *   scores  [n_frames][n_tables] int64 (out), zeroed first
 * WM_ERR_BADARG, before anything is written: a NULL pointer; tables at an odd address; s1 or scores not aligned to its
 * element; n_frames, n_tables, ny or nx < 1 (or n_frames, n_tables above 2^24); ty < 0, tx < 0, ty + ny > nby or
 * tx + nx > nbx; nby nbx above 2^30; s1_window_stride 0; delta outside 8..512.  The sums are integers and leave by 64-bit
 * integer atomic adds: the same inputs give the same bits. */
int wm_payload_frame_scores_dev(wm_ctx* ctx, const float* s1, size_t s1_window_stride, size_t s1_frame_stride, int n_frames,
                                const uint16_t* tables, int n_tables, int64_t* scores, int ny, int nx, int nby, int nbx, int ty, int tx,
                                float delta);
int wm_payload_frame_scores(wm_ctx* ctx, const float* s1, size_t s1_window_stride, size_t s1_frame_stride, int n_frames,
                            const uint16_t* tables, int n_tables, int64_t* scores, int ny, int nx, int nby, int nbx, int ty, int tx,
                            float delta);

/* --------------------------------------------------------------------------
 * Channel code of the blind payload (optional; the meta's ``code`` member = 1): the industry-standard rate-1/2 convolutional
 * code of constraint length 7, generators 171 and 133 octal, with a zero tail, decoded by a soft-decision Viterbi decoder on
 * the device.  Part of the meta format like the rule and the dither table; DESIGN.md section 14, "Channel code".
 *
 * Info bits.  u[0 .. n_info) is the payload's frame (length header, bytes, CRC: the bits embedded without a code), followed
 *   by 6 zero tail bits: n_steps = n_info + 6.
 * Encoder (host work).  A 7-bit register r starts at 0; step t shifts u[t] in: r = ((r << 1) | u[t]) & 127, and puts out
 *   coded[2 t] = parity(r & 0171), coded[2 t + 1] = parity(r & 0133).  n_coded = 2 n_steps.
 * Map.  The keyed tile-to-bit map over n_coded bits: tile t carries coded[perm[t] % n_coded].  It is the interleaver.
 *   n_coded <= n_tiles.
 * Soft input (host work).  soft[j], the float64 sum of the votes of coded bit j (positive: a 0), is quantised to an integer
 *   L[j] = clip(rint(soft[j] * (1024 / peak)), -1024, 1024), peak = max |soft| (1 where that is 0), in float64, rint to even.
 *   A coded bit without a tile (a crop) has soft = 0 and L = 0: an erasure.
 * Decoder.  Integers from here on.  The decoder clamps L to -1024 .. 1024 again on load (part of the rule: any int32 is a
 *   valid input).  State s = r & 63; path metrics pm[0] = 0, pm[s != 0] = -2^30.  Step t, for every new state s': the
 *   predecessors are p_b = (s' >> 1) | (b << 5), b = 0, 1, their registers r_b = s' | (b << 6),
 *     bm_b = (1 - 2 parity(r_b & 0171)) L[2 t] + (1 - 2 parity(r_b & 0133)) L[2 t + 1]        (bm_1 = -bm_0: both generators
 *     c_b  = pm[p_b] + bm_b                                                                     hold bits 0 and 6)
 *   the new pm[s'] is the larger candidate, b = 1 iff c_1 > c_0 (a tie goes to b = 0), and bit s' of the 64-bit decision
 *   word D[t] is that b.  Traceback: s = 0 at t = n_steps - 1, going down: u[t] = s & 1, b = (D[t] >> s) & 1,
 *   s = (s >> 1) | (b << 5).  The info bits are u[0 .. n_info); the final metric is pm[0] after the last step.
 * Limit.  n_steps <= 2^18: every metric then stays inside (-2^30 - 2^29, 2^29] and nothing is normalised.
 *
 *   llr           [n_codewords] rows of 2 n_steps int32, row c at llr + c * llr_stride (elements)
 *   info_bits     [n_codewords][n_info] uint8 (out), 0 or 1
 *   final_metric  [n_codewords] int32 (out), may be NULL
 *   decisions     [n_codewords][n_steps] uint64 (out), may be NULL: the context then keeps the words in a buffer of its own
 *                 (8 n_steps bytes a codeword, at most 2 MiB)
 * One wave per codeword, one launch: the forward pass and the traceback.  WM_ERR_BADARG, before any launch: n_info < 1,
 * n_steps > 2^18, n_codewords < 1, llr_stride < 2 n_steps, llr or info_bits NULL (device form: a misaligned pointer). */
int wm_payload_decode_k7_dev(wm_ctx* ctx, const int32_t* llr, int n_info, int n_codewords, size_t llr_stride, uint8_t* info_bits,
                             int32_t* final_metric, uint64_t* decisions);
int wm_payload_decode_k7(wm_ctx* ctx, const int32_t* llr, int n_info, int n_codewords, size_t llr_stride, uint8_t* info_bits,
                         int32_t* final_metric, uint64_t* decisions);

/* ---- Blind payload, resize resynchronisation: a stego that was resized as a whole --
 * sigma_1 of an 8x8 tile is dominated by 8 x the tile's mean, and a smooth resize followed by a smooth resize back to the
 * marked size moves that mean very little.  The meta holds the marked shape (H, W), so a whole-frame resize needs no
 * search: the stego's luma is resampled back to H x W by the filter below and decoded as an unresized one (DESIGN.md,
 * "Resize resynchronisation").  The filter is separable and integer, so the device and a NumPy restatement agree to the bit.
 * The horizontal pass runs first, into a uint8 intermediate [h_in][w_out]; then the vertical pass.  Each pass rounds to uint8.
 *
 * Taps of one axis, n_in -> n_out samples, float64 on the host (resample.py: resample_taps):
 *   scale = n_in / n_out;  fs = max(scale, 1);  sup = 2 fs;  T = 2 ceil(sup) + 1        (5 when enlarging, at most 33)
 *   output i:  c = (i + 0.5) scale;  lo = max(0, int(c - sup + 0.5));  hi = min(n_in, int(c + sup + 0.5))
 *              f_k = cubic((k + 0.5 - c) / fs) for k in [lo, hi), cubic the Catmull-Rom kernel with a = -0.5:
 *                ((a + 2) |x| - (a + 3)) x^2 + 1 for |x| < 1,  a (((|x| - 5) |x| + 8) |x| - 4) for 1 <= |x| < 2,  0 otherwise
 *              the f_k normalised to sum 1;  iw_k = rint(f_k 2^14);  the residue 2^14 - sum iw is added to the largest tap,
 *              the first of equals: a constant row stays constant to the byte
 *   first[i] = lo;  w[i][0 .. hi - lo) = iw, the rest of the row of T is 0
 * A pixel:  acc = sum over t < T of w[i][t] * px[min(first[i] + t, n_in - 1)]  in int32 (|acc| < 2^23)
 *           out = clip((acc + 2^13) >> 14, 0, 255)  with an arithmetic (floor) shift
 * n_in == n_out gives w = 2^14 at the centre: the pass is the identity.  Neither axis may change by more than 8x.
 *
 *   src      [n_planes] uint8 planes [h_in][w_in], src_row_stride / src_plane_stride in elements
 *   dst      [n_planes] uint8 planes [h_out][w_out] (out), dst_row_stride / dst_plane_stride in elements; never in place
 *   first_x  [w_out] int32, w_x [w_out][T_x] int16: the horizontal taps (w_in -> w_out)
 *   first_y  [h_out] int32, w_y [h_out][T_y] int16: the vertical taps (h_in -> h_out)
 * The intermediate lives in a buffer the context owns.  An index first[i] + t outside the source reads its last sample: the
 * device does not trust the tables.  n_planes == 0 returns WM_OK without a launch.  WM_ERR_BADARG, before any launch: NULL
 * pointers, non-positive sizes, more than 65535 rows or planes, a ratio beyond 8 on either axis, strides smaller than a row
 * or a plane, T outside 1..33, an odd-addressed w or a first off a 4-byte boundary.  A destination whose base or strides are
 * not multiples of 16 is written byte by byte. */
int wm_resample_planes_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int n_planes, int h_in, int w_in, int src_row_stride,
                              size_t src_plane_stride, int h_out, int w_out, int dst_row_stride, size_t dst_plane_stride,
                              const int32_t* first_x, const int16_t* w_x, int T_x, const int32_t* first_y, const int16_t* w_y,
                              int T_y);
int wm_resample_planes_u8(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int n_planes, int h_in, int w_in, int src_row_stride,
                          size_t src_plane_stride, int h_out, int w_out, int dst_row_stride, size_t dst_plane_stride,
                          const int32_t* first_x, const int16_t* w_x, int T_x, const int32_t* first_y, const int16_t* w_y, int T_y);

/* ---- Blind payload, rotation resynchronisation: a stego that was rotated about its centre --
 * A rotation resamples every tile, so no window has its sigma_1 on the lattice - until the rotation is undone.  The meta
 * holds everything but the angle; the angle is searched for: every candidate rotates the stego's luma back onto the marked
 * H x W frame by the filter below, the plain metric reads the restored plane, and the candidate whose valid tiles sit
 * closest to their lattice points (the largest mean |m|) wins and is decoded ("Rotation resynchronisation").
 * Integers throughout, so the device and a NumPy restatement (tests/rotate_refs.py) agree to the bit.
 *
 * Candidate: an angle theta, on the host in float64:  C = rint(cos theta 2^16),  S = rint(sin theta 2^16),  both int32.
 * Coordinates: the source is h x w, the destination the marked H x W, their centres coincide (a same-size canvas with cut
 *   corners and an expanded canvas are one case).  Destination pixel (y, x):
 *     X2 = 2 x + 1 - W;   Y2 = 2 y + 1 - H
 *     U = C X2 - S Y2 + (w - 1) 2^16;   V = S X2 + C Y2 + (h - 1) 2^16        int32, in units of 2^-17 source pixels
 *     x0 = U >> 17,  fx = (U >> 9) & 255;   y0 = V >> 17,  fy = (V >> 9) & 255  (floor shifts)
 *   Every side is at most 8192, so U and V fit 32 bits.
 * Weights: K[256][4] int16 (resample.py: rotate_weights), row f the Catmull-Rom kernel (a = -0.5, as above) at offsets
 *   -1, 0, 1, 2 for phase f / 256:  rint(cubic(f / 256 + 1 - i) 2^14), i = 0..3, the residue to 2^14 added to the largest
 *   tap, the first of equals.  K[0] = (0, 2^14, 0, 0): theta = 0 onto the same size is the identity to the byte.
 * A pixel, all int32:
 *     row_j = (sum_i K[fx][i] px[clamp(y0 - 1 + j)][clamp(x0 - 1 + i)] + 2^7) >> 8                       j = 0..3
 *     out   = clip((sum_j K[fy][j] row_j + 2^19) >> 20, 0, 255)
 *   clamp: the index brought into the source (the device does not trust the candidates).
 * A destination TILE is valid iff at each of its four corner pixels x0 - 1 >= 0, x0 + 2 <= w - 1, y0 - 1 >= 0 and
 *   y0 + 2 <= h - 1; the map is affine, so the interior follows.  Invalid tiles neither score nor vote.
 * Score of a candidate: sum of payload_vote(|m|) over its valid tiles (int64), m the metric of the restored plane read with
 *   the meta's dither table or without one; count: the number of valid tiles.  The largest score / count wins, compared
 *   exactly (cross-multiplied integers, payload.py: pick_angle), ties to the smallest candidate index; count 0 takes no part.
 * Schedule (payload.py: angle_candidates): R = hypot(H, W) / 2; coarse theta_k = k / R, |k| <= floor(radians(max_angle) R);
 *   fine theta = (8 k* + j) / (8 R), |j| <= 8, around the coarse winner k*.  Only the fine winner is decoded.
 *
 *   src    [n_planes] uint8 planes [h][w], src_row_stride / src_plane_stride in elements
 *   dst    [n_angles][n_planes] uint8 planes [H][W] (out): plane (a, p) at dst + (a n_planes + p) dst_plane_stride,
 *          dst_row_stride in elements; never in place
 *   cand   [n_angles][2] int32: (C, S)
 *   K      [256][4] int16, on an 8-byte boundary in the device form
 * WM_ERR_BADARG, before any launch: NULL pointers, a side outside 1..8192, n_angles < 1, n_planes < 1, n_angles * n_planes
 * above 65535, strides smaller than a row or a plane, (device form) misaligned cand or K.  A destination whose base or
 * strides are not multiples of 4 is written byte by byte. */
int wm_rotate_planes_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int n_planes, int h, int w, int src_row_stride,
                            size_t src_plane_stride, int H, int W, int dst_row_stride, size_t dst_plane_stride, const int32_t* cand,
                            int n_angles, const int16_t* K);
int wm_rotate_planes_u8(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int n_planes, int h, int w, int src_row_stride,
                        size_t src_plane_stride, int H, int W, int dst_row_stride, size_t dst_plane_stride, const int32_t* cand,
                        int n_angles, const int16_t* K);

/* The scores of the candidates:
 *   metric  [n_angles][n_tiles] float32, n_tiles = (H / 8) (W / 8): wm_payload_metric_tiles[_dither]_u8_dev of the n_angles
 *           restored planes (a shared dither table: dither_plane_stride 0)
 *   cand    [n_angles][2] int32, as above;  h, w: the source the planes were restored from
 *   scores  [n_angles] int64 (out), counts [n_angles] int32 (out): zeroed by the call
 *   valid   [n_angles][n_tiles] uint8 (out), may be NULL: 1 for a valid tile
 * WM_ERR_BADARG, before any launch: NULL pointers (valid excepted), a side outside 1..8192, H or W not a multiple of 8,
 * n_angles outside 1..65535, (device form) a misaligned pointer. */
int wm_payload_angle_scores_dev(wm_ctx* ctx, const float* metric, const int32_t* cand, int n_angles, int64_t* scores, int32_t* counts,
                                uint8_t* valid, int h, int w, int H, int W);
int wm_payload_angle_scores(wm_ctx* ctx, const float* metric, const int32_t* cand, int n_angles, int64_t* scores, int32_t* counts,
                            uint8_t* valid, int h, int w, int H, int W);


/* ==========================================================================
 * Full-frame mode ("tile=None", the reference's own semantics): ONE dense
 * DCT + SVD over the whole plane.  Host-pointer entry points, one plane per
 * call; L = min(H, W).  Singular values are returned sorted descending like
 * np.linalg.svd; singular vectors are unique up to sign.
 * ========================================================================== */

/* Replaces  C = dct2(Y); Uc, Sc, Vct = np.linalg.svd(C); S_[:K] = Sc[:K] +
 * alpha*Sw[:K]; Cw = Uc @ diag(S_) @ Vct; Yw = idct2(Cw); clip/astype(uint8)
 * (single:172-177, 27; per colour plane single:127-147).
 *   sigma_w [L] watermark singular values (sorted), sigma_c [L] out,
 *   yw optional [H][W] float32 unclipped stego, K in 0..L. */
int wm_ref_embed_u8(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego,
                    float* sigma_c, float* yw, int H, int W, int row_stride, float alpha, int K);

/* Replaces  _, S_cw, _ = np.linalg.svd(dct2(Y))  (single:205, 297).  sigma [L]. */
int wm_ref_sigma_u8(wm_ctx* ctx, const uint8_t* plane, float* sigma, int H, int W, int row_stride);

/* Batched forms: n_planes planes (B,G,R of a colour image - single:127-147 - or frames
 * of a video) go through every launch together (the per-plane SVD is latency-bound on
 * its own).  sigma_w: plane p reads sigma_w + p * sigma_w_plane_stride (0 = shared);
 * sigma_c / sigma: [n_planes][L]; yw: [n_planes][H][W]. */
int wm_ref_embed_planes_u8(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego,
                           float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                           size_t plane_stride, size_t sigma_w_plane_stride, float alpha, int K);
int wm_ref_sigma_planes_u8(wm_ctx* ctx, const uint8_t* planes, float* sigma, int n_planes, int H, int W,
                           int row_stride, size_t plane_stride);
/* The same embed for a caller that is still computing sigma_w: single:172-173 are two independent decompositions (the host
 * plane's and the watermark's), and one full-frame SVD occupies a fraction of the chip - run on two contexts and two host
 * threads they overlap.  sigma_w is first read after the host planes' decomposition; until then *sigma_w_ready may be 0.
 * The caller stores > 0 (release order) once sigma_w is written, or < 0 to abandon the call (returns WM_ERR_BADARG).
 * sigma_w_ready == NULL: sigma_w is valid on entry (wm_ref_embed_planes_u8). */
int wm_ref_embed_planes_u8_when(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, const int* sigma_w_ready,
                                uint8_t* stego, float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                                size_t plane_stride, size_t sigma_w_plane_stride, float alpha, int K);

/* Replaces  Wm = dct2(wy_s); Uw, Sw, Vwt = np.linalg.svd(Wm, full_matrices=False)
 * (single:173, 131-134) when apply_dct != 0 (plain thin SVD of the plane otherwise).
 *   U [H][L], S [L], Vt [L][W].
 * A rank-deficient plane (a blank, sparse or constant logo plane) returns U and Vt with L orthonormal columns / rows all the
 * same: the singular vectors of its null singular values (S at rounding level, 0 for a zero plane) are a deterministic
 * orthonormal completion, as arbitrary as LAPACK's. */
int wm_ref_svd_f32(wm_ctx* ctx, const float* plane, float* U, float* S, float* Vt, int H, int W,
                   int row_stride, int apply_dct);

/* The same for n_planes planes in ONE batch (the B, G, R planes of a colour watermark, single:128-134:
 * `UWb, SWb, VWbt = svd(dct2(wb_s))` ... three times): every launch carries all planes.
 *   planes [n][H][row_stride], U [n][H][L], S [n][L], Vt [n][L][W], host memory. */
int wm_ref_svd_planes_f32(wm_ctx* ctx, const float* planes, float* U, float* S, float* Vt, int n_planes, int H, int W,
                          int row_stride, size_t plane_stride, int apply_dct);

/* Replaces single:205-218: sigma of the stego -> Sw_hat = (S_cw - Sc)/max(alpha,1e-8),
 * Sw_hat[K:] = 0 -> Uw[:L,:L] @ diag(Sw_hat) @ Vwt[:L,:L] zero-padded into H x W
 * (the reference's [:L,:L] truncation on non-square planes is reproduced) -> idct2.
 *   Uw [H][L], Vwt [L][W], out [H][W] float32. */
int wm_ref_extract_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                      const float* Vwt, float* out, int H, int W, int row_stride, float alpha, int K);

/* Replaces single:214-218 on their own, with the estimates given by the caller:
 * Uw[:L,:L] @ diag(sw_hat[:L]) @ Vwt[:L,:L] into the top-left corner of a zero H x W plane
 * (single:215-217), then idct2 (single:218).  L <= min(H, W) is the reference's truncation
 * length `min(len(Sc), len(S_cw), Uw.shape[0], Vwt.shape[0])` (single:210): it is shorter than
 * the meta's own when the stego handed to extract is not the size the meta was written for
 * (resized / cropped stego) - the drop-in then takes sigma of the stego with wm_ref_sigma_u8,
 * forms Sw_hat on the host (single:211-213) and calls this.
 *   Uw [H][min(H,W)], sw_hat [L], Vwt [min(H,W)][W], out [H][W] float32, all host memory.
 * Any finite factors and estimates are accepted; they need not be orthonormal.  Factors whose [:L,:L] corners have a row of
 * Uw or a column of Vwt longer than 1 + 2^-10 take the f32 products instead of the split-f16 ones. */
int wm_ref_reconstruct_f32(wm_ctx* ctx, const float* Uw, const float* sw_hat, const float* Vwt, float* out,
                           int H, int W, int L);

/* The same for n_planes stego planes that share ONE watermark decomposition (the frames
 * of a clip, single:205-218 applied per frame): their SVDs run as one batch.
 *   sigma_c [n_planes][L], out [n_planes][H][W] float32. */
int wm_ref_extract_planes_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                             const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                             size_t plane_stride, float alpha, int K);

/* Device-pointer forms of the batched full-frame entry points: the planes and the big factors
 * (Uw [H][L], Vwt [L][W], out, yw) are DEVICE memory and never cross PCIe - the frames of a clip
 * or the per-rank frame range of bench.py --mode fullframe stay resident.  The meta-sized vectors
 * (sigma_w, sigma_c, sigma, scores) are device memory too; they are sorted / classified on the
 * host inside the call (L floats per plane), so these calls synchronise the context's stream.
 * Same statements of the reference as the host-pointer forms above. */
int wm_ref_embed_planes_u8_dev(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego,
                               float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                               size_t plane_stride, size_t sigma_w_plane_stride, float alpha, int K);
int wm_ref_sigma_planes_u8_dev(wm_ctx* ctx, const uint8_t* planes, float* sigma, int n_planes, int H, int W,
                               int row_stride, size_t plane_stride);
int wm_ref_extract_planes_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                                 const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                                 size_t plane_stride, float alpha, int K);
int wm_ref_detect_planes_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                                double* scores, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                float alpha);

/* Diagnostics: outer Jacobi sweeps the last full-frame SVD on this context needed. */
int wm_ref_last_sweeps(wm_ctx* ctx, int* sweeps_out);
/* Diagnostics (roofline accounting of bench.py): matrix-core flops the block Jacobi of the last full-frame SVD on this
 * context issued - Gram and rotation products as launched, pairs skipped as converged included - and whether it ran the
 * two-level (super-block) scheme (1) or the flat tournament (0). */
int wm_ref_last_flops(wm_ctx* ctx, double* flops_out, int* two_level_out);

/* Replaces single:297-301 + _nc (single:284-289): score over all L singular values. */
int wm_ref_detect_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                     double* score, int H, int W, int row_stride, float alpha);

/* The same for n_planes stego planes carrying ONE watermark (frames of a clip): their SVDs
 * run as one batch.  sigma_c [n_planes][L], sigma_w [L], scores [n_planes]. */
int wm_ref_detect_planes_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                            double* scores, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                            float alpha);

/* ==========================================================================
 * Pixel-side kernels either side of the hot path.  Colour
 * conversion is OpenCV's 8-bit fixed point, bit-exact integer work; images
 * are contiguous interleaved 3-channel uint8 (n_px pixels), planes contiguous.
 * *_dev: device pointers (16-byte aligned), asynchronous on the context stream.
 * ========================================================================== */
/* cv2.cvtColor(BGR2YCrCb) / (YCrCb2BGR) / (BGR2GRAY)          single:22, 30, 45, 170 */
int wm_bgr_to_ycrcb_u8_dev(wm_ctx* ctx, const uint8_t* bgr, uint8_t* ycrcb, size_t n_px);
int wm_ycrcb_to_bgr_u8_dev(wm_ctx* ctx, const uint8_t* ycrcb, uint8_t* bgr, size_t n_px);
int wm_bgr_to_gray_u8_dev(wm_ctx* ctx, const uint8_t* bgr, uint8_t* gray, size_t n_px);
/* _to_Y (single:21-24): the Y plane of BGR2YCrCb only */
int wm_bgr_to_y_u8_dev(wm_ctx* ctx, const uint8_t* bgr, uint8_t* y, size_t n_px);
/* _from_Y (single:26-30): YCrCb of `bgr` with Y replaced by y_new, back to BGR */
int wm_replace_y_u8_dev(wm_ctx* ctx, const uint8_t* bgr, const uint8_t* y_new, uint8_t* bgr_out, size_t n_px);
/* sum of squared differences of two uint8 buffers (exact integer; psnr of single:38-42 follows) */
int wm_sqdiff_u8_dev(wm_ctx* ctx, const uint8_t* a, const uint8_t* b, size_t n, unsigned long long* ssd_dev);
/* mean SSIM (single:44-57: 11x11 sigma 1.5 Gaussian, reflect-101 border) of two planes;
 * strides in elements; kind bit0 / bit1: img1 / img2 is float32 instead of uint8 */
int wm_ssim_dev(wm_ctx* ctx, const void* img1, size_t stride1, const void* img2, size_t stride2,
                int H, int W, int kind, double* ssim_dev);
/* uint8(clip(cv2.normalize(x, 0, 255, NORM_MINMAX), 0, 255))  (single:221-222); do_norm=0: clip only.
 * x must be 16-byte aligned (any wm_malloc'd plane is). */
int wm_normalize_u8_dev(wm_ctx* ctx, const float* x, size_t n, int do_norm, uint8_t* out);
/* Keyed scramble / unscramble of the watermark plane, single:66-80 (`_permute`: flat[idx];
 * `_unpermute`: inv[idx] = arange; flat[inv]).  idx is the int32 copy of the permutation NumPy's
 * PCG64 shuffle produced on the host (bit-exact there by construction; this is only the index pass).
 * n elements per plane, n_planes planes share idx; dst float32 [n_planes][n], never in place.
 *   permute:    dst[i] = (float) src[idx[i]]        unpermute:  dst[idx[i]] = src[i] */
int wm_permute_u8_f32_dev(wm_ctx* ctx, const uint8_t* src, const int* idx, float* dst, size_t n, int n_planes);
int wm_permute_f32_dev(wm_ctx* ctx, const float* src, const int* idx, float* dst, size_t n, int n_planes);
int wm_unpermute_f32_dev(wm_ctx* ctx, const float* src, const int* idx, float* dst, size_t n, int n_planes);
/* The end of the reference's extract in one routed, fully coalesced chain (single:74-80 `_unpermute` +
 * single:221-222 cv2.normalize(NORM_MINMAX) / clip / uint8, per plane):
 *     dst[p][idx[i]] = uint8(clip((src[p][i] - min src[p]) * 255 / (max src[p] - min src[p]), 0, 255))
 * (do_norm == 0: clip + truncate only).  A random permutation of a whole plane makes the literal index pass touch one
 * cache line per element; a wm_route factors idx ONCE per key into two block-local permutations around a block
 * transpose, after which the per-frame work streams (csrc/wm_route.hip).  wm_route_create_dev reads the int32 index
 * from device memory, synchronises the stream and returns WM_ERR_BADARG when idx is not a permutation of 0..n-1;
 * the route holds 6 bytes per element of device memory until wm_route_destroy.  src [n_planes][n] float32,
 * dst [n_planes][n] uint8, min / max per plane; bytes identical to wm_unpermute_f32_dev + wm_normalize_u8_dev. */
typedef struct wm_route wm_route;
int wm_route_create_dev(wm_ctx* ctx, const int* idx, size_t n, wm_route** route_out);
int wm_route_destroy(wm_ctx* ctx, wm_route* route);
int wm_unpermute_normalize_u8_dev(wm_ctx* ctx, const float* src, const wm_route* route, uint8_t* dst, size_t n,
                                  int n_planes, int do_norm);
/* The reference's extract per plane in ONE call (single:203-222 gray, :232-274 per colour plane): sigma of every stego tile,
 * (S_cw - Sc) / max(alpha, 1e-8) with [K:] = 0, the rank-8 product with the watermark's factors (px != 0: pixel-domain
 * factors from wm_tile_factors_to_pixel_dev, no per-tile IDCT; px == 0: Uw / Vwt as stored in the meta), the keyed
 * unscramble through `route`, min-max normalise (do_norm) / clip / uint8.  The float estimate never leaves a buffer of
 * the context and its min / max are taken by the extract kernel itself.  out [n_planes][H*W] uint8; bytes identical
 * to wm_extract_tiles[_px]_u8_dev + wm_unpermute_normalize_u8_dev. */
int wm_extract_unscrambled_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw, const float* Vwt,
                                  const wm_route* route, uint8_t* out, int n_planes, int H, int W, int row_stride,
                                  size_t plane_stride, size_t uv_plane_stride, float alpha, int K, int px, int do_norm);
/* The same with texture-masked strength (the rule above wm_mask_sigma_w_tiles_u8_dev): sw_hat by the rule's extract. */
int wm_extract_unscrambled_masked_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                                         const float* Vwt, const wm_route* route, uint8_t* out, int n_planes, int H, int W,
                                         int row_stride, size_t plane_stride, size_t uv_plane_stride, float alpha, int K,
                                         int px, int do_norm, float lo, float hi, float cut);
/* the scramble direction through the same route (single:66-72, 124-126): dst[p][i] = (float) src[p][idx[i]], uint8 planes
 * in, float32 out; values identical to wm_permute_u8_f32_dev */
int wm_permute_u8_f32_routed_dev(wm_ctx* ctx, const uint8_t* src, const wm_route* route, float* dst, size_t n, int n_planes);
/* The frame codec of the colour video functions: stored planar Y, Cb, Cr frames <-> planar B, G, R, a whole batch of
 * frames per launch.  Replaces, per frame, the host-side np.stack / cvtColor(YCrCb2BGR) / moveaxis chain (and its
 * reverse) that wraps single:21-30's conversion around a 4:4:4 frame, and adds the chroma resampling a 4:2:0 or 4:2:2
 * container needs, which the reference (cv2.VideoCapture hands it BGR) never sees.
 *   frames  [n_frames] frames of Y [H][W], Cb [ch][cw], Cr [ch][cw] (the YUV4MPEG2 frame layout, packed), frame_stride
 *           BYTES apart (>= H*W + 2*ch*cw); ch x cw = ceil(H / sub_y) x ceil(W / sub_x)
 *   planes  [n_frames][3][H][W] contiguous, B, G, R
 *   sub_x, sub_y   1, 1 (4:4:4), 2, 1 (4:2:2) or 2, 2 (4:2:0); chroma siting is not modelled
 * to_bgr: every pixel (r, c) takes chroma sample (r / sub_y, c / sub_x) (replication) through YCrCb2BGR.  to_yuv: every
 * pixel through BGR2YCrCb; Y as is; Cb, Cr the mean over the block's pixels inside the plane, rounded half up in integers.
 * sub 1, 1 gives wm_ycrcb_to_bgr_u8_dev / wm_bgr_to_ycrcb_u8_dev on the interleaved form, bit for bit.  Any H, W >= 1 and
 * any alignment; W % 16 == 0 with 16-byte aligned bases (and frame_stride) takes 16-byte accesses.  Never in place. */
int wm_yuv_frames_to_bgr_planes_u8_dev(wm_ctx* ctx, const uint8_t* frames, uint8_t* planes, int n_frames, int H, int W,
                                       int sub_x, int sub_y, size_t frame_stride);
int wm_bgr_planes_to_yuv_frames_u8_dev(wm_ctx* ctx, const uint8_t* planes, uint8_t* frames, int n_frames, int H, int W,
                                       int sub_x, int sub_y, size_t frame_stride);
/* the same on host memory: one upload, one launch, one download and one synchronise per call; bytes between the frames
 * (frame_stride > a frame) are neither read nor written */
int wm_yuv_frames_to_bgr_planes_u8(wm_ctx* ctx, const uint8_t* frames, uint8_t* planes, int n_frames, int H, int W,
                                   int sub_x, int sub_y, size_t frame_stride);
int wm_bgr_planes_to_yuv_frames_u8(wm_ctx* ctx, const uint8_t* planes, uint8_t* frames, int n_frames, int H, int W,
                                   int sub_x, int sub_y, size_t frame_stride);
/* host-pointer conveniences; op: 0 BGR->YCrCb, 1 YCrCb->BGR, 2 BGR->gray plane, 3 BGR->Y plane,
 * 4 replace Y (plane_in) and return BGR */
int wm_color_u8(wm_ctx* ctx, int op, const uint8_t* in3, const uint8_t* plane_in, uint8_t* out3,
                uint8_t* plane_out, size_t n_px);
int wm_psnr_u8(wm_ctx* ctx, const uint8_t* a, const uint8_t* b, size_t n, double* psnr_out);
int wm_ssim(wm_ctx* ctx, const void* img1, const void* img2, int H, int W, int kind, double* ssim_out);
int wm_normalize_u8(wm_ctx* ctx, const float* x, size_t n, int do_norm, uint8_t* out);

/* ---- extract post-processing (single:223-227 gray, 275-277 colour, 88-110) ----------------------------
 * The reference writes, as the _wm.png, the estimate after cv2.fastNlMeansDenoising(wy, None, 7, 7, 21) + CLAHE(2.0,
 * 8x8) + unsharp (gray) or cv2.fastNlMeansDenoisingColored(out, None, 3, 3, 7, 21) + CLAHE on Y of YCrCb + unsharp
 * (colour).  OpenCV 4.x's 8-bit algorithms, restated in tests/enhance_oracle.py.  Images are
 * dense, row-major, interleaved uint8.  Unsupported sizes / parameters return WM_ERR_BADARG.
 *   wm_nlmeans_u8_dev   channels 1 or 2 (interleaved); template_ws 7 with search_ws 21 only; not in place
 *   wm_clahe_u8_dev     tiles_x, tiles_y 1..16; may run in place
 *   wm_unsharp_u8_dev   GaussianBlur(sigma 1) + addWeighted(e, 1 + amount, blur, -amount, 0); channels 1 or 3; not in place
 *   wm_*_lab_*          COLOR_LBGR2Lab / COLOR_Lab2LBGR (linear RGB, D65), n_px interleaved pixels
 *   wm_enhance_extract  the whole chain: channels 1 (gray) or 3 (BGR); src may equal dst
 * The _dev forms keep their intermediates in the context's grow-only workspace (nothing allocated once warm). */
int wm_nlmeans_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, int channels,
                      float h, int template_ws, int search_ws);
int wm_clahe_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, float clip_limit, int tiles_x, int tiles_y);
int wm_unsharp_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, int channels, float amount);
int wm_bgr_to_lab_u8_dev(wm_ctx* ctx, const uint8_t* bgr, uint8_t* lab, size_t n_px);
int wm_lab_to_bgr_u8_dev(wm_ctx* ctx, const uint8_t* lab, uint8_t* bgr, size_t n_px);
int wm_enhance_extract_u8_dev(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, int channels);
int wm_enhance_extract_u8(wm_ctx* ctx, const uint8_t* src, uint8_t* dst, int H, int W, int channels);

#ifdef __cplusplus
}
#endif
#endif /* WMHIP_H */
