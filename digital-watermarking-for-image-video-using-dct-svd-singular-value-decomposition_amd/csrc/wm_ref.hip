// Full-frame ("reference semantics", tile=None) mode of the DCT-SVD watermark
// on gfx950: ONE dense SVD per plane instead of one per 8x8 tile
// (app_dct_svd_single.py:172-177 embed, :205-218 extract, :297-301 detect).
//
// Algorithm:
//  * the orthonormal DCT cancels (svd(D_H Y D_W^T) = (D_H Ux) S (D_W Vx)^T), so
//    embed/sigma/detect work on the pixel plane itself;
//  * block one-sided Jacobi on the SHORT side: A (L x M, L <= M; the plane or
//    its transpose) is augmented with the identity, Aug = [A | I_L]; row
//    rotations turn it into [B | Qt] with B = Qt A having mutually orthogonal
//    rows, |b_i| = sigma_i, Qt^T = left singular vectors.  Rows are processed in
//    blocks of RB: a step takes disjoint block pairs (round-robin tournament),
//    forms each pair's 2RB x 2RB Gram matrix (k_rf_gram), runs one cyclic
//    two-sided Jacobi sweep on it in LDS (k_rf_inner -> rotation block R) and
//    applies R^T to the 2RB rows of Aug as a small GEMM (k_rf_apply);
//  * embed is V-free: Yw = Y + Q diag(alpha*sw_rank(i) / sigma_i) B.
// DCT-domain factors (watermark side / extract) use plain tiled SGEMMs with the
// DCT basis matrices.
#include <chrono>
#include <thread>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <new>
#include <numeric>
#include <utility>
#include <vector>

#include "wm_internal.h"

using namespace wmi;

namespace {

constexpr int RB = 32;        // rows per Jacobi block
constexpr int RP = 2 * RB;    // rows per block pair
constexpr int GRAM_CC = 128;  // columns per Gram partial
constexpr int MAX_SWEEPS = 40;
constexpr int FULL_INNER_SWEEPS = 0;   // outer sweeps whose every step runs the full 63-step inner schedule
constexpr float CONV_COS = 2e-5f;   // float32 Gram entries resolve cos down to ~eps*sqrt(M)
// sigma-only calls (extract, detect): row norms are exact to O(cos^2), and the sweep that
// observes max cos < c still rotates (leaving ~c^2), so they may stop an order earlier (2e-3 already costs 7e-5 relative on dense spectra: tools/ff_sigma_thr.py)
constexpr float CONV_COS_SIGMA = 2e-4f;
constexpr float SKIP_FRACTION = 0.25f;    // a block pair below this fraction of the (embed) stopping cosine is left alone
constexpr double RESIDUE_RHO = 10.0;      // |A0 b_i^T| / |b_i|^2 above this: b_i is not a singular direction at all
constexpr double T_SWITCH = 200.0;        // |A0 b_i^T| / |b_i| is used for s_i >= T_SWITCH * (residual cosine) * s_max
constexpr int HIER_F16_DEFAULT = 3;         // two-level scheme, split-f16 operands on the f16 matrix pipe: bit 0 Gram tiles (k_hgram_t<true>), bit 1 rotation products (k_happly_h); WM_RF_HIER_F16 overrides
constexpr int HIER_MIN_PLANES = 20;         // ... with the f32 kernels
constexpr int HIER_MIN_PLANES_F16 = 3;      // planes per call from which the two-level scheme is the default when its split-f16 kernels apply        // planes per call from which the two-level scheme (wm_ref_hier.inc) is the default
constexpr int DEFAULT_QUEUES = 2;         // plane groups of a batched Jacobi, each on its own HIP queue
constexpr double DRIFT_TOL = 1e-2;        // |T[:, i]| / |b_i|^2 may differ from 1 by the scale drift, not more
constexpr double NULL_ROW_RATIO = 1e-5;   // rows below this fraction of |A|_F do not take part in the convergence test
constexpr double NULL_RATIO = 1e-6;   // embed: singular directions below this fraction of s_1 get no watermark energy

// ---------------------------------------------------------------------------
// Tile vocabulary of the full-frame kernels (this file and wm_ref_hier.inc): every rule below is stated here, once.
// Functions where the kernels compile to the same code with them; the four macros (capitals) are the rules that hipcc
// optimises on their own before it inlines them, after which a kernel's instruction stream comes out different.
// ---------------------------------------------------------------------------
typedef float v16f __attribute__((ext_vector_type(16)));     // the accumulator of one 32 x 32 MFMA tile
typedef float f2v __attribute__((ext_vector_type(2)));
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));    // one lane's operand of v_mfma_f32_32x32x16_f16: 8 consecutive k
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));

// Accumulator register v of lane (j, h = lane / 32) holds row ACC_ROW(v, h, base) of the 32 x 32 tile (column j); base: the tile's
// first row in whatever it is a tile of (added first: as a function, or with the base added last, the sum is associated
// differently and the address arithmetic of k_sgemm, k_hgemm and k_hupdate comes out in another order).
#define ACC_ROW(v, h, base) ((base) + 8 * ((v) / 4) + 4 * (h) + ((v) % 4))

// row (or column) r of a block pair's 64 -> row of the enclosing matrix whose blocks la, lb the pair is made of
__device__ __forceinline__ constexpr int pair_row(const int r, const int la, const int lb) { return (r < RB) ? la * RB + r : lb * RB + r - RB; }

// A unit of a stage of the two-level scheme: two blocks (local indices la, lb of the super-pair) that are rotated against each
// other, or an idle pair that only keeps k_hupdate's pairing complete (R = I); -1: no such unit at this stage.
constexpr int UNIT_NONE = -1;
__host__ __device__ constexpr int unit_make(const int la, const int lb, const bool real) { return la | (lb << 8) | (real ? 1 << 16 : 0); }
__host__ __device__ constexpr int unit_la(const int e) { return e & 0xff; }
__host__ __device__ constexpr int unit_lb(const int e) { return (e >> 8) & 0xff; }
// (as a function: other code in k_happly_h's stage prologue)
#define UNIT_ROTATES(e) ((e) >= 0 && (((e) >> 16) & 1))

// XCD-aware orders.  Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share an L2 - observed placement, speed
// only), so id -> (xcd = id % 8, q = id / 8).
//  * groups (Gram kernels): `per` consecutive q on ONE XCD are the workgroups w of one (super-pair, split, plane) group - they
//    read the same row panels and meet in that XCD's L2.  Returns the group, which lies beyond the grid's nsp * KS * nz for
//    the workgroups that pad the launch to a multiple of 8 groups.
__device__ __forceinline__ int xcd_group(const int id, const int per, int& w) {
  const int xcd = id & 7, q = id >> 3;
  w = q % per;
  return (q / per) * 8 + xcd;
}
__device__ __forceinline__ void group_decode(const int grp, const int nsp, const int KS, int& sp, int& ks, int& zl) {
  sp = grp % nsp; ks = (grp / nsp) % KS; zl = grp / (nsp * KS);
}
//  * tasks (apply kernels): the ntask tasks in contiguous ranges, XCD x takes [ntask x / 8, ntask (x + 1) / 8) - a super-pair's
//    rotations serve all of its strips from one or two L2s.  Returns the task; at or beyond `end` this workgroup has none.
//  (Plain arithmetic, the early return stays with the kernel: a helper that returns "no work" compiles to another prologue.)
__device__ __forceinline__ int xcd_task(const unsigned id, const int ntask, int& end) {
  const int xcd = id & 7, q = id >> 3;
  const int x0 = (int)((long)ntask * xcd / 8);
  end = (int)((long)ntask * (xcd + 1) / 8);
  return x0 + q;
}

// Of the 16-byte load v of columns col .. col + 3 of a row of M columns, what lies behind the row's end is zeroed.  (The load
// itself may run past M: every row of Aug has its identity part and padding behind it.  k_hgemm's operands are dense matrices
// with nothing behind a row, so its load4 does not load what this masks - a bounded load, not a fourth copy of this mask.)
// (as a function, by value or by reference: other register assignments in k_hgram_h3 and k_hgram_t<true>)
#define MASK_TAIL4(v, col, M) \
  do { if ((col) + 3 >= (M)) { if ((col) >= (M)) (v).x = 0.0f; if ((col) + 1 >= (M)) (v).y = 0.0f; if ((col) + 2 >= (M)) (v).z = 0.0f; (v).w = 0.0f; } } while (0)

// The three hi / lo splits of an f32 value for the f16 matrix pipe.  They differ in what happens to
// the low part, and so in their bits - they are kept apart on purpose:
//  * split4_f16     x = hi + lo, lo = f16(x - hi) UNSCALED.  k_hgram_t<true>, k_hgram_h3, k_hgemm: Gram entries only steer the
//                   rotations and the finalisation's operands are pre-scaled into [~1, 3e4), so losing lo where it is an f16
//                   denormal (|x| < 0.125) costs < 2^-22 of the products, and the accumulator needs no rescaling.
//  * split4_scaled  x = hi + lo' / 2048, lo' = f16((x - hi) * 2048).  k_happly_h's strip image, staged and written back every
//                   stage: the rows themselves live in this form, so lo' keeps 22 significant bits down to |x| ~ 3e-8 (f16
//                   subnormals are kept by the conversion and honoured by the matrix pipe: tools/ubench_f16_denorm.hip); the
//                   cross products go to a second accumulator that is scaled by 2^-11 at the end.
//  * SPLIT1_FLUSHED the scaled rule for ONE value with hi flushed to 0 below f16's normal range (6.2e-5): k_rf_inner's packed
//                   rotation for k_happly_h.  Such an entry sits wholly in lo' instead of in a subnormal hi; the matrix pipe
//                   would take the subnormal as well, but dropping the flush changes R's bits, so it stays.
__device__ __forceinline__ void split4_f16(const float4 v, uint2& hi, uint2& lo) {
  const h2_t a = {(_Float16)v.x, (_Float16)v.y}, b = {(_Float16)v.z, (_Float16)v.w};
  const h2_t la = {(_Float16)(v.x - (float)a[0]), (_Float16)(v.y - (float)a[1])};
  const h2_t lb = {(_Float16)(v.z - (float)b[0]), (_Float16)(v.w - (float)b[1])};
  hi = make_uint2(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b));
  lo = make_uint2(__builtin_bit_cast(unsigned, la), __builtin_bit_cast(unsigned, lb));
}
// (six VALU instructions per two values: packed f32 subtract and scale)
__device__ __forceinline__ void split4_scaled(const float x0, const float x1, const float x2, const float x3, h4_t& hi, h4_t& lo) {
  const f2v a = {x0, x1}, b = {x2, x3};
  const h2_t ha = __builtin_convertvector(a, h2_t), hb = __builtin_convertvector(b, h2_t);
  const f2v ra = (a - __builtin_convertvector(ha, f2v)) * 2048.0f, rb = (b - __builtin_convertvector(hb, f2v)) * 2048.0f;
  const h2_t la = __builtin_convertvector(ra, h2_t), lb = __builtin_convertvector(rb, h2_t);
  hi = h4_t{ha[0], ha[1], hb[0], hb[1]};
  lo = h4_t{la[0], la[1], lb[0], lb[1]};
}
// (as a function: k_rf_inner's stores of the packed R in another order)
#define SPLIT1_FLUSHED(v, hi, lo) \
  do { const _Float16 h_ = fabsf(v) < 6.2e-5f ? (_Float16)0.0f : (_Float16)(v); (hi) = h_; (lo) = (_Float16)(((v) - (float)h_) * 2048.0f); } while (0)

// acc += a b^T from split operands: hi hi, hi lo, lo hi (lo lo is below 2^-22 of the product).  k_happly_h issues the same three
// with the two cross products in an accumulator of their own (its lo' is scaled); k_hgemm drops the third where A has no lo.
__device__ __forceinline__ void mfma3_f16(const h8_t ah, const h8_t al, const h8_t bh, const h8_t bl, v16f& acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
}

// ---------------------------------------------------------------------------
// generic row-major SGEMM:  C = alpha * op(A) op(B) + beta * C  on MFMA
// (v_mfma_f32_32x32x2_f32).  64x64 tile of C per workgroup, one 32x32 quadrant per wave,
// K step 32 staged through LDS in operand-friendly layouts - As[m][k] pitch 33 (the A operand
// A[m0 + lane%32][k + lane/32] hits 32 banks), Bs[k][n] pitch 65 - with the next step's global
// loads issued before this step's 16 MFMAs.  Plain-library-GEMM shaped work of the full-frame
// mode (DCT as two GEMMs, T = A0 B^T, U diag V^T products).
// ---------------------------------------------------------------------------
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void k_sgemm(const int M, const int N, const int K, const float alpha,
                                              const float* __restrict__ A, const int lda, const size_t sA,
                                              const float* __restrict__ B, const int ldb, const size_t sB,
                                              const float beta, float* __restrict__ C, const int ldc, const size_t sC) {
  constexpr int KS = 32;
  A += (size_t)blockIdx.z * sA; B += (size_t)blockIdx.z * sB; C += (size_t)blockIdx.z * sC;   // batch: one product per grid.z
  __shared__ float As[2][64][KS + 1];   // [m][k]
  __shared__ float Bs[2][KS][64 + 1];   // [k][n]
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63, j = lane & 31, h = lane >> 5;
  const int bm = blockIdx.y * 64, bn = blockIdx.x * 64;
  // staging maps: 2048 elements of each tile, 8 per thread, lanes along the contiguous global axis
  //   A stored [m][k] (TA = false): e -> m = e >> 5, k = e & 31;   A stored [k][m] (TA): k = e >> 6, m = e & 63
  //   B stored [k][n] (TB = false): e -> k = e >> 6, n = e & 63;   B stored [n][k] (TB): n = e >> 5, k = e & 31
  float ra[8], rb[8];
  auto fetch = [&](const int k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = t + 256 * i;
      const int m = TA ? (e & 63) : (e >> 5), ka = TA ? (e >> 6) : (e & 31);
      const int gm = bm + m, gk = k0 + ka;
      const bool oka = gm < M && gk < K;
      const size_t ia = TA ? (size_t)(oka ? gk : 0) * lda + (oka ? gm : 0) : (size_t)(oka ? gm : 0) * lda + (oka ? gk : 0);
      const float va = A[ia];
      ra[i] = oka ? va : 0.0f;
      const int n = TB ? (e >> 5) : (e & 63), kb = TB ? (e & 31) : (e >> 6);
      const int gn = bn + n, gkb = k0 + kb;
      const bool okb = gn < N && gkb < K;
      const size_t ib = TB ? (size_t)(okb ? gn : 0) * ldb + (okb ? gkb : 0) : (size_t)(okb ? gkb : 0) * ldb + (okb ? gn : 0);
      const float vb = B[ib];
      rb[i] = okb ? vb : 0.0f;
    }
  };
  auto stash = [&](const int buf) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = t + 256 * i;
      const int m = TA ? (e & 63) : (e >> 5), ka = TA ? (e >> 6) : (e & 31);
      As[buf][m][ka] = ra[i];
      const int n = TB ? (e >> 5) : (e & 63), kb = TB ? (e & 31) : (e >> 6);
      Bs[buf][kb][n] = rb[i];
    }
  };
  const int m0 = (wv >> 1) * 32, n0 = (wv & 1) * 32;
  // Two-level accumulation: every K step of 32 is summed from zero in the matrix core (which adds its products to
  // C one by one, round-to-nearest: tools/mfma_round_probe.hip) and the step sums are added up by the VALU.  One long
  // chain loses every term that follows a dominant one below that term's ulp - the DC coefficient of a DCT plane
  // leads its row by 2^11 - which made sigma_1 of the watermark-side SVD 5e-6 (1080p) to 4e-5 (8K) low.
  v16f acc = {0};
  fetch(0);
  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += KS, buf ^= 1) {
    stash(buf);
    if (k0 + KS < K) fetch(k0 + KS);
    __syncthreads();                    // double-buffered LDS: one barrier per K step
    const float* pa = &As[buf][m0 + j][h];
    const float* pb = &Bs[buf][h][n0 + j];
    v16f part = {0};
#pragma unroll
    for (int kk = 0; kk < KS / 2; ++kk)
      part = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * kk], pb[2 * kk * 65], part, 0, 0, 0);
    acc += part;
  }
  const int gn = bn + n0 + j;
  if (gn < N) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int gm = ACC_ROW(v, h, bm + m0);
      if (gm < M) {
        float* c = C + (size_t)gm * ldc + gn;
        *c = (beta == 0.0f) ? alpha * acc[v] : __builtin_fmaf(beta, *c, alpha * acc[v]);
      }
    }
  }
}

// `batch` products per launch (grid.z); sA / sB / sC = elements between consecutive operands (0: shared)
int sgemm_b(wm_ctx* ctx, bool ta, bool tb, int M, int N, int K, float alpha, const float* A, int lda, size_t sA,
            const float* B, int ldb, size_t sB, float beta, float* C, int ldc, size_t sC, int batch) {
  if (M <= 0 || N <= 0 || batch <= 0) return WM_OK;
  const dim3 grid((N + 63) / 64, (M + 63) / 64, batch), block(256);
  if (ta && tb) hipLaunchKernelGGL((k_sgemm<true, true>), grid, block, 0, ctx->stream, M, N, K, alpha, A, lda, sA, B, ldb, sB, beta, C, ldc, sC);
  else if (ta) hipLaunchKernelGGL((k_sgemm<true, false>), grid, block, 0, ctx->stream, M, N, K, alpha, A, lda, sA, B, ldb, sB, beta, C, ldc, sC);
  else if (tb) hipLaunchKernelGGL((k_sgemm<false, true>), grid, block, 0, ctx->stream, M, N, K, alpha, A, lda, sA, B, ldb, sB, beta, C, ldc, sC);
  else hipLaunchKernelGGL((k_sgemm<false, false>), grid, block, 0, ctx->stream, M, N, K, alpha, A, lda, sA, B, ldb, sB, beta, C, ldc, sC);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

int sgemm(wm_ctx* ctx, bool ta, bool tb, int M, int N, int K, float alpha, const float* A, int lda,
          const float* B, int ldb, float beta, float* C, int ldc) {
  return sgemm_b(ctx, ta, tb, M, N, K, alpha, A, lda, 0, B, ldb, 0, beta, C, ldc, 0, 1);
}

// ---------------------------------------------------------------------------
// Aug = [A | I]:  A[i][j] = src(i, j) (or src(j, i) when `transpose`), rows
// i >= L are zero padding; the identity block is Lp x Lp.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void k_rf_load(const T* __restrict__ src, const size_t src_stride, const size_t src_plane_stride,
                          const int transpose, float* __restrict__ aug, const size_t aug_plane_stride,
                          const int ld, const int L, const int Lp, const int M) {
  const int i = blockIdx.y;
  src += (size_t)blockIdx.z * src_plane_stride;
  aug += (size_t)blockIdx.z * aug_plane_stride;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < M + Lp; j += gridDim.x * blockDim.x) {
    float v;
    if (j < M) v = (i < L) ? (float)(transpose ? src[(size_t)j * src_stride + i] : src[(size_t)i * src_stride + j]) : 0.0f;
    else v = (j - M == i) ? 1.0f : 0.0f;
    aug[(size_t)i * ld + j] = v;
  }
}

// ---------------------------------------------------------------------------
// Gram partials: for pair p = (I, J) and column chunk ch,
//   G[r][c] = sum_{k in chunk} X[r][k] X[c][k],  X = rows of blocks I,J; stored as the three quadrants
//   partial[p][ch] = [G_II | G_IJ | G_JJ] (32 x 32 each) - G_JI is the transpose (k_rf_inner mirrors it)
// ---------------------------------------------------------------------------
// MFMA form: the 64 x 128 chunk of X is staged row-major in LDS (pitch 129: the operand reads
// X[i0 + lane%32][k + lane/32] of a wave hit 32 distinct banks twice), wave w owns the 32 x 32
// quadrant (w >> 1, w & 1) of the Gram matrix and issues 64 v_mfma_f32_32x32x2_f32 whose A and B
// operands both come from X (D = X_I X_J^T).
constexpr int GP = GRAM_CC + 1;
constexpr int GRAM_PART = 3 * RB * RB;      // floats per (pair, chunk) partial: the quadrants (I,I), (I,J), (J,J)

__global__ __launch_bounds__(256) void k_rf_gram(const float* __restrict__ aug, const size_t aug_plane_stride,
                                                const int ld, const int M, const int2* __restrict__ pairs,
                                                float* __restrict__ partials) {
  __shared__ float Xs[RP][GP];
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63, j = lane & 31, h = lane >> 5;
  const int p = blockIdx.x, ch = blockIdx.y, nch = gridDim.y;
  aug += (size_t)blockIdx.z * aug_plane_stride;
  partials += (size_t)blockIdx.z * gridDim.x * nch * GRAM_PART;
  const int2 pr = pairs[p];
  const int c_begin = ch * GRAM_CC;
  {
    // 64 rows x GRAM_CC columns: thread t takes column t % GRAM_CC of rows t / GRAM_CC + RSTEP i; all loads are
    // issued before the LDS stores
    constexpr int RSTEP = 256 / GRAM_CC, NLD = RP / RSTEP;
    const int c = t % GRAM_CC, r0 = t / GRAM_CC, gc = c_begin + c;
    const bool valid = gc < M;
    const int gcc = valid ? gc : M - 1;
    float v[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int r = r0 + RSTEP * i;
      const int grow = pair_row(r, pr.x, pr.y);
      v[i] = aug[(size_t)grow * ld + gcc];
    }
#pragma unroll
    for (int i = 0; i < NLD; ++i) Xs[r0 + RSTEP * i][c] = valid ? v[i] : 0.0f;
  }
  __syncthreads();
  // G is symmetric: the quadrant (J, I) is the transpose of (I, J) and is neither computed nor stored - a partial
  // is [Q_II | Q_IJ | Q_JJ], 3 x 32 x 32 floats (GRAM_PART); wave 2 has nothing to do after the staging
  if (wv == 2) return;
  const int i0 = (wv >> 1) * 32, j0 = (wv & 1) * 32;
  const float* ra = &Xs[i0 + j][h];
  const float* rb = &Xs[j0 + j][h];
  v16f acc = {0};
#pragma unroll 16
  for (int kk = 0; kk < GRAM_CC / 2; ++kk)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[2 * kk], rb[2 * kk], acc, 0, 0, 0);
  float* out = partials + ((size_t)p * nch + ch) * GRAM_PART + (wv == 3 ? 2 : wv) * (RB * RB);
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    out[ACC_ROW(v, h, 0) * RB + j] = acc[v];
  }
}

// ---------------------------------------------------------------------------
// One cyclic two-sided Jacobi sweep on the pair's 64x64 Gram matrix in LDS.
// Parallel (round-robin) ordering: 63 steps x 32 disjoint rotations; de Rijk
// rule per rotation (larger diagonal entry to the lower index).  Outputs the
// accumulated rotation block R (G' = R^T G R) and the sweep-wide maximum of
// |G_rc| / sqrt(G_rr G_cc) (convergence measure, before rotating).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int rr_elem(const int pos, const int step) {
  // round-robin tournament over 64 players: position 0 is fixed, the others rotate
  if (pos == 0) return 0;
  int v = pos - 1 - step;          // step < 63
  if (v < 0) v += RP - 1;
  return v + 1;
}

// cross_only != 0: only the 32 x 32 pairs between the two row blocks are rotated
// (bipartite schedule, 32 steps); the within-block pairs are covered once per
// outer sweep by the full 63-step schedule (every block sits in exactly one
// pair of the sweep's first step).
// Thread layout: thread (kr = t >> 5, k2 = t & 31) owns column pair k2 and the row pairs kr + KR i: with
// INNER_NT = 512 threads two 2x2 blocks of G and four (row, column pair) items of R per step.
// What bounds a step (measured, profiles/r02_fullframe_inner.md): in-kernel stamps give 1 716 cycles per
// cross-only step for 1024 AND for 512 threads (2 540 with the full 63-step schedule, whose index arithmetic
// branches) - a step is the LDS pipe's time, not the instruction count: every step reads and rewrites all of
// G and R (19.5 k dword accesses; 8 192 of them ds_write_b32 at 64 B/clk/CU = 512 cycles, the reads 350) in
// lock-step bursts between two barriers, plus the angle arithmetic's two v_rsq_f32 chains (~250 cycles)
// that nothing else can run under.  256 threads (one wave per SIMD) lose the latency hiding (39.7 us per
// solve against 30.1); 512 threads issue the per-pair angle and index arithmetic half as often as 1024 and
// are 14 % faster on an 8-plane batch (98 against 86 frames/s), equal on a single plane.
// Two-level (super-block) scheme, see "hierarchical block Jacobi" further down: a super-pair is at most HSB
// 32-row blocks (HN rows); its Gram matrix G_s and accumulated rotation Q_s are HN x HN arrays (pitch HN) in
// global memory, and a stage rotates HU disjoint block pairs ("units") of it.
constexpr int HSB = 12;
constexpr int HN = HSB * RB;
constexpr int HU = HSB / 2;
constexpr int INNER_NT = 512;
constexpr int INNER_NW = INNER_NT / 64;
constexpr int INNER_KR = INNER_NT / 32;        // row pairs a thread column covers per pass (stride between a thread's row pairs)
constexpr int INNER_NB = 32 / INNER_KR;        // 2x2 blocks of G per thread

__global__ __launch_bounds__(INNER_NT) void k_rf_inner(const float* __restrict__ partials, const int nch,
                                                      float* __restrict__ Rout, unsigned* __restrict__ maxcos_bits,
                                                      const float* __restrict__ floor2, const int cross_only,
                                                      int* __restrict__ skip_flags, const float skip_thr,
                                                      const int* __restrict__ h_units, float* __restrict__ h_Gs,
                                                      int* __restrict__ h_anyrot, const int h_nsp,
                                                      float* __restrict__ h_Rpk, int* __restrict__ h_skipT, const int h_f16) {
  // h_units != NULL: two-level scheme.  blockIdx.x = super-pair * HU + unit; the unit's two 32-row blocks (local
  // indices la, lb of the super-pair) are read straight out of the tracked Gram matrix G_s (no partial sums), and
  // the rotated 64 x 64 matrix R^T G R is written back into G_s at the end.
  __shared__ float GG[2][RP][RP + 1];   // double-buffered: a step reads one copy, writes the other
  float (*G)[RP + 1] = GG[0];
  __shared__ float R[RP][RP + 1];
  __shared__ float red[INNER_NW];
  const int t = threadIdx.x, p = blockIdx.x;
  partials += (size_t)blockIdx.z * gridDim.x * nch * GRAM_PART;
  Rout += (size_t)blockIdx.z * gridDim.x * RP * RP;
  maxcos_bits += blockIdx.z;
  // rows whose squared norm is below this plane's floor are numerically null (rounding residue of
  // a rank-deficient plane): their mutual cosines are O(1) noise and must not hold convergence up
  const float fl2 = floor2[blockIdx.z];
  int la = 0, lb = 0;
  float* gs = nullptr;
  if (h_units) {
    const int unit = h_units[p];
    if (!UNIT_ROTATES(unit)) return;               // no such unit in this super-pair at this stage / an idle pair
    la = unit_la(unit); lb = unit_lb(unit);
    gs = h_Gs + ((size_t)blockIdx.z * h_nsp + p / HU) * HN * HN;
  }
  const float* src = partials + (size_t)p * nch * GRAM_PART;
  // Sum of the column-chunk partials, as 16-byte loads with up to 16 chunks (128 VGPRs) in flight per thread: the
  // workgroup is alone on its CU and this phase is one CU's fetch rate (profiles/r02_fullframe_inner.md).
  // A partial holds the quadrants (I,I), (I,J), (J,J) (k_rf_gram): float4 f = t + INNER_NT i < 768 is quadrant f >> 8,
  // row (f & 255) >> 3, columns 4 (f & 7) ..; the chunks are added in index order.
  constexpr int NF4 = GRAM_PART / 4;
  constexpr int PER4 = (NF4 + INNER_NT - 1) / INNER_NT;
  constexpr int UN = 16;
  float4 acc[PER4];
#pragma unroll
  for (int i = 0; i < PER4; ++i) acc[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (h_units) {
    for (int f = t; f < RP * RP / 4; f += INNER_NT) {
      const int r = f >> 4, c4 = (f & 15) * 4;
      const int gr = pair_row(r, la, lb), gc = pair_row(c4, la, lb);
      const float4 v = *reinterpret_cast<const float4*>(gs + (size_t)gr * HN + gc);
      G[r][c4] = v.x; G[r][c4 + 1] = v.y; G[r][c4 + 2] = v.z; G[r][c4 + 3] = v.w;
      if (!cross_only) {
#pragma unroll
        for (int k = 0; k < 4; ++k) R[r][c4 + k] = (r == c4 + k) ? 1.0f : 0.0f;
      }
    }
  } else {
    const float4* src4 = reinterpret_cast<const float4*>(src);
    for (int ch = 0; ch < nch; ch += UN) {
      float4 v[UN][PER4];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int c = min(ch + u, nch - 1);            // past the end: a repeated (cached) load, masked below
#pragma unroll
        for (int i = 0; i < PER4; ++i) v[u][i] = src4[(size_t)c * NF4 + min(t + INNER_NT * i, NF4 - 1)];
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const bool in = ch + u < nch;
#pragma unroll
        for (int i = 0; i < PER4; ++i) {
          acc[i].x += in ? v[u][i].x : 0.0f; acc[i].y += in ? v[u][i].y : 0.0f;
          acc[i].z += in ? v[u][i].z : 0.0f; acc[i].w += in ? v[u][i].w : 0.0f;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < PER4; ++i) {
      const int f = t + INNER_NT * i;
      if (f < NF4) {
        const int qd = f >> 8, r = ((f & 255) >> 3) + (qd == 2 ? RB : 0), c = 4 * (f & 7) + (qd >= 1 ? RB : 0);
        const float av[4] = {acc[i].x, acc[i].y, acc[i].z, acc[i].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          G[r][c + k] = av[k];
          if (qd == 1) G[c + k][r] = av[k];           // the (J, I) quadrant is the transpose
          if (!cross_only) {                          // the cross-only path keeps R in registers
            R[r][c + k] = (r == c + k) ? 1.0f : 0.0f;
            if (qd == 1) R[c + k][r] = 0.0f;
          }
        }
      }
    }
  }
  __syncthreads();
  // largest cosine between two rows of the pair, from the sums still in registers and the diagonal in LDS
  float mx = 0.0f;
  if (h_units) {
    for (int f = t; f < RP * RP; f += INNER_NT) {
      const int r = f >> 6, c = f & 63;
      if (r < c) {
        const float grr = G[r][r], gcc = G[c][c];
        if (grr > fl2 && gcc > fl2) mx = fmaxf(mx, fabsf(G[r][c]) * __builtin_amdgcn_rsqf(grr * gcc));
      }
    }
  } else {
#pragma unroll
  for (int i = 0; i < PER4; ++i) {
    const int f = t + INNER_NT * i;
    if (f < NF4) {
      const int qd = f >> 8, r = ((f & 255) >> 3) + (qd == 2 ? RB : 0), c = 4 * (f & 7) + (qd >= 1 ? RB : 0);
      const float grr = G[r][r];
      const float av[4] = {acc[i].x, acc[i].y, acc[i].z, acc[i].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gcc = G[c + k][c + k];
        if (r != c + k && grr > fl2 && gcc > fl2) mx = fmaxf(mx, fabsf(av[k]) * __builtin_amdgcn_rsqf(grr * gcc));
      }
    }
  }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_down(mx, o, 64));
  if ((t & 63) == 0) red[t >> 6] = mx;
  __syncthreads();
  __shared__ int s_skip;
  if (t == 0) {
    float m = red[0];
#pragma unroll
    for (int i = 1; i < INNER_NW; ++i) m = fmaxf(m, red[i]);
    atomicMax(maxcos_bits, __float_as_uint(m));
    // a pair whose Gram matrix is already diagonal far below the stopping cosine has nothing left to
    // rotate (the sweeps converge quadratically, so this is the whole last sweep): no solve, and the
    // apply kernel skips the pair's rows as well
    s_skip = (m < skip_thr) ? 1 : 0;
    skip_flags[(size_t)blockIdx.z * gridDim.x + p] = s_skip;
    if (h_skipT) h_skipT[(size_t)blockIdx.z * gridDim.x + p] = s_skip;       // this stage's copy, read by k_happly at the end of the super-step
  }
  __syncthreads();
  if (s_skip) return;
  if (h_units && t == 0) h_anyrot[(size_t)blockIdx.z * h_nsp + p / HU] = 1;     // this super-pair's rows do get rotated
  // two-level scheme: R also in the order k_happly's waves consume it - for the wave that owns output rows 32 hf .. of the
  // pair, lane (j, h), MFMA step kk: R[2 kk + h][32 hf + j] at ((hf * 8 + kk / 4) * 64 + j + 32 h) * 4 + kk % 4, so that four
  // steps' operands are one 16-byte load and a wave's load is 1 KB contiguous
  float* rpk = h_Rpk ? h_Rpk + ((size_t)blockIdx.z * gridDim.x + p) * RP * RP : nullptr;
  auto pk_index = [](const int r, const int c) { return (((c >> 5) * 8 + (r >> 3)) * 64 + (c & 31) + 32 * (r & 1)) * 4 + ((r >> 1) & 3); };
  // h_f16: the same 16 KB as split f16 for k_happly_h (v_mfma_f32_32x32x16_f16: lane (i, kg) holds 8 consecutive k):
  // R[k][c] = hi + lo' / 2048 (SPLIT1_FLUSHED);
  // half index ((c / 32 * 4 + k / 16) * 64 + c % 32 + 32 * (k / 8 % 2)) * 8 + k % 8, hi in the first 4096 halfs, lo' behind
  auto put_r = [&](const int r, const int c, const float v) {
    if (!h_f16) { rpk[pk_index(r, c)] = v; return; }
    _Float16* hp = reinterpret_cast<_Float16*>(rpk);
    const int idx = (((c >> 5) * 4 + (r >> 4)) * 64 + (c & 31) + 32 * ((r >> 3) & 1)) * 8 + (r & 7);
    SPLIT1_FLUSHED(v, hp[idx], hp[RP * RP + idx]);
  };
  // two-level scheme: the rotated Gram matrix (pitch RP + 1 in LDS) goes back into G_s
  auto writeback = [&](const float* gf) {
    for (int f = t; f < RP * RP / 4; f += INNER_NT) {
      const int r = f >> 4, c4 = (f & 15) * 4;
      const int gr = pair_row(r, la, lb), gc = pair_row(c4, la, lb);
      const float* q = gf + r * (RP + 1) + c4;
      *reinterpret_cast<float4*>(gs + (size_t)gr * HN + gc) = make_float4(q[0], q[1], q[2], q[3]);
    }
  };

  // Every lane computes the rotation of pair (lane & 31) - the wave's two halves redundantly - so the
  // rotation of the thread's COLUMN pair k2 is in its own registers, and those of its ROW pairs
  // kr + KR i (kr uniform per half-wave) come from lanes kr + KR i by v_readlane: no rotation table in
  // LDS, one workgroup barrier per step.
  const int k2 = t & 31;
  const int wv_s = __builtin_amdgcn_readfirstlane(t >> 6);
  const bool hi = (t & 32) != 0;
  const int kr = 2 * wv_s + (hi ? 1 : 0);
  const int n_inner = cross_only ? RB : RP - 1;           // (RP - 1 where it is used: hipcc compiles the step loop differently for a literal bound)
  float* out = Rout + (size_t)p * RP * RP;
  if (cross_only) {
    // Cross-block schedule (32 steps; every step of a sweep but the first): block-I row k meets block-J row
    // (k + step) mod 32.  R never touches LDS here: thread (kr, k2) keeps R[r][k2] (its block-I column, fixed) and
    // R[r][32 + (k2 + step) mod 32] (the block-J column of its current pair) for its rows r = kr + KR j in
    // registers; after a step the block-J values move one lane down (ds_bpermute, no LDS memory), so that every
    // lane holds the column of its next partner.  After 32 steps they are back where they started.  This takes
    // the 8 192 R accesses (half of them ds_write_b32 at 64 B/clk) out of each step's LDS time.
    float ri[2 * INNER_NB], rj[2 * INNER_NB];
#pragma unroll
    for (int j = 0; j < 2 * INNER_NB; ++j) {
      const int r = kr + INNER_KR * j;
      ri[j] = (r == k2) ? 1.0f : 0.0f;            // R starts as the identity (the LDS copy is not used on this path)
      rj[j] = (r == RB + k2) ? 1.0f : 0.0f;
    }
    const int shl = ((t & 32) | ((t + 1) & 31)) << 2;     // byte address of the lane one up within the half-wave
    // The LDS offsets of the moving (block-J) row and column are carried from step to step (add + wrap) instead of
    // rebuilt from (k + step) mod 32, and the two G buffers are compile-time bases (two steps per loop iteration): the
    // address arithmetic in front of a step's reads goes from ~35 to ~12 instructions (reads phase 490 -> 360 cycles).
    // A row pair's rotation comes by v_readlane from the lane that computed it; fetching it by ds_bpermute instead
    // saves 16 more instructions and is SLOWER (its latency sits in the step's dependent chain; 8 planes 107 -> 101).
    constexpr int PITCH = RP + 1;
    float* const gbuf0 = &GG[0][0][0];
    float* const gbuf1 = &GG[1][0][0];
    const int dp = k2 * (PITCH + 1);                       // G[p2][p2]
    int cq = RB + k2;                                      // column q2 of this step's pair
    int dq = cq * (PITCH + 1);                             // G[q2][q2]
    int rp_[INNER_NB], rq_[INNER_NB];
#pragma unroll
    for (int i = 0; i < INNER_NB; ++i) {
      rp_[i] = (kr + INNER_KR * i) * PITCH;                // row p1 (fixed)
      rq_[i] = (RB + kr + INNER_KR * i) * PITCH;           // row q1 (moves one row down per step, wraps to row 32)
    }
    auto one_step = [&](const float* __restrict__ Gs, float* __restrict__ Gd) {
      const float app = Gs[dp], aqq = Gs[dq], apq = Gs[k2 * PITCH + cq];
      float g[INNER_NB][4];
#pragma unroll
      for (int i = 0; i < INNER_NB; ++i) {
        g[i][0] = Gs[rp_[i] + k2]; g[i][1] = Gs[rp_[i] + cq]; g[i][2] = Gs[rq_[i] + k2]; g[i][3] = Gs[rq_[i] + cq];
      }
      const float tau = aqq - app, g2 = apq + apq;
      const float ta = fabsf(tau) + 1e-18f;
      const float ih = __builtin_amdgcn_rsqf(fmaf(g2, g2, ta * ta));
      const float x = fmaf(0.5f * ta, ih, 0.5f);
      const float rx = __builtin_amdgcn_rsqf(x);
      float c0 = x * rx, s0 = (apq * ih) * rx;
      const float nrm = fmaf(-0.5f, fmaf(c0, c0, s0 * s0), 1.5f);
      c0 *= nrm; s0 *= nrm;
      const bool sw = tau > 0.0f;
      const float C2 = sw ? s0 : c0, S2 = sw ? -c0 : -s0;
      const f2v cs2 = {C2, S2}, ns2 = {-S2, C2};
#pragma unroll
      for (int i = 0; i < INNER_NB; ++i) {
        const int la = 2 * wv_s + INNER_KR * i;            // the lanes that hold the row pairs' rotations (wave-uniform)
        const float C1a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(C2), la));
        const float C1b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(C2), la + 1));
        const float S1a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(S2), la));
        const float S1b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(S2), la + 1));
        const float C1 = hi ? C1b : C1a, S1 = hi ? S1b : S1a;
        // two-wide (v_pk_mul_f32 / v_pk_fma_f32): X = row p1 and Y = row q1 with the columns rotated, then the rows
        const f2v X = g[i][0] * cs2 + g[i][1] * ns2;           // (C2 gpp - S2 gpq, S2 gpp + C2 gpq)
        const f2v Y = g[i][2] * cs2 + g[i][3] * ns2;
        const f2v P = C1 * X - S1 * Y, Q = S1 * X + C1 * Y;
        Gd[rp_[i] + k2] = P.x; Gd[rp_[i] + cq] = P.y;
        Gd[rq_[i] + k2] = Q.x; Gd[rq_[i] + cq] = Q.y;
      }
#pragma unroll
      for (int j = 0; j < 2 * INNER_NB; ++j) {
        const f2v rr = ri[j] * cs2 + rj[j] * ns2;              // (C2 rp - S2 rq, S2 rp + C2 rq)
        ri[j] = rr.x;
        rj[j] = __int_as_float(__builtin_amdgcn_ds_bpermute(shl, __float_as_int(rr.y)));   // lane k2 takes lane k2 + 1's block-J column
      }
      // next step: column q2 and the rows q1 move on by one, from 63 back to 32
      const bool wc = cq == RP - 1;
      cq = wc ? RB : cq + 1;
      dq = wc ? RB * (PITCH + 1) : dq + (PITCH + 1);
#pragma unroll
      for (int i = 0; i < INNER_NB; ++i) rq_[i] = (rq_[i] == (RP - 1) * PITCH) ? RB * PITCH : rq_[i] + PITCH;
      __syncthreads();
    };
    for (int it = 0; it < RB / 2; ++it) {      // G starts in buffer 0 and is back there after an even number of steps
      one_step(gbuf0, gbuf1);
      one_step(gbuf1, gbuf0);
    }
#pragma unroll
    for (int j = 0; j < 2 * INNER_NB; ++j) {
      const int r = kr + INNER_KR * j;
      // (two-level scheme: Rout in the packed order as well - k_hupdate takes its MFMA operands straight from it)
      out[h_units ? pk_index(r, k2) : r * RP + k2] = ri[j];
      out[h_units ? pk_index(r, RB + k2) : r * RP + RB + k2] = rj[j];
      if (rpk) { put_r(r, k2, ri[j]); put_r(r, RB + k2, rj[j]); }
    }
    if (h_units) writeback(gbuf0);             // 32 steps: the result is back in buffer 0, behind the last step's barrier
    return;
  }
  // not cross_only from here on: the full 63-step round-robin schedule over the pair's 64 rows, R through LDS
  for (int step = 0; step < n_inner; ++step) {
    float (*Gn)[RP + 1] = GG[(step + 1) & 1];
    // ---- indices of this step's pairs ----
    const int a2 = rr_elem(k2, step), b2 = rr_elem(RP - 1 - k2, step);
    const int p2 = min(a2, b2), q2 = max(a2, b2);
    int p1[INNER_NB], q1[INNER_NB];
#pragma unroll
    for (int i = 0; i < INNER_NB; ++i) {
      const int k1 = kr + INNER_KR * i;
      const int a1 = rr_elem(k1, step), b1 = rr_elem(RP - 1 - k1, step);
      p1[i] = min(a1, b1); q1[i] = max(a1, b1);
    }
    // ---- every LDS read of the step, issued before the angle arithmetic ----
    const float app = G[p2][p2], aqq = G[q2][q2], apq = G[p2][q2];
    float g[INNER_NB][4], rp_[2 * INNER_NB], rq_[2 * INNER_NB];
#pragma unroll
    for (int i = 0; i < INNER_NB; ++i) {
      g[i][0] = G[p1[i]][p2]; g[i][1] = G[p1[i]][q2]; g[i][2] = G[q1[i]][p2]; g[i][3] = G[q1[i]][q2];
    }
#pragma unroll
    for (int j = 0; j < 2 * INNER_NB; ++j) {
      const int r = kr + INNER_KR * j;
      rp_[j] = R[r][p2]; rq_[j] = R[r][q2];
    }
    // ---- rotation of column pair k2 ----
    const float tau = aqq - app, g2 = apq + apq;
    const float ta = fabsf(tau) + 1e-18f;   // all-zero (padding) rows: cos = 1, sin = 0
    const float ih = __builtin_amdgcn_rsqf(fmaf(g2, g2, ta * ta));   // 1/h, h^2 = tau^2 + 4 apq^2
    const float x = fmaf(0.5f * ta, ih, 0.5f);                       // cos^2 in [0.5, 1]
    const float rx = __builtin_amdgcn_rsqf(x);
    float c0 = x * rx, s0 = (apq * ih) * rx;                         // cos, sin * sign(apq)
    // v_rsq_f32 leaves cos^2 + sin^2 a few 1e-8 off 1, always to the same side: after ~3e4 rotations
    // the rows' scale has drifted by 1e-4.  One Newton step on the pair's norm removes the bias.
    const float nrm = fmaf(-0.5f, fmaf(c0, c0, s0 * s0), 1.5f);
    c0 *= nrm; s0 *= nrm;
    const bool sw = tau > 0.0f;                                      // de Rijk: larger diagonal to p
    // X[:,p] <- C x_p - S x_q ; X[:,q] <- S x_p + C x_q   (same convention as the tile kernels)
    const float C2 = sw ? s0 : c0, S2 = sw ? -c0 : -s0;
    // ---- G <- J^T G J on the thread's 2x2 blocks (rows of pair kr + 8 i, columns of pair k2) ----
#pragma unroll
    for (int i = 0; i < INNER_NB; ++i) {
      const int la = 2 * wv_s + INNER_KR * i;                        // wave-uniform lane holding the row pair's rotation
      const float C1a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(C2), la));
      const float C1b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(C2), la + 1));
      const float S1a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(S2), la));
      const float S1b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(S2), la + 1));
      const float C1 = hi ? C1b : C1a, S1 = hi ? S1b : S1a;
      const float gpp = g[i][0], gpq = g[i][1], gqp = g[i][2], gqq = g[i][3];
      const float a0 = C2 * gpp - S2 * gpq, a1 = S2 * gpp + C2 * gpq;   // row p1, columns rotated
      const float b0 = C2 * gqp - S2 * gqq, b1 = S2 * gqp + C2 * gqq;   // row q1
      Gn[p1[i]][p2] = C1 * a0 - S1 * b0; Gn[p1[i]][q2] = C1 * a1 - S1 * b1;    // rows rotated
      Gn[q1[i]][p2] = S1 * a0 + C1 * b0; Gn[q1[i]][q2] = S1 * a1 + C1 * b1;
    }
    // ---- R <- R J : rows kr + 8 j, column pair k2 ----
#pragma unroll
    for (int j = 0; j < 2 * INNER_NB; ++j) {
      const int r = kr + INNER_KR * j;
      R[r][p2] = C2 * rp_[j] - S2 * rq_[j]; R[r][q2] = S2 * rp_[j] + C2 * rq_[j];
    }
    __syncthreads();
    G = Gn;
  }
  for (int e = t; e < RP * RP; e += INNER_NT) {
    out[h_units ? pk_index(e >> 6, e & 63) : e] = R[e >> 6][e & 63];
    if (rpk) put_r(e >> 6, e & 63, R[e >> 6][e & 63]);
  }
  if (h_units) writeback(&G[0][0]);
}

// ---------------------------------------------------------------------------
// Aug rows of the pair <- R^T x rows, one 64-column tile per workgroup.
// ---------------------------------------------------------------------------
// MFMA form (v_mfma_f32_32x32x2_f32; operand layout checked by tools/mfma_probe.hip):
//   out[i][c] = sum_k R[k][i] X[k][c],  i, k in 0..63 (the pair's rows), c = a 32-column block.
// A wave owns 32 columns: it loads the 64 x 32 block of X straight from global memory into the B
// operands (lane j + 32 h holds X[2m + h][c0 + j] for m = 0..31: two coalesced 128-byte rows per
// load), takes the A operands R[2m + h][i0 + j] from the LDS copy of R, and accumulates both row
// halves (i0 = 0, 32) in 2 x 16 accumulator registers: 64 MFMAs per block, no LDS traffic for X,
// in place (the block is fully in registers before the first store).
__global__ __launch_bounds__(256) void k_rf_apply(float* __restrict__ aug, const size_t aug_plane_stride,
                                                 const int ld, const int ncols, const int blocks_per_wave,
                                                 const int2* __restrict__ pairs, const float* __restrict__ Rall,
                                                 const int* __restrict__ skip_flags) {
  __shared__ float Rs[RP][RP + 1];      // [k][i]
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63, j = lane & 31, h = lane >> 5;
  const int p = blockIdx.x;
  if (skip_flags[(size_t)blockIdx.z * gridDim.x + p]) return;      // the inner solve found nothing to rotate
  aug += (size_t)blockIdx.z * aug_plane_stride;
  const float* Rp = Rall + ((size_t)blockIdx.z * gridDim.x + p) * RP * RP;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int e = t + 256 * i;
    Rs[e >> 6][e & 63] = Rp[e];
  }
  __syncthreads();
  const int2 pr = pairs[p];
  const size_t row_x = (size_t)(pr.x * RB + h) * ld, row_y = (size_t)(pr.y * RB + h) * ld;
  const int blk0 = (blockIdx.y * 4 + wv) * blocks_per_wave;
  for (int bk = 0; bk < blocks_per_wave; ++bk) {
    const int c0 = (blk0 + bk) * 32;
    if (c0 >= ncols) break;                        // wave-uniform
    const int col = c0 + j;
    const bool valid = col < ncols;
    const int colc = valid ? col : ncols - 1;      // loads stay unconditional (a clamped column): per-element
    const float* px = aug + row_x + colc;          // selects turn into branches that serialise the 32 loads
    const float* py = aug + row_y + colc;
    float x[32];
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      x[m] = px[(size_t)(2 * m) * ld];
      x[16 + m] = py[(size_t)(2 * m) * ld];
    }
    v16f acc0 = {0}, acc1 = {0};
#pragma unroll
    for (int m = 0; m < 32; ++m) {
      const float a0 = Rs[2 * m + h][j], a1 = Rs[2 * m + h][32 + j];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, x[m], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, x[m], acc1, 0, 0, 0);
    }
    if (valid) {
      float* ox = aug + (size_t)(pr.x * RB) * ld + col;
      float* oy = aug + (size_t)(pr.y * RB) * ld + col;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int i = ACC_ROW(v, h, 0);
        ox[(size_t)i * ld] = acc0[v];
        oy[(size_t)i * ld] = acc1[v];
      }
    }
  }
}

// squared norms of the B part (first M columns) and the Qt part of every row
__global__ __launch_bounds__(256) void k_rf_rownorms(const float* __restrict__ aug, const size_t aug_plane_stride,
                                                    const int ld, const int M, const int Lq,
                                                    double* __restrict__ b2, double* __restrict__ q2) {
  __shared__ double red[2][4];
  const int i = blockIdx.x, t = threadIdx.x;
  const int Lp = Lq;
  aug += (size_t)blockIdx.y * aug_plane_stride;
  b2 += (size_t)blockIdx.y * gridDim.x; q2 += (size_t)blockIdx.y * gridDim.x;
  const float* row = aug + (size_t)i * ld;
  double sb = 0.0, sq = 0.0;
  for (int j = t; j < M; j += 256) sb += (double)row[j] * (double)row[j];
  for (int j = t; j < Lp; j += 256) sq += (double)row[M + j] * (double)row[M + j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sb += __shfl_down(sb, o, 64); sq += __shfl_down(sq, o, 64); }
  if ((t & 63) == 0) { red[0][t >> 6] = sb; red[1][t >> 6] = sq; }
  __syncthreads();
  if (t == 0) {
    b2[i] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    q2[i] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

// t2[i] = sum_j T[j][i]^2 (float64) of the dense [rows x cols] matrix T of every plane
__global__ __launch_bounds__(256) void k_rf_colnorms(const float* __restrict__ T, const size_t plane_stride,
                                                    const int rows, const int cols, double* __restrict__ t2) {
  __shared__ double red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rs = threadIdx.x >> 6;
  T += (size_t)blockIdx.y * plane_stride;
  double acc = 0.0;
  if (c < cols)
    for (int j = rs; j < rows; j += 4) { const double v = (double)T[(size_t)j * cols + c]; acc += v * v; }
  red[rs][threadIdx.x & 63] = acc;
  __syncthreads();
  if (rs == 0 && c < cols) t2[(size_t)blockIdx.y * cols + c] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// rows of the B part scaled in place:  B[i][:] *= d[i]
__global__ void k_rf_scale_rows(float* __restrict__ aug, const size_t aug_plane_stride, const int ld,
                                const int M, const float* __restrict__ d) {
  const int i = blockIdx.y;
  aug += (size_t)blockIdx.z * aug_plane_stride;
  const float s = d[(size_t)blockIdx.z * gridDim.y + i];
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < M; j += gridDim.x * blockDim.x)
    aug[(size_t)i * ld + j] *= s;
}

// Yw (float, logical A layout L x M or its transpose) -> clip/truncate -> uint8 plane; optional float copy
__global__ void k_rf_quant(const float* __restrict__ yw, const size_t yw_plane_stride, const int ldy,
                           const int transpose, uint8_t* __restrict__ dst, const size_t dst_stride,
                           const size_t dst_plane_stride, float* __restrict__ ywout, const int H, const int W) {
  const int r = blockIdx.y;
  yw += (size_t)blockIdx.z * yw_plane_stride;
  dst += (size_t)blockIdx.z * dst_plane_stride;
  if (ywout) ywout += (size_t)blockIdx.z * (size_t)H * W;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < W; c += gridDim.x * blockDim.x) {
    const float v = transpose ? yw[(size_t)c * ldy + r] : yw[(size_t)r * ldy + c];
    if (ywout) ywout[(size_t)r * W + c] = v;
    dst[(size_t)r * dst_stride + c] = (uint8_t)(unsigned)fminf(fmaxf(v, 0.0f), 255.0f);
  }
}

// gather sorted, normalised factors:  out[k][:] = src_row[order[k]][:] * scale[k]
__global__ void k_rf_gather_rows(const float* __restrict__ src, const int ld, const int ncols,
                                 const int* __restrict__ order, const float* __restrict__ scale,
                                 float* __restrict__ dst, const int ldd) {
  const int k = blockIdx.y;
  const float* row = src + (size_t)order[k] * ld;
  const float s = scale[k];
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < ncols; j += gridDim.x * blockDim.x)
    dst[(size_t)k * ldd + j] = row[j] * s;
}

// the sorted, normalised factors of all planes of a batch (grid.z = plane):
//   straight:    dst[z][k][c] = src[z][order[z][k]][c] * scale[z][k]          (grid: column blocks x rows k)
//   transposing: dst[z][c][k] = src[z][order[z][k]][c] * scale[z][k]          (32 x 32 tiles through LDS, both sides coalesced)
__global__ void k_rf_gather_rows_b(const float* __restrict__ src, const size_t src_ps, const int ld, const int ncols,
                                   const int* __restrict__ order, const float* __restrict__ scale, const int os,
                                   float* __restrict__ dst, const size_t dst_ps, const int ldd) {
  const int k = blockIdx.y, z = blockIdx.z;
  const float* row = src + (size_t)z * src_ps + (size_t)order[(size_t)z * os + k] * ld;
  const float sc = scale[(size_t)z * os + k];
  float* d = dst + (size_t)z * dst_ps + (size_t)k * ldd;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < ncols; j += gridDim.x * blockDim.x) d[j] = row[j] * sc;
}

__global__ __launch_bounds__(256) void k_rf_gather_rows_t(const float* __restrict__ src, const size_t src_ps, const int ld, const int ncols,
                                                         const int nk, const int* __restrict__ order, const float* __restrict__ scale,
                                                         const int os, float* __restrict__ dst, const size_t dst_ps, const int ldd) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, z = blockIdx.z;
  const int c0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  src += (size_t)z * src_ps; dst += (size_t)z * dst_ps; order += (size_t)z * os; scale += (size_t)z * os;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = k0 + ty + 8 * i, c = c0 + tx;
    tile[ty + 8 * i][tx] = (k < nk && c < ncols) ? src[(size_t)order[k] * ld + c] * scale[k] : 0.0f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, k = k0 + tx;
    if (c < ncols && k < nk) dst[(size_t)c * ldd + k] = tile[tx][ty + 8 * i];
  }
}

// rows of a dense [n][ncols] matrix into chosen slots of a gathered factor:  dst[pos[k] * ld_slot + j * ld_elem] = src[k][j]
// (ld_elem = 1: the slot is a row of Vt;  ld_slot = 1: the slot is a column of U)
__global__ void k_rf_put_rows(const float* __restrict__ src, const int ncols, const int* __restrict__ pos,
                              float* __restrict__ dst, const size_t ld_slot, const size_t ld_elem) {
  const int k = blockIdx.y;
  float* d = dst + (size_t)pos[k] * ld_slot;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < ncols; j += gridDim.x * blockDim.x)
    d[(size_t)j * ld_elem] = src[(size_t)k * ncols + j];
}

// deterministic pseudo-random pattern in (-1, 1): the start vectors of the null-space completion
// (rank-deficient planes); element (r, c) of the matrix with seed `seed`
__global__ void k_rf_pattern(float* __restrict__ dst, const int cols, const unsigned seed) {
  const int r = blockIdx.y;          // grid.y = rows
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += gridDim.x * blockDim.x) {
    unsigned h = (unsigned)r * 0x9E3779B1u ^ ((unsigned)c + seed) * 0x85EBCA77u;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    dst[(size_t)r * cols + c] = (float)(h >> 8) * (2.0f / 16777216.0f) - 1.0f;
  }
}

// dst[r][k] = src[r][k] * d[k]   (rows x cols, dense, batch = grid.z with strides)
__global__ void k_rf_scale_cols_b(const float* __restrict__ src, const size_t s_src, float* __restrict__ dst,
                                  const size_t s_dst, const int cols, const float* __restrict__ d, const size_t s_d) {
  const int r = blockIdx.y;
  src += (size_t)blockIdx.z * s_src; dst += (size_t)blockIdx.z * s_dst; d += (size_t)blockIdx.z * s_d;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < cols; k += gridDim.x * blockDim.x)
    dst[(size_t)r * cols + k] = src[(size_t)r * cols + k] * d[k];
}

// The guard of the split-f16 reconstruct: the largest squared row norm of U[:n,:n] (leading dimension lu) into mx[0] and the
// largest squared column norm of V[:n,:n] (leading dimension lv) into mx[1], as float bits (non-negative floats and NaN order
// like their bits; the caller zeroes mx).  Blocks below nbu take four rows of U, a wave each; the others 16 columns of V in 16
// row phases.  Fixed summation order: the same factors give the same bits.
__global__ __launch_bounds__(256) void k_rf_corner_norms(const float* __restrict__ U, const int lu, const float* __restrict__ V,
                                                          const int lv, const int n, const int nbu, unsigned* __restrict__ mx) {
  __shared__ float part[16][17];
  __shared__ unsigned colmax[16];
  const int t = threadIdx.x;
  if ((int)blockIdx.x < nbu) {
    const int r = 4 * blockIdx.x + (t >> 6);
    float s = 0.0f;
    if (r < n)
      for (int k = t & 63; k < n; k += 64) { const float u = U[(size_t)r * lu + k]; s = fmaf(u, u, s); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((t & 63) == 0 && r < n) atomicMax(&mx[0], __float_as_uint(s));
    return;
  }
  const int c = 16 * ((int)blockIdx.x - nbu) + (t & 15), ph = t >> 4;
  float s0 = 0.0f, s1 = 0.0f;
  if (c < n) {
    int k = ph;
    for (; k + 16 < n; k += 32) {
      const float a = V[(size_t)k * lv + c], b = V[(size_t)(k + 16) * lv + c];
      s0 = fmaf(a, a, s0); s1 = fmaf(b, b, s1);
    }
    if (k < n) { const float a = V[(size_t)k * lv + c]; s0 = fmaf(a, a, s0); }
  }
  part[ph][t & 15] = s0 + s1;
  __syncthreads();
  if (t < 16) {
    float s = 0.0f;
    for (int i = 0; i < 16; ++i) s += part[i][t];
    colmax[t] = __float_as_uint(s);
  }
  __syncthreads();
  if (t == 0) {
    unsigned m = 0;
    for (int i = 0; i < 16; ++i) m = colmax[i] > m ? colmax[i] : m;
    atomicMax(&mx[1], m);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct RefPlan {
  int H, W, L, M, Lp, ld, nbk, npairs, nsteps, nch, B;
  int apply_tiles;       // 32-column blocks per wave of an apply workgroup (4 waves)
  size_t aug_ps;         // floats between the Aug matrices of consecutive planes
  bool transpose;        // A = plane^T (portrait planes: the short side must index rows)
};

// Every WM_RF_* environment knob, with its default and its range.  The values are read where they were always read - at
// the start of the call that uses them: tests switch WM_RF_HIER*, WM_RF_QUEUES, WM_RF_HGRAM3 and WM_RF_FINAL_F16 between
// calls on one context - except the three marked "process", which keep what the first call saw.
struct RefKnobs {
  int apply_tiles, full_sweeps, queues, hier, hier_f16, hier_sb, hgram3;
  float conv_sigma;
  bool drift_cal, debug_drift, final_f16;
};

RefKnobs ref_knobs() {
  auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
  auto flag = [](const char* name) { const char* e = getenv(name); return e ? (atoi(e) != 0 ? 1 : 0) : -1; };     // -1: unset
  static const int full_sweeps = num("WM_RF_FULL_SWEEPS", FULL_INNER_SWEEPS);                        // process
  static const float conv_sigma = getenv("WM_RF_CONV_SIGMA") ? (float)atof(getenv("WM_RF_CONV_SIGMA")) : CONV_COS_SIGMA;   // process
  static const bool drift_cal = flag("WM_RF_DRIFT_CAL") != 0;                                        // process; 0: rows below the switch stay uncalibrated
  RefKnobs k;
  k.full_sweeps = full_sweeps; k.conv_sigma = conv_sigma; k.drift_cal = drift_cal;
  k.apply_tiles = num("WM_RF_APPLY_TILES", 1);                  // 1..8: 32-column blocks per wave of k_rf_apply (tuning)
  if (k.apply_tiles < 1 || k.apply_tiles > 8) k.apply_tiles = 1;
  k.debug_drift = getenv("WM_RF_DEBUG_DRIFT") != nullptr;       // set: print each plane's drift factors
  // plane groups (HIP queues) 1..1 + MAX_AUX, WM_RF_ONE_QUEUE=1 is the old spelling of 1; 0: by batch size
  k.queues = flag("WM_RF_ONE_QUEUE") == 1 ? 1 : std::min(std::max(num("WM_RF_QUEUES", 0), 0), 1 + wm_ctx::MAX_AUX);
  k.hier = flag("WM_RF_HIER");                                  // 0 / 1: the flat tournament / the two-level scheme; unset: by batch size
  k.hier_f16 = num("WM_RF_HIER_F16", HIER_F16_DEFAULT);         // bit 0: Gram tiles, bit 1: rotation products from split-f16 operands
  k.hier_sb = num("WM_RF_HIER_SB", 6);                          // 2, 4 or 6 blocks per super-block
  if (k.hier_sb != 2 && k.hier_sb != 4 && k.hier_sb != 6) k.hier_sb = 6;
  k.hgram3 = flag("WM_RF_HGRAM3");                              // 0 / 1: never / always k_hgram_h3 where it applies; unset: where it fills the chip
  k.final_f16 = flag("WM_RF_FINAL_F16") != 0;                   // 0 keeps the finalisation's large products in f32
  return k;
}

RefPlan make_plan(int H, int W, int B = 1) {
  RefPlan p;
  p.H = H; p.W = W; p.B = B;
  p.transpose = H > W;
  p.L = std::min(H, W); p.M = std::max(H, W);
  p.Lp = (p.L + RP - 1) / RP * RP;
  p.ld = (p.M + p.Lp + 3) & ~3;
  p.aug_ps = (size_t)p.Lp * p.ld;
  p.nbk = p.Lp / RB; p.npairs = p.nbk / 2; p.nsteps = p.nbk - 1;
  // Work per workgroup grows with the batch: with many planes in a launch the grid is large anyway,
  // so a workgroup takes more columns (R / partial-sum traffic amortised, loads pipelined); a single
  // plane keeps the small units that fill the chip.
  // (round 2 gave a workgroup two 32-column blocks per wave from 96 (pair, plane) items per step on; with the batch split
  // into two or three plane groups a launch rarely gets there, and one block per wave measures the same or better at every
  // batch size: 8 planes 106.8 / 106.4, 16 planes 139.3 / 137.2, 24 planes 140.4 / 139.4 frames/s - profiles/r03z_fullframe_queues.log)
  p.apply_tiles = ref_knobs().apply_tiles;
  p.nch = (p.M + GRAM_CC - 1) / GRAM_CC;    // Gram stays in many small units: a float4 / double-buffered / 512-column variant measured slower (36-40 vs 31 us)
  return p;
}

struct RefWs {           // carved out of a grow-only context buffer; every per-plane array is [B][...]
  float* aug; float* partials; float* R; const int2* pairs; unsigned* maxcos; float* floor2; int* skip; double* b2; double* q2;
  float* dvec; int* order; float* scale; float* tmp1; float* tmp2;
  float* a0; float* t;   // plan_decompose_ws: tmp2 split into A0 (the embed's Yw) [B][L][M] | T = A0 B^T [B][L][Lp]
};

// The round-robin tournament of a plan depends on its block count only: built once per context and
// block count (a handful of sizes per process), kept on the device, handed out without a copy or a sync.
int get_pairs(wm_ctx* ctx, const RefPlan& p, const int2** out) {
  for (int i = 0; i < wm_ctx::MAX_PAIR_TABS; ++i)
    if (ctx->pair_tab[i] && ctx->pair_tab_nbk[i] == p.nbk) { *out = (const int2*)ctx->pair_tab[i]; return WM_OK; }
  int slot = -1;
  for (int i = 0; i < wm_ctx::MAX_PAIR_TABS; ++i) if (!ctx->pair_tab[i]) { slot = i; break; }
  if (slot < 0) {                                   // full: recycle round-robin (nothing in flight may still read it)
    slot = ctx->pair_tab_next; ctx->pair_tab_next = (ctx->pair_tab_next + 1) % wm_ctx::MAX_PAIR_TABS;
    WM_HIP(hipStreamSynchronize(ctx->stream));
    WM_HIP(hipFree(ctx->pair_tab[slot]));
    ctx->pair_tab[slot] = nullptr;
  }
  std::vector<int2> tab((size_t)p.nsteps * p.npairs);
  std::vector<int> idx(p.nbk);
  std::iota(idx.begin(), idx.end(), 0);
  for (int s = 0; s < p.nsteps; ++s) {
    for (int k = 0; k < p.npairs; ++k) {
      const int a = idx[k], b = idx[p.nbk - 1 - k];
      tab[(size_t)s * p.npairs + k] = make_int2(std::min(a, b), std::max(a, b));
    }
    const int last = idx[p.nbk - 1];
    for (int j = p.nbk - 1; j > 1; --j) idx[j] = idx[j - 1];
    idx[1] = last;
  }
  if (hipMalloc(&ctx->pair_tab[slot], std::max<size_t>(tab.size(), 1) * sizeof(int2)) != hipSuccess) {
    (void)hipGetLastError();
    ctx->pair_tab[slot] = nullptr;
    return set_err(WM_ERR_NOMEM, "hipMalloc failed for %s", "pair table");
  }
  if (!tab.empty()) {
    WM_HIP(hipMemcpyAsync(ctx->pair_tab[slot], tab.data(), tab.size() * sizeof(int2), hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));     // tab is a local
  }
  ctx->pair_tab_nbk[slot] = p.nbk;
  *out = (const int2*)ctx->pair_tab[slot];
  return WM_OK;
}

// which = 0: the context's main full-frame workspace; 1: the second one (null-space completion, so that the
// first call's arrays stay where they are)
int plan_workspace(wm_ctx* ctx, const RefPlan& p, RefWs& w, size_t extra_f32_a, size_t extra_f32_b, int which = 0) {
  const size_t B = (size_t)p.B;
  auto lay = [&](Carve& cv) {
    w.aug = cv.take<float>(B * p.aug_ps); w.partials = cv.take<float>(B * p.npairs * p.nch * GRAM_PART);
    w.R = cv.take<float>(B * p.npairs * RP * RP);
    w.maxcos = cv.take<unsigned>(B + 64); w.floor2 = cv.take<float>(B + 64);
    w.skip = cv.take<int>(B * p.npairs + (size_t)(2 + wm_ctx::MAX_AUX) * 64); w.b2 = cv.take<double>(B * p.Lp); w.q2 = cv.take<double>(B * p.Lp);
    w.dvec = cv.take<float>(2 * B * p.Lp); w.order = cv.take<int>((size_t)p.Lp); w.scale = cv.take<float>((size_t)p.Lp);
    w.tmp1 = cv.take<float>(extra_f32_a); w.tmp2 = cv.take<float>(extra_f32_b);
  };
  if (which == 0) WM_TRY(staged(ctx, &ctx->ref_ws, &ctx->ref_ws_bytes, "full-frame workspace", lay));
  else WM_TRY(staged(ctx, &ctx->ref_ws2, &ctx->ref_ws2_bytes, "full-frame completion workspace", lay));
  w.a0 = w.t = nullptr;
  WM_TRY(get_pairs(ctx, p, &w.pairs));
  return WM_OK;
}

// the main workspace of a call that decomposes uint8 planes: tmp2 holds A0 [B][L][M] | T [B][L][Lp] (and min_f32_b floats
// at least, for what the call keeps there afterwards), handed out as w.a0 and w.t
int plan_decompose_ws(wm_ctx* ctx, const RefPlan& p, RefWs& w, size_t extra_f32_a, size_t min_f32_b = 0) {
  const size_t n_a0 = (size_t)p.B * p.L * p.M;
  WM_TRY(plan_workspace(ctx, p, w, extra_f32_a, std::max(n_a0 + (size_t)p.B * p.L * p.Lp, min_f32_b)));
  w.a0 = w.tmp2; w.t = w.tmp2 + n_a0;
  return WM_OK;
}

// orthonormal DCT-II basis D_n (float64 on the host, rounded to float32) into cache slot `slot`
int fill_dct(wm_ctx* ctx, int n, int slot) {
  if (ctx->dct_mat[slot]) {
    WM_HIP(hipStreamSynchronize(ctx->stream));
    WM_HIP(hipFree(ctx->dct_mat[slot]));
    ctx->dct_mat[slot] = nullptr; ctx->dct_n[slot] = 0;
  }
  if (hipMalloc((void**)&ctx->dct_mat[slot], (size_t)2 * n * n * 4) != hipSuccess) {       // D, then D^T (row-major A operand of the split-f16 inverse DCT)
    (void)hipGetLastError();
    return set_err(WM_ERR_NOMEM, "hipMalloc failed for %s", "DCT basis");
  }
  std::vector<float> D((size_t)2 * n * n);
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < n; ++k) {
    const double s = (k == 0) ? sqrt(1.0 / n) : sqrt(2.0 / n);
    for (int m = 0; m < n; ++m) D[(size_t)n * n + (size_t)m * n + k] = D[(size_t)k * n + m] = (float)(s * cos(pi * (2.0 * m + 1.0) * k / (2.0 * n)));
  }
  WM_HIP(hipMemcpyAsync(ctx->dct_mat[slot], D.data(), D.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  ctx->dct_n[slot] = n;
  return WM_OK;
}

// D_H and D_W of one plane, from the two-slot per-context cache.  Both are resolved in ONE
// call: a slot that already holds one of the two sizes is never the one evicted for the other
// (fetching them one after the other could free the matrix just handed out - found by the
// re-entrancy test, which ran 96x128 on a context whose cache held 64 and 96).
int get_dct_pair(wm_ctx* ctx, int H, int W, float** dH, float** dW) {
  int sh = -1, sw = -1;
  for (int i = 0; i < 2; ++i) {
    if (ctx->dct_mat[i] && ctx->dct_n[i] == H && sh < 0) sh = i;
    if (ctx->dct_mat[i] && ctx->dct_n[i] == W && sw < 0) sw = i;
  }
  if (sh < 0) {
    sh = (sw == 0) ? 1 : 0;                      // any slot that does not hold W
    WM_TRY(fill_dct(ctx, H, sh));
    if (H == W) sw = sh;
  }
  if (sw < 0) {
    sw = 1 - sh;                                 // the slot that does not hold H
    WM_TRY(fill_dct(ctx, W, sw));
  }
  *dH = ctx->dct_mat[sh];
  *dW = ctx->dct_mat[sw];
  return WM_OK;
}

#include "wm_ref_hier.inc"

// (NULL_ROW_RATIO * |A|_F)^2 of one plane from the squared norms of its Lp rows: the numerical-null floor.  Rotations
// preserve the Frobenius norm, so the rotated rows give the same floor as the loaded input.
double null_floor2(const double* row2, const int Lp) {
  double f2 = 0.0;
  for (int i = 0; i < Lp; ++i) f2 += row2[i];
  return NULL_ROW_RATIO * NULL_ROW_RATIO * f2;
}

// numerical-null floor per plane into w.floor2, from the row norms of the loaded input
int load_null_floors(wm_ctx* ctx, const RefPlan& p, const RefWs& w) {
  hipLaunchKernelGGL(k_rf_rownorms, dim3(p.Lp, p.B), dim3(256), 0, ctx->stream, w.aug, p.aug_ps, p.ld, p.M, 0, w.b2, w.q2);
  std::vector<double> r2((size_t)p.B * p.Lp);
  WM_HIP(hipMemcpyAsync(r2.data(), w.b2, r2.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<float> fl(p.B);
  for (int z = 0; z < p.B; ++z) fl[z] = (float)null_floor2(&r2[(size_t)z * p.Lp], p.Lp);
  WM_HIP(hipMemcpyAsync(w.floor2, fl.data(), fl.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));       // fl is a local
  return WM_OK;
}

struct JacobiRun {                       // what one jacobi_rows call fixes for all its sweeps
  RefKnobs k;
  int ncols;                             // columns the rotations are applied to: A, and the accumulated factor of JR_SVD
  float skip_thr;
  int NQ, zb[2 + wm_ctx::MAX_AUX];       // plane groups: group g owns planes [zb[g], zb[g + 1]) and runs on queue g
  bool gram_f16, apply_f16;              // two-level scheme: which of its products take split-f16 operands
  const HierTab* ht; HierWs hw;          // ... its tables and workspace
  hipStream_t q(const wm_ctx* ctx, int g) const { return g == 0 ? ctx->stream : ctx->aux_stream[g - 1]; }
};

// one sweep of the flat tournament.  A step is gram -> inner -> apply, and k_rf_inner is one latency-bound workgroup per
// block pair (~35 us with most of the chip idle): group g starts one gram after group g - 1, so that the groups' inner
// solves fall under each other's gram / apply tiles instead of all at the same time
int flat_sweep(wm_ctx* ctx, const RefPlan& p, const RefWs& w, const JacobiRun& r, int sweep) {
  const size_t par_ps = (size_t)p.npairs * p.nch * GRAM_PART, r_ps = (size_t)p.npairs * RP * RP;
  auto step = [&](int g, int s, int part) {       // part: 1 = gram, 2 = inner + apply
    const hipStream_t st = r.q(ctx, g);
    const int z0 = r.zb[g], nz = r.zb[g + 1] - r.zb[g];
    const int2* pr = w.pairs + (size_t)s * p.npairs;
    float* aug = w.aug + (size_t)z0 * p.aug_ps;
    float* par = w.partials + (size_t)z0 * par_ps;
    float* R = w.R + (size_t)z0 * r_ps;
    if (part & 1)
      hipLaunchKernelGGL(k_rf_gram, dim3(p.npairs, p.nch, nz), dim3(256), 0, st, aug, p.aug_ps, p.ld, p.M, pr, par);
    if (part & 2) {
      hipLaunchKernelGGL(k_rf_inner, dim3(p.npairs, 1, nz), dim3(INNER_NT), 0, st, par, p.nch, R, w.maxcos + z0,
                         w.floor2 + z0, (s == 0 || sweep < r.k.full_sweeps) ? 0 : 1, hier_flag_base(w.skip, (size_t)p.npairs, z0, g),
                         r.skip_thr, (const int*)nullptr, (float*)nullptr, (int*)nullptr, 0, (float*)nullptr, (int*)nullptr, 0);
      const int n_blk = (r.ncols + 31) / 32, per_wg = 4 * p.apply_tiles;     // 32-column blocks, 4 waves per workgroup
      hipLaunchKernelGGL(k_rf_apply, dim3(p.npairs, (n_blk + per_wg - 1) / per_wg, nz), dim3(256), 0, st,
                         aug, p.aug_ps, p.ld, r.ncols, p.apply_tiles, pr, R, hier_flag_base(w.skip, (size_t)p.npairs, z0, g));
    }
  };
  for (int g = 0; g < r.NQ; ++g) {
    if (g > 0) WM_HIP(hipStreamWaitEvent(r.q(ctx, g), ctx->ev_fork[g - 1], 0));
    step(g, 0, 1);
    if (g + 1 < r.NQ) WM_HIP(hipEventRecord(ctx->ev_fork[g], r.q(ctx, g)));
  }
  for (int g = 0; g < r.NQ; ++g) step(g, 0, 2);
  for (int s = 1; s < p.nsteps; ++s)
    for (int g = 0; g < r.NQ; ++g) step(g, s, 3);
  return WM_OK;
}

// one sweep of the two-level scheme (wm_ref_hier.inc): the same rotations with the rows streamed 3 times per SUPER-step
int hier_sweep(wm_ctx* ctx, const RefPlan& p, const RefWs& w, const JacobiRun& r) {
  const HierTab* ht = r.ht;
  const HierWs& hw = r.hw;
  for (int g = 1; g < r.NQ; ++g) {               // the other queues start behind the sweep's memset
    if (g == 1) WM_HIP(hipEventRecord(ctx->ev_fork[0], ctx->stream));
    WM_HIP(hipStreamWaitEvent(r.q(ctx, g), ctx->ev_fork[0], 0));
  }
  for (int s1 = 0; s1 < ht->nsteps1; ++s1)
    for (int g = 0; g < r.NQ; ++g) {               // super-step s1 of plane group g
      const hipStream_t st = r.q(ctx, g);
      const int z0 = r.zb[g], nz = r.zb[g + 1] - r.zb[g], nsp = ht->nsp;
      const HSuper* sup = ht->d_super + (size_t)s1 * nsp;
      float* aug = w.aug + (size_t)z0 * p.aug_ps;
      float* Gs = hw.Gs + (size_t)z0 * nsp * HN * HN;
      float* R = hw.R + (size_t)z0 * nsp * HU * RP * RP;
      float* par = hw.partials + (size_t)z0 * nsp * HG_TILES * hw.KS * HG_T * HG_T;
      int* skip = hier_flag_base(hw.skip, (size_t)nsp * HU, z0, g);
      int* anyrot = hier_flag_base(hw.anyrot, (size_t)nsp, z0, g);
      // per-stage rotations (packed) and skip flags of this group's planes: [stage][plane][super-pair * HU + unit]
      float* Rpk = hw.Rpk + (size_t)z0 * HT_MAX * nsp * HU * RP * RP;
      int* skipT = hier_flag_base(hw.skipT, (size_t)HT_MAX * nsp * HU, z0, g);
      const size_t rpk_stage = (size_t)nz * nsp * HU * RP * RP, skip_stage = (size_t)nz * nsp * HU;
      const int n32 = ht->nmax * RB, npmax = (n32 + HG_T - 1) / HG_T;
      const int nchunk = (p.M + HG_KC - 1) / HG_KC;
      // (one workgroup per (super-pair, plane, split) instead of three: only where that still fills the chip - from 11 planes per launch on;
      //  16 planes on three queues: 209 against 213 frames/s with it, 64 planes: 308 against 297)
      const bool h3 = r.k.hgram3 >= 0 ? r.k.hgram3 != 0 : nsp * hw.KS * nz >= 256;
      const bool use_h3 = r.gram_f16 && npmax == 3 && h3;     // (its column splits weigh more: every split writes the whole upper triangle - 2.0 against 0.25: +2 % at 64 and 128 planes)
      const int KS = hier_ks(nsp, nz, use_h3 ? 1 : npmax, nchunk, hw.KS, use_h3 ? 2.0 : 0.25), cps = (nchunk + KS - 1) / KS;
      const int ngrp = nsp * KS * nz;               // (super-pair, split, plane) groups of npmax workgroups, dealt over the XCDs
      // Gram tiles on the f16 matrix pipe with split operands (k_hgram_t<true>; WM_RF_HIER_F16=0: the f32 instance)
      if (use_h3)                                     // three panels: the rows fetched once per chunk (k_hgram_h3)
        hipLaunchKernelGGL(k_hgram_h3, dim3(((ngrp + 7) / 8) * 8), dim3(H3_NT), 0, st, aug, p.aug_ps, p.ld, p.M, sup, nsp,
                           par, KS, cps, nz);
      else if (r.gram_f16)
        hipLaunchKernelGGL(k_hgram_t<true>, dim3(((ngrp + 7) / 8) * 8 * npmax), dim3(512), 0, st, aug, p.aug_ps, p.ld, p.M, sup, nsp,
                           par, KS, cps, npmax, nz);
      else
        hipLaunchKernelGGL(k_hgram_t<false>, dim3(((ngrp + 7) / 8) * 8 * npmax), dim3(512), 0, st, aug, p.aug_ps, p.ld, p.M, sup, nsp,
                           par, KS, cps, npmax, nz);
      hipLaunchKernelGGL(k_hreduce, dim3(HSB * (HSB + 1) / 2, nsp, nz), dim3(256), 0, st, par, sup, nsp, KS, Gs, anyrot);
      constexpr int NG = HU * (HU - 1) / 2;
      const int T = ht->T[s1];
      const int* un0 = ht->d_units + (size_t)ht->stage_off[s1] * nsp * HU;
      for (int t = 0; t < T; ++t) {
        const int* un = un0 + (size_t)t * nsp * HU;
        hipLaunchKernelGGL(k_rf_inner, dim3(nsp * HU, 1, nz), dim3(INNER_NT), 0, st, (const float*)nullptr, 0, R, w.maxcos + z0,
                           w.floor2 + z0, (s1 == 0 && t == 0) ? 0 : 1, skip, r.skip_thr, un, Gs, anyrot, nsp, Rpk + t * rpk_stage,
                           skipT + t * skip_stage, r.apply_f16 ? 1 : 0);
        if (t + 1 < T)                               // nothing reads G_s after the last stage
          hipLaunchKernelGGL(k_hupdate, dim3(NG, nsp, nz), dim3(256), 0, st, un, sup, nsp, R, skip, Gs);
      }
      const int ntask = nsp * nz * ((r.ncols + 63) / 64);
      if (r.apply_f16)
        hipLaunchKernelGGL((k_happly_h<64>), dim3(8 * ((ntask + 7) / 8)), dim3(64 * ht->nmax), (size_t)2 * 64 * HA_CP * 2, st, aug, p.aug_ps, p.ld,
                           r.ncols, sup, nsp, nz, un0, T, Rpk, skipT, rpk_stage, skip_stage, anyrot);
      else
        hipLaunchKernelGGL(k_happly, dim3(8 * ((ntask + 7) / 8)), dim3(64 * ht->nmax), (size_t)n32 * 65 * 4, st, aug, p.aug_ps, p.ld, r.ncols,
                           sup, nsp, nz, un0, T, Rpk, skipT, rpk_stage, skip_stage, anyrot);
    }
  return WM_OK;
}

// block one-sided Jacobi on the B Aug matrices (already loaded); every launch covers
// a group of planes (grid.z), sweeps continue until every plane's Gram matrices are
// diagonal to CONV_COS.  sweeps_out: sweeps used (negative: bound hit).
// what the rotated rows are needed for: their norms only (extract / detect), their directions too (embed:
// u_i, v_i enter the stego), or the accumulated left factor as well (watermark-side SVD, [A | I])
// JR_ORTH: orthogonalise the rows only (null-space completion): no left factor, the tight stopping cosine
enum JacobiUse { JR_SIGMA, JR_EMBED, JR_SVD, JR_ORTH };

int jacobi_rows(wm_ctx* ctx, const RefPlan& p, const RefWs& w, const JacobiUse use, int* sweeps_out) {
  const bool with_q = use == JR_SVD;
  JacobiRun r{};
  r.k = ref_knobs();
  r.ncols = with_q ? p.M + p.Lp : p.M;
  // plane groups (HIP queues), by default two, three from 12 planes on (16 planes: 131 -> 137 frames/s on two boxes, 24: 138 -> 139; 8 planes: 107 / 106)
  const int max_queues = r.k.queues ? r.k.queues : std::min(1 + wm_ctx::MAX_AUX, p.B >= 12 ? DEFAULT_QUEUES + 1 : DEFAULT_QUEUES);
  // The accumulated factor of JR_SVD needs every rotation; the other two uses stop earlier: a residual
  // cosine c moves the stego by c * s_max / s_i of a (sub-LSB) term and the singular values by the
  // bounds documented at fetch_norms_t, the same for embed and extract so that it cancels in S_cw - Sc.
  const float conv_cos = (with_q || use == JR_ORTH) ? CONV_COS : r.k.conv_sigma;
  r.skip_thr = SKIP_FRACTION * conv_cos;
  ctx->ref_skip_thr = r.skip_thr;
  r.NQ = std::min(max_queues, p.B);
  for (int g = 0; g <= r.NQ; ++g) r.zb[g] = (int)((long long)g * p.B / r.NQ);
  for (int g = 1; g < r.NQ; ++g)
    if (!ctx->aux_stream[g - 1]) {
      WM_HIP(hipStreamCreateWithFlags(&ctx->aux_stream[g - 1], hipStreamNonBlocking));
      WM_HIP(hipEventCreateWithFlags(&ctx->ev_fork[g - 1], hipEventDisableTiming));
      WM_HIP(hipEventCreateWithFlags(&ctx->ev_join[g - 1], hipEventDisableTiming));
    }
  WM_TRY(load_null_floors(ctx, p, w));
  // Flat or two-level by default (measured on 1080p planes, profiles/r04_hier_crossover.log): with the split-f16 kernels - uint8 planes, i.e. every
  // embed / sigma / extract / detect call - the two-level scheme wins from 4 planes per call on (2: 44 / 44, 4: 72 / 79, 8: 104 / 128,
  // 16: 138 / 180, 64: 140 / 242 frames/s flat / two-level) and is used from HIER_MIN_PLANES_F16 = 3; with the f32 kernels (float
  // inputs: the watermark-side SVD, the completion) only from HIER_MIN_PLANES = 20 (2 planes: 20.9 / 26.5 ms - a small batch is
  // latency-bound and the flat step's chain gram - inner - apply is the shorter one).
  // Row entries of uint8 planes are bounded by 255 sqrt(L) < 65 504 under orthogonal rotations: beyond L = 65 536 (never a plane)
  // f16 would overflow, and float inputs (the watermark-side SVD of a DCT plane, the completion's random vectors) have no such
  // bound - those uses keep the f32 kernels.
  const bool f16_ok = use == JR_SIGMA || use == JR_EMBED;
  r.gram_f16 = (r.k.hier_f16 & 1) && f16_ok; r.apply_f16 = (r.k.hier_f16 & 2) && f16_ok;
  const bool hier = r.k.hier >= 0 ? r.k.hier != 0 : p.B >= ((r.gram_f16 && r.apply_f16) ? HIER_MIN_PLANES_F16 : HIER_MIN_PLANES);
  if (hier) {
    WM_TRY(get_hier(ctx, p.nbk, r.k.hier_sb, &r.ht));
    WM_TRY(plan_hier_ws(ctx, p, *r.ht, r.hw));
    if (!ctx->hier_attr_set) {                     // per context: the limit belongs to the device the context made current
      WM_HIP(hipFuncSetAttribute((const void*)k_happly, hipFuncAttributeMaxDynamicSharedMemorySize, HN * 65 * 4));
      WM_HIP(hipFuncSetAttribute((const void*)k_happly_h<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 64 * HA_CP * 2));
      ctx->hier_attr_set = true;
    }
  }
  int sweep = 0;
  bool done = false;
  std::vector<unsigned> bits(p.B);
  while (!done && sweep < MAX_SWEEPS) {
    WM_HIP(hipMemsetAsync(w.maxcos, 0, (size_t)p.B * sizeof(unsigned), ctx->stream));
    if (hier) WM_TRY(hier_sweep(ctx, p, w, r));
    else WM_TRY(flat_sweep(ctx, p, w, r, sweep));
    for (int g = 1; g < r.NQ; ++g) {
      WM_HIP(hipEventRecord(ctx->ev_join[g - 1], r.q(ctx, g)));
      WM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join[g - 1], 0));
    }
    WM_HIP(hipGetLastError());
    WM_HIP(hipMemcpyAsync(bits.data(), w.maxcos, (size_t)p.B * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    ++sweep;
    done = true;
    for (int z = 0; z < p.B; ++z) { float mc; memcpy(&mc, &bits[z], 4); if (!(mc < conv_cos)) done = false; }
  }
  *sweeps_out = done ? sweep : -sweep;
  ctx->ref_last_sweeps = sweep;
  {   // nominal matrix-core flops of one sweep (every pair counted as rotated), for bench.py's roofline
    double f = 0.0;
    if (hier) {
      for (int s1 = 0; s1 < r.ht->nsteps1; ++s1) {
        // the host copy of the tables holds the stage counts; the super-pairs' sizes follow from the block counts
        f += r.ht->flops_step[s1] * ((double)p.M) + r.ht->flops_apply_step[s1] * (double)r.ncols + r.ht->flops_stage_step[s1];
      }
    } else {
      f = (double)p.nsteps * p.npairs * (2.0 * 3 * RB * RB * p.M + 2.0 * RP * RP * r.ncols);
    }
    ctx->ref_last_flops = f * sweep * p.B;
    ctx->ref_last_hier = hier ? 1 : 0;
  }
  return WM_OK;
}

// row norms of every plane -> host (b2, q2 are [B][Lp])
int fetch_norms(wm_ctx* ctx, const RefPlan& p, const RefWs& w, bool with_q, std::vector<double>& b2,
                std::vector<double>& q2) {
  hipLaunchKernelGGL(k_rf_rownorms, dim3(p.Lp, p.B), dim3(256), 0, ctx->stream, w.aug, p.aug_ps, p.ld, p.M,
                     with_q ? p.Lp : 0, w.b2, w.q2);
  WM_HIP(hipGetLastError());
  b2.resize((size_t)p.B * p.Lp); q2.resize((size_t)p.B * p.Lp);
  WM_HIP(hipMemcpyAsync(b2.data(), w.b2, b2.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  WM_HIP(hipMemcpyAsync(q2.data(), w.q2, q2.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  if (!with_q) std::fill(q2.begin(), q2.end(), 1.0);
  return WM_OK;
}

static bool final_f16() { return ref_knobs().final_f16; }      // (read on every call, like WM_RF_HIER: tests switch it)

// The spectrum rule of one plane: which estimate of s_i each of the Lp rotated rows gets.
//   b2 = |b_i|^2;  q2 in: |q_i|^2 of the accumulated factor's row ([A | I] formulation; all 1 where there is none, and every
//   term below then reduces exactly: b2 / 1, sqrt(t2 * 1), 1 * gcal);  t2 = |T[:, i]|^2 = |A0 b_i^T|^2.
//   q2 out: the factor that makes sqrt(b2 / q2) the singular value.
// |T[:, i]| = |b_i| s_i must agree with |b_i|^2 / |q_i| up to the rotations' scale drift (a few 1e-4).
// A row that fails this is rounding residue of a rank-deficient plane - its direction is noise,
// A0 b_i^T measures nothing - and keeps its own (tiny) norm as singular value; reliable (optional) marks the rows that pass.
// zero_residue: a row below the numerical-null floor (the one the convergence test uses) whose A0 b_i^T is RESIDUE_RHO times
// larger than a singular direction of that norm could give is rounding residue: its singular value is 0 (b2 = 0), as the
// float32 cast of LAPACK's 1e-13-sized values would be.  A genuinely small value (clean synthetic images)
// has rho near 1 - off by c^2 (s_max / s_i)^2 / 2 at worst - and keeps its norm.
void spectrum_rule(const int Lp, double* b2, double* q2, const double* t2, const double skip_thr, const bool zero_residue,
                   const bool drift_cal, const int debug_plane, unsigned char* reliable) {
  const double floor2 = null_floor2(b2, Lp);
  double smax2 = 0.0;
  for (int i = 0; i < Lp; ++i) if (q2[i] > 0.0) smax2 = std::max(smax2, b2[i] / q2[i]);
  // |A0 b_i^T| / |b_i| against |b_i| / |q_i|: 1 up to the scale drift unless b_i is residue
  auto rho_of = [&](int i) { return (b2[i] > 0.0 && q2[i] > 0.0 && t2[i] > 0.0) ? sqrt(t2[i] * q2[i]) / b2[i] : 1e300; };
  // Which estimate: with a residual cosine c between rows i and j, |A0 b_i^T| / |b_i| is off by
  // c^2 (s_j / s_i)^2 / 2 relative, |b_i| by c^2 plus the scale drift (1e-4 relative, i.e. nothing in
  // absolute terms for a small value).  The Jacobi leaves c <= skip_thr, so the first estimate is
  // used down to s_i = T_SWITCH * c * s_max (error <= 1.25e-5) and the plain norm below.
  const double ratio = T_SWITCH * skip_thr;
  // Scale drift of the rotated rows, measured: every row goes through the same ~3e4..3e5 rotations, each of which
  // shrinks it by the few 1e-8 that v_rsq_f32 leaves cos^2 + sin^2 below 1, so |b_i|^2 / s_i^2 is nearly the SAME
  // factor g < 1 for all rows of a plane (1 - g = 6e-4 at 1080p, 1.6e-3 at 8K).  Where both estimates exist (the
  // rows above the switch) g_i = |b_i|^4 / (|q_i|^2 |T[:, i]|^2) is known; its median calibrates the rows below the
  // switch, whose |b_i| / |q_i| is the only estimate: s_i = |b_i| / (|q_i| sqrt(g)).  Without it the largest error of a whole
  // spectrum sat right below the switch (3.3e-6 s_1 at 4K, 7.8e-6 at 8K - tests/test_gpu_fullframe_large.py).
  std::vector<double> g;
  std::vector<unsigned char> above(Lp, 0);
  for (int i = 0; i < Lp; ++i) {
    const bool consistent = fabs(rho_of(i) - 1.0) < DRIFT_TOL;
    if (reliable) reliable[i] = consistent ? 1 : 0;
    if (consistent && b2[i] / q2[i] >= ratio * ratio * smax2) { above[i] = 1; g.push_back(b2[i] * b2[i] / (q2[i] * t2[i])); }
  }
  double gcal = 1.0;
  if (g.size() >= 8) {
    std::sort(g.begin(), g.end());
    if (drift_cal) gcal = g[g.size() / 2];
    if (debug_plane >= 0)
      fprintf(stderr, "[wm_ref] plane %d: drift factor g over %zu rows: p05 %.3e  median %.3e  p95 %.3e  (1 - g)\n", debug_plane,
              g.size(), 1.0 - g[g.size() / 20], 1.0 - g[g.size() / 2], 1.0 - g[g.size() - 1 - g.size() / 20]);
  }
  for (int i = 0; i < Lp; ++i) {
    if (above[i]) {
      q2[i] = b2[i] * b2[i] / t2[i];                                    // sigma = |T[:, i]| / |b_i|
    } else if (zero_residue && rho_of(i) > RESIDUE_RHO && b2[i] < floor2) {
      b2[i] = 0.0; q2[i] = 1.0;                                         // residue below the floor: sigma = 0
    } else {
      q2[i] = q2[i] * gcal;                                             // sigma = |b_i| / (|q_i| sqrt(g)): the norm, drift calibrated
    }
  }
}

struct RefSpectrum {                     // host-side result of one batched Jacobi + T = A0 B^T pass
  std::vector<double> b2, q2, t2;        // [B][Lp] |b_i|^2, the factor that turns it into sigma_i^2, |T[:, i]|^2
  std::vector<unsigned char> reliable;   // [B][Lp] u_i = T[:, i] / (|b_i| s_i) is a usable left vector
};

// Q-free finalisation after jacobi_rows(JR_SIGMA / JR_EMBED).  The rotated rows are b_i = s_i v_i^T
// up to the scale drift of ~3e4 float32 rotations per row (v_rsq_f32 rounds cos^2 + sin^2 a few
// 1e-8 below 1, every time); the DIRECTION v_i is good to the convergence threshold.  So the
// singular value is measured on the untouched input instead:  T = A0 B^T  (T[:, i] = A0 b_i^T =
// |b_i| s_i u_i), s_i = |T[:, i]| / |b_i| - the drift cancels, and T doubles as the left factor
// of the embed (u_i = T[:, i] / (|b_i| s_i)).  sp.b2 = |b_i|^2, and sp.q2 is returned as
// b2^2 / |T[:, i]|^2 so that sqrt(b2 / q2) is s_i like in the [A | I] formulation (spectrum_rule).
//   w.a0: dense [B][L][M] copy of the input rows;  w.t: T, dense [B][L][Lp] (left on the device).
// The finalisation's large products from split-f16 operands (k_hgemm, wm_ref_hier.inc) unless WM_RF_FINAL_F16=0 or the shapes
// do not allow 16-byte loads; the f32 k_sgemm otherwise.
int fetch_norms_t(wm_ctx* ctx, const RefPlan& p, const RefWs& w, RefSpectrum& sp) {
  // all planes' products in one launch (grid.z = plane)
  hipLaunchKernelGGL(k_rf_rownorms, dim3(p.Lp, p.B), dim3(256), 0, ctx->stream, w.aug, p.aug_ps, p.ld, p.M, 0, w.b2, w.q2);
  if (final_f16() && hgemm_ok(w.a0, p.M, w.aug, p.ld)) {
    // A0 holds uint8 samples (every caller decomposes uint8 planes): exact in f16; B's rows are bounded by 255 sqrt(L)
    hipLaunchKernelGGL((k_hgemm<true, true, false>), dim3((p.Lp + 127) / 128, (p.L + 127) / 128, p.B), dim3(256), 0, ctx->stream, p.L, p.Lp, p.M,
                       w.a0, p.M, (size_t)p.L * p.M, w.aug, p.ld, p.aug_ps, 0, w.t, p.Lp, (size_t)p.L * p.Lp, (const float*)nullptr, (size_t)0, 1.0f,
                       1.0f, (const float*)nullptr);
  } else
  WM_TRY(sgemm_b(ctx, false, true, p.L, p.Lp, p.M, 1.0f, w.a0, p.M, (size_t)p.L * p.M, w.aug, p.ld, p.aug_ps, 0.0f, w.t, p.Lp,
                 (size_t)p.L * p.Lp, p.B));
  hipLaunchKernelGGL(k_rf_colnorms, dim3((p.Lp + 63) / 64, p.B), dim3(256), 0, ctx->stream, w.t, (size_t)p.L * p.Lp, p.L, p.Lp, w.q2);
  WM_HIP(hipGetLastError());
  const size_t n = (size_t)p.B * p.Lp;
  sp.b2.resize(n); sp.t2.resize(n);
  WM_HIP(hipMemcpyAsync(sp.b2.data(), w.b2, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  WM_HIP(hipMemcpyAsync(sp.t2.data(), w.q2, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  sp.q2.assign(n, 1.0); sp.reliable.assign(n, 0);
  const RefKnobs k = ref_knobs();
  for (int z = 0; z < p.B; ++z) {
    const size_t o = (size_t)z * p.Lp;
    spectrum_rule(p.Lp, &sp.b2[o], &sp.q2[o], &sp.t2[o], (double)ctx->ref_skip_thr, true, k.drift_cal, k.debug_drift ? z : -1, &sp.reliable[o]);
  }
  return WM_OK;
}

// copy the A part (first L rows, M columns) of every plane's Aug into a dense [B][L][M] array
int copy_a_part(wm_ctx* ctx, const RefPlan& p, const RefWs& w, float* dst) {
  for (int z = 0; z < p.B; ++z)
    WM_HIP(hipMemcpy2DAsync(dst + (size_t)z * p.L * p.M, (size_t)p.M * 4, w.aug + (size_t)z * p.aug_ps, (size_t)p.ld * 4,
                            (size_t)p.M * 4, p.L, hipMemcpyDeviceToDevice, ctx->stream));
  return WM_OK;
}

// sigma_i = |b_i| / |q_i| of one plane's Lp rows, sorted descending -> order, sig[L]
void sort_sigma(const RefPlan& p, const double* b2, const double* q2, std::vector<int>& order, std::vector<float>& sig) {
  std::vector<double> s(p.Lp);
  for (int i = 0; i < p.Lp; ++i) s[i] = sqrt(b2[i] / (q2[i] > 0 ? q2[i] : 1.0));
  order.resize(p.Lp);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return s[a] > s[b]; });
  sig.resize(p.L);
  for (int k = 0; k < p.L; ++k) sig[k] = (float)s[order[k]];
}

int check_ref_args(wm_ctx* ctx, const void* plane, int n_planes, int H, int W, int row_stride, size_t plane_stride) {
  WM_TRY(wmi::use_ctx(ctx));
  if (H <= 0 || W <= 0) return set_err(WM_ERR_BADARG, "H and W must be positive");
  if (n_planes <= 0 || n_planes > 65535) return set_err(WM_ERR_BADARG, "n_planes must be in 1..65535");
  if (!plane) return set_err(WM_ERR_BADARG, "plane pointer is NULL");
  if (row_stride < W) return set_err(WM_ERR_BADARG, "row_stride < W");
  if (n_planes > 1 && plane_stride < (size_t)row_stride * (H - 1) + W)
    return set_err(WM_ERR_BADARG, "plane_stride smaller than one plane");
  return WM_OK;
}


// ---------------------------------------------------------------------------
// cores: every plane-sized array is DEVICE memory; the small per-plane vectors (singular values, the
// embed coefficients) cross to the host once per call, where they are sorted / classified
// ---------------------------------------------------------------------------
// planes (uint8, device) -> rotated rows B in w.aug, A0 copy in w.a0 [B][L][M], T = A0 B^T in w.t [B][L][Lp],
// spectrum on the host
int ref_decompose(wm_ctx* ctx, const RefPlan& p, const RefWs& w, const uint8_t* d_planes, size_t row_stride,
                  size_t plane_stride, JacobiUse use, RefSpectrum& sp) {
  hipLaunchKernelGGL((k_rf_load<uint8_t>), dim3(8, p.Lp, p.B), dim3(256), 0, ctx->stream, d_planes, row_stride,
                     plane_stride, p.transpose ? 1 : 0, w.aug, p.aug_ps, p.ld, p.L, p.Lp, p.M);
  WM_TRY(copy_a_part(ctx, p, w, w.a0));
  int sweeps = 0;
  WM_TRY(jacobi_rows(ctx, p, w, use, &sweeps));
  if (sweeps < 0) return set_err(WM_ERR_NOCONV, "SVD did not converge");
  WM_TRY(fetch_norms_t(ctx, p, w, sp));
  return WM_OK;
}

// singular values of n planes on the device -> host sig [B][L]
int ref_sigma_core(wm_ctx* ctx, const RefPlan& p, const RefWs& w, const uint8_t* d_planes, size_t row_stride,
                   size_t plane_stride, float* sig_host) {
  RefSpectrum sp;
  WM_TRY(ref_decompose(ctx, p, w, d_planes, row_stride, plane_stride, JR_SIGMA, sp));
  std::vector<int> order; std::vector<float> sig;
  for (int z = 0; z < p.B; ++z) {
    sort_sigma(p, &sp.b2[(size_t)z * p.Lp], &sp.q2[(size_t)z * p.Lp], order, sig);
    memcpy(sig_host + (size_t)z * p.L, sig.data(), (size_t)p.L * 4);
  }
  return WM_OK;
}

// The core of every null-space completion: the n vectors Z [n][len] (device) become an orthonormal set orthogonal to the
// valid vectors of a basis - `rounds` times: projected off the basis (twice), orthogonalised by the block Jacobi (the row
// span is preserved), the n largest rows gathered back into Z, normalised.
//   basis, ldb: Lp vectors of length len - rows of basis (by_rows: the rotated rows B, the Qt part) or its columns (T);
//   coef [Lp] HOST: 1 / |vector i|^2 of the valid ones, 0 for the others;
//   wv: a workspace planned for make_plan(n, len) or a longer vector length with the same n (its arrays are then large
//   enough), with C [n][Lp] and d_coef [Lp] in its tmp1.  The caller plans it: a second set of vectors may live there too.
int ref_complete_vectors(wm_ctx* ctx, const RefWs& wv, float* Z, const int n, const int len, const float* basis, const int ldb,
                         const int Lp, const bool by_rows, const std::vector<float>& coef, float* C, float* d_coef, const int rounds) {
  const RefPlan pp = make_plan(n, len);
  RefWs ww = wv;
  WM_TRY(get_pairs(ctx, pp, &ww.pairs));
  WM_HIP(hipMemcpyAsync(d_coef, coef.data(), (size_t)Lp * 4, hipMemcpyHostToDevice, ctx->stream));
  for (int round = 0; round < rounds; ++round) {
    for (int pass = 0; pass < 2; ++pass) {          // project twice: classical Gram-Schmidt loses digits once
      if (by_rows) WM_TRY(sgemm(ctx, false, true, n, Lp, len, 1.0f, Z, len, basis, ldb, 0.0f, C, Lp));            // Z B^T
      else WM_TRY(sgemm(ctx, false, false, n, Lp, len, 1.0f, Z, len, basis, ldb, 0.0f, C, Lp));                   // Z T
      hipLaunchKernelGGL(k_rf_scale_cols_b, dim3(8, n, 1), dim3(256), 0, ctx->stream, C, (size_t)0, C, (size_t)0, Lp, d_coef, (size_t)0);
      if (by_rows) WM_TRY(sgemm(ctx, false, false, n, len, Lp, -1.0f, C, Lp, basis, ldb, 1.0f, Z, len));          // Z -= C B
      else WM_TRY(sgemm(ctx, false, true, n, len, Lp, -1.0f, C, Lp, basis, ldb, 1.0f, Z, len));                   // Z -= C T^T
    }
    WM_HIP(hipStreamSynchronize(ctx->stream));      // coef is the caller's, d_coef may be reused
    hipLaunchKernelGGL((k_rf_load<float>), dim3(8, pp.Lp, 1), dim3(256), 0, ctx->stream, Z, (size_t)len, (size_t)0, 0,
                       ww.aug, pp.aug_ps, pp.ld, pp.L, pp.Lp, pp.M);
    int sweeps = 0;
    WM_TRY(jacobi_rows(ctx, pp, ww, JR_ORTH, &sweeps));
    if (sweeps < 0) return set_err(WM_ERR_NOCONV, "null-space completion did not converge");
    std::vector<double> norms2, dummy;
    WM_TRY(fetch_norms(ctx, pp, ww, false, norms2, dummy));
    std::vector<int> ord(pp.Lp);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return norms2[a] > norms2[b]; });
    // gather the n largest rows back into Z, normalised
    std::vector<float> sc(n);
    for (int k = 0; k < n; ++k) sc[k] = norms2[ord[k]] > 0.0 ? (float)(1.0 / sqrt(norms2[ord[k]])) : 0.0f;
    WM_HIP(hipMemcpyAsync(ww.order, ord.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipMemcpyAsync(ww.scale, sc.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_rf_gather_rows, dim3(8, n), dim3(256), 0, ctx->stream, ww.aug, pp.ld, len, ww.order, ww.scale, Z, len);
    WM_HIP(hipStreamSynchronize(ctx->stream));      // ord / sc are locals; ww.order is free again
  }
  return WM_OK;
}

// Null-space completion of ONE rank-deficient plane z.  The reference injects alpha*Sw[k]
// for EVERY k < K (single:174-176): where the plane has no k-th singular direction LAPACK supplies some
// orthonormal completion of the null spaces.  Here: n deterministic pseudo-random vectors per side are
// projected off the valid singular vectors (twice), orthogonalised by the same block Jacobi, normalised
// (ref_complete_vectors, one round), and  sum_k w_k u_k v_k^T  is added to Yw.  With every u and every v orthonormal,
// svd(Yw) = {s_i + w_i} U {w_k}: the reference's invariant  S(Cw)[:K] = Sc[:K] + alpha Sw[:K].
//   valid [Lp]: 1 for rows of B that are singular directions; wk [n]: the energies of the missing ranks;
//   tnorm2 [Lp]: |T[:, i]|^2.  d_yw: this plane's Yw in A layout [L][M].
int ref_complete_plane(wm_ctx* ctx, const RefPlan& p, const RefWs& w, int z, const std::vector<unsigned char>& valid,
                       const double* b2, const double* tnorm2, const std::vector<float>& wk, const float* d_t_z,
                       float* d_yw_z) {
  const int n = (int)wk.size();
  if (n == 0) return WM_OK;
  const float* Bz = w.aug + (size_t)z * p.aug_ps;
  RefWs wv;
  // second workspace, planned for the larger of the two Jacobi runs (n x M; the n x L one has the same
  // block count and fewer columns and reuses its arrays).  tmp1: Zv [n][M] | Zu [n][L] | C [n][Lp] | coefficients [Lp]
  // Zv and Zu both live until the product below, so both sides share this one plan
  WM_TRY(plan_workspace(ctx, make_plan(n, p.M), wv, (size_t)n * (p.M + p.L + p.Lp) + p.Lp + 64, 16, 1));
  float* Zv = wv.tmp1; float* Zu = Zv + (size_t)n * p.M; float* C = Zu + (size_t)n * p.L; float* coef = C + (size_t)n * p.Lp;
  std::vector<float> gv(p.Lp), gu(p.Lp);
  for (int i = 0; i < p.Lp; ++i) {
    gv[i] = (valid[i] && b2[i] > 0.0) ? (float)(1.0 / b2[i]) : 0.0f;
    gu[i] = (valid[i] && tnorm2[i] > 0.0) ? (float)(1.0 / tnorm2[i]) : 0.0f;
  }
  hipLaunchKernelGGL(k_rf_pattern, dim3(8, n), dim3(256), 0, ctx->stream, Zv, p.M, 0x1234567u);
  hipLaunchKernelGGL(k_rf_pattern, dim3(8, n), dim3(256), 0, ctx->stream, Zu, p.L, 0x7654321u);
  // right vectors (length M, against the rows of B), then left vectors (length L, against the columns of T)
  WM_TRY(ref_complete_vectors(ctx, wv, Zv, n, p.M, Bz, p.ld, p.Lp, true, gv, C, coef, 1));
  WM_TRY(ref_complete_vectors(ctx, wv, Zu, n, p.L, d_t_z, p.Lp, p.Lp, false, gu, C, coef, 1));
  // Zu rows scaled by the energies, then Yw += Zu^T Zv   ([L x n] [n x M])
  WM_HIP(hipMemcpyAsync(coef, wk.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_rf_scale_rows, dim3(8, n, 1), dim3(256), 0, ctx->stream, Zu, (size_t)0, p.L, p.L, coef);
  WM_TRY(sgemm(ctx, true, false, p.L, p.M, n, 1.0f, Zu, p.L, Zv, p.M, 1.0f, d_yw_z, p.M));
  WM_HIP(hipStreamSynchronize(ctx->stream));         // wk is the caller's, coef reused
  return WM_OK;
}

// Null-space completion of one factor of ONE rank-deficient plane z of the watermark-side SVD.  The rows of [B | Qt] whose B
// part is below the Jacobi's numerical-null floor are rounding residue - they take no part in its convergence test, so
// nothing makes them orthogonal - and b_i / |b_i| of such a row is not a singular vector.  Their Qt parts were measured
// non-orthogonal too on planes whose DCT has exactly vanishing rows (an unscrambled logo of two bars: |U^T U - I| = 1.0 on
// the null columns, the valid ones exact).  LAPACK returns an orthonormal completion there; here the slots of those rows
// in BOTH gathered factors get one, side 0 of ref_complete_plane: deterministic start vectors, projected twice off the
// valid rows, orthogonalised by the block Jacobi, normalised (ref_complete_vectors, two rounds).
//   side 0: the long-side factor (B part, vectors of length M);  side 1: the short-side factor (first L columns of the Qt part)
//   valid [Lp]: 1 for rows that are singular directions;  n2 [Lp]: squared norms of that part of the rows;
//   slots [n]: where the n completed vectors go;  dst + slot * ld_slot + j * ld_elem: element j of that slot's vector
int ref_complete_factor(wm_ctx* ctx, const RefPlan& p, const RefWs& w, int z, int side, const std::vector<unsigned char>& valid,
                        const double* n2, const std::vector<int>& slots, float* dst, size_t ld_slot, size_t ld_elem) {
  const int n = (int)slots.size();
  if (n == 0) return WM_OK;
  const float* Bz = w.aug + (size_t)z * p.aug_ps + (side == 0 ? 0 : p.M);
  const int len = side == 0 ? p.M : p.L;
  RefWs wv;
  // tmp1: Z [n][len] | C [n][Lp] | coefficients [Lp]
  WM_TRY(plan_workspace(ctx, make_plan(n, len), wv, (size_t)n * (len + p.Lp) + p.Lp + 64, 16, 1));
  float* Z = wv.tmp1; float* C = Z + (size_t)n * len; float* coef = C + (size_t)n * p.Lp;
  std::vector<float> gv(p.Lp);
  for (int i = 0; i < p.Lp; ++i) gv[i] = (valid[i] && n2[i] > 0.0) ? (float)(1.0 / n2[i]) : 0.0f;
  hipLaunchKernelGGL(k_rf_pattern, dim3(8, n), dim3(256), 0, ctx->stream, Z, len, side == 0 ? 0x1234567u : 0x7654321u);
  // Two rounds of (project, orthonormalise).  The complement of the valid short-side vectors has exactly n dimensions, so the
  // n projected start vectors are a SQUARE random matrix there, condition ~n..n^2: the Jacobi works on float32 Gram entries
  // and leaves its small rows eps * cond^2 off (measured 3.3e-4 on a 56x40 plane of rank 3), and normalising a small row
  // amplifies what the projection left of the valid vectors.  The second round starts from rows that are orthonormal to
  // that error, condition 1, and ends at rounding level.
  WM_TRY(ref_complete_vectors(ctx, wv, Z, n, len, Bz, p.ld, p.Lp, true, gv, C, coef, 2));
  WM_HIP(hipMemcpyAsync(wv.order, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_rf_put_rows, dim3(8, n), dim3(256), 0, ctx->stream, Z, len, wv.order, dst, ld_slot, ld_elem);
  WM_HIP(hipGetLastError());
  WM_HIP(hipStreamSynchronize(ctx->stream));        // slots is the caller's
  return WM_OK;
}

// embed of p.B planes on the device.  d_in / d_out: uint8 planes (same strides; may alias);
// d_ywout: optional dense float [B][H][W]; sigma_w: HOST [B or 1][L]; sigma_c: HOST [B][L] out.
// Yw [B][L][M] is built in w.a0, beside T in w.t.
int ref_embed_core(wm_ctx* ctx, const RefPlan& p, const RefWs& w, const uint8_t* d_in, uint8_t* d_out, float* d_ywout,
                   size_t row_stride, size_t plane_stride, const float* sigma_w,
                   size_t sigma_w_plane_stride, float* sigma_c, float alpha, int K, const int* sigma_w_ready = nullptr) {
  const size_t yw_ps = (size_t)p.L * p.M;
  float* const d_yw = w.a0; float* const d_t = w.t;
  RefSpectrum sp;
  // Yw starts as A itself (exactly the pixels): ref_decompose leaves that copy in w.a0
  WM_TRY(ref_decompose(ctx, p, w, d_in, row_stride, plane_stride, JR_EMBED, sp));
  // sigma_w is first read here, after the host planes' decomposition (the long part of the call): a caller that is still
  // computing it - the watermark's own SVD on another context and thread, single:172-173's two independent statements -
  // says so with a flag: > 0 once sigma_w is written, < 0 if it never will be
  if (sigma_w_ready) {
    for (;;) {
      const int v = __atomic_load_n(sigma_w_ready, __ATOMIC_ACQUIRE);
      if (v > 0) break;
      if (v < 0) return set_err(WM_ERR_BADARG, "sigma_w was not produced (sigma_w_ready < 0)");
      std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
  }
  // U diag(alpha Sw) V^T = T diag(e) B  with  e_i = alpha * sw[rank(i)] / (s_i |b_i|^2), rank < K
  // (u_i = T[:, i] / (|b_i| s_i), v_i^T = b_i / |b_i|;  S_[:K] = Sc[:K] + alpha*Sw[:K]).
  // Split-f16 form of the product (k_hgemm): the factor e_i = ca_i cb_i goes half to each operand - B's rows to unit norm
  // (cb_i = 1 / |b_i|), T's columns to alpha sw (ca_i = alpha sw / (s_i |b_i|)) - so that both are inside f16's range whatever
  // the plane's scale; alpha * max(sw) must be (f32 product otherwise).
  bool f16_prod = final_f16() && hgemm_ok(d_t, p.Lp, w.aug, p.ld) && p.M % 4 == 0;
  for (int z = 0; z < p.B && f16_prod; ++z) {
    const float* sw = sigma_w + (size_t)z * sigma_w_plane_stride;
    for (int k = 0; k < std::min(K, p.L); ++k) if (!(fabs((double)alpha * sw[k]) < 3.0e4)) { f16_prod = false; break; }
  }
  std::vector<float> d((size_t)p.B * p.Lp * (f16_prod ? 2 : 1), 0.0f);       // row scales of B [, then column scales of T]
  std::vector<int> order; std::vector<float> sig;
  struct Todo { int z; std::vector<unsigned char> valid; std::vector<float> wk; };
  std::vector<Todo> todo;
  for (int z = 0; z < p.B; ++z) {
    const double* pb = &sp.b2[(size_t)z * p.Lp]; const double* pq = &sp.q2[(size_t)z * p.Lp];
    sort_sigma(p, pb, pq, order, sig);
    memcpy(sigma_c + (size_t)z * p.L, sig.data(), (size_t)p.L * 4);
    const float* sw = sigma_w + (size_t)z * sigma_w_plane_stride;
    const double s1 = sig.empty() ? 0.0 : (double)sig[0];
    Todo td; td.z = z; td.valid.assign(p.Lp, 0);
    for (int i = 0; i < p.Lp; ++i) {
      // a singular direction: consistent T column, above the null ratio (sigma_i^2 = b2 / q2)
      const double s2 = pb[i] / (pq[i] > 0 ? pq[i] : 1.0);
      td.valid[i] = (sp.reliable[(size_t)z * p.Lp + i] && sqrt(s2) > NULL_RATIO * s1 && pb[i] > 0.0) ? 1 : 0;
    }
    for (int k = 0; k < std::min(K, p.L); ++k) {
      const int i = order[k];
      const double si = (double)sig[k];
      if (td.valid[i]) {
        if (f16_prod) {
          const double nb = sqrt(pb[i]);
          d[(size_t)z * p.Lp + i] = (float)(1.0 / nb);
          d[(size_t)(p.B + z) * p.Lp + i] = (float)((double)alpha * (double)sw[k] / (si * nb));
        } else d[(size_t)z * p.Lp + i] = (float)((double)alpha * (double)sw[k] / (si * pb[i]));
      } else td.wk.push_back(alpha * sw[k]);           // rank k has no singular direction in this plane: completed below
    }
    if (!td.wk.empty()) todo.push_back(std::move(td));
  }
  WM_HIP(hipMemcpyAsync(w.dvec, d.data(), d.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  // completion reads the unscaled rows of B: it runs before the rows are scaled in place
  if (!todo.empty()) {
    WM_HIP(hipStreamSynchronize(ctx->stream));
    for (const Todo& td : todo)
      WM_TRY(ref_complete_plane(ctx, p, w, td.z, td.valid, &sp.b2[(size_t)td.z * p.Lp], &sp.t2[(size_t)td.z * p.Lp], td.wk,
                                d_t + (size_t)td.z * p.L * p.Lp, d_yw + (size_t)td.z * yw_ps));
  }
  hipLaunchKernelGGL(k_rf_scale_rows, dim3(8, p.Lp, p.B), dim3(256), 0, ctx->stream, w.aug, p.aug_ps, p.ld, p.M, w.dvec);
  // Yw += T (diag(e) B):   [L x Lp] times [Lp x M], all planes in one launch
  if (f16_prod)
    hipLaunchKernelGGL((k_hgemm<false, false, true>), dim3((p.M + 127) / 128, (p.L + 127) / 128, p.B), dim3(256), 0, ctx->stream, p.L, p.M, p.Lp,
                       d_t, p.Lp, (size_t)p.L * p.Lp, w.aug, p.ld, p.aug_ps, 1, d_yw, p.M, yw_ps, w.dvec + (size_t)p.B * p.Lp, (size_t)p.Lp, 1.0f,
                       1.0f, (const float*)nullptr);
  else
  WM_TRY(sgemm_b(ctx, false, false, p.L, p.M, p.Lp, 1.0f, d_t, p.Lp, (size_t)p.L * p.Lp, w.aug, p.ld, p.aug_ps, 1.0f,
                 d_yw, p.M, yw_ps, p.B));
  hipLaunchKernelGGL(k_rf_quant, dim3(8, p.H, p.B), dim3(256), 0, ctx->stream, d_yw, yw_ps, p.M, p.transpose ? 1 : 0,
                     d_out, row_stride, plane_stride, d_ywout, p.H, p.W);
  WM_HIP(hipGetLastError());
  WM_HIP(hipStreamSynchronize(ctx->stream));         // d is a local
  return WM_OK;
}

// extract of B planes: sigma(stego) -> Sw_hat -> Uw[:L,:L] diag(Sw_hat) Vwt[:L,:L], zero-padded -> idct2.
// d_uw [H][L] and d_vwt [L][W] are the meta factors on the device (leading dimensions L and W);
// sigma_c HOST [B][L]; d_out dense float [B][H][W].  ws: tmp1 = Uw diag(sh) [B][L][L], tmp2 tail = GEMM intermediate [B][H][W].
// the product and the inverse DCT of single:214-218 for B planes with the estimates given: sh HOST [B][p.Lp] (entries at and
// beyond Lx are not read), Lx <= p.L the reference's truncation length - Uw[:Lx,:Lx] diag(sh) Vwt[:Lx,:Lx] lands in the
// top-left Lx x Lx corner of the zero plane (single:215-217), then idct2 of the whole H x W plane.
int ref_reconstruct_core(wm_ctx* ctx, const RefPlan& p, const RefWs& w, const std::vector<float>& sh, const int Lx,
                         const float* d_uw, const float* d_vwt, float* d_us, float* d_mid, float* d_out) {
  const int L = p.L, H = p.H, W = p.W;
  float *dH, *dW;
  WM_TRY(get_dct_pair(ctx, H, W, &dH, &dW));
  if (final_f16() && L % 4 == 0 && W % 4 == 0 && H % 4 == 0 && hgemm_ok(d_uw, L, d_vwt, W) && hgemm_ok(d_mid, W, d_out, W)) {
    // Split-f16 products (k_hgemm), only for factors whose corners have rows of Uw / columns of Vwt of norm mu / mv <= 1 + 2^-10
    // (corners of orthonormal factors always do); k_sgemm for any other factors.  Every f16 operand is then brought into
    // [~1, 3e4) by powers of two (exact both ways): per plane, sw_hat by 2^-e so that max |sw_hat| mu lies in [1.5e4, 3e4)
    // (this bounds |Uw diag(sh)| and |X|); a Vwt with mv < 1/2 by 2^sv up to [1/2, 1); D_H^T X, whose entries are bounded by
    // the column norms of X, up to sqrt(Lx) |X| for factors that are not orthonormal, by 2^-m < 1 / sqrt(Lx).  The last
    // product multiplies 2^(e + m - sv) out again, per plane.
    float* d_az = w.dvec + (size_t)p.B * p.Lp;                 // after the estimates: per-plane alphas, then the guard's bits
    unsigned* d_mx = reinterpret_cast<unsigned*>(d_az + p.B);
    WM_HIP(hipMemsetAsync(d_mx, 0, 2 * sizeof(unsigned), ctx->stream));
    const int nbu = (Lx + 3) / 4;
    hipLaunchKernelGGL(k_rf_corner_norms, dim3(nbu + (Lx + 15) / 16), dim3(256), 0, ctx->stream, d_uw, L, d_vwt, W, Lx, nbu, d_mx);
    unsigned mxb[2] = {0u, 0u};
    WM_HIP(hipMemcpyAsync(mxb, d_mx, sizeof(mxb), hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    const double mu = sqrt((double)__builtin_bit_cast(float, mxb[0])), mv = sqrt((double)__builtin_bit_cast(float, mxb[1]));
    const double lim = 1.0 + 1.0 / 1024.0;
    bool ok = mu > 0.0 && mv > 0.0 && mu <= lim && mv <= lim;          // (false for NaN)
    int ev = 0, m = 0;
    if (ok) { (void)frexp(mv, &ev); (void)frexp(sqrt((double)Lx), &m); }
    const int sv = ev < 0 ? -ev : 0;
    std::vector<float> dv((size_t)p.B * p.Lp + p.B, 0.0f);           // sw_hat 2^-e [B][Lp] | 2^(e + m - sv) [B]
    for (int z = 0; z < p.B && ok; ++z) {
      const float* shz = &sh[(size_t)z * p.Lp];
      float mx = 0.0f;
      for (int i = 0; i < Lx; ++i) mx = fmaxf(mx, fabsf(shz[i]));
      const double bound = (double)mx * mu;
      int e = 0;
      if (bound > 0.0) (void)frexp(bound / 3.0e4, &e);
      // every scale a normal float (estimates within ~2^+-100 of 3e4 / mu; k_sgemm beyond)
      if (!std::isfinite(bound) || sv > 100 || e < -100 || e > 100) { ok = false; break; }
      for (int i = 0; i < p.Lp; ++i) dv[(size_t)z * p.Lp + i] = ldexpf(shz[i], -e);
      dv[(size_t)p.B * p.Lp + z] = ldexpf(1.0f, e + m - sv);
    }
    if (ok) {
      WM_HIP(hipMemcpyAsync(w.dvec, dv.data(), dv.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      WM_HIP(hipMemsetAsync(d_out, 0, (size_t)p.B * H * W * 4, ctx->stream));                                   // single:215
      const float* dHt = dH + (size_t)H * H;
      hipLaunchKernelGGL((k_hgemm<false, false, true>), dim3((Lx + 127) / 128, (Lx + 127) / 128, p.B), dim3(256), 0, ctx->stream, Lx, Lx, Lx,
                         d_uw, L, (size_t)0, d_vwt, W, (size_t)0, 0, d_out, W, (size_t)H * W, w.dvec, (size_t)p.Lp, 1.0f,
                         ldexpf(1.0f, sv), (const float*)nullptr);                                                 // single:214, 216-217
      hipLaunchKernelGGL((k_hgemm<false, false, false>), dim3((W + 127) / 128, (H + 127) / 128, p.B), dim3(256), 0, ctx->stream, H, W, H,
                         dHt, H, (size_t)0, d_out, W, (size_t)H * W, 0, d_mid, W, (size_t)H * W, (const float*)nullptr, (size_t)0,
                         ldexpf(1.0f, -m), 1.0f, (const float*)nullptr);                                           // idct2: D_H^T X
      hipLaunchKernelGGL((k_hgemm<false, false, false>), dim3((W + 127) / 128, (H + 127) / 128, p.B), dim3(256), 0, ctx->stream, H, W, W,
                         d_mid, W, (size_t)H * W, dW, W, (size_t)0, 0, d_out, W, (size_t)H * W, (const float*)nullptr, (size_t)0, 1.0f,
                         1.0f, d_az);                                                                              //        ... D_W   single:218
      WM_HIP(hipGetLastError());
      WM_HIP(hipStreamSynchronize(ctx->stream));       // (dv is a local)
      return WM_OK;
    }
  }
  WM_HIP(hipMemcpyAsync(w.dvec, sh.data(), sh.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  // Uw[:Lx,:Lx] * sh (column scaling) per plane: the first Lx rows of Uw (leading dimension L)
  hipLaunchKernelGGL(k_rf_scale_cols_b, dim3(8, Lx, p.B), dim3(256), 0, ctx->stream, d_uw, (size_t)0, d_us, (size_t)L * L, L,
                     w.dvec, (size_t)p.Lp);
  WM_HIP(hipMemsetAsync(d_out, 0, (size_t)p.B * H * W * 4, ctx->stream));                                     // single:215
  WM_TRY(sgemm_b(ctx, false, false, Lx, Lx, Lx, 1.0f, d_us, L, (size_t)L * L, d_vwt, W, 0, 0.0f, d_out, W, (size_t)H * W, p.B));  // single:214, 216-217 (Vwt[:L,:L]: ld W)
  WM_TRY(sgemm_b(ctx, true, false, H, W, H, 1.0f, dH, H, 0, d_out, W, (size_t)H * W, 0.0f, d_mid, W, (size_t)H * W, p.B));   // idct2: D_H^T X
  WM_TRY(sgemm_b(ctx, false, false, H, W, W, 1.0f, d_mid, W, (size_t)H * W, dW, W, 0, 0.0f, d_out, W, (size_t)H * W, p.B));  //        ... D_W   single:218
  WM_HIP(hipStreamSynchronize(ctx->stream));         // sh may be a local of the caller
  return WM_OK;
}

int ref_extract_core(wm_ctx* ctx, const RefPlan& p, const RefWs& w, const float* s_cw, const float* sigma_c,
                     const float* d_uw, const float* d_vwt, float* d_us, float* d_mid, float* d_out, float alpha, int K) {
  const int L = p.L;
  const float a = fmaxf(alpha, 1e-8f);
  std::vector<float> sh((size_t)p.B * p.Lp, 0.0f);
  for (int z = 0; z < p.B; ++z)
    for (int i = 0; i < K; ++i)
      sh[(size_t)z * p.Lp + i] = (s_cw[(size_t)z * L + i] - sigma_c[(size_t)z * L + i]) / a;                  // single:212-213
  return ref_reconstruct_core(ctx, p, w, sh, L, d_uw, d_vwt, d_us, d_mid, d_out);
}

double nc_score(const float* sw, const float* scw, const float* sc, int L, float alpha) {
  // _nc(Sw[:L], (S_cw - Sc) / max(alpha, 1e-8))     single:297-301, 284-289
  const float a = fmaxf(alpha, 1e-8f);
  std::vector<double> x(L), y(L);
  double sa = 0, sb = 0;
  for (int i = 0; i < L; ++i) { x[i] = sw[i]; y[i] = (double)((scw[i] - sc[i]) / a); sa += x[i]; sb += y[i]; }
  sa /= L; sb /= L;
  double cov = 0, va = 0, vb = 0;
  for (int i = 0; i < L; ++i) { const double dx = x[i] - sa, dy = y[i] - sb; cov += dx * dy; va += dx * dx; vb += dy * dy; }
  return cov / (sqrt(va) * sqrt(vb) + 1e-8);
}

// small device -> host copy of a float vector (meta-sized arrays of the *_dev entry points)
int fetch_f32(wm_ctx* ctx, const float* d, size_t n, std::vector<float>& h) {
  h.resize(n);
  if (n) {
    WM_HIP(hipMemcpyAsync(h.data(), d, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
  }
  return WM_OK;
}

}  // namespace

namespace wmi {
void hier_host_free(void* tab) { delete static_cast<HierTab*>(tab); }
}

// ===========================================================================
// C ABI (see include/wmhip.h)
// ===========================================================================
extern "C" {

// ---- device-pointer entry points: frames stay resident -------------------------------------
int wm_ref_sigma_planes_u8_dev(wm_ctx* ctx, const uint8_t* planes, float* sigma, int n_planes, int H, int W,
                               int row_stride, size_t plane_stride) {
  WM_TRY(check_ref_args(ctx, planes, n_planes, H, W, row_stride, plane_stride));
  if (!sigma) return set_err(WM_ERR_BADARG, "sigma is NULL");
  const RefPlan p = make_plan(H, W, n_planes);
  RefWs w;
  WM_TRY(plan_decompose_ws(ctx, p, w, 16));
  std::vector<float> sig((size_t)n_planes * p.L);
  WM_TRY(ref_sigma_core(ctx, p, w, planes, (size_t)row_stride, plane_stride, sig.data()));
  WM_HIP(hipMemcpyAsync(sigma, sig.data(), sig.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  return WM_OK;
}

int wm_ref_embed_planes_u8_dev(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego, float* sigma_c,
                               float* yw, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                               size_t sigma_w_plane_stride, float alpha, int K) {
  WM_TRY(check_ref_args(ctx, host, n_planes, H, W, row_stride, plane_stride));
  if (!sigma_w || !stego || !sigma_c) return set_err(WM_ERR_BADARG, "NULL argument");
  const RefPlan p = make_plan(H, W, n_planes);
  if (K < 0 || K > p.L) return set_err(WM_ERR_BADARG, "K must be in 0..min(H,W)");
  RefWs w;
  WM_TRY(plan_decompose_ws(ctx, p, w, 16));
  std::vector<float> sw, sc((size_t)n_planes * p.L);
  WM_TRY(fetch_f32(ctx, sigma_w, sigma_w_plane_stride ? (size_t)(n_planes - 1) * sigma_w_plane_stride + p.L : (size_t)p.L, sw));
  // pixels the tiles do not cover do not exist in this mode: every pixel of stego is written by the quantiser
  WM_TRY(ref_embed_core(ctx, p, w, host, stego, yw, (size_t)row_stride, plane_stride, sw.data(), sigma_w_plane_stride, sc.data(),
                        alpha, K));
  WM_HIP(hipMemcpyAsync(sigma_c, sc.data(), sc.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  return WM_OK;
}

int wm_ref_extract_planes_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                                 const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                                 size_t plane_stride, float alpha, int K) {
  WM_TRY(check_ref_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  if (!sigma_c || !Uw || !Vwt || !out) return set_err(WM_ERR_BADARG, "NULL argument");
  const RefPlan p = make_plan(H, W, n_planes);
  const int L = p.L;
  if (K < 0 || K > L) return set_err(WM_ERR_BADARG, "K must be in 0..min(H,W)");
  RefWs w;
  // tmp1: Uw diag(sh) [B][L][L];  tmp2: A0 [B][L][M] | T [B][L][Lp], reused afterwards as the GEMM intermediate [B][H][W]
  WM_TRY(plan_decompose_ws(ctx, p, w, (size_t)n_planes * L * L + 16, (size_t)n_planes * H * W));
  std::vector<float> s_cw((size_t)n_planes * L), sc;
  WM_TRY(ref_sigma_core(ctx, p, w, stego, (size_t)row_stride, plane_stride, s_cw.data()));                // single:205
  WM_TRY(fetch_f32(ctx, sigma_c, (size_t)n_planes * L, sc));
  return ref_extract_core(ctx, p, w, s_cw.data(), sc.data(), Uw, Vwt, w.tmp1, w.tmp2, out, alpha, K);
}

int wm_ref_detect_planes_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                                double* scores, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                float alpha) {
  WM_TRY(check_ref_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  if (!sigma_c || !sigma_w || !scores) return set_err(WM_ERR_BADARG, "NULL argument");
  const RefPlan p = make_plan(H, W, n_planes);
  RefWs w;
  WM_TRY(plan_decompose_ws(ctx, p, w, 16));
  std::vector<float> s_cw((size_t)n_planes * p.L), sc, sw;
  WM_TRY(ref_sigma_core(ctx, p, w, stego, (size_t)row_stride, plane_stride, s_cw.data()));
  WM_TRY(fetch_f32(ctx, sigma_c, (size_t)n_planes * p.L, sc));
  WM_TRY(fetch_f32(ctx, sigma_w, (size_t)p.L, sw));
  std::vector<double> sco(n_planes);
  for (int z = 0; z < n_planes; ++z)
    sco[z] = nc_score(sw.data(), &s_cw[(size_t)z * p.L], &sc[(size_t)z * p.L], p.L, alpha);
  WM_HIP(hipMemcpyAsync(scores, sco.data(), sco.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  return WM_OK;
}

// ---- host-pointer entry points ------------------------------------------------------------------
int wm_ref_sigma_planes_u8(wm_ctx* ctx, const uint8_t* planes, float* sigma, int n_planes, int H, int W,
                           int row_stride, size_t plane_stride) {
  WM_TRY(check_ref_args(ctx, planes, n_planes, H, W, row_stride, plane_stride));
  if (!sigma) return set_err(WM_ERR_BADARG, "sigma is NULL");
  const RefPlan p = make_plan(H, W, n_planes);
  RefWs w;
  const size_t n_in = plane_span(n_planes, H, row_stride, plane_stride, W);
  // tmp1: uint8 input span
  WM_TRY(plan_decompose_ws(ctx, p, w, (n_in + 3) / 4 + 4));
  uint8_t* d_in = (uint8_t*)w.tmp1;
  WM_HIP(hipMemcpyAsync(d_in, planes, n_in, hipMemcpyHostToDevice, ctx->stream));
  return ref_sigma_core(ctx, p, w, d_in, (size_t)row_stride, plane_stride, sigma);
}

int wm_ref_sigma_u8(wm_ctx* ctx, const uint8_t* plane, float* sigma, int H, int W, int row_stride) {
  return wm_ref_sigma_planes_u8(ctx, plane, sigma, 1, H, W, row_stride, (size_t)H * row_stride);
}

int wm_ref_embed_planes_u8_when(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, const int* sigma_w_ready,
                                uint8_t* stego, float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                                size_t plane_stride, size_t sigma_w_plane_stride, float alpha, int K) {
  WM_TRY(check_ref_args(ctx, host, n_planes, H, W, row_stride, plane_stride));
  if (!sigma_w || !stego || !sigma_c) return set_err(WM_ERR_BADARG, "NULL argument");
  const RefPlan p = make_plan(H, W, n_planes);
  if (K < 0 || K > p.L) return set_err(WM_ERR_BADARG, "K must be in 0..min(H,W)");
  RefWs w;
  const size_t n_in = plane_span(n_planes, H, row_stride, plane_stride, W);
  const size_t n_in16 = (n_in + 15) & ~(size_t)15;
  const size_t yw_elems = yw ? (size_t)n_planes * H * W : 0;
  // tmp1: uint8 input + output spans (+ dense float Yw for the caller)
  WM_TRY(plan_decompose_ws(ctx, p, w, (2 * n_in16) / 4 + 8 + yw_elems));
  uint8_t* d_in = (uint8_t*)w.tmp1;
  uint8_t* d_out = d_in + n_in16;
  float* d_ywout = yw ? (float*)(d_out + n_in16) : nullptr;
  WM_HIP(hipMemcpyAsync(d_in, host, n_in, hipMemcpyHostToDevice, ctx->stream));
  // bytes between rows / planes that belong to the caller's stego buffer are carried through
  if (stego != host) WM_HIP(hipMemcpyAsync(d_out, stego, n_in, hipMemcpyHostToDevice, ctx->stream));
  else WM_HIP(hipMemcpyAsync(d_out, d_in, n_in, hipMemcpyDeviceToDevice, ctx->stream));
  WM_TRY(ref_embed_core(ctx, p, w, d_in, d_out, d_ywout, (size_t)row_stride, plane_stride, sigma_w, sigma_w_plane_stride, sigma_c,
                        alpha, K, sigma_w_ready));
  WM_HIP(hipMemcpyAsync(stego, d_out, n_in, hipMemcpyDeviceToHost, ctx->stream));
  if (yw) WM_HIP(hipMemcpyAsync(yw, d_ywout, yw_elems * 4, hipMemcpyDeviceToHost, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  return WM_OK;
}

int wm_ref_embed_planes_u8(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego, float* sigma_c,
                           float* yw, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                           size_t sigma_w_plane_stride, float alpha, int K) {
  return wm_ref_embed_planes_u8_when(ctx, host, sigma_w, nullptr, stego, sigma_c, yw, n_planes, H, W, row_stride, plane_stride,
                                     sigma_w_plane_stride, alpha, K);
}

int wm_ref_embed_u8(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego, float* sigma_c,
                    float* yw, int H, int W, int row_stride, float alpha, int K) {
  return wm_ref_embed_planes_u8(ctx, host, sigma_w, stego, sigma_c, yw, 1, H, W, row_stride,
                                (size_t)H * row_stride, 0, alpha, K);
}

// thin SVD of dct2(plane) (apply_dct != 0) or of the plane itself: U [H x L], S [L], Vt [L x W]
// Watermark-side SVD of n_planes planes (the B, G, R planes of a colour watermark, single:128-134) in ONE batch: a single
// full-frame SVD is latency-bound on a fraction of the chip, three planes in every launch cost 1.4 x one.
//   planes [n][H][row_stride..] float32 host, U [n][H][L], S [n][L], Vt [n][L][W] host
int wm_ref_svd_planes_f32(wm_ctx* ctx, const float* planes, float* U, float* S, float* Vt, int n_planes, int H, int W,
                          int row_stride, size_t plane_stride, int apply_dct) {
  WM_TRY(check_ref_args(ctx, planes, n_planes, H, W, row_stride, plane_stride));
  if (!U || !S || !Vt) return set_err(WM_ERR_BADARG, "U/S/Vt is NULL");
  const int B = n_planes;
  const RefPlan p = make_plan(H, W, B);
  RefWs w;
  const size_t n_in = plane_span(B, H, row_stride, plane_stride, W);
  const size_t n_in_a = (n_in + 63) & ~(size_t)63, hw = (size_t)H * W, fl = (size_t)p.L * (p.M + p.L), lp64 = ((size_t)p.Lp + 63) & ~(size_t)63;
  // tmp1: input planes | DCT planes [B][H][W] | every plane's sorted factors in the caller's layout, U [H][L] | Vt [L][W] | per plane: order, 1 / |q_i|,
  // 1 / |b_i|;  tmp2: DCT intermediate [B][H][W], then T = A0 B^T [B][L][Lp]
  WM_TRY(plan_workspace(ctx, p, w, n_in_a + (size_t)B * hw + (size_t)B * fl + 3 * (size_t)B * lp64, std::max((size_t)B * hw, (size_t)B * p.L * p.Lp)));
  float* d_in = w.tmp1;
  float* d_c = d_in + n_in_a;            // [B][H][W]
  float* d_f = d_c + (size_t)B * hw;     // [B]( U [H][L] | Vt [L][W] )
  int* d_ord = (int*)(d_f + (size_t)B * fl);
  float* d_sq = (float*)(d_ord + (size_t)B * lp64);
  float* d_sb = d_sq + (size_t)B * lp64;
  WM_HIP(hipMemcpyAsync(d_in, planes, n_in * 4, hipMemcpyHostToDevice, ctx->stream));
  const float* src = d_in; size_t src_stride = (size_t)row_stride, src_ps = plane_stride;
  if (apply_dct) {
    float *dH, *dW;
    WM_TRY(get_dct_pair(ctx, H, W, &dH, &dW));
    WM_TRY(sgemm_b(ctx, false, false, H, W, H, 1.0f, dH, H, 0, d_in, row_stride, plane_stride, 0.0f, w.tmp2, W, hw, B));   // D_H X
    WM_TRY(sgemm_b(ctx, false, true, H, W, W, 1.0f, w.tmp2, W, hw, dW, W, 0, 0.0f, d_c, W, hw, B));                      // (D_H X) D_W^T
    src = d_c; src_stride = (size_t)W; src_ps = hw;
  }
  hipLaunchKernelGGL((k_rf_load<float>), dim3(8, p.Lp, B), dim3(256), 0, ctx->stream, src, src_stride, src_ps,
                     p.transpose ? 1 : 0, w.aug, p.aug_ps, p.ld, p.L, p.Lp, p.M);
  int sweeps = 0;
  WM_TRY(jacobi_rows(ctx, p, w, JR_SVD, &sweeps));
  if (sweeps < 0) return set_err(WM_ERR_NOCONV, "SVD did not converge");
  std::vector<double> b2, q2;
  WM_TRY(fetch_norms(ctx, p, w, true, b2, q2));
  // Singular values.  |b_i| / |q_i| is exact as long as B = Qt A holds, but the two parts of a row round
  // independently through ~1e5 MFMA row updates: measured 7e-5 relative low at 8K (3e-5 at 1080p), the same for
  // every value.  Like the sigma-only path (fetch_norms_t) the large values are therefore measured on the untouched
  // input, s_i = |A0 b_i^T| / |b_i| (error c^2 (s_max / s_i)^2 / 2 with the residual cosine c <= ref_skip_thr), and
  // the ratio of the two estimates there (median) calibrates |b_i| / |q_i| for the values below the switch (spectrum_rule;
  // a row that is residue keeps its |b_i| / |q_i| here: its slot is completed below).
  float* d_T = w.tmp2;
  WM_TRY(sgemm_b(ctx, p.transpose, true, p.L, p.Lp, p.M, 1.0f, src, (int)src_stride, src_ps, w.aug, p.ld, p.aug_ps, 0.0f, d_T, p.Lp,
                 (size_t)p.L * p.Lp, B));
  hipLaunchKernelGGL(k_rf_colnorms, dim3((p.Lp + 63) / 64, B), dim3(256), 0, ctx->stream, d_T, (size_t)p.L * p.Lp, p.L, p.Lp, w.q2);
  WM_HIP(hipGetLastError());
  std::vector<double> t2all((size_t)B * p.Lp);
  WM_HIP(hipMemcpyAsync(t2all.data(), w.q2, t2all.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<float> sq((size_t)B * lp64, 0.0f), sb((size_t)B * lp64, 0.0f), sig;
  std::vector<int> order, ord_all((size_t)B * lp64, 0);
  struct NullRows { int z; std::vector<unsigned char> valid; std::vector<int> slots; };
  std::vector<NullRows> todo;                           // rank-deficient planes: slots of the long-side factor to complete
  for (int z = 0; z < B; ++z) {
    double* b2z = &b2[(size_t)z * p.Lp]; const double* q2z = &q2[(size_t)z * p.Lp];
    std::vector<double> q2s(q2z, q2z + p.Lp);           // q2 itself still normalises the columns of the short-side factor
    spectrum_rule(p.Lp, b2z, q2s.data(), &t2all[(size_t)z * p.Lp], (double)ctx->ref_skip_thr, false, true, -1, nullptr);
    sort_sigma(p, b2z, q2s.data(), order, sig);
    memcpy(S + (size_t)z * p.L, sig.data(), (size_t)p.L * 4);
    // short-side factor: columns q_i/|q_i|   (rows of Qt), long-side factor: rows b_i/|b_i|
    // A row of B at or below the Jacobi's numerical-null floor is rounding residue of a rank-deficient plane, not a singular
    // direction: its slot is completed below.
    const double floor2 = null_floor2(b2z, p.Lp);
    NullRows nr; nr.z = z; nr.valid.assign(p.Lp, 0);
    for (int i = 0; i < p.Lp; ++i) nr.valid[i] = b2z[i] > floor2 ? 1 : 0;
    for (int k = 0; k < p.L; ++k) {
      const int i = order[k];
      ord_all[(size_t)z * lp64 + k] = i;
      sq[(size_t)z * lp64 + k] = q2z[i] > 0 ? (float)(1.0 / sqrt(q2z[i])) : 0.0f;
      sb[(size_t)z * lp64 + k] = b2z[i] > 0 ? (float)(1.0 / sqrt(b2z[i])) : 0.0f;
      if (!nr.valid[i]) nr.slots.push_back(k);
    }
    if (!nr.slots.empty()) todo.push_back(std::move(nr));
  }
  WM_HIP(hipMemcpyAsync(d_ord, ord_all.data(), ord_all.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  WM_HIP(hipMemcpyAsync(d_sq, sq.data(), sq.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  WM_HIP(hipMemcpyAsync(d_sb, sb.data(), sb.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  // The factors leave the device in the caller's layout (round 3 downloaded both sorted factors row-major and transposed one
  // of them on the host, element by element: 5 - 10 ms of a 1080p call, ~0.3 s of an 8K one).
  //   A = X   (H <= W): U[r][k] = q_k[r] / |q_k|  (transposing gather of the Qt part),  Vt[k][c] = b_k[c] / |b_k|  (straight)
  //   A = X^T (H >  W): U[r][k] = b_k[r] / |b_k|  (transposing gather of the B part),   Vt[k][c] = q_k[c] / |q_k|  (straight)
  float* d_u = d_f; float* d_vt = d_f + (size_t)H * p.L;
  const int lp = (int)lp64;
  if (!p.transpose) {
    hipLaunchKernelGGL(k_rf_gather_rows_t, dim3((p.L + 31) / 32, (p.L + 31) / 32, B), dim3(256), 0, ctx->stream, w.aug + p.M, p.aug_ps, p.ld,
                       p.L, p.L, d_ord, d_sq, lp, d_u, fl, p.L);
    hipLaunchKernelGGL(k_rf_gather_rows_b, dim3(8, p.L, B), dim3(256), 0, ctx->stream, w.aug, p.aug_ps, p.ld, p.M, d_ord, d_sb, lp, d_vt, fl, W);
  } else {
    hipLaunchKernelGGL(k_rf_gather_rows_t, dim3((p.M + 31) / 32, (p.L + 31) / 32, B), dim3(256), 0, ctx->stream, w.aug, p.aug_ps, p.ld,
                       p.M, p.L, d_ord, d_sb, lp, d_u, fl, p.L);
    hipLaunchKernelGGL(k_rf_gather_rows_b, dim3(8, p.L, B), dim3(256), 0, ctx->stream, w.aug + p.M, p.aug_ps, p.ld, p.L, d_ord, d_sq, lp, d_vt, fl, W);
  }
  WM_HIP(hipGetLastError());
  for (const NullRows& nr : todo) {                     // full-rank planes: nothing to do, the factors are the gathered rows
    float* fu = d_u + (size_t)nr.z * fl; float* fv = d_vt + (size_t)nr.z * fl;
    const double* nb = &b2[(size_t)nr.z * p.Lp]; const double* nq = &q2[(size_t)nr.z * p.Lp];
    if (!p.transpose) {
      WM_TRY(ref_complete_factor(ctx, p, w, nr.z, 0, nr.valid, nb, nr.slots, fv, (size_t)W, 1));            // rows of Vt
      WM_TRY(ref_complete_factor(ctx, p, w, nr.z, 1, nr.valid, nq, nr.slots, fu, 1, (size_t)p.L));          // columns of U
    } else {
      WM_TRY(ref_complete_factor(ctx, p, w, nr.z, 0, nr.valid, nb, nr.slots, fu, 1, (size_t)p.L));          // columns of U
      WM_TRY(ref_complete_factor(ctx, p, w, nr.z, 1, nr.valid, nq, nr.slots, fv, (size_t)W, 1));            // rows of Vt
    }
  }
  for (int z = 0; z < B; ++z) {
    WM_HIP(hipMemcpyAsync(U + (size_t)z * H * p.L, d_u + (size_t)z * fl, (size_t)H * p.L * 4, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipMemcpyAsync(Vt + (size_t)z * p.L * W, d_vt + (size_t)z * fl, (size_t)p.L * W * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  WM_HIP(hipStreamSynchronize(ctx->stream));
  return WM_OK;
}

int wm_ref_svd_f32(wm_ctx* ctx, const float* plane, float* U, float* S, float* Vt, int H, int W,
                   int row_stride, int apply_dct) {
  return wm_ref_svd_planes_f32(ctx, plane, U, S, Vt, 1, H, W, row_stride, (size_t)H * row_stride, apply_dct);
}


// extract: n_planes stego planes share one watermark decomposition (frames of a video): their SVDs
// run batched, the three GEMMs per plane run as one launch each (grid.z = plane).
int wm_ref_extract_planes_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                             const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                             size_t plane_stride, float alpha, int K) {
  WM_TRY(check_ref_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  if (!sigma_c || !Uw || !Vwt || !out) return set_err(WM_ERR_BADARG, "NULL argument");
  const RefPlan p = make_plan(H, W, n_planes);
  const int L = p.L;
  if (K < 0 || K > L) return set_err(WM_ERR_BADARG, "K must be in 0..min(H,W)");
  RefWs w;
  const size_t n_in = plane_span(n_planes, H, row_stride, plane_stride, W);
  const size_t n_in4 = (n_in + 3) / 4 + 4;
  // tmp1: uint8 stego span | Uw[:L,:L] | Vwt [L][W] | Uw diag(sh) [B][L][L] | result [B][H][W]
  // tmp2: A0 [B][L][M] | T [B][L][Lp], reused afterwards as the GEMM intermediate [B][H][W]
  WM_TRY(plan_decompose_ws(ctx, p, w, n_in4 + (size_t)L * L + (size_t)L * W + (size_t)n_planes * L * L + (size_t)n_planes * H * W,
                           (size_t)n_planes * H * W));
  uint8_t* d_in = (uint8_t*)w.tmp1;
  float* d_u = w.tmp1 + n_in4; float* d_v = d_u + (size_t)L * L; float* d_us = d_v + (size_t)L * W;
  float* d_full = d_us + (size_t)n_planes * L * L;
  WM_HIP(hipMemcpyAsync(d_in, stego, n_in, hipMemcpyHostToDevice, ctx->stream));
  WM_HIP(hipMemcpyAsync(d_u, Uw, (size_t)L * L * 4, hipMemcpyHostToDevice, ctx->stream));            // Uw[:L,:L] (H x L, rows < L)
  WM_HIP(hipMemcpyAsync(d_v, Vwt, (size_t)L * W * 4, hipMemcpyHostToDevice, ctx->stream));           // Vwt [L][W]; [:L,:L] = leading dimension W
  std::vector<float> s_cw((size_t)n_planes * L);
  WM_TRY(ref_sigma_core(ctx, p, w, d_in, (size_t)row_stride, plane_stride, s_cw.data()));                 // single:205
  WM_TRY(ref_extract_core(ctx, p, w, s_cw.data(), sigma_c, d_u, d_v, d_us, w.tmp2, d_full, alpha, K));
  WM_HIP(hipMemcpyAsync(out, d_full, (size_t)n_planes * H * W * 4, hipMemcpyDeviceToHost, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  return WM_OK;
}

int wm_ref_extract_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw, const float* Vwt,
                      float* out, int H, int W, int row_stride, float alpha, int K) {
  return wm_ref_extract_planes_u8(ctx, stego, sigma_c, Uw, Vwt, out, 1, H, W, row_stride, (size_t)H * row_stride,
                                  alpha, K);
}

// single:214-218 on its own, with the estimates given: the drop-in uses it when the stego's size is not the meta's (a
// resized or cropped stego - the reference goes on with L = the shortest of the four lengths, single:210)
int wm_ref_reconstruct_f32(wm_ctx* ctx, const float* Uw, const float* sw_hat, const float* Vwt, float* out, int H, int W,
                           int L) {
  WM_TRY(check_ref_args(ctx, Uw, 1, H, W, W, (size_t)H * W));
  if (!sw_hat || !Vwt || !out) return set_err(WM_ERR_BADARG, "NULL argument");
  const RefPlan p = make_plan(H, W, 1);
  const int Lm = p.L;
  if (L < 0 || L > Lm) return set_err(WM_ERR_BADARG, "L must be in 0..min(H,W)");
  RefWs w;
  // tmp1: Uw[:Lm,:Lm] | Vwt [Lm][W] | Uw diag(sh) [Lm][Lm] | result [H][W];  tmp2: GEMM intermediate [H][W]
  WM_TRY(plan_workspace(ctx, p, w, 2 * (size_t)Lm * Lm + (size_t)Lm * W + (size_t)H * W + 16, (size_t)H * W));
  float* d_u = w.tmp1; float* d_v = d_u + (size_t)Lm * Lm; float* d_us = d_v + (size_t)Lm * W;
  float* d_full = d_us + (size_t)Lm * Lm;
  WM_HIP(hipMemcpyAsync(d_u, Uw, (size_t)Lm * Lm * 4, hipMemcpyHostToDevice, ctx->stream));          // Uw[:Lm,:Lm] (H x Lm, rows < Lm)
  WM_HIP(hipMemcpyAsync(d_v, Vwt, (size_t)Lm * W * 4, hipMemcpyHostToDevice, ctx->stream));
  std::vector<float> sh((size_t)p.Lp, 0.0f);
  for (int i = 0; i < L; ++i) sh[i] = sw_hat[i];
  if (L == 0) {
    WM_HIP(hipMemsetAsync(d_full, 0, (size_t)H * W * 4, ctx->stream));       // idct2 of the zero plane
  } else {
    WM_TRY(ref_reconstruct_core(ctx, p, w, sh, L, d_u, d_v, d_us, w.tmp2, d_full));
  }
  WM_HIP(hipMemcpyAsync(out, d_full, (size_t)H * W * 4, hipMemcpyDeviceToHost, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  return WM_OK;
}

int wm_ref_last_flops(wm_ctx* ctx, double* flops_out, int* two_level_out) {
  if (!ctx || !flops_out || !two_level_out) return set_err(WM_ERR_BADARG, "NULL argument");
  *flops_out = ctx->ref_last_flops; *two_level_out = ctx->ref_last_hier;
  return WM_OK;
}

// outer sweeps the last full-frame SVD on this context took (for flop accounting)
int wm_ref_last_sweeps(wm_ctx* ctx, int* sweeps_out) {
  if (!ctx || !sweeps_out) return set_err(WM_ERR_BADARG, "NULL argument");
  *sweeps_out = ctx->ref_last_sweeps;
  return WM_OK;
}

// detect over n_planes stego planes of one watermark (frames of a clip): batched SVDs, NC per plane
int wm_ref_detect_planes_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                            double* scores, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                            float alpha) {
  WM_TRY(check_ref_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  if (!sigma_c || !sigma_w || !scores) return set_err(WM_ERR_BADARG, "NULL argument");
  const int L = std::min(H, W);
  std::vector<float> s_cw((size_t)n_planes * L);
  WM_TRY(wm_ref_sigma_planes_u8(ctx, stego, s_cw.data(), n_planes, H, W, row_stride, plane_stride));
  for (int z = 0; z < n_planes; ++z)
    scores[z] = nc_score(sigma_w, &s_cw[(size_t)z * L], sigma_c + (size_t)z * L, L, alpha);
  return WM_OK;
}

int wm_ref_detect_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                     double* score, int H, int W, int row_stride, float alpha) {
  return wm_ref_detect_planes_u8(ctx, stego, sigma_c, sigma_w, score, 1, H, W, row_stride, (size_t)H * row_stride, alpha);
}

}  // extern "C"
