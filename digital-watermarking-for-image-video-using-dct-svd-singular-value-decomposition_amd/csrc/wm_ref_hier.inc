// Hierarchical (two-level) block Jacobi of the full-frame mode - included by wm_ref.hip inside its anonymous namespace.
//
// The flat scheme (k_rf_gram -> k_rf_inner -> k_rf_apply per tournament step) streams every row of the plane three
// times per step, 99 passes per sweep at 1080p, and runs at the memory system's speed (profiles/r04_a_fullframe_*).
// Here the 32-row blocks are grouped into SUPER-BLOCKS of up to 6; a level-1 tournament step pairs super-blocks, and
// for each super-pair (n <= 12 blocks, <= 384 rows X_s):
//   1. k_hgram_t + k_hreduce  G_s = X_s X_s^T  (one read of the rows, 128 x 128 MFMA tiles, split over column ranges)
//   2. stages of a sub-tournament among the n blocks (all of them in the first step of a sweep, the bipartite
//      cross pairs afterwards): k_rf_inner reads each block pair's 64 x 64 Gram matrix straight out of G_s, solves it
//      and writes the rotated diagonal block back (and R, also in the order k_happly consumes it); k_hupdate keeps the
//      rest of G_s up to date two-sidedly (G_pq <- R_p^T G_pq R_q).  Only the n32 x n32 matrix is touched.
//   3. k_happly              X_s <- P_T^T .. P_1^T X_s: the stages' rotations applied one after the other to a strip of
//                            the rows held in LDS (one read and one write of the rows)
// so the rows are streamed 3 times per SUPER-step (15 passes per sweep at 1080p with super-blocks of 6) for the
// same rotations, pair for pair, as 6 flat steps.  The ordering is a cyclic one (every pair of rows meets once per
// sweep): tools/hier_order_study.py counts the same or fewer sweeps than the flat tournament.
// Everything is deterministic (fixed summation orders, no float atomics).

constexpr int HT_MAX = HSB - 1;               // most stages of a super-step (full tournament over 12 blocks)
constexpr int HG_T = 128;                     // Gram tile edge
constexpr int HG_TILES = 6;                   // 128 x 128 tiles (ti <= tj) of a 384 x 384 matrix: (0,0) (0,1) (1,1) (0,2) (1,2) (2,2)
constexpr int HG_KC = 32;                     // columns per staged chunk
constexpr int HG_KS_MAX = 8;                  // most column splits of a Gram tile

struct HSuper { int n; int blk[HSB]; };       // a super-pair: n blocks, their global block indices in local order

__device__ __forceinline__ int hg_tile_i(const int tile) { return (tile == 0 || tile == 1 || tile == 3) ? 0 : (tile == 2 || tile == 4) ? 1 : 2; }
__device__ __forceinline__ int hg_tile_j(const int tile) { return tile == 0 ? 0 : tile <= 2 ? 1 : 2; }
__device__ __forceinline__ int hg_tile_of(const int ti, const int tj) { return tj == 0 ? 0 : tj == 1 ? 1 + ti : 3 + ti; }

constexpr int CU_LDS_BYTES = 160 * 1024;      // LDS of one CU (gfx950)

// ---------------------------------------------------------------------------
// partial[z][sp][tile][ks] = X_a X_b^T over the column range of split ks; X_a / X_b = 128-row panels of super-pair sp.
// One workgroup (512 threads) stages TWO panels (a, b = a + 1 mod np) per chunk of 32 columns and computes the diagonal
// tile (a, a) with waves 0-3 and the tile (a, b) with waves 4-7 - each wave a 64 x 64 quadrant as 2 x 2 MFMA tiles.  With
// three panels the workgroups (0,1), (1,2), (2,0) cover all six tiles of the symmetric matrix from 768 staged rows.
// Why this shape (in-kernel stamps, profiles/r04_hier_kernels.md): a wave sits ~900 cycles in the issue of every 1 KB
// load (a CU takes 5 - 10 B/clk from beyond L2), so the first version - one 128 x 128 tile per 256-thread workgroup,
// 1 152 staged rows per group - spent 7 000 of a chunk's 12 000 cycles issuing its loads; here a chunk's loads are 4 per
// thread for 64 MFMAs per wave, spread over the MFMA steps.
// One matrix-core chain per workgroup column range (<= a few hundred columns); k_hreduce adds the ranges on the VALU, so the
// accumulation is two-level like the flat kernel's.
// F16 selects the LDS image, the stash and the MFMA group; everything else is one skeleton:
//  * f32 (float inputs, WM_RF_HIER_F16 bit 0 clear): image k-major ([k][row], pitch 257: operand reads of 32 consecutive rows
//    are conflict-free), v_mfma_f32_32x32x2_f32, the next chunk's loads one every four MFMA steps;
//  * split f16 (the default for uint8 planes): x = hi + lo (split4_f16; 22 significant bits together), X_a X_b^T ~ hi hi^T +
//    hi lo^T + lo hi^T accumulated in f32 - three v_mfma_f32_32x32x16_f16 (32 cycles, 16 values of k each) where the f32 form
//    issues eight v_mfma_f32_32x32x2_f32 (64 cycles, 2 values of k each): 5.3 x fewer matrix-pipe cycles.  What is dropped
//    (lo lo^T, and lo itself for |x| < 0.125 where it is an f16 denormal) is below 2^-22 of the products' magnitude: the Gram
//    entries only steer the rotations, and every row entry is bounded by 255 sqrt(L) < 65 504 (f16's range) up to 8K planes
//    because the rotations are orthogonal.  Rows are converted once, while they are staged: the image is row-major f16
//    ([row][k], pitch 40 halfs = 80 bytes: a lane's 16-byte operand reads are conflict-free), two loads per MFMA step.
// Both images are double-buffered (one barrier per chunk).
// Reproducibility: ONE workgroup of the f16 form per CU, enforced by its LDS footprint (84.5 KB with the padding rows): with
// two of them co-resident (a single-image form, 40 KB each, was 2 % faster) G_s differed from run to run at 1080p - sigma off
// by up to 7e-5 sigma_1, 13 or 14 sweeps - although they share no LDS and write disjoint partial sums; neither an extra
// barrier per chunk nor 96 instead of 126 VGPRs changed that, one workgroup per CU is bit-reproducible (HISTORY.md).
// ---------------------------------------------------------------------------
constexpr int HG_HP = 40;                     // halfs per row of the f16 image (32 + 8 of padding)
constexpr int HG_NB = 2;                      // LDS images in flight
constexpr int HG_PADROWS = 8;                 // rows of the f16 image that only hold its footprint above half a CU's LDS

template <bool F16>
__global__ __launch_bounds__(512, 1) void k_hgram_t(const float* __restrict__ aug, const size_t aug_ps, const int ld, const int M,
                                                    const HSuper* __restrict__ supers, const int nsp, float* __restrict__ partials,
                                                    const int KS, const int cps, const int npmax, const int nz) {
  // the image of the instance's form (the other form's arrays shrink to one unused element and take no LDS)
  __shared__ float S[F16 ? 1 : HG_NB][F16 ? 1 : HG_KC][F16 ? 1 : 2 * HG_T + 1];
  __shared__ __attribute__((aligned(16))) _Float16 Sh[F16 ? HG_NB : 1][F16 ? 2 * HG_T + HG_PADROWS : 1][F16 ? HG_HP : 8];
  __shared__ __attribute__((aligned(16))) _Float16 Sl[F16 ? HG_NB : 1][F16 ? 2 * HG_T + HG_PADROWS : 1][F16 ? HG_HP : 8];
  static_assert(!F16 || (sizeof(Sh) + sizeof(Sl) == 84480 && 2 * (sizeof(Sh) + sizeof(Sl)) > CU_LDS_BYTES),
                "two workgroups of the f16 form must not fit one CU: co-resident they are not bit-reproducible");
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63, j = lane & 31, h = lane >> 5;
  int w, sp, ks, zl;
  const int grp = xcd_group(blockIdx.x, npmax, w);
  if (grp >= nsp * KS * nz) return;
  group_decode(grp, nsp, KS, sp, ks, zl);
  // the block numbers of this thread's rows, fetched together with the super-pair's size (panel pb = (w + 1) % np is w + 1 or 0:
  // both candidates are read) - one round trip to L2 in front of the row loads instead of two
  const int bsel = (t >> 8);             // rows (t >> 3) + 64 i of a panel lie in block 4 panel + (t >> 8) + 2 i
  int blk_a[2], blk_b1[2], blk_b0[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    blk_a[i] = supers[sp].blk[min(4 * w + bsel + 2 * i, HSB - 1)];
    blk_b1[i] = supers[sp].blk[min(4 * (w + 1) + bsel + 2 * i, HSB - 1)];
    blk_b0[i] = supers[sp].blk[bsel + 2 * i];
  }
  const int n = supers[sp].n, n32 = n * RB;
  const int np = (n32 + HG_T - 1) / HG_T;                  // panels of this super-pair
  if (w >= np) return;
  const int pa = w, pb = (w + 1) % np;
  const bool second = np == 3 || (np == 2 && w == 0);      // the tile (pa, pb) is this workgroup's to compute
  aug += (size_t)zl * aug_ps;
  const int nchunk = (M + HG_KC - 1) / HG_KC;
  const int c_begin = ks * cps, c_end = min(nchunk, c_begin + cps);
  // thread t stages row (t >> 3) + 64 i of the 256-row image (i < 2: panel pa, i >= 2: panel pb), columns 4 (t & 7) .. + 3
  const float* rowp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (t >> 3) + 64 * (i & 1), lr = HG_T * (i < 2 ? pa : pb) + r;
    const int bk = i < 2 ? blk_a[i & 1] : (pb == 0 ? blk_b0[i & 1] : blk_b1[i & 1]);
    rowp[i] = ((i < 2 || second) && lr < n32) ? aug + (size_t)(bk * RB + (lr & 31)) * ld : nullptr;
  }
  const int cq = 4 * (t & 7);
  float4 rr[4];
  auto fetch1 = [&](const int c, const int i) {            // one of the 4 loads of chunk c
    const int col = c * HG_KC + cq;                        // col + 3 < ld always (ld >= M + 64)
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (rowp[i]) v = *reinterpret_cast<const float4*>(rowp[i] + col);
    MASK_TAIL4(v, col, M);
    rr[i] = v;
  };
  auto stash = [&](const int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (t >> 3) + 64 * i;
      if constexpr (F16) {
        uint2 hi, lo;
        split4_f16(rr[i], hi, lo);
        *reinterpret_cast<uint2*>(&Sh[buf][r][cq]) = hi;
        *reinterpret_cast<uint2*>(&Sl[buf][r][cq]) = lo;
      } else {
        S[buf][cq][r] = rr[i].x; S[buf][cq + 1][r] = rr[i].y; S[buf][cq + 2][r] = rr[i].z; S[buf][cq + 3][r] = rr[i].w;
      }
    }
  };
  const int tsel = wv >> 2, wi = (wv >> 1) & 1, wj = wv & 1;
  const bool idle = (tsel == 0 && wi == 1 && wj == 0) || (tsel == 1 && !second);   // mirrored quadrant of the diagonal tile / no second tile
  v16f acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = v16f{0};
  if (c_begin < c_end) {
#pragma unroll
    for (int i = 0; i < 4; ++i) fetch1(c_begin, i);
  }
  int buf = 0;
  for (int c = c_begin; c < c_end; ++c, buf = (buf + 1) % HG_NB) {
    stash(buf);
    const bool more = c + 1 < c_end;
    if (more && idle) {
#pragma unroll
      for (int i = 0; i < 4; ++i) fetch1(c + 1, i);
    }
    __syncthreads();
    if (idle) continue;
    // the next chunk's loads are spread over this chunk's MFMA steps
    if constexpr (F16) {
      const int ra = 64 * wi + j, rb = HG_T * tsel + 64 * wj + j;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {                 // two MFMA steps of 16 values of k; lane half h takes 8 of them
        if (more) { fetch1(c + 1, 2 * s2); fetch1(c + 1, 2 * s2 + 1); }
        h8_t ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
          ah[x] = *reinterpret_cast<const h8_t*>(&Sh[buf][ra + 32 * x][16 * s2 + 8 * h]);
          al[x] = *reinterpret_cast<const h8_t*>(&Sl[buf][ra + 32 * x][16 * s2 + 8 * h]);
          bh[x] = *reinterpret_cast<const h8_t*>(&Sh[buf][rb + 32 * x][16 * s2 + 8 * h]);
          bl[x] = *reinterpret_cast<const h8_t*>(&Sl[buf][rb + 32 * x][16 * s2 + 8 * h]);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) mfma3_f16(ah[a], al[a], bh[b], bl[b], acc[a][b]);
      }
    } else {
      const float* pA = &S[buf][h][64 * wi + j];
      const float* pB = &S[buf][h][HG_T * tsel + 64 * wj + j];
#pragma unroll
      for (int kk = 0; kk < HG_KC / 2; ++kk) {
        if (more && (kk & 3) == 0) fetch1(c + 1, kk >> 2);
        const float a0 = pA[2 * kk * (2 * HG_T + 1)], a1 = pA[2 * kk * (2 * HG_T + 1) + 32];
        const float b0 = pB[2 * kk * (2 * HG_T + 1)], b1 = pB[2 * kk * (2 * HG_T + 1) + 32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
  }
  if (idle) return;
  // the tile in the upper triangle that this quadrant belongs to; (2, 0) is stored as the transpose of (0, 2)
  const int ta = tsel == 0 ? pa : min(pa, pb), tb = tsel == 0 ? pa : max(pa, pb);
  const bool tr = tsel == 1 && pa > pb;
  float* out = partials + ((((size_t)zl * nsp + sp) * HG_TILES + hg_tile_of(ta, tb)) * KS + ks) * (HG_T * HG_T);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = ACC_ROW(v, h, 64 * wi + 32 * a), col = 64 * wj + 32 * b + j;
        out[tr ? col * HG_T + row : row * HG_T + col] = acc[a][b][v];
      }
}

// ---------------------------------------------------------------------------
// The split-f16 Gram tiles for super-pairs of three panels (more than 256 rows): ONE workgroup per (super-pair, plane, split) stages all
// <= 384 rows of a 32-column chunk once and computes the whole upper triangle of G_s from them - 78 blocks of 32 x 32, six or
// seven per wave (768 threads), each one accumulator tile.  The two-panel form loads every panel twice (three workgroups x 256
// rows for the same six tiles) and is bound by what a CU can fetch (10 B/clk): here the rows are fetched once.
// LDS: the split image [384][40] halfs x 2 (hi, lo), double-buffered: 123 KB - one workgroup per CU (see the note on
// reproducibility above k_hgram_t).  A wave's blocks are consecutive in row-major order, so most of them share their row block
// (the A operand is re-read only when it changes).  Same partial-sum layout as k_hgram_t (k_hreduce reads either).
// ---------------------------------------------------------------------------
constexpr int H3_NT = 768, H3_NW = H3_NT / 64, H3_TASKS = HSB * (HSB + 1) / 2, H3_TPW = (H3_TASKS + H3_NW - 1) / H3_NW;

__global__ __launch_bounds__(H3_NT) void k_hgram_h3(const float* __restrict__ aug, const size_t aug_ps, const int ld, const int M,
                                                   const HSuper* __restrict__ supers, const int nsp, float* __restrict__ partials,
                                                   const int KS, const int cps, const int nz) {
  __shared__ __attribute__((aligned(16))) _Float16 Sh[2][HN][HG_HP];
  __shared__ __attribute__((aligned(16))) _Float16 Sl[2][HN][HG_HP];
  static_assert(sizeof(Sh) + sizeof(Sl) == 122880 && 2 * (sizeof(Sh) + sizeof(Sl)) > CU_LDS_BYTES, "one workgroup per CU, like k_hgram_t<true>");
  const int t = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, j = lane & 31, h = lane >> 5;
  int w, sp, ks, zl;                     // (one workgroup per group: w = 0)
  const int grp = xcd_group(blockIdx.x, 1, w);
  if (grp >= nsp * KS * nz) return;
  group_decode(grp, nsp, KS, sp, ks, zl);
  // this thread's four rows of the image, (t >> 3) + 96 i: their block numbers fetched together with the super-pair's size
  int blk[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) blk[i] = supers[sp].blk[min(((t >> 3) + 96 * i) >> 5, HSB - 1)];
  const int n = supers[sp].n, n32 = n * RB;
  aug += (size_t)zl * aug_ps;
  const int nchunk = (M + HG_KC - 1) / HG_KC;
  const int c_begin = ks * cps, c_end = min(nchunk, c_begin + cps);
  int rowo[4];                           // element offset of the row in the plane (rows * ld < 2^31 for every supported plane), -1: none
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (t >> 3) + 96 * i;
    rowo[i] = r < n32 ? (blk[i] * RB + (r & 31)) * ld : -1;
  }
  const int cq = 4 * (t & 7);
  float4 rr[4];
  auto fetch1 = [&](const int c, const int i) {
    const int col = c * HG_KC + cq;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (rowo[i] >= 0) v = *reinterpret_cast<const float4*>(aug + (size_t)rowo[i] + col);
    MASK_TAIL4(v, col, M);
    rr[i] = v;
  };
  auto stash = [&](const int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (t >> 3) + 96 * i;
      uint2 hi, lo;
      split4_f16(rr[i], hi, lo);
      *reinterpret_cast<uint2*>(&Sh[buf][r][cq]) = hi;
      *reinterpret_cast<uint2*>(&Sl[buf][r][cq]) = lo;
    }
  };
  // this wave's blocks: tasks [first, first + cnt) of the row-major enumeration of (rb <= cb); blocks beyond the super-pair's n are skipped
  const int first = wv * H3_TASKS / H3_NW, cnt = (wv + 1) * H3_TASKS / H3_NW - first;
  int rb[H3_TPW], cb[H3_TPW];
  {
    int br = 0, rem = first;
    while (rem >= HSB - br) { rem -= HSB - br; ++br; }
    int bc = br + rem;
#pragma unroll
    for (int k = 0; k < H3_TPW; ++k) {
      rb[k] = br; cb[k] = bc;
      if (++bc == HSB) { ++br; bc = br; }
    }
  }
  v16f acc[H3_TPW];
#pragma unroll
  for (int k = 0; k < H3_TPW; ++k) acc[k] = v16f{0};
  if (c_begin < c_end) {
#pragma unroll
    for (int i = 0; i < 4; ++i) fetch1(c_begin, i);
  }
  int buf = 0;
  for (int c = c_begin; c < c_end; ++c, buf ^= 1) {
    stash(buf);
    const bool more = c + 1 < c_end;
    if (more) {
#pragma unroll
      for (int i = 0; i < 4; ++i) fetch1(c + 1, i);
    }
    __syncthreads();                     // double-buffered image: one barrier per chunk
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      h8_t ah, al;
      int cur = -1;
#pragma unroll
      for (int k = 0; k < H3_TPW; ++k) {
        if (k >= cnt || cb[k] >= n) continue;
        if (rb[k] != cur) {
          cur = rb[k];
          ah = *reinterpret_cast<const h8_t*>(&Sh[buf][32 * cur + j][16 * s2 + 8 * h]);
          al = *reinterpret_cast<const h8_t*>(&Sl[buf][32 * cur + j][16 * s2 + 8 * h]);
        }
        const h8_t bh = *reinterpret_cast<const h8_t*>(&Sh[buf][32 * cb[k] + j][16 * s2 + 8 * h]);
        const h8_t bl = *reinterpret_cast<const h8_t*>(&Sl[buf][32 * cb[k] + j][16 * s2 + 8 * h]);
        mfma3_f16(ah, al, bh, bl, acc[k]);
      }
    }
  }
  float* base = partials + (((size_t)zl * nsp + sp) * HG_TILES * KS + ks) * (HG_T * HG_T);
#pragma unroll
  for (int k = 0; k < H3_TPW; ++k) {
    if (k >= cnt || cb[k] >= n) continue;
    float* out = base + (size_t)hg_tile_of(rb[k] / 4, cb[k] / 4) * KS * (HG_T * HG_T) + ((rb[k] % 4) * 32) * HG_T + (cb[k] % 4) * 32;
#pragma unroll
    for (int v = 0; v < 16; ++v) out[ACC_ROW(v, h, 0) * HG_T + j] = acc[k][v];
  }
}

// ---------------------------------------------------------------------------
// The finalisation's two large products on the f16 matrix pipe, operands split like the Gram kernels' (split4_f16):
//   C[M][N] (+)= alpha A[M][K] op(B),   op(B) = B[N][K]^T (TB) or B[K][N],   batched over grid.z.
//   T = A0 B^T   (single:172's U and sigma measured on the input, fetch_norms_t): A0 holds the uint8 samples - exact in f16,
//                no lo part (A_EXACT: two products per tile step instead of three);
//   Yw += (T diag(ca)) (diag(cb) B)   (the embed's U diag(alpha Sw) V^T, ref_embed_core): the caller has scaled B's rows to
//                unit norm, ca[k] = alpha sw / (sigma |b|) is applied to A's columns while they are staged (SCALE_A), so both
//                operands are far inside f16's range whatever the plane's scale;
//   the extract's  Uw diag(sw_hat) Vwt  and its inverse DCT  D_H^T X D_W  (ref_reconstruct_core): factors whose corner rows /
//                columns have norms <= 1 + 2^-10, every operand brought into [~1, 3e4) by powers of two (per plane for sw_hat,
//                bscale for a small Vwt, alpha for D_H^T X), undone by the last product's per-plane alphaZ.
// 128 x 128 tile of C per 256-thread workgroup (a 64 x 64 quarter per wave), K in chunks of 32 through one LDS image per operand
// ([row][k], pitch 40 halfs: 16-byte operand reads conflict-free); a [K][N] operand is transposed on the way in as 4 x 4
// register pieces (lane (kg, ng): 8-byte writes that cover the 64 banks once per pass, like k_happly_h's staging).
// Against k_sgemm (f32 MFMA, 64 x 64 tiles, scalar loads: 54 - 74 TF on these shapes) the matrix-pipe time is 5.3 x / 8 x shorter.
// Preconditions (hgemm_ok): row strides multiples of 4 floats, 16-byte aligned bases.  B is multiplied by bscale while it is
// staged; alphaZ (optional, [grid.z]) multiplies alpha per plane.  Both are meant to be powers of two (exact).
// ---------------------------------------------------------------------------
template <bool TB, bool A_EXACT, bool SCALE_A>
__global__ __launch_bounds__(256) void k_hgemm(const int M, const int N, const int K, const float* __restrict__ A, const int lda, const size_t sA,
                                              const float* __restrict__ B, const int ldb, const size_t sB, const int accumulate,
                                              float* __restrict__ C, const int ldc, const size_t sC,
                                              const float* __restrict__ scaleA, const size_t sS, const float alpha,
                                              const float bscale, const float* __restrict__ alphaZ) {
  constexpr int TM = 128, KC = 32;
  __shared__ __attribute__((aligned(16))) _Float16 Ah[TM][HG_HP];
  __shared__ __attribute__((aligned(16))) _Float16 Al[A_EXACT ? 1 : TM][HG_HP];
  __shared__ __attribute__((aligned(16))) _Float16 Bh[TM][HG_HP];
  __shared__ __attribute__((aligned(16))) _Float16 Bl[TM][HG_HP];
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63, j = lane & 31, h = lane >> 5;
  A += (size_t)blockIdx.z * sA; B += (size_t)blockIdx.z * sB; C += (size_t)blockIdx.z * sC;
  if (SCALE_A) scaleA += (size_t)blockIdx.z * sS;
  const int bm = blockIdx.y * TM, bn = blockIdx.x * TM;
  // staging maps.  Row-major [row][k] operands: float4 f = t + 256 i -> row f / 8, k 4 (f % 8).  [K][N] operand: lane (kg, ng) =
  // (lane % 8, 8 wave + lane / 8) -> rows k 4 kg .. + 3, columns 4 ng .. + 3.
  float4 ra[4], rb[4];
  auto load4 = [&](const float* base, const int ld, const int row, const int nrows, const int col, const int ncols) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (row < nrows && col < ncols) {
      const float* q = base + (size_t)row * ld + col;
      if (col + 3 < ncols) v = *reinterpret_cast<const float4*>(q);
      else { v.x = q[0]; if (col + 1 < ncols) v.y = q[1]; if (col + 2 < ncols) v.z = q[2]; }
    }
    return v;
  };
  auto fetch = [&](const int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = t + 256 * i, r = f >> 3, k4 = (f & 7) * 4;
      float4 v = load4(A, lda, bm + r, M, k0 + k4, K);
      if (SCALE_A) {
        const float4 sc = load4(scaleA, 0, 0, 1, k0 + k4, K);
        v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w;
      }
      ra[i] = v;
      if (TB) rb[i] = load4(B, ldb, bn + r, N, k0 + k4, K);
    }
    if (!TB) {
      const int kg = lane & 7, ng = wv * 8 + (lane >> 3);
#pragma unroll
      for (int r = 0; r < 4; ++r) rb[r] = load4(B, ldb, k0 + 4 * kg + r, K, bn + 4 * ng, N);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { rb[i].x *= bscale; rb[i].y *= bscale; rb[i].z *= bscale; rb[i].w *= bscale; }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = t + 256 * i, r = f >> 3, k4 = (f & 7) * 4;
      uint2 hi, lo;
      split4_f16(ra[i], hi, lo);
      *reinterpret_cast<uint2*>(&Ah[r][k4]) = hi;
      if (!A_EXACT) *reinterpret_cast<uint2*>(&Al[r][k4]) = lo;
      if (TB) {
        split4_f16(rb[i], hi, lo);
        *reinterpret_cast<uint2*>(&Bh[r][k4]) = hi;
        *reinterpret_cast<uint2*>(&Bl[r][k4]) = lo;
      }
    }
    if (!TB) {
      const int kg = lane & 7, ng = wv * 8 + (lane >> 3);
      const float cx[4][4] = {{rb[0].x, rb[1].x, rb[2].x, rb[3].x}, {rb[0].y, rb[1].y, rb[2].y, rb[3].y},
                              {rb[0].z, rb[1].z, rb[2].z, rb[3].z}, {rb[0].w, rb[1].w, rb[2].w, rb[3].w}};   // [column][k]
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        uint2 hi, lo;
        split4_f16(make_float4(cx[e][0], cx[e][1], cx[e][2], cx[e][3]), hi, lo);
        *reinterpret_cast<uint2*>(&Bh[4 * ng + e][4 * kg]) = hi;
        *reinterpret_cast<uint2*>(&Bl[4 * ng + e][4 * kg]) = lo;
      }
    }
  };
  const int wi = wv >> 1, wj = wv & 1;
  v16f acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = v16f{0};
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += KC) {
    if (k0 > 0) __syncthreads();         // the previous chunk's operand reads are done
    stash();
    if (k0 + KC < K) fetch(k0 + KC);
    __syncthreads();
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      h8_t ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        ah[x] = *reinterpret_cast<const h8_t*>(&Ah[64 * wi + 32 * x + j][16 * s2 + 8 * h]);
        if (!A_EXACT) al[x] = *reinterpret_cast<const h8_t*>(&Al[64 * wi + 32 * x + j][16 * s2 + 8 * h]);
        bh[x] = *reinterpret_cast<const h8_t*>(&Bh[64 * wj + 32 * x + j][16 * s2 + 8 * h]);
        bl[x] = *reinterpret_cast<const h8_t*>(&Bl[64 * wj + 32 * x + j][16 * s2 + 8 * h]);
      }
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
          if (!A_EXACT) mfma3_f16(ah[x], al[x], bh[y], bl[y], acc[x][y]);
          else {                           // A has no lo part
            acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[x], bh[y], acc[x][y], 0, 0, 0);
            acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[x], bl[y], acc[x][y], 0, 0, 0);
          }
        }
    }
  }
  const float az = alphaZ ? alpha * alphaZ[blockIdx.z] : alpha;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const int gn = bn + 64 * wj + 32 * y + j;
      if (gn >= N) continue;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int gm = ACC_ROW(v, h, bm + 64 * wi + 32 * x);
        if (gm < M) {
          float* c = C + (size_t)gm * ldc + gn;
          *c = accumulate ? *c + az * acc[x][y][v] : az * acc[x][y][v];
        }
      }
    }
}

inline bool hgemm_ok(const void* A, int lda, const void* B, int ldb) {
  return lda % 4 == 0 && ldb % 4 == 0 && ((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0;
}

// G_s = sum of the splits, the super-pair's "rotated" flag cleared.  One 32 x 32 block (br <= bc) per workgroup: read coalesced
// from the upper-triangle tiles, written to (br, bc) and - transposed through LDS - to (bc, br), so G_s is exactly symmetric
// and every access is a 128-byte row segment.
__global__ __launch_bounds__(256) void k_hreduce(const float* __restrict__ partials, const HSuper* __restrict__ supers, const int nsp,
                                                const int KS, float* __restrict__ Gs, int* __restrict__ anyrot) {
  __shared__ float Ts[32][33];
  const int sp = blockIdx.y, z = blockIdx.z, t = threadIdx.x;
  const int nb = supers[sp].n;
  if (blockIdx.x == 0 && t == 0) anyrot[(size_t)z * nsp + sp] = 0;
  int br = 0, rem = blockIdx.x;                 // (br, bc), br <= bc, enumerated row by row over HSB x HSB
  while (rem >= HSB - br) { rem -= HSB - br; ++br; }
  const int bc = br + rem;
  if (bc >= nb) return;
  const int tile = hg_tile_of(br / 4, bc / 4);
  const float* p = partials + (((size_t)z * nsp + sp) * HG_TILES + tile) * KS * (HG_T * HG_T) + ((br % 4) * 32) * HG_T + (bc % 4) * 32;
  const size_t o = ((size_t)z * nsp + sp) * HN * HN;
  const int c = t & 31, r0 = t >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + 8 * i;
    float s = 0.0f;
    for (int k = 0; k < KS; ++k) s += p[(size_t)k * (HG_T * HG_T) + r * HG_T + c];
    Gs[o + (size_t)(br * 32 + r) * HN + bc * 32 + c] = s;
    Ts[r][c] = s;
  }
  if (br == bc) return;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + 8 * i;
    Gs[o + (size_t)(bc * 32 + r) * HN + br * 32 + c] = Ts[c][r];
  }
}

// ---------------------------------------------------------------------------
// After a stage's inner solves: the off-diagonal blocks of the tracked Gram matrix, one unit pair (p < q) per workgroup:
//   G[p][q] <- R_p^T G[p][q] R_q   (and its mirror image G[q][p])
// A unit is two 32-row blocks (la, lb) of the super-pair - a rotated pair, or an idle pair (R = I); a pair whose solve was
// skipped (already diagonal) has R = I as well.  64 x 64 x 64 products on v_mfma_f32_32x32x2_f32, one 32 x 32 quadrant per
// wave with two accumulation chains; the block goes through LDS (pitch 65), the rotations come packed from k_rf_inner.
// (Round 4 first accumulated Q_s <- Q_s P here as well - 18 more tasks per super-pair and stage that read and rewrote the
// whole of Q_s: the largest item of the scheme's HBM traffic and, at 48 planes per step, of its time; k_happly now applies
// the stages' rotations itself.)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256, 4) void k_hupdate(const int* __restrict__ units, const HSuper* __restrict__ supers, const int nsp,
                                                const float* __restrict__ Rall, const int* __restrict__ skip,
                                                float* __restrict__ Gs) {
  __shared__ float Bm[RP][RP + 1];       // the block, then T = R_p^T B: 16.6 KB, so that a stage's <= 945 workgroups are resident at once
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63, j = lane & 31, h = lane >> 5;
  const int sp = blockIdx.y, z = blockIdx.z;
  const int* un = units + sp * HU;
  const size_t zs = (size_t)z * nsp + sp;
  int up = 0, rem = blockIdx.x;          // (p, q), p < q, enumerated row by row
  while (rem >= HU - 1 - up) { rem -= HU - 1 - up; ++up; }
  const int uq = up + 1 + rem;
  // the five words that decide what this workgroup does, fetched together (one round trip to L2 instead of three in a row
  // in front of the block's own loads: a workgroup lives ~10 us)
  const int nu = supers[sp].n / 2, ep = un[up], eq = un[uq], skp = skip[zs * HU + up], skq = skip[zs * HU + uq];
  if (uq >= nu) return;
  if (ep < 0 || eq < 0) return;          // this super-pair has no such stage
  const bool rot_p = UNIT_ROTATES(ep) && !skp;
  const bool rot_q = UNIT_ROTATES(eq) && !skq;
  if (!rot_p && !rot_q) return;
  const int pa = unit_la(ep), pb = unit_lb(ep), qa = unit_la(eq), qb = unit_lb(eq);
  float* mat = Gs + zs * HN * HN;
  const int wi = wv >> 1, wj = wv & 1, i0 = wi * 32, c0 = wj * 32;
  // element (r, c) of the 64 x 64 block lives at row rmap(r), column cmap(c) of the matrix
  auto rmap = [&](const int r) { return pair_row(r, pa, pb); };
  auto cmap = [&](const int c) { return pair_row(c, qa, qb); };
  // The rotations are MFMA operands straight from k_rf_inner's packed copy (R[2 kk + h][32 hf + j] at ((hf * 8 + kk / 4) * 64 + lane) * 4
  // + kk % 4): the A operand of the left product is R_p's half wi, the B operand of the right product R_q's half wj - eight 16-byte
  // loads each, no LDS.
  float ap[RP / 2], bq[RP / 2];
  if (rot_p) {
    const float4* rp = reinterpret_cast<const float4*>(Rall + (zs * HU + up) * RP * RP) + (wi * 8) * 64 + lane;
#pragma unroll
    for (int kq = 0; kq < 8; ++kq) { const float4 v = rp[kq * 64]; ap[4 * kq] = v.x; ap[4 * kq + 1] = v.y; ap[4 * kq + 2] = v.z; ap[4 * kq + 3] = v.w; }
  }
  if (rot_q) {
    const float4* rq = reinterpret_cast<const float4*>(Rall + (zs * HU + uq) * RP * RP) + (wj * 8) * 64 + lane;
#pragma unroll
    for (int kq = 0; kq < 8; ++kq) { const float4 v = rq[kq * 64]; bq[4 * kq] = v.x; bq[4 * kq + 1] = v.y; bq[4 * kq + 2] = v.z; bq[4 * kq + 3] = v.w; }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {          // 16 bytes per lane
    const int f = t + 256 * i, r = f >> 4, c4 = (f & 15) * 4;
    const float4 v = *reinterpret_cast<const float4*>(mat + (size_t)rmap(r) * HN + cmap(c4));
    Bm[r][c4] = v.x; Bm[r][c4 + 1] = v.y; Bm[r][c4 + 2] = v.z; Bm[r][c4 + 3] = v.w;
  }
  __syncthreads();
  // two accumulation chains per product (even / odd steps): a dependent MFMA issues 64 cycles after its predecessor
  v16f acc = {0}, acc2 = {0};
  if (rot_p) {                           // T[i][c] = sum_k R_p[k][i] B[k][c]
#pragma unroll
    for (int kk = 0; kk < RP / 2; kk += 2) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], Bm[2 * kk + h][c0 + j], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk + 1], Bm[2 * kk + 2 + h][c0 + j], acc2, 0, 0, 0);
    }
    acc += acc2;
    if (rot_q) {
      __syncthreads();                   // every wave has read B
#pragma unroll
      for (int v = 0; v < 16; ++v) Bm[ACC_ROW(v, h, i0)][c0 + j] = acc[v];
      __syncthreads();
    }
  }
  if (rot_q) {                           // out[r][i] = sum_c T[r][c] R_q[c][i]
    acc = v16f{0}; acc2 = v16f{0};
#pragma unroll
    for (int kk = 0; kk < RP / 2; kk += 2) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Bm[i0 + j][2 * kk + h], bq[kk], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(Bm[i0 + j][2 * kk + 2 + h], bq[kk + 1], acc2, 0, 0, 0);
    }
    acc += acc2;
  }
  // the block, and its mirror image G[q][p] = (G[p][q])^T (which keeps G_s exactly symmetric): back through the LDS tile, so that both
  // go out as 16-byte pieces of 256-byte row segments (straight from the accumulators the mirror image was 32 scattered 4-byte stores
  // per lane: 6 400 of the workgroup's 18 600 cycles)
  __syncthreads();                       // every wave has read the tile
#pragma unroll
  for (int v = 0; v < 16; ++v) Bm[ACC_ROW(v, h, i0)][c0 + j] = acc[v];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int f = t + 256 * i, a = f >> 4, b4 = (f & 15) * 4;
    *reinterpret_cast<float4*>(mat + (size_t)rmap(a) * HN + cmap(b4)) = make_float4(Bm[a][b4], Bm[a][b4 + 1], Bm[a][b4 + 2], Bm[a][b4 + 3]);
    *reinterpret_cast<float4*>(mat + (size_t)cmap(a) * HN + rmap(b4)) = make_float4(Bm[b4][a], Bm[b4 + 1][a], Bm[b4 + 2][a], Bm[b4 + 3][a]);
  }
}

// ---------------------------------------------------------------------------
// X_s <- P_T^T .. P_1^T X_s, in place: one 64-column strip of all the rows of one (plane, super-pair) per workgroup, staged
// in LDS ([row][col], pitch 65); the super-step's stages are applied to it one after the other.  In a stage the two waves
// 2 u, 2 u + 1 own unit u (two 32-row blocks la, lb): wave half hf computes the 32 output rows of block (hf ? lb : la) as
// two 32 x 32 tiles (two independent accumulation chains), K = the unit's 64 rows read from LDS as the B operand, A = R_u
// in the packed order k_rf_inner left it (eight 16-byte loads per wave and stage, issued a stage ahead); a workgroup barrier
// separates a stage's reads of the strip from the write-back of its results.  Idle and skipped units cost nothing.
// Tasks are ordered (plane, super-pair)-major and dealt to the XCDs in contiguous ranges (workgroup b runs on XCD b % 8 -
// observed placement, speed only), so a super-pair's rotations serve all of its strips from one or two L2s.  Nothing of a
// strip is stored before the whole strip is in LDS, so the update is safe in place.
// Measured alternatives (profiles/r04_hier_kernels.md): an accumulated Q_s applied as one (<= 384)^2 product per strip
// (-15 % matrix-core work here, but its maintenance in k_hupdate was the scheme's largest cost at 48 planes per step); a
// persistent workgroup per CU walking 32-column strips with a double-buffered LDS image (slower: 118 - 143 against 98 us).
// Threads: 64 x (most blocks of a super-pair); dynamic LDS: n32_max x 65 floats.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64 * HSB) void k_happly(float* __restrict__ aug, const size_t aug_ps, const int ld, const int ncols,
                                                    const HSuper* __restrict__ supers, const int nsp, const int nz,
                                                    const int* __restrict__ units, const int T, const float* __restrict__ Rpk,
                                                    const int* __restrict__ skipT, const size_t rpk_stage, const size_t skip_stage,
                                                    const int* __restrict__ anyrot) {
  extern __shared__ float Xs[];          // [n32][65]
  const int t = threadIdx.x, nthr = blockDim.x, wv = t >> 6, lane = t & 63, j = lane & 31, h = lane >> 5;
  const int nstrips = (ncols + 63) / 64;
  const int ntask = nsp * nz * nstrips;
  int tk_end;
  const int tk = xcd_task(blockIdx.x, ntask, tk_end);
  if (tk >= tk_end) return;
  const int g = tk / nstrips, sp = g % nsp, z = g / nsp, c0 = (tk % nstrips) * 64;      // g = z * nsp + sp
  const int n = supers[sp].n;
  if (n == 0 || !anyrot[g]) return;      // no such super-pair / every pair of every stage was already diagonal
  const int n32 = n * RB;
  aug += (size_t)z * aug_ps;
  for (int f = t; f < n32 * 16; f += nthr) {
    const int r = f >> 4, c4 = (f & 15) * 4;
    const float4 v = *reinterpret_cast<const float4*>(aug + (size_t)(supers[sp].blk[r >> 5] * RB + (r & 31)) * ld + c0 + c4);   // within the row: ld >= ncols rounded up to 64
    float* d = Xs + r * 65 + c4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  const int u = wv >> 1, hf = wv & 1;    // this wave's unit and which of its two blocks it produces
  const bool wave_on = 2 * u < n;        // (waves beyond the super-pair's units only keep the barriers company)
  // a stage's operands: the unit's entry, whether it rotates, and - if so - R_u's 32 steps for this wave's 32 output rows
  float a_cur[32], a_nxt[32];
  int e_cur = -1, e_nxt = -1;
  auto fetch_stage = [&](const int st, int& e, float* a) {
    e = -1;
    if (!wave_on || st >= T) return;
    const int ent = units[((size_t)st * nsp + sp) * HU + u];
    if (!UNIT_ROTATES(ent) || skipT[(size_t)st * skip_stage + (size_t)g * HU + u]) return;
    e = ent;
    const float4* rp = reinterpret_cast<const float4*>(Rpk + (size_t)st * rpk_stage + ((size_t)g * HU + u) * RP * RP) + (hf * 8) * 64 + lane;
#pragma unroll
    for (int kq = 0; kq < 8; ++kq) {
      const float4 v = rp[kq * 64];
      a[4 * kq] = v.x; a[4 * kq + 1] = v.y; a[4 * kq + 2] = v.z; a[4 * kq + 3] = v.w;
    }
  };
  fetch_stage(0, e_cur, a_cur);
  __syncthreads();
  for (int st = 0; st < T; ++st) {
    fetch_stage(st + 1, e_nxt, a_nxt);
    v16f acc0 = {0}, acc1 = {0};
    const int la = unit_la(e_cur), lb = unit_lb(e_cur);
    if (e_cur >= 0) {
      const float* xa = Xs + (la * RB + h) * 65 + j;        // k < 32: row la * 32 + k;  k >= 32: row lb * 32 + k - 32
      const float* xb = Xs + (lb * RB + h) * 65 + j;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[kk], xa[2 * kk * 65], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[kk], xa[2 * kk * 65 + 32], acc1, 0, 0, 0);
      }
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[16 + kk], xb[2 * kk * 65], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[16 + kk], xb[2 * kk * 65 + 32], acc1, 0, 0, 0);
      }
    }
    __syncthreads();                     // every wave has read this stage's rows
    if (e_cur >= 0) {
      float* o = Xs + ((hf ? lb : la) * RB) * 65 + j;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int i = ACC_ROW(v, h, 0);
        o[i * 65] = acc0[v]; o[i * 65 + 32] = acc1[v];
      }
    }
    __syncthreads();
    e_cur = e_nxt;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) a_cur[kk] = a_nxt[kk];
  }
  for (int f = t; f < n32 * 16; f += nthr) {
    const int r = f >> 4, c4 = (f & 15) * 4;
    const float* d = Xs + r * 65 + c4;
    float* o = aug + (size_t)(supers[sp].blk[r >> 5] * RB + (r & 31)) * ld + c0 + c4;
    if (c0 + c4 + 3 < ncols) *reinterpret_cast<float4*>(o) = make_float4(d[0], d[1], d[2], d[3]);
    else
      for (int e = 0; e < 4; ++e) if (c0 + c4 + e < ncols) o[e] = d[e];
  }
}

// ---------------------------------------------------------------------------
// k_happly on the f16 matrix pipe with split operands (see k_hgram_t).  The strip's LDS image IS the split form: two f16
// planes [column][row] (k-contiguous for the B operand: a lane's 8 consecutive rows are one 16-byte read; pitch HA_CP halfs),
// x = hi + lo' / 2048 (split4_scaled) - 22 significant bits, so
// what a stage writes back is the f32 result rounded to 2^-23 relative (an f32 product chain of 64 terms rounds more).
// Per stage a wave issues 24 v_mfma_f32_32x32x16_f16 (R_hi X_hi into one accumulator pair, R_hi X_lo' + R_lo' X_hi into a
// second that is scaled by 2^-11 at the end) instead of 64 v_mfma_f32_32x32x2_f32: 768 matrix-pipe cycles instead of 4 096.
// R arrives split and packed from k_rf_inner (h_f16).  Row entries are bounded by 255 sqrt(L) < 65 504 for every plane
// (orthogonal rotations of uint8 rows); float inputs without that bound keep the f32 kernel (jacobi_rows).
// ---------------------------------------------------------------------------
constexpr int HA_CP = HN + 8;                 // halfs per column of the split image: 784 bytes = 196 dwords = 4 mod 64: 16-byte reads of 16 lanes are conflict-free

template <int SW>                      // strip width in columns: 64 (100 KB of LDS, one workgroup per CU)
__global__ __launch_bounds__(64 * HSB) void k_happly_h(float* __restrict__ aug, const size_t aug_ps, const int ld, const int ncols,
                                                      const HSuper* __restrict__ supers, const int nsp, const int nz,
                                                      const int* __restrict__ units, const int T, const float* __restrict__ Rpk,
                                                      const int* __restrict__ skipT, const size_t rpk_stage, const size_t skip_stage,
                                                      const int* __restrict__ anyrot) {
  constexpr int NT = SW / 32;                          // 32-column tiles per wave
  extern __shared__ __attribute__((aligned(16))) _Float16 Xh[];          // [SW columns][HA_CP], then the lo' plane
  _Float16* const Xl = Xh + SW * HA_CP;
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63, j = lane & 31, h = lane >> 5;
  const int nstrips = (ncols + SW - 1) / SW;
  const int ntask = nsp * nz * nstrips;
  int tk_end;
  const int tk = xcd_task(blockIdx.x, ntask, tk_end);
  if (tk >= tk_end) return;
  const int g = tk / nstrips, sp = g % nsp, z = g / nsp, c0 = (tk % nstrips) * SW;      // g = z * nsp + sp
  // (the words this workgroup's first loads depend on, fetched together: the super-pair's size, whether any of its pairs
  // rotated, and this wave's block)
  const int n = supers[sp].n, any = anyrot[g], myblk = supers[sp].blk[min(wv, HSB - 1)];
  if (n == 0 || !any) return;
  aug += (size_t)z * aug_ps;
  // Staging: wave wv takes the super-pair's block wv (32 rows) as NT pieces of 32 x 32, lane (i, m) = (lane % 8, lane / 8) the
  // 4 x 4 piece at rows 4 i, columns 4 m: four 16-byte loads (a row's eight lanes fetch one 128-byte line), transposed in
  // registers for free, split, and written as 8-byte column pieces of four rows - bank (16 m + 2 i) mod 64 (+ 0 / 1): the 32
  // lanes of a pass cover the 64 banks exactly once.
  // every stage's unit entries of this (plane, super-pair), with the skip flags folded in: read once, here - fetched stage by
  // stage they were two dependent L2 round trips in front of every stage's barrier (3 000 of a stage's 7 500 cycles)
  __shared__ int s_ent[HT_MAX][HU];
  if (t < T * HU) {
    const int st = t / HU, uu = t % HU;
    const int ent = units[((size_t)st * nsp + sp) * HU + uu], sk = skipT[(size_t)st * skip_stage + (size_t)g * HU + uu];
    s_ent[st][uu] = (!UNIT_ROTATES(ent) || sk) ? UNIT_NONE : ent;
  }
  const int ti = lane & 7, tm = lane >> 3;
  if (wv < n) {
    const float* src = aug + (size_t)(myblk * RB + 4 * ti) * ld + c0 + 4 * tm;     // within the row: ld >= ncols rounded up to 64
    float4 v[NT][4];
#pragma unroll
    for (int tl = 0; tl < NT; ++tl)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[tl][k] = *reinterpret_cast<const float4*>(src + (size_t)k * ld + 32 * tl);
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
      const float xv[4][4] = {{v[tl][0].x, v[tl][1].x, v[tl][2].x, v[tl][3].x}, {v[tl][0].y, v[tl][1].y, v[tl][2].y, v[tl][3].y},
                              {v[tl][0].z, v[tl][1].z, v[tl][2].z, v[tl][3].z}, {v[tl][0].w, v[tl][1].w, v[tl][2].w, v[tl][3].w}};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h4_t hi, lo;
        split4_scaled(xv[e][0], xv[e][1], xv[e][2], xv[e][3], hi, lo);
        const int at = (32 * tl + 4 * tm + e) * HA_CP + wv * RB + 4 * ti;
        *reinterpret_cast<h4_t*>(Xh + at) = hi; *reinterpret_cast<h4_t*>(Xl + at) = lo;
      }
    }
  }
  const int u = wv >> 1, hf = wv & 1;    // this wave's unit and which of its two blocks it produces
  const bool wave_on = 2 * u < n;
  // a stage's operands for this wave: R_u's rows for its 32 output rows, 4 steps of 16 values of k, hi and lo'
  h8_t ah0[4], al0[4], ah1[4], al1[4];     // two named operand sets used alternately (copies between them make hipcc wait for the newest loads)
  int e0 = -1, e1 = -1;
  auto fetch_stage = [&](const int st, int& e, h8_t* ah, h8_t* al) {
    e = -1;
    if (!wave_on || st >= T) return;
    int ent;                             // (-1: no such unit, idle pair, or already diagonal at that stage)
    if (st == 0) {                       // (before the first barrier: straight from the tables, under the staging loads)
      ent = units[(size_t)sp * HU + u];
      const int sk = skipT[(size_t)g * HU + u];
      if (!UNIT_ROTATES(ent) || sk) ent = UNIT_NONE;
    } else ent = s_ent[st][u];
    if (ent < 0) return;
    e = ent;
    const h8_t* rp = reinterpret_cast<const h8_t*>(Rpk + (size_t)st * rpk_stage + ((size_t)g * HU + u) * RP * RP) + (hf * 4) * 64 + lane;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) { ah[s2] = rp[s2 * 64]; al[s2] = rp[RP * RP / 8 + s2 * 64]; }
  };
  // One 32-column tile's products of a stage (accumulators pa: hi hi, pb: the two cross products, x 2^11), and its write-back.
  auto mfma_tile = [&](const int tl, const int e, const h8_t* ah, const h8_t* al, v16f& pa, v16f& pb) {
    pa = v16f{0}; pb = v16f{0};
    if (e < 0) return;
    const int la = unit_la(e), lb = unit_lb(e);
    const _Float16* xhc = Xh + (32 * tl + j) * HA_CP; const _Float16* xlc = Xl + (32 * tl + j) * HA_CP;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      // unit-local rows 16 s2 + 8 h .. + 7: the first 32 are block la, the rest block lb
      const int row = (s2 < 2 ? la * RB : lb * RB - 32) + 16 * s2 + 8 * h;
      const h8_t xh = *reinterpret_cast<const h8_t*>(xhc + row);
      const h8_t xl = *reinterpret_cast<const h8_t*>(xlc + row);
      pa = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s2], xh, pa, 0, 0, 0);
      pb = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s2], xl, pb, 0, 0, 0);
      pb = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[s2], xh, pb, 0, 0, 0);
    }
  };
  auto wb_tile = [&](const int tl, const int e, const v16f& pa, const v16f& pb) {
    if (e < 0) return;
    // ACC_ROW: the registers 4 qd .. + 3 of a lane are four consecutive rows from row 8 qd + 4 h on = four consecutive halfs of
    // the column-major image
    const int rb0 = (hf ? unit_lb(e) : unit_la(e)) * RB + ACC_ROW(0, h, 0);
    _Float16* ch = Xh + (32 * tl + j) * HA_CP + rb0; _Float16* cl = Xl + (32 * tl + j) * HA_CP + rb0;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      h4_t hh, ll;
      constexpr float SC = 1.0f / 2048.0f;
      split4_scaled(fmaf(pb[4 * qd], SC, pa[4 * qd]), fmaf(pb[4 * qd + 1], SC, pa[4 * qd + 1]),
                    fmaf(pb[4 * qd + 2], SC, pa[4 * qd + 2]), fmaf(pb[4 * qd + 3], SC, pa[4 * qd + 3]), hh, ll);
      *reinterpret_cast<h4_t*>(ch + 8 * qd) = hh;
      *reinterpret_cast<h4_t*>(cl + 8 * qd) = ll;
    }
  };
  // The two tiles of the strip run half a stage apart: while a wave's matrix instructions of one tile execute, its (and the
  // SIMD's other waves') VALU work splits and stores the other tile's results - the two pipes overlap instead of alternating
  // between the stage's two barriers.  Tile 0 of stage st + 1 is read after the barrier that follows tile 0's write-back of
  // stage st, tile 1 likewise; the tiles are disjoint columns of the image.
  static_assert(NT == 2, "the stage pipeline alternates between two 32-column tiles");
  fetch_stage(0, e0, ah0, al0);
  __syncthreads();
  v16f pa0, pb0, pa1, pb1;
  mfma_tile(0, e0, ah0, al0, pa0, pb0);
  // one stage: A = its operands (resident), B = the next stage's (fetched here, first used after the second barrier)
  const bool vfirst = ((wv >> 2) & 1) != 0;
  auto stage = [&](const int st, const int eA, const h8_t* ahA, const h8_t* alA, int& eB, h8_t* ahB, h8_t* alB) {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): nothing is in flight here (set A was waited for a phase ago) - said explicitly, or hipcc makes this stage's
                                         // matrix instructions wait for the loads issued on the next line (its counters merge the two sets across the loop)
    fetch_stage(st + 1, eB, ahB, alB);
    __syncthreads();                     // every wave has read tile 0 of this stage (and stored tile 1 of the previous one)
    // (a phase's two parts touch different tiles, so either order is valid: the SIMD's waves 0, 8 start with the products,
    // wave 4 with the write-back - matrix pipe and VALU have work from the first cycle of the phase)
    if (vfirst) { wb_tile(0, eA, pa0, pb0); mfma_tile(1, eA, ahA, alA, pa1, pb1); }
    else { mfma_tile(1, eA, ahA, alA, pa1, pb1); wb_tile(0, eA, pa0, pb0); }
    __syncthreads();                     // tile 1 read, tile 0 stored
    if (vfirst) { wb_tile(1, eA, pa1, pb1); mfma_tile(0, eB, ahB, alB, pa0, pb0); }
    else { mfma_tile(0, eB, ahB, alB, pa0, pb0); wb_tile(1, eA, pa1, pb1); }
  };
  for (int st = 0; st < T; st += 2) {
    stage(st, e0, ah0, al0, e1, ah1, al1);
    if (st + 1 < T) stage(st + 1, e1, ah1, al1, e0, ah0, al0);
  }
  __syncthreads();
  if (wv < n) {                          // the image back to f32 rows: the staging's pieces in reverse
    float* dst = aug + (size_t)(myblk * RB + 4 * ti) * ld + c0 + 4 * tm;
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
      float xv[4][4];                    // [column][row]
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int at = (32 * tl + 4 * tm + e) * HA_CP + wv * RB + 4 * ti;
        const h4_t hi = *reinterpret_cast<const h4_t*>(Xh + at), lo = *reinterpret_cast<const h4_t*>(Xl + at);
#pragma unroll
        for (int k = 0; k < 4; ++k) xv[e][k] = fmaf((float)lo[k], 1.0f / 2048.0f, (float)hi[k]);
      }
      const int cb = c0 + 32 * tl + 4 * tm;
      if (c0 + SW <= ncols) {            // (uniform) the whole strip lies inside the plane: 16-byte stores
#pragma unroll
        for (int k = 0; k < 4; ++k)
          *reinterpret_cast<float4*>(dst + (size_t)k * ld + 32 * tl) = make_float4(xv[0][k], xv[1][k], xv[2][k], xv[3][k]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int e = 0; e < 4; ++e) if (cb + e < ncols) dst[(size_t)k * ld + 32 * tl + e] = xv[e][k];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host side: tables of the two-level tournament, by block count and super-block size
// ---------------------------------------------------------------------------
struct HierTab {
  int nbk, sb, nsb, nsteps1, nsp, nmax;
  std::vector<double> flops_step, flops_apply_step, flops_stage_step;   // matrix-core flops of super-step s1: Gram per column, rotation per column, stage updates
  std::vector<int> T;            // stages of super-step s1
  std::vector<int> stage_off;    // first stage of super-step s1 in d_units
  HSuper* d_super;               // [nsteps1][nsp]
  int* d_units;                  // [stages][nsp][HU]: unit_make(la, lb, real), or UNIT_NONE
};

void round_robin(int m, std::vector<std::vector<std::pair<int, int>>>& steps) {      // m even
  std::vector<int> idx(m);
  std::iota(idx.begin(), idx.end(), 0);
  steps.assign(m - 1, {});
  for (int s = 0; s < m - 1; ++s) {
    for (int k = 0; k < m / 2; ++k) steps[s].push_back({idx[k], idx[m - 1 - k]});
    const int last = idx[m - 1];
    for (int j2 = m - 1; j2 > 1; --j2) idx[j2] = idx[j2 - 1];
    if (m > 1) idx[1] = last;
  }
}

int get_hier(wm_ctx* ctx, const int nbk, const int sb, const HierTab** out) {
  const int key = nbk * 16 + sb;
  for (int i = 0; i < wm_ctx::MAX_PAIR_TABS; ++i)
    if (ctx->hier_host[i] && ctx->hier_key[i] == key) { *out = (const HierTab*)ctx->hier_host[i]; return WM_OK; }
  int slot = -1;
  for (int i = 0; i < wm_ctx::MAX_PAIR_TABS; ++i) if (!ctx->hier_host[i]) { slot = i; break; }
  if (slot < 0) {
    slot = ctx->hier_next; ctx->hier_next = (ctx->hier_next + 1) % wm_ctx::MAX_PAIR_TABS;
    WM_HIP(hipStreamSynchronize(ctx->stream));
    for (int g = 0; g < wm_ctx::MAX_AUX; ++g) if (ctx->aux_stream[g]) WM_HIP(hipStreamSynchronize(ctx->aux_stream[g]));
    WM_HIP(hipFree(ctx->hier_dev[slot]));
    wmi::hier_host_free(ctx->hier_host[slot]);
    ctx->hier_dev[slot] = nullptr; ctx->hier_host[slot] = nullptr;
  }
  HierTab* ht = new (std::nothrow) HierTab();
  if (!ht) return set_err(WM_ERR_NOMEM, "out of host memory for %s", "the tournament tables");
  ht->nbk = nbk; ht->sb = sb;
  // super-blocks: the nbk / 2 block pairs are dealt as evenly as possible over ceil(nbk / sb) super-blocks, so every
  // super-block has an even number of blocks (a sub-tournament over an even count has no bye)
  std::vector<int> size, off;
  if (nbk == 2) { size = {1, 1}; }
  else {
    const int doubles = nbk / 2, per = std::max(1, sb / 2);
    const int nsb = std::min(doubles, std::max(2, (doubles + per - 1) / per));
    for (int i = 0; i < nsb; ++i) size.push_back(2 * (doubles / nsb + (i < doubles % nsb ? 1 : 0)));
  }
  ht->nsb = (int)size.size();
  off.resize(size.size());
  for (size_t i = 0, o = 0; i < size.size(); ++i) { off[i] = (int)o; o += size[i]; }
  const int m = ht->nsb + (ht->nsb & 1);
  std::vector<std::vector<std::pair<int, int>>> l1;
  round_robin(m, l1);
  ht->nsteps1 = m - 1; ht->nsp = m / 2; ht->nmax = 0;
  std::vector<HSuper> supers((size_t)ht->nsteps1 * ht->nsp);
  std::vector<int> units;
  ht->T.assign(ht->nsteps1, 0); ht->stage_off.assign(ht->nsteps1, 0);
  for (int s1 = 0; s1 < ht->nsteps1; ++s1) {
    // per super-pair: stage lists
    std::vector<std::vector<std::array<int, HU>>> st(ht->nsp);
    int Tmax = 0;
    for (int k = 0; k < ht->nsp; ++k) {
      HSuper& su = supers[(size_t)s1 * ht->nsp + k];
      su.n = 0;
      for (int i = 0; i < HSB; ++i) su.blk[i] = 0;
      int A = std::min(l1[s1][k].first, l1[s1][k].second), B = std::max(l1[s1][k].first, l1[s1][k].second);
      const bool bye = B >= ht->nsb;                 // paired with the dummy of an odd count
      if (bye && s1 != 0) continue;                  // idle this step (its own pairs were rotated in step 0)
      const int na = size[A], nb = bye ? 0 : size[B];
      for (int i = 0; i < na; ++i) su.blk[su.n++] = off[A] + i;
      for (int i = 0; i < nb; ++i) su.blk[su.n++] = off[B] + i;
      ht->nmax = std::max(ht->nmax, su.n);
      if (s1 == 0) {                                 // every pair among the n blocks (n even)
        std::vector<std::vector<std::pair<int, int>>> l2;
        round_robin(su.n, l2);
        for (auto& stage : l2) {
          std::array<int, HU> row; row.fill(UNIT_NONE);
          for (size_t u = 0; u < stage.size(); ++u)
            row[u] = unit_make(std::min(stage[u].first, stage[u].second), std::max(stage[u].first, stage[u].second), true);
          st[k].push_back(row);
        }
      } else {                                       // the na x nb cross pairs: the smaller side meets the larger one cyclically
        const int big = std::max(na, nb), small = std::min(na, nb);
        for (int tt = 0; tt < big; ++tt) {
          std::array<int, HU> row; row.fill(UNIT_NONE);
          std::vector<char> used(su.n, 0);
          int u = 0;
          for (int i = 0; i < small; ++i) {
            const int jb = (i + tt) % big;
            const int la = na >= nb ? jb : i, lb = na >= nb ? na + i : na + jb;     // local indices: A first, then B
            row[u++] = unit_make(la, lb, true);
            used[la] = used[lb] = 1;
          }
          int pend = -1;                             // idle blocks in pairs (their count is even): R = I
          for (int b2 = 0; b2 < su.n; ++b2)
            if (!used[b2]) { if (pend < 0) pend = b2; else { row[u++] = unit_make(pend, b2, false); pend = -1; } }
          st[k].push_back(row);
        }
      }
      Tmax = std::max(Tmax, (int)st[k].size());
    }
    ht->T[s1] = Tmax; ht->stage_off[s1] = (int)(units.size() / ((size_t)ht->nsp * HU));
    {   // what the kernels issue for this super-step (k_hgram_t: 3 of a diagonal tile's 4 quadrants; k_happly: a 64 x 64 rotation per
        // rotated unit, stage and column; k_hupdate: two 64^3 products per unit pair and stage but the last)
      double fg = 0.0, fa = 0.0, fs = 0.0;
      for (int k = 0; k < ht->nsp; ++k) {
        const int nb = supers[(size_t)s1 * ht->nsp + k].n, n32 = nb * RB, np = (n32 + HG_T - 1) / HG_T;
        if (!nb) continue;
        const int quads = np == 1 ? 3 : np == 2 ? 3 + 4 + 3 : 3 * 3 + 3 * 4;
        fg += 2.0 * quads * 64 * 64;
        const int nu = nb / 2;
        int real_units = 0;                          // k_happly: one 64 x 64 rotation per rotated unit and stage, per column
        for (auto& row : st[k]) for (int u2 = 0; u2 < HU; ++u2) if (UNIT_ROTATES(row[u2])) ++real_units;
        fa += 2.0 * real_units * RP * RP;
        fs += (double)(st[k].size() > 0 ? st[k].size() - 1 : 0) * (nu * (nu - 1) / 2 * 2) * 2.0 * RP * RP * RP;
      }
      ht->flops_step.push_back(fg); ht->flops_apply_step.push_back(fa); ht->flops_stage_step.push_back(fs);
    }
    for (int tt = 0; tt < Tmax; ++tt)
      for (int k = 0; k < ht->nsp; ++k)
        for (int u = 0; u < HU; ++u) units.push_back(tt < (int)st[k].size() ? st[k][tt][u] : UNIT_NONE);
  }
  const size_t b_sup = pad256(supers.size() * sizeof(HSuper)), b_un = units.size() * sizeof(int);
  void* dev = nullptr;
  if (hipMalloc(&dev, b_sup + std::max<size_t>(b_un, 4)) != hipSuccess) {
    (void)hipGetLastError();
    delete ht;
    return set_err(WM_ERR_NOMEM, "hipMalloc failed for %s", "the tournament tables");
  }
  ht->d_super = (HSuper*)dev; ht->d_units = (int*)((char*)dev + b_sup);
  hipError_t e = hipMemcpyAsync(ht->d_super, supers.data(), supers.size() * sizeof(HSuper), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && b_un) e = hipMemcpyAsync(ht->d_units, units.data(), b_un, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // supers / units are locals
  if (e != hipSuccess) { (void)hipFree(dev); delete ht; return set_err(WM_ERR_HIP, "tournament tables: %s", hipGetErrorString(e)); }
  ctx->hier_dev[slot] = dev; ctx->hier_host[slot] = ht; ctx->hier_key[slot] = key;
  *out = ht;
  return WM_OK;
}

// column splits of the Gram tiles of one launch: the (super-pair, plane, split) groups are dealt over the 8 XCDs, whose 32 CUs hold one
// workgroup each; the estimate is rounds of resident workgroups x chunks per workgroup (+ the partial sums' traffic)
int hier_ks(const int nsp, const int nz, const int np, const int nchunk, const int ksmax, const double pen = 0.25) {
  int best = 1; double best_cost = 1e300;
  for (int ks = 1; ks <= ksmax; ++ks) {
    const int per_xcd = ((nsp * nz * ks + 7) / 8) * np;              // workgroups (one per CU: 8 waves, 66 KB of LDS) on the fullest XCD
    const double cost = (double)((per_xcd + 31) / 32) * ((nchunk + ks - 1) / ks) + pen * ks;
    if (cost < best_cost) { best_cost = cost; best = ks; }
  }
  return best;
}

// Base of plane group g's slice of a per-plane array of 4-byte flags (ints_per_plane each, z0 = the group's first plane): slices
// of different groups start on different 256-byte lines.  The groups run on different HIP queues, their workgroups on any XCD,
// and the XCDs' L2s are not coherent with each other: with two groups' flags in ONE line, an L2 that holds the line dirty for
// group B's flags can serve group A's kernels a stale copy of group A's (a dirty line survives A's kernel-boundary invalidate).
// Hygiene, not a measured fix: the run-to-run differences of HISTORY.md round 4 item 10 did not go away with it.
inline int* hier_flag_base(int* arr, const size_t ints_per_plane, const int z0, const int g) {
  const size_t off = (size_t)z0 * ints_per_plane;                 // dense position
  return arr + ((off + 63) / 64) * 64 + (size_t)g * 64;           // rounded up to a line, one spare line per earlier group
}
struct HierWs { float* Rpk; int* skipT; float* Gs; float* R; float* partials; int* skip; int* anyrot; int KS; int cps; };

int plan_hier_ws(wm_ctx* ctx, const RefPlan& p, const HierTab& ht, HierWs& hw) {
  // column splits of a Gram tile: enough workgroups to fill the chip, few enough that the partial sums stay a
  // fraction of the rows' own bytes
  const int nchunk = (p.M + HG_KC - 1) / HG_KC;
  int KS = std::min(HG_KS_MAX, std::max(1, nchunk / 4));      // the most any launch may use (hier_ks picks per launch)
  hw.KS = KS; hw.cps = (nchunk + KS - 1) / KS;
  const size_t B = (size_t)p.B, nsp = (size_t)ht.nsp;
  constexpr size_t GSLACK = (size_t)(2 + wm_ctx::MAX_AUX) * 64;      // flag arrays: one spare line per plane group (hier_flag_base)
  return staged(ctx, &ctx->hier_ws, &ctx->hier_ws_bytes, "full-frame two-level workspace", [&](Carve& cv) {
    hw.Rpk = cv.take<float>(B * HT_MAX * nsp * HU * RP * RP); hw.skipT = cv.take<int>(B * HT_MAX * nsp * HU + GSLACK);
    hw.Gs = cv.take<float>(B * nsp * HN * HN); hw.R = cv.take<float>(B * nsp * HU * RP * RP);
    hw.partials = cv.take<float>(B * nsp * HG_TILES * KS * HG_T * HG_T); hw.skip = cv.take<int>(B * nsp * HU + GSLACK);
    hw.anyrot = cv.take<int>(B * nsp + GSLACK);
  });
}
