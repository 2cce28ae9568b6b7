// Per-tile arithmetic of the DCT-SVD watermark hot path: one 8x8 tile per
// GPU lane, everything in registers (no LDS, no cross-lane traffic).
//
// Reference statements this replaces (citations into /root/reference,
// app_dct_svd_single.py = "single"), applied to one 8x8 tile instead of the
// whole plane (tile-mode):
//   a2  dct2            single:32-33   -> dct8x8()
//   a3  np.linalg.svd   single:172-173 -> jacobi_svd8()   (one-sided Jacobi)
//   a4  S_[:K] += a*Sw  single:174-175 -> embed_tile()
//   a5  U diag(S_) Vt   single:176     -> embed_tile()
//   a6  idct2           single:35-36   -> idct8x8()
//   a7  clip + astype   single:27      -> quant_u8()       (truncation)
//   a8  (S_cw-Sc)/alpha single:212-213 -> extract_tile()
//   a9  Uw diag() Vwt   single:214-218 -> extract_tile()
//
// The header is host/device: hipcc compiles it into the gfx950 kernels
// (wm_kernels.hip); tests compile the very same functions with g++ to check
// the arithmetic on the CPU (tests/host_harness.cpp).  The host build is a
// test harness, never a product path.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define WM_HD __host__ __device__ __forceinline__
#else
#define WM_HD inline
#endif

namespace wm {

// ---- fast reciprocal / sqrt (v_rcp_f32, v_rsq_f32, v_sqrt_f32: 1 ulp) -------
WM_HD float frcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcpf(x);
#else
  return 1.0f / x;
#endif
}
WM_HD float frsq(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rsqf(x);
#else
  return 1.0f / sqrtf(x);
#endif
}
WM_HD float fsqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sqrtf(x);
#else
  return sqrtf(x);
#endif
}
WM_HD float ffma(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fmaf(a, b, c);
#else
  return fmaf(a, b, c);
#endif
}
// wave-wide OR of a per-lane predicate (host: identity)
WM_HD bool wave_any(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ballot_w64(p) != 0ull;
#else
  return p;
#endif
}

// ---- 8-point orthonormal DCT-II constants: D[k][m] = ck*cos((2m+1)k*pi/16) --
// c_k = 0.5*cos(k*pi/16) for k>=1; row 0 is sqrt(1/8) = C4.
constexpr float C1 = 0.49039264020161522f;
constexpr float C2 = 0.46193976625564337f;
constexpr float C3 = 0.41573480615127262f;
constexpr float C4 = 0.35355339059327379f;
constexpr float C5 = 0.27778511650980114f;
constexpr float C6 = 0.19134171618254492f;
constexpr float C7 = 0.09754516100806417f;

// forward 1-D DCT-II of 8 samples, even/odd split (36 flop-instr)
WM_HD void dct8(float& x0, float& x1, float& x2, float& x3,
                float& x4, float& x5, float& x6, float& x7) {
  const float s0 = x0 + x7, s1 = x1 + x6, s2 = x2 + x5, s3 = x3 + x4;
  const float d0 = x0 - x7, d1 = x1 - x6, d2 = x2 - x5, d3 = x3 - x4;
  const float e0 = s0 + s3, e1 = s1 + s2, e2 = s0 - s3, e3 = s1 - s2;
  x0 = C4 * (e0 + e1);
  x4 = C4 * (e0 - e1);
  x2 = ffma(C2, e2, C6 * e3);
  x6 = ffma(C6, e2, -C2 * e3);
  x1 = ffma(C1, d0, ffma(C3, d1, ffma(C5, d2, C7 * d3)));
  x3 = ffma(C3, d0, ffma(-C7, d1, ffma(-C1, d2, -C5 * d3)));
  x5 = ffma(C5, d0, ffma(-C1, d1, ffma(C7, d2, C3 * d3)));
  x7 = ffma(C7, d0, ffma(-C5, d1, ffma(C3, d2, -C1 * d3)));
}

// inverse (DCT-III with the same orthonormal scaling)
WM_HD void idct8(float& x0, float& x1, float& x2, float& x3,
                 float& x4, float& x5, float& x6, float& x7) {
  const float p = C4 * (x0 + x4), q = C4 * (x0 - x4);
  const float r = ffma(C2, x2, C6 * x6), t = ffma(C6, x2, -C2 * x6);
  const float e0 = p + r, e3 = p - r, e1 = q + t, e2 = q - t;
  const float o0 = ffma(C1, x1, ffma(C3, x3, ffma(C5, x5, C7 * x7)));
  const float o1 = ffma(C3, x1, ffma(-C7, x3, ffma(-C1, x5, -C5 * x7)));
  const float o2 = ffma(C5, x1, ffma(-C1, x3, ffma(C7, x5, C3 * x7)));
  const float o3 = ffma(C7, x1, ffma(-C5, x3, ffma(C3, x5, -C1 * x7)));
  x0 = e0 + o0; x7 = e0 - o0;
  x1 = e1 + o1; x6 = e1 - o1;
  x2 = e2 + o2; x5 = e2 - o2;
  x3 = e3 + o3; x4 = e3 - o3;
}

// 2-D transforms on a[row][col]:  C = D X D^T   /   X = D^T C D
WM_HD void dct8x8(float (&a)[8][8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c)
    dct8(a[0][c], a[1][c], a[2][c], a[3][c], a[4][c], a[5][c], a[6][c], a[7][c]);
#pragma unroll
  for (int r = 0; r < 8; ++r)
    dct8(a[r][0], a[r][1], a[r][2], a[r][3], a[r][4], a[r][5], a[r][6], a[r][7]);
}
WM_HD void idct8x8(float (&a)[8][8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
    idct8(a[r][0], a[r][1], a[r][2], a[r][3], a[r][4], a[r][5], a[r][6], a[r][7]);
#pragma unroll
  for (int c = 0; c < 8; ++c)
    idct8(a[0][c], a[1][c], a[2][c], a[3][c], a[4][c], a[5][c], a[6][c], a[7][c]);
}

// ---- one-sided (Hestenes) Jacobi SVD of an 8x8 matrix ------------------------
// Row-cyclic pair order with de Rijk's norm ordering (the larger column of a
// pair always ends in the lower index), so singular values come out sorted
// descending like LAPACK's.  On return
//   a  = B = A*V     (mutually orthogonal columns, |b_i| descending)
//   v  = V           (accumulated plane rotations; WITH_V only)
//   n2 = |b_i|^2 ,  vn2 = |v_i|^2 (exactly 1 in exact arithmetic; carried so the
//        1-ulp drift of v_rsq_f32 cancels in sigma_i = |b_i| / |v_i|).
// Sweeps stop when a whole sweep saw no pair with cos^2 > CONV2 for any tile
// of the wave (Jacobi converges quadratically: a sweep that starts below
// 3e-4 ends at rounding level), bounded by MAX_SWEEPS.
constexpr float JAC_TOL2 = 1e-15f;   // skip a rotation below cos = 3.2e-8
constexpr float JAC_CONV2 = 1e-7f;   // "converged" sweep: max cos < 3.2e-4
constexpr int JAC_MAX_SWEEPS = 12;
constexpr int JAC_DEFI_FROM = 6;     // sweeps after which a rank-deficient tile stops counting as "not converged"
constexpr int JAC_SIGMA_FOLD_AT = 6;  // sigma-only iteration: the 0-based sweep ahead of whose norms the scales go into B, once
// Singular VALUES alone converge one order ahead of the vectors: after a sweep that saw
// max cos c the columns are orthogonal to ~c^2 and |b_i| = s_i (1 + O(c^4)), so the
// sigma-only kernels (extract, detect, K2) may stop well above the embed's threshold.  The embed keeps
// JAC_CONV2: its reconstruction needs the VECTORS (B orthogonal to 1e-7).
// How far above is set by near-degenerate pairs, whose values move by c s_i / 2 where a separated pair's move by
// c^2 s_i s_j^2 / gap: a cosine alone cannot tell them apart.  Behind the LQ prelude most waves end on their 3rd sweep, which
// sits closer to the threshold than the 4th used to, and at cos^2 <= 1e-3 alone (the test before the prelude: 4.1 sweeps
// per wave, every error at the float32 floor of 8.6e-7 s_1) 7 of 25 600 noise tiles come out above 2e-6 s_1, the worst
// at 2.6e-5 - enough to move an extracted watermark pixel by 0.2 grey levels.  So a tested rotation also reports what
// it did to the VALUES: w = |t g| is what it moves the two squared norms by (|g| for a degenerate pair, g^2 / gap for
// a separated one), and a sweep is the last one only if no rotation of it had w > sqrt(JAC_MOVE2) s_1 s_p (w^2 >
// JAC_MOVE2 n2[0] max(n2[p], n2[q])).  With that test next to it the cosine bound may be loose: at cos^2 <= 1e-2 and
// JAC_MOVE2 = 1e-6 every tile of tools/conv_study.cpp 3 is at the floor (1.1e-6 s_1) with 3.2 sweeps per wave; the cosine
// alone needs 3e-4 for that, at 3.5.  A sweep that passes JAC_CONV2 passes the move test too (w <= |g| <= 3.2e-4 s_p s_q):
// the embed's iteration is unchanged by it.
constexpr float JAC_CONV2_SIGMA = 1e-2f;
constexpr float JAC_MOVE2 = 1e-6f;
// From the 4th sweep on - the first that can be the last behind the LQ prelude - the embed's sweeps test every pair
// before rotating it: a pair below cos^2 = 1e-12 in all 64 tiles of a wave is left alone and costs its dot product
// only (tools/skip_study.cpp lq: profiles/r05_skip_study_lq.txt has the share of such pair visits per sweep).  1e-12 is
// cos = 1e-6, an order above the float32 floor the full sweeps end at (1.2e-7): measured against the
// round-1 kernel the stego differs by 1 LSB on 4.5e-6 of the pixels (profiles/r02_embed_variants.md).
constexpr float JAC_SKIP2 = 1e-12f;

template <bool WITH_V>
WM_HD void jacobi_rot(float (&a)[8][8], float (&v)[8][8], float (&n2)[8],
                      const int p, const int q, bool& notconv) {
  float g = a[0][p] * a[0][q];
#pragma unroll
  for (int r = 1; r < 8; ++r) g = ffma(a[r][p], a[r][q], g);
  const float al = n2[p], be = n2[q];
  const float ab = al * be, gg = g * g;
  const bool big = gg > JAC_TOL2 * ab;
  notconv = notconv || (gg > JAC_CONV2 * ab);
  const float tau = be - al, g2 = g + g;
  const float h = fsqrt(ffma(tau, tau, g2 * g2));
  float t = g2 * frcp(fabsf(tau) + h);     // 0/0 only when g == 0 -> !big
  t = (tau < 0.0f) ? -t : t;
  t = big ? t : 0.0f;
  const float c = frsq(ffma(t, t, 1.0f)), s = c * t;
  const float tg = t * g;
  const float aln = al - tg, ben = be + tg;
  const bool sw = tau > 0.0f;              // |a_q| > |a_p|: rotate a further 90 deg
  const float C = sw ? s : c, S = sw ? -c : s;
  n2[p] = sw ? ben : aln;
  n2[q] = sw ? aln : ben;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const float x = a[r][p], y = a[r][q];
    a[r][p] = ffma(C, x, -S * y);
    a[r][q] = ffma(S, x, C * y);
  }
  if (WITH_V) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const float x = v[r][p], y = v[r][q];
      v[r][p] = ffma(C, x, -S * y);
      v[r][q] = ffma(S, x, C * y);
    }
  }
}

WM_HD void col_norms2(const float (&a)[8][8], float (&n2)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float s = a[0][c] * a[0][c];
#pragma unroll
    for (int r = 1; r < 8; ++r) s = ffma(a[r][c], a[r][c], s);
    n2[c] = s;
  }
}

template <bool WITH_V>
WM_HD int jacobi_svd8(float (&a)[8][8], float (&v)[8][8], float (&n2)[8], float (&vn2)[8]) {
  if (WITH_V) {
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int c = 0; c < 8; ++c) v[r][c] = (r == c) ? 1.0f : 0.0f;
  }
  int sweep = 0;
  bool more = true;
  while (more && sweep < JAC_MAX_SWEEPS) {
    col_norms2(a, n2);
    bool notconv = false;
#pragma unroll
    for (int p = 0; p < 7; ++p)
#pragma unroll
      for (int q = p + 1; q < 8; ++q) jacobi_rot<WITH_V>(a, v, n2, p, q, notconv);
    ++sweep;
    more = wave_any(notconv);
  }
  col_norms2(a, n2);
  if (WITH_V) col_norms2(v, vn2);
  else {
#pragma unroll
    for (int c = 0; c < 8; ++c) vn2[c] = 1.0f;
  }
  return more ? -sweep : sweep;   // negative: sweep bound hit before convergence
}

// ============================================================================
// Packed (v_pk_*_f32) V-free formulation - the production embed/sigma path.
//
// Two identities remove ~45 % of the arithmetic of the literal chain
// dct2 -> svd -> U diag(S') V^T -> idct2 without changing its result beyond
// float32 rounding (parity is checked against the literal oracle):
//  (1) the DCT is orthonormal:  svd(D X D^T) = (D Ux) S (D Vx)^T, so the
//      singular values of the DCT plane ARE those of the pixel tile and
//      idct2(Uc S' Vc^T) = Ux S' Vx^T: forward and inverse DCT cancel.
//  (2) with S' = S + w (w_i = alpha*sw_i for i < K):
//      Ux S' Vx^T = X + Ux diag(w_i / s_i) Ux^T X,  because Vx^T = S^-1 Ux^T X.
//      One-sided Jacobi delivers B = X V = Ux S directly, so V is never formed.
// Rounding noise of (2) is (w_i/s_i) * eps * |X|; tiles whose smallest singular
// value is below SIGMA_RATIO_MIN * s_1 (flat / rank-deficient tiles) take the
// literal DCT-domain path (embed_tile) instead.
//
// Register layout: rows are packed in pairs, a[rp][c] = (x[2rp][c], x[2rp+1][c]),
// so a column rotation is the same packed op on 4 registers per column.
// ============================================================================
typedef float v2f __attribute__((vector_size(8)));

WM_HD v2f splat2(float s) { v2f r = {s, s}; return r; }
WM_HD v2f fma2(v2f a, v2f b, v2f c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_elementwise_fma(a, b, c);
#else
  v2f r = {fmaf(a[0], b[0], c[0]), fmaf(a[1], b[1], c[1])};
  return r;
#endif
}

// dct8 / idct8 on packed row pairs (both rows of a pair at once): the row pass of the 2-D transform in the layout
// the iteration works in.  Same formulas as the scalar forms above.
WM_HD void dct8_pk(v2f& x0, v2f& x1, v2f& x2, v2f& x3, v2f& x4, v2f& x5, v2f& x6, v2f& x7) {
  const v2f s0 = x0 + x7, s1 = x1 + x6, s2 = x2 + x5, s3 = x3 + x4;
  const v2f d0 = x0 - x7, d1 = x1 - x6, d2 = x2 - x5, d3 = x3 - x4;
  const v2f e0 = s0 + s3, e1 = s1 + s2, e2 = s0 - s3, e3 = s1 - s2;
  x0 = splat2(C4) * (e0 + e1);
  x4 = splat2(C4) * (e0 - e1);
  x2 = fma2(splat2(C2), e2, splat2(C6) * e3);
  x6 = fma2(splat2(C6), e2, splat2(-C2) * e3);
  x1 = fma2(splat2(C1), d0, fma2(splat2(C3), d1, fma2(splat2(C5), d2, splat2(C7) * d3)));
  x3 = fma2(splat2(C3), d0, fma2(splat2(-C7), d1, fma2(splat2(-C1), d2, splat2(-C5) * d3)));
  x5 = fma2(splat2(C5), d0, fma2(splat2(-C1), d1, fma2(splat2(C7), d2, splat2(C3) * d3)));
  x7 = fma2(splat2(C7), d0, fma2(splat2(-C5), d1, fma2(splat2(C3), d2, splat2(-C1) * d3)));
}
WM_HD void idct8_pk(v2f& x0, v2f& x1, v2f& x2, v2f& x3, v2f& x4, v2f& x5, v2f& x6, v2f& x7) {
  const v2f p = splat2(C4) * (x0 + x4), q = splat2(C4) * (x0 - x4);
  const v2f r = fma2(splat2(C2), x2, splat2(C6) * x6), t = fma2(splat2(C6), x2, splat2(-C2) * x6);
  const v2f e0 = p + r, e3 = p - r, e1 = q + t, e2 = q - t;
  const v2f o0 = fma2(splat2(C1), x1, fma2(splat2(C3), x3, fma2(splat2(C5), x5, splat2(C7) * x7)));
  const v2f o1 = fma2(splat2(C3), x1, fma2(splat2(-C7), x3, fma2(splat2(-C1), x5, splat2(-C5) * x7)));
  const v2f o2 = fma2(splat2(C5), x1, fma2(splat2(-C1), x3, fma2(splat2(C7), x5, splat2(C3) * x7)));
  const v2f o3 = fma2(splat2(C7), x1, fma2(splat2(-C5), x3, fma2(splat2(C3), x5, splat2(-C1) * x7)));
  x0 = e0 + o0; x7 = e0 - o0;
  x1 = e1 + o1; x6 = e1 - o1;
  x2 = e2 + o2; x5 = e2 - o2;
  x3 = e3 + o3; x4 = e3 - o3;
}
// dct2 of a[row][col] into the packed form b[rp][c] = (C[2 rp][c], C[2 rp + 1][c]): column pass on the scalars, row pass
// on the pairs; and back.  (Packing the result of dct8x8 instead makes the compiler re-pair through scratch memory.)
WM_HD void dct8x8_to_pk(const float (&a)[8][8], v2f (&b)[4][8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {               // column pass, results straight into the pairs
    float x0 = a[0][c], x1 = a[1][c], x2 = a[2][c], x3 = a[3][c], x4 = a[4][c], x5 = a[5][c], x6 = a[6][c], x7 = a[7][c];
    dct8(x0, x1, x2, x3, x4, x5, x6, x7);
    const v2f p0 = {x0, x1}, p1 = {x2, x3}, p2 = {x4, x5}, p3 = {x6, x7};
    b[0][c] = p0; b[1][c] = p1; b[2][c] = p2; b[3][c] = p3;
  }
#pragma unroll
  for (int rp = 0; rp < 4; ++rp)
    dct8_pk(b[rp][0], b[rp][1], b[rp][2], b[rp][3], b[rp][4], b[rp][5], b[rp][6], b[rp][7]);
}
WM_HD void idct8x8_from_pk(v2f (&b)[4][8], float (&a)[8][8]) {
#pragma unroll
  for (int rp = 0; rp < 4; ++rp)
    idct8_pk(b[rp][0], b[rp][1], b[rp][2], b[rp][3], b[rp][4], b[rp][5], b[rp][6], b[rp][7]);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float x0 = b[0][c][0], x1 = b[0][c][1], x2 = b[1][c][0], x3 = b[1][c][1];
    float x4 = b[2][c][0], x5 = b[2][c][1], x6 = b[3][c][0], x7 = b[3][c][1];
    idct8(x0, x1, x2, x3, x4, x5, x6, x7);
    a[0][c] = x0; a[1][c] = x1; a[2][c] = x2; a[3][c] = x3; a[4][c] = x4; a[5][c] = x5; a[6][c] = x6; a[7][c] = x7;
  }
}

// acc + (ab[HALF], ab[HALF]) * x  and  (ab[HALF], ab[HALF]) * x : the broadcast is the packed
// instruction's op_sel, written out so that the compiler cannot materialise (and then hoist and
// spill) the 64 broadcast pairs of B the embed epilogue reads.
template <int HALF>
WM_HD v2f fma2_bcast(const v2f ab, const v2f x, v2f acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (HALF == 0) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(ab), "v"(x));
  else asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0]" : "+v"(acc) : "v"(ab), "v"(x));
  return acc;
#else
  return fma2(splat2(ab[HALF]), x, acc);
#endif
}
template <int HALF>
WM_HD v2f mul2_bcast(const v2f ab, const v2f x) {
#if defined(__HIP_DEVICE_COMPILE__)
  v2f r;
  if (HALF == 0) asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(ab), "v"(x));
  else asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0]" : "=v"(r) : "v"(ab), "v"(x));
  return r;
#else
  return splat2(ab[HALF]) * x;
#endif
}

constexpr float SIGMA_RATIO_MIN2 = 1e-10f;   // (s_8 / s_1)^2 below this -> literal path

// one Jacobi rotation of columns p,q (no V).  c0 = cos, s0 = sin*sign(g) from
// two v_rsq_f32:  cos^2 = (1 + |tau|/h)/2,  sin = g / (h cos),  h^2 = tau^2+4g^2.
// CHECK: 0 = no convergence test, 1 = JAC_CONV2 (vectors needed), 2 = JAC_CONV2_SIGMA.
template <int CHECK, bool SKIP = false>
WM_HD void jacobi_rot_pk(v2f (&a)[4][8], float (&n2)[8], const int p, const int q, bool& notconv) {
  v2f gv = a[0][p] * a[0][q];
#pragma unroll
  for (int rp = 1; rp < 4; ++rp) gv = fma2(a[rp][p], a[rp][q], gv);
  const float g = gv[0] + gv[1];
  const float al = n2[p], be = n2[q];
  if (CHECK) notconv = notconv || (g * g > (CHECK == 2 ? JAC_CONV2_SIGMA : JAC_CONV2) * (al * be));
  // late sweeps: a pair that is below JAC_SKIP2 (cos^2) in every tile of the wave is left alone
  // (wave-uniform branch; the dot product and the test are all it costs)
  if (SKIP && !wave_any(g * g > JAC_SKIP2 * (al * be))) return;
  const float tau = be - al;
  const float ta = fabsf(tau) + 1e-18f;          // keeps 0/0 out: g == 0 -> cos = 1 exactly
  const float g2 = g + g;
  const float ih = frsq(ffma(g2, g2, ta * ta));  // 1/h
  const float x = ffma(0.5f * ta, ih, 0.5f);     // cos^2 in [0.5, 1]
  const float rx = frsq(x);
  const float c0 = x * rx;
  const float s0 = (g * ih) * rx;
  const bool sw = tau > 0.0f;                    // de Rijk: larger column ends in p
  const float C = sw ? s0 : c0, Sn = sw ? c0 : s0;
  const float w = fabsf((s0 * rx) * g);          // |t * g|: the larger norm grows by it
  if (CHECK) notconv = notconv || (w * w > (JAC_MOVE2 * fmaxf(al, be)) * n2[0]);
  n2[p] = fmaxf(al, be) + w;                     // (cancellation-free, unlike (al+be+-h)/2)
  n2[q] = fminf(al, be) - w;
  const v2f Cv = splat2(C), Sv = splat2(Sn);
#pragma unroll
  for (int rp = 0; rp < 4; ++rp) {
    const v2f X = a[rp][p], Y = a[rp][q];
    a[rp][p] = fma2(Cv, X, Sv * Y);
    a[rp][q] = fma2(Cv, Y, -(Sv * X));
  }
}

// jacobi_rot_pk<0> on SCALED columns a_c = sqrt(w2[c]) at_c, for the untested sweeps: `a` holds at_c, w2 the squared
// scales (rotation_scaled() of tools/gen_jacobi_asm.py, same operations).  wave_swaps: some tile of the wave wants the
// de Rijk swap at this pair (tau > 0).  Where none does, the update is two FMAs per element and no product:
//   at_p += t_p at_q ; at_q -= t_q at_p'     t_p = (gt / h) w_q / c^2,  t_q = (gt / h) w_p,  w_p *= c^2,  w_q /= c^2
// (a_p' = c (a_p + t a_q), a_q' = a_q / c - t a_p'; gt = at_p . at_q, g^2 = gt^2 w_p w_q); c^2 and 1 / c^2 come out of
// the angle's two rsq.  Where one does, the wave takes jacobi_rot_pk's four-product update with the scale ratios folded
// into its coefficients; the scales stay.  n2 are the TRUE squared norms throughout.
// c^2 is in [0.5, 1] and a column meets 7 rotations in each of at most 3 such sweeps: 2^-21 <= w2 <= 2^21, no rescaling.
// RCP: 1 / c^2 of the swap-free path is one v_rcp_f32 of c^2, not v_rsq_f32 and a square (the sigma-only iteration).
// TESTED: the tested form of the sigma-only iteration, whose columns stay scaled to the end - jacobi_rot_pk<2>'s
// convergence and norm-move tests on the true g^2 and the true norms (jacobi_cols_pk<true> keeps the scales in range).
template <bool TESTED, bool RCP>
WM_HD void jacobi_rot_scaled_pk(v2f (&a)[4][8], float (&n2)[8], float (&w2)[8], const int p, const int q, const bool wave_swaps,
                                bool& notconv) {
  v2f gv = a[0][p] * a[0][q];
#pragma unroll
  for (int rp = 1; rp < 4; ++rp) gv = fma2(a[rp][p], a[rp][q], gv);
  const float gt = gv[0] + gv[1];
  const float al = n2[p], be = n2[q];
  const float gg = (gt * (w2[p] * w2[q])) * gt;  // g^2
  if (TESTED) notconv = notconv || (gg > JAC_CONV2_SIGMA * (al * be));
  const float tau = be - al;
  const float ta = fabsf(tau) + 1e-18f;
  const float ih = frsq(ffma(gg, 4.0f, ta * ta));  // 1/h
  const float x = ffma(0.5f * ta, ih, 0.5f);       // cos^2 in [0.5, 1]
  const float u = gt * ih;
  const float gh = gg * ih;
  if (!wave_swaps) {                               // tau <= 0 in every tile: al IS the larger norm, no max / min
    const float rx2 = RCP ? frcp(x) : frsq(x) * frsq(x);   // 1 / cos^2
    const float tq = u * w2[p];
    const float v = u * rx2;
    const float w = gh * rx2;                      // |t g|
    w2[p] *= x;
    const float tp = v * w2[q];
    w2[q] *= rx2;
    const v2f Tp = splat2(tp), Tq = splat2(-tq);
#pragma unroll
    for (int rp = 0; rp < 4; ++rp) {
      a[rp][p] = fma2(Tp, a[rp][q], a[rp][p]);
      a[rp][q] = fma2(Tq, a[rp][p], a[rp][q]);
    }
    if (TESTED) notconv = notconv || (w * w > (JAC_MOVE2 * al) * n2[0]);
    n2[p] = al + w;
    n2[q] = be - w;
  } else {
    const float rx = frsq(x);
    const float pq = w2[p] * w2[q];
    const float c0 = x * rx;
    const float r = frsq(pq);                      // 1 / (d_p d_q)
    const float w = (gh * rx) * rx;
    const float s0 = (u * rx) * (pq * r);          // sin * sign(g)
    const float rq = w2[q] * r, rp_ = w2[p] * r;   // d_q / d_p, d_p / d_q
    const bool sw = tau > 0.0f;                    // de Rijk: larger column ends in p
    const float Sn = sw ? c0 : s0, C = sw ? s0 : c0;
    const v2f Cv = splat2(C), Sp = splat2(Sn * rq), Sq = splat2(Sn * rp_);
#pragma unroll
    for (int rp = 0; rp < 4; ++rp) {
      const v2f X = a[rp][p], Y = a[rp][q];
      a[rp][p] = fma2(Cv, X, Sp * Y);
      a[rp][q] = fma2(Cv, Y, -(Sq * X));
    }
    if (TESTED) notconv = notconv || (w * w > (JAC_MOVE2 * fmaxf(al, be)) * n2[0]);
    n2[p] = fmaxf(al, be) + w;
    n2[q] = fminf(al, be) - w;
  }
}
WM_HD void jacobi_rot_scaled_pk(v2f (&a)[4][8], float (&n2)[8], float (&w2)[8], const int p, const int q, const bool wave_swaps) {
  bool unused = false;
  jacobi_rot_scaled_pk<false, false>(a, n2, w2, p, q, wave_swaps, unused);
}

WM_HD void col_norms2_pk(const v2f (&a)[4][8], float (&n2)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    v2f s = a[0][c] * a[0][c];
#pragma unroll
    for (int rp = 1; rp < 4; ++rp) s = fma2(a[rp][c], a[rp][c], s);
    n2[c] = s[0] + s[1];
  }
}

// B = X V with orthogonal columns sorted by norm; n2 = |b_i|^2.  Returns the
// sweep count (negative: bound hit).
template <int CHECK, bool SKIP = false>
WM_HD void jacobi_sweep_pk(v2f (&a)[4][8], float (&n2)[8], bool& notconv) {
#pragma unroll
  for (int p = 0; p < 7; ++p)
#pragma unroll
    for (int q = p + 1; q < 8; ++q) jacobi_rot_pk<CHECK, SKIP>(a, n2, p, q, notconv);
}
// an untested sweep of jacobi_cols_pk: scaled columns, the swap decided per pair for the whole wave
template <bool RCP = false>
WM_HD void jacobi_sweep_scaled_pk(v2f (&a)[4][8], float (&n2)[8], float (&w2)[8]) {
  bool unused = false;
#pragma unroll
  for (int p = 0; p < 7; ++p)
#pragma unroll
    for (int q = p + 1; q < 8; ++q) jacobi_rot_scaled_pk<false, RCP>(a, n2, w2, p, q, wave_any(n2[q] - n2[p] > 0.0f), unused);
}
// a tested sweep of the sigma-only iteration: the same on scaled columns, with jacobi_rot_pk<2>'s tests
WM_HD void jacobi_sweep_scaled_tested_pk(v2f (&a)[4][8], float (&n2)[8], float (&w2)[8], bool& notconv) {
#pragma unroll
  for (int p = 0; p < 7; ++p)
#pragma unroll
    for (int q = p + 1; q < 8; ++q) jacobi_rot_scaled_pk<true, true>(a, n2, w2, p, q, wave_any(n2[q] - n2[p] > 0.0f), notconv);
}
// n2 of the scaled columns made true, and the scales folded back into B
WM_HD void col_norms2_scaled_pk(const v2f (&a)[4][8], const float (&w2)[8], float (&n2)[8]) {
  col_norms2_pk(a, n2);
#pragma unroll
  for (int c = 0; c < 8; ++c) n2[c] *= w2[c];
}
WM_HD void fold_scales_pk(v2f (&a)[4][8], const float (&w2)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const v2f d = splat2(w2[c] * frsq(w2[c]));
#pragma unroll
    for (int rp = 0; rp < 4; ++rp) a[rp][c] = d * a[rp][c];
  }
}

// ---- LQ prelude: B0 = X Q ahead of the sweeps ----------------------------------------------------------------------
// Householder LQ of the tile with greedy ROW pivoting, the reflectors applied from the right.  Step k = 0 .. 6: among the
// rows not used yet the one with the largest |x[k:]|^2 is the pivot, H = I - vh vh^T with vh = (x + sign(x_k) |x| e_k)
// sqrt(2 / v^T v) on columns k .. 7 zeroes its entries k+1 .. 7, and H is applied to all eight rows (used rows hold zeros
// there).  B0's column Gram matrix is that of the row-pivoted R^T: R R^T, one QR-algorithm step further on than X^T X,
// which costs the sweeps about one sweep (tools/conv_study.cpp; Jacobi on the columns of R itself would see X^T X again
// and gain nothing).  The row permutation never has to be applied - row order does not enter a column Gram matrix - and
// B0 = X * (orthogonal), so the sweeps still deliver B = X V and everything downstream of them is unchanged.
// A wrong pivot (exact ties: the first row wins; cancellation in the downdated norms) only costs convergence; a zero
// row gives vh = 0.  Same operations in the same order as lq_prelude() of tools/gen_jacobi_asm.py.
WM_HD float fmax3(const float a, const float b, const float c) { return fmaxf(fmaxf(a, b), c); }
WM_HD void lq_prelude_pk(v2f (&a)[4][8]) {
  v2f rn[4];                                       // |row[k:]|^2, row r in rn[r >> 1][r & 1]; -1e30 once the row is used
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int rp = 0; rp < 4; ++rp) rn[rp] = (c == 0) ? a[rp][c] * a[rp][c] : fma2(a[rp][c], a[rp][c], rn[rp]);
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    float m = fmax3(rn[0][0], rn[0][1], rn[1][0]);
    const float m2 = fmax3(rn[1][1], rn[2][0], rn[2][1]);
    m = fmaxf(fmax3(rn[3][0], rn[3][1], m), m2);
    float x[8];
    bool found = false;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const bool hit = rn[r >> 1][r & 1] == m;
      const bool mine = hit && !found;             // first match wins: exactly one pivot row
      found = found || hit;
      rn[r >> 1][r & 1] = mine ? -1e30f : rn[r >> 1][r & 1];
      if (r) {
#pragma unroll
        for (int c = k; c < 8; ++c) x[c] = mine ? a[r >> 1][c][r & 1] : (r == 1 ? a[0][c][0] : x[c]);
      }
    }
    float t2 = x[7] * x[7];
#pragma unroll
    for (int c = 6; c > k; --c) t2 = ffma(x[c], x[c], t2);                  // |x[k+1:]|^2
    const float nx2 = ffma(x[k], x[k], t2);
    const float nrm = copysignf(nx2 * frsq(fmaxf(1e-36f, nx2)), x[k]);      // sign(x_k) |x|, 0 for a zero row
    const float vk = x[k] + nrm;                                            // no cancellation
    const float sb = frsq(fmaxf(1e-36f, 0.5f * ffma(vk, vk, t2)));          // sqrt(2 / v^T v)
    x[k] = vk;
#pragma unroll
    for (int c = k; c < 8; ++c) x[c] *= sb;
    v2f w[4];                                                               // W = A vh
#pragma unroll
    for (int c = k; c < 8; ++c)
#pragma unroll
      for (int rp = 0; rp < 4; ++rp) w[rp] = (c == k) ? splat2(x[c]) * a[rp][c] : fma2(splat2(x[c]), a[rp][c], w[rp]);
#pragma unroll
    for (int c = k; c < 8; ++c)
#pragma unroll
      for (int rp = 0; rp < 4; ++rp) a[rp][c] = fma2(splat2(x[c]), -w[rp], a[rp][c]);
    if (k < 6) {
#pragma unroll
      for (int rp = 0; rp < 4; ++rp) rn[rp] = fma2(-a[rp][k], a[rp][k], rn[rp]);   // trailing norms lose column k
    }
  }
}

template <bool SIGMA_ONLY = false>
WM_HD int jacobi_cols_pk(v2f (&a)[4][8], float (&n2)[8]) {
  // The sweeps run on B0 = X Q (LQ prelude above).  Sweeps 1 and 2 carry no convergence test (a sweep can only be the
  // last one if it tested every pair, so these two are never last).  Column norms are recomputed before odd sweeps and
  // tracked through the even ones.
  // The untested sweeps work on scaled columns (jacobi_rot_scaled_pk): a holds a_c / sqrt(w2[c]) until the scales are
  // folded back behind the last of them; n2 are the true squared norms throughout.
  lq_prelude_pk(a);
  bool notconv = false;
  float w2[8] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
  col_norms2_pk(a, n2);
  jacobi_sweep_scaled_pk<SIGMA_ONLY>(a, n2, w2);
  jacobi_sweep_scaled_pk<SIGMA_ONLY>(a, n2, w2);
  int sweep = 2;
  // The embed's third sweep carries no test either: behind the prelude no image or noise tile is done after three
  // sweeps at cos^2 <= 1e-7 (tools/skip_study.cpp), so the earliest last sweep is the 4th - and that one already tests
  // every pair before rotating it (JAC_SKIP2), as every later one does.
  if (!SIGMA_ONLY) {
    col_norms2_scaled_pk(a, w2, n2);
    jacobi_sweep_scaled_pk(a, n2, w2);
    sweep = 3;
  }
  // The sigma-only iteration hands out nothing but the norms: its columns stay scaled to the end (no fold here, scaled
  // rotations in the tested sweeps, every recomputed norm multiplied by its scale).  A scale moves by at most 2^+-7 per
  // sweep, so the scales are folded into B once, ahead of the 7th sweep's norms: 2^+-42 on either side of it up to the
  // sweep bound (only a wave with rank-deficient tiles gets there).
  if (!SIGMA_ONLY) fold_scales_pk(a, w2);
  bool more = true;
  while (more && sweep < JAC_MAX_SWEEPS) {
    if ((sweep & 1) == 0) {
      if (SIGMA_ONLY && sweep == JAC_SIGMA_FOLD_AT) {
        fold_scales_pk(a, w2);
#pragma unroll
        for (int c = 0; c < 8; ++c) w2[c] = 1.0f;
      }
      if (SIGMA_ONLY) col_norms2_scaled_pk(a, w2, n2);
      else col_norms2_pk(a, n2);
    }
    notconv = false;
    if (!SIGMA_ONLY) jacobi_sweep_pk<1, true>(a, n2, notconv);
    else jacobi_sweep_scaled_tested_pk(a, n2, w2, notconv);
    ++sweep;
    // a rank-deficient tile's null columns are rounding residue whose cosines never fall (and whose tracked norms
    // cancel to garbage): after JAC_DEFI_FROM sweeps such a lane no longer keeps its wave iterating (gen_jacobi_asm.py)
    if (sweep >= JAC_DEFI_FROM && !(n2[7] > SIGMA_RATIO_MIN2 * n2[0])) notconv = false;
    more = wave_any(notconv);
  }
  if (SIGMA_ONLY) {
    col_norms2_scaled_pk(a, w2, n2);
    fold_scales_pk(a, w2);               // a caller that looks at B gets the true columns (dead code where none does)
  } else {
    col_norms2_pk(a, n2);
  }
  return more ? -sweep : sweep;
}

// raw tile: 8 rows x (lo, hi) little-endian byte words, as loaded from memory
struct RawTile { uint32_t lo[8], hi[8]; };

WM_HD float raw_px(const RawTile& t, const int r, const int c) {
  const uint32_t w = (c < 4) ? t.lo[r] : t.hi[r];
  return (float)((w >> (8 * (c & 3))) & 0xffu);
}
WM_HD void raw_to_pk(const RawTile& t, v2f (&a)[4][8]) {
#pragma unroll
  for (int rp = 0; rp < 4; ++rp)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      v2f v = {raw_px(t, 2 * rp, c), raw_px(t, 2 * rp + 1, c)};
      a[rp][c] = v;
    }
}
WM_HD void raw_to_f32(const RawTile& t, float (&a)[8][8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) a[r][c] = raw_px(t, r, c);
}

// singular values of a raw uint8 tile (pixel domain == DCT domain, identity (1))
WM_HD int sigma_tile_pk(const RawTile& t, float (&s)[8]) {
  v2f a[4][8];
  float n2[8];
  raw_to_pk(t, a);
  const int sweeps = jacobi_cols_pk<true>(a, n2);
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = fsqrt(n2[i]);
  return sweeps;
}

// ---- uint8 quantisation: np.clip(x, 0, 255).astype(np.uint8) ----------------
WM_HD uint32_t quant_u8(float x) {
  x = fminf(fmaxf(x, 0.0f), 255.0f);   // NaN -> 0 via fmaxf
  return (uint32_t)x;                  // truncation toward zero
}

// V-free embed of a raw tile.  `out` receives the quantised stego bytes, sc the
// host singular values Sc; when YW is true the unclipped float stego is written
// through `yw` (row stride `yw_stride` floats).  Returns sweeps; `deficient` is
// set when the tile must take the literal path instead.
// Phase 1 (registers: B only): B = X V from the raw tile.
WM_HD int embed_jacobi_pk(const RawTile& t, v2f (&a)[4][8], float (&n2)[8]) {
  raw_to_pk(t, a);
  return jacobi_cols_pk(a, n2);
}

// Phase 2a: singular values out, e_i = alpha_i sw_i / s_i^3, rank-deficiency flag.
WM_HD void embed_coeffs_pk(const float (&n2)[8], const float (&sw)[8], const float (&alpha_k)[8],
                           float (&e)[8], float (&sc)[8], bool& deficient) {
  deficient = !(n2[7] > SIGMA_RATIO_MIN2 * n2[0]);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float rs = frsq(fmaxf(n2[i], 1e-30f));
    sc[i] = n2[i] * rs;
    e[i] = (alpha_k[i] * sw[i]) * (rs * rs * rs);
  }
}

// Phase 2b: four columns of Y = X + B G, G = diag(e) (B^T X), from the eight row words `w`
// (little-endian bytes = the four pixels of each row in this half), one column pair at a time
// so that only 8 packed registers of G are live next to B:  g[i] = (G[i][c], G[i][c+1]);
// b_i[r] is one half of a[r>>1][i], broadcast by the packed FMA's op_sel.  Columns of X only
// enter their own columns of Y, so the two halves of a tile are independent (the kernel loads,
// finishes and stores them one after the other to stay within 128 VGPRs).
// outw: quantised stego bytes; with YW the unclipped floats go to yw[r * yw_stride + 0..3].
template <bool YW>
WM_HD void embed_half_pk(const uint32_t (&w)[8], const v2f (&a)[4][8], const float (&e)[8],
                         uint32_t (&outw)[8], float* yw, const size_t yw_stride) {
#pragma unroll
  for (int r = 0; r < 8; ++r) outw[r] = 0u;
#pragma unroll
  for (int cp = 0; cp < 2; ++cp) {
    const int sh = 16 * cp;
    v2f g[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t ww = w[r] >> sh;
      const v2f x = {(float)(ww & 0xffu), (float)((ww >> 8) & 0xffu)};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const v2f ab = a[r >> 1][i];
        if (r == 0) g[i] = mul2_bcast<0>(ab, x);
        else g[i] = (r & 1) ? fma2_bcast<1>(ab, x, g[i]) : fma2_bcast<0>(ab, x, g[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = g[i] * splat2(e[i]);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t ww = w[r] >> sh;
      v2f y = {(float)(ww & 0xffu), (float)((ww >> 8) & 0xffu)};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const v2f ab = a[r >> 1][i];
        y = (r & 1) ? fma2_bcast<1>(ab, g[i], y) : fma2_bcast<0>(ab, g[i], y);
      }
      if (YW) {
        float* o = yw + (size_t)r * yw_stride + 2 * cp;
        o[0] = y[0]; o[1] = y[1];
      }
      outw[r] |= (quant_u8(y[0]) | (quant_u8(y[1]) << 8)) << sh;
    }
  }
}

// Phase 2 in one piece (CPU harness / simple callers): the raw tile in, the stego tile out.
template <bool YW>
WM_HD void embed_finish_pk(const RawTile& t, const v2f (&a)[4][8], const float (&n2)[8],
                           const float (&sw)[8], const float (&alpha_k)[8], float (&sc)[8],
                           RawTile& out, float* yw, const size_t yw_stride, bool& deficient) {
  float e[8];
  embed_coeffs_pk(n2, sw, alpha_k, e, sc, deficient);
  embed_half_pk<YW>(t.lo, a, e, out.lo, yw, yw_stride);
  embed_half_pk<YW>(t.hi, a, e, out.hi, YW ? yw + 4 : nullptr, yw_stride);
}

// both phases back to back (CPU harness / simple callers)
template <bool YW>
WM_HD int embed_tile_pk(const RawTile& t, const float (&sw)[8], const float (&alpha_k)[8],
                        float (&sc)[8], RawTile& out, float* yw, const size_t yw_stride,
                        bool& deficient) {
  v2f a[4][8];
  float n2[8];
  const int sweeps = embed_jacobi_pk(t, a, n2);
  embed_finish_pk<YW>(t, a, n2, sw, alpha_k, sc, out, yw, yw_stride, deficient);
  return sweeps;
}


// ---- embed: tile (already float, pixel domain) -> stego tile (float) --------
// sw[8]: the watermark tile's singular values; alpha_k[i] = alpha for i < K,
// 0 otherwise.  sc[8] receives the host tile's singular values.
WM_HD int embed_tile(float (&a)[8][8], const float (&sw)[8], const float (&alpha_k)[8],
                     float (&sc)[8]) {
  float v[8][8], n2[8], vn2[8];
  dct8x8(a);
  const int sweeps = jacobi_svd8<true>(a, v, n2, vn2);
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float nb = fsqrt(n2[i]), nv = fsqrt(vn2[i]);
    const float sig = nb * frcp(nv);                      // sigma_i = |b_i| / |v_i|
    sc[i] = sig;
    const float sp = ffma(alpha_k[i], sw[i], sig);        // S_[:K] = Sc[:K] + alpha*Sw[:K]
    const float den = nb * nv;
    f[i] = (den > 0.0f) ? sp * frcp(den) : 0.0f;          // sigma'_i / (|b_i| |v_i|)
  }
  // Cw = sum_i (b_i f_i) v_i^T   ==  U diag(S_) V^T
  float cw[8][8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    float bs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bs[i] = a[r][i] * f[i];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float s = bs[0] * v[c][0];
#pragma unroll
      for (int i = 1; i < 8; ++i) s = ffma(bs[i], v[c][i], s);
      cw[r][c] = s;
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) a[r][c] = cw[r][c];
  idct8x8(a);
  return sweeps;
}

// ---- rank-deficient tiles: deterministic orthonormal completion ---------------
// A flat / saturated tile has singular values that are exactly 0; its singular
// vectors there are arbitrary (LAPACK returns *some* orthonormal completion) but
// the scheme still injects alpha*sw_i along them (single:175-176).  One-sided
// Jacobi resolves directions to high *relative* accuracy, so adding
// COMPLETION_DELTA x a fixed full-rank pattern (cond 3.7) to the DCT tile makes
// U and V complete orthonormal bases; the pattern is subtracted again after
// the reconstruction, so the output moves by O(eps), not O(delta).
constexpr float COMPLETION_DELTA = 6.103515625e-05f;   // 2^-14
constexpr float COMPLETION_PATTERN[8][8] = {
  {-0.371394f, -0.079717f, -0.983650f, -0.554458f, -0.658720f, -0.953876f, +0.008741f, +0.773822f},
  {+0.770895f, +0.280528f, -0.063239f, +0.001315f, +0.675874f, -0.488476f, +0.610478f, +0.151159f},
  {+0.434160f, -0.517163f, -0.154770f, +0.779245f, -0.744333f, +0.573436f, +0.871420f, -0.682901f},
  {-0.025223f, -0.797351f, +0.189486f, -0.674952f, -0.442962f, +0.883550f, -0.294998f, +0.418505f},
  {-0.560398f, +0.910414f, +0.028949f, -0.670469f, -0.276553f, +0.424304f, +0.871431f, -0.253670f},
  {-0.405084f, +0.378566f, +0.483330f, +0.296345f, -0.562919f, -0.634010f, -0.141621f, +0.624869f},
  {+0.385623f, -0.252198f, +0.255703f, +0.219000f, -0.437414f, -0.709251f, -0.041911f, -0.468894f},
  {+0.789973f, +0.864080f, -0.920759f, -0.063243f, +0.524377f, -0.040678f, +0.003126f, -0.226323f}};

#include "wm_completion_tables.inc"     // CONST_TILE_S / CONST_TILE_M (tools/gen_completion_tables.py)

// ---- constant tiles (letterbox bars, flat backgrounds): the literal chain in closed form -------------
// Every pixel = v: dct2 is 8 v E00, and to first order in delta / (8 v) the SVD of 8 v E00 + delta P is the
// pattern's own (v = 0) or e0 followed by that of P[1:, 1:] (v > 0) - fixed vectors, so the chain
// "+ delta P -> svd -> U diag(S + alpha Sw) V^T -> - delta P -> idct2" is  v + alpha sum_i sw_i M_i  with the tabulated
// pixel-domain matrices M_i, and Sc = (8 v, 0, ..) + delta * (tabulated values).  Same completion as
// embed_tile_completed (which such a tile would otherwise go through, at ~40 k instructions per wave) to
// ~1e-2 grey levels; a constant tile takes THIS path whatever shares its wave, so results stay reproducible.
WM_HD bool raw_is_constant(const RawTile& t) {
  const uint32_t w = (t.lo[0] & 0xffu) * 0x01010101u;
  uint32_t diff = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) diff |= (t.lo[r] ^ w) | (t.hi[r] ^ w);
  return diff == 0;
}
WM_HD bool tile_is_constant(const float (&a)[8][8]) {
  bool same = true;
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) same = same && (a[r][c] == a[0][0]);
  return same;
}
// out <- Yw of the constant tile of value v; sc <- its (completed) singular values
WM_HD void embed_tile_constant(const float v, const float (&sw)[8], const float (&alpha_k)[8], float (&sc)[8],
                               float (&out)[8][8]) {
  const bool black = v == 0.0f;
  float w0[8], w1[8];                       // weights of the v == 0 / v > 0 tables: one of the two sets is zero
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float w = alpha_k[i] * sw[i];
    w0[i] = black ? w : 0.0f;
    w1[i] = black ? 0.0f : w;
    sc[i] = black ? CONST_TILE_S[0][i] : CONST_TILE_S[1][i];
  }
  sc[0] = ffma(8.0f, v, sc[0]);
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float acc = v;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = ffma(w0[i], CONST_TILE_M[0][i][r][c], ffma(w1[i], CONST_TILE_M[1][i][r][c], acc));
      out[r][c] = acc;
    }
}

// the same with the table known at compile time (a wave whose constant tiles are all black, or none of them):
// bit-identical to embed_tile_constant, whose other table only ever adds 0 * M
template <int TABLE>
WM_HD void embed_tile_constant_t(const float v, const float (&sw)[8], const float (&alpha_k)[8], float (&sc)[8],
                                 float (&out)[8][8]) {
  float w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    w[i] = alpha_k[i] * sw[i];
    sc[i] = CONST_TILE_S[TABLE][i];
  }
  sc[0] = ffma(8.0f, v, sc[0]);
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float acc = v;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = ffma(w[i], CONST_TILE_M[TABLE][i][r][c], acc);
      out[r][c] = acc;
    }
}

// ---- rank-1 tiles: the literal chain in closed form ------------------------------------------------------------
// X = a b^T with a, b >= 0: the edges of flat rectangles (rows or columns all equal), 1-pixel rules and their crossings
// on a flat background, one-axis gradients - 34 % + 4 % of the tiles of the synthetic screen content against 0.5 % of
// rank 2.  sigma_1 = |a| |b|, u_1 = a / |a|, v_1 = b / |b|; the other seven singular values are 0 and their vectors
// arbitrary (LAPACK returns SOME orthonormal completion; any one gives the reference's svd(Yw) = Sc + alpha Sw,
// single:174-176).  The completion taken here, in the pixel domain (the DCT is orthonormal and cancels):
//   U = H_u diag(-1, 1, ..),  V = H_v diag(-1, 1, ..),   H_u = I - beta_u p p^T with p = u_1 + e_0, beta_u = 1 / (1 + u_1[0])
//   (a Householder reflection with H_u e_0 = -u_1; pixels are >= 0, so u_1[0] >= 0 and p never cancels), H_v likewise from v_1:
//   Yw = U diag(Sc + w) V^T = X + H_u diag(w) H_v,      w = alpha Sw[:K]
//      = X + diag(w) - beta_u p (p o w)^T - beta_v (w o q) q^T + beta_u beta_v (p^T diag(w) q) p q^T
// - four FMAs per pixel instead of a Jacobi with V (~40 000 instructions per wave).  a and b are read off the row and
// column sums (R = a sum(b), C = b sum(a)): u_1 = R / |R|, v_1 = C / |C|, sigma_1 = |R| |C| / sum(X).
// Rank 1 is decided EXACTLY on the integer pixels: X_ij * S == R_i * C_j for every i, j (S = sum(X) > 0).
WM_HD bool raw_rank1_pretest(const RawTile& t) {      // three 2x2 minors: textured tiles almost never pass, rank-1 tiles always
  const uint32_t x00 = t.lo[0] & 0xffu, x04 = t.hi[0] & 0xffu, x07 = t.hi[0] >> 24;
  const uint32_t x33 = t.lo[3] >> 24, x34 = t.hi[3] & 0xffu;
  const uint32_t x40 = t.lo[4] & 0xffu, x43 = t.lo[4] >> 24, x44 = t.hi[4] & 0xffu;
  const uint32_t x70 = t.lo[7] & 0xffu, x77 = t.hi[7] >> 24;
  return x00 * x77 == x07 * x70 && x33 * x44 == x34 * x43 && x00 * x44 == x04 * x40;
}
WM_HD bool raw_is_rank1(const RawTile& t) {
  uint32_t R[8], Cs[8], S = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) Cs[j] = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t b = ((j < 4 ? t.lo[r] : t.hi[r]) >> (8 * (j & 3))) & 0xffu;
      s += b; Cs[j] += b;
    }
    R[r] = s; S += s;
  }
  uint32_t bad = (S == 0) ? 1u : 0u;                  // the zero tile is a constant tile, not a rank-1 one
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t b = ((j < 4 ? t.lo[r] : t.hi[r]) >> (8 * (j & 3))) & 0xffu;
      bad |= (b * S) ^ (R[r] * Cs[j]);                // <= 255 * 16 320 and 2 040^2: no overflow
    }
  return bad == 0;
}
// x: the tile's pixels (rank 1, not zero); out <- Yw, sc <- singular values.  out may alias x.
WM_HD void embed_tile_rank1(const float (&x)[8][8], const float (&sw)[8], const float (&alpha_k)[8], float (&sc)[8],
                            float (&out)[8][8]) {
  float R[8], Cs[8], S = 0.0f;                        // sums of integers <= 16 320: exact in float
#pragma unroll
  for (int j = 0; j < 8; ++j) Cs[j] = 0.0f;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { s += x[r][j]; Cs[j] += x[r][j]; }
    R[r] = s; S += s;
  }
  float nr2 = 0.0f, nc2 = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) { nr2 = ffma(R[i], R[i], nr2); nc2 = ffma(Cs[i], Cs[i], nc2); }
  const float rr = frsq(nr2), rc = frsq(nc2);
  float p[8], q[8], w[8], pw[8], wq[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { p[i] = R[i] * rr; q[i] = Cs[i] * rc; w[i] = alpha_k[i] * sw[i]; sc[i] = 0.0f; }
  p[0] += 1.0f; q[0] += 1.0f;
  sc[0] = (nr2 * rr) * (nc2 * rc) * frcp(S);          // |R| |C| / S
  const float bu = frcp(p[0]), bv = frcp(q[0]);
  float gamma = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) { pw[i] = p[i] * w[i]; wq[i] = w[i] * q[i]; gamma = ffma(pw[i], q[i], gamma); }
  const float bg = bu * bv * gamma;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float c_p = -bu * p[i], c_q = -bv * wq[i], c_pq = bg * p[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = x[i][j] + ((i == j) ? w[i] : 0.0f);
      v = ffma(c_p, pw[j], v);
      v = ffma(c_q, q[j], v);
      v = ffma(c_pq, q[j], v);
      out[i][j] = v;
    }
  }
}

// ---- tiles with exactly ONE singular value out of the V-free form's reach (s_7 > 1e-5 s_1 >= s_8) --------------
// On noise and camera content this is what the flagged tiles are (~50 per 4K frame): full rank but with s_8 so small
// that  e_8 = w_8 / s_8^3  and  b_8^T X  cancel catastrophically - or rank 7 exactly.  They do not need the literal chain
// (Jacobi with V, ~40 k instructions per wave): the seven good vectors of either side come from the fast path's own
// B = X V (u_i = b_i / |b_i|, v_i = X^T b_i / s_i^2), and the eighth of either side is DETERMINED by them - the orthogonal
// complement of seven vectors in R^8 is a line:  P = I - sum_i q_i q_i^T  is  q_8 q_8^T, so its column with the largest
// diagonal entry (>= 1/8), orthogonalised once more and normalised, is q_8 up to sign (better than b_8 / |b_8|, whose
// direction is only good to eps s_1 / s_8).  The joint sign of (u_8, v_8) is that of u_8^T X v_8 = +-s_8, evaluated in
// FLOAT64: the vectors' float32 errors enter it only in second order (each is orthogonal to its side's other seven), so
// the sign is right down to s_8 ~ 1e-12 s_1 - where the reference's float64 LAPACK stops resolving it too.  With
// s_8 == 0 exactly the reference's pair is arbitrary and so is this one.   Yw = X + sum_i alpha sw_i u_i v_i^T, Sc = |b_i|.
// bb[r][i] = component r of b_i (the layout of the fast kernel's packed a[r >> 1][i][r & 1]).
WM_HD bool n2_one_small(const float (&n2)[8]) { return n2[6] > SIGMA_RATIO_MIN2 * n2[0]; }
// r <- unit vector orthogonal to q_0 .. q_6, q_i[a] = Q(i, a) * scale[i]
template <typename QF>
WM_HD void complement_of_seven(const QF& Q, float (&r)[8]) {
  float diag[8];                                   // of P = I - sum q_i q_i^T: only the diagonal and ONE column are formed
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    float acc = 1.0f;
#pragma unroll
    for (int i = 0; i < 7; ++i) acc = ffma(-Q(i, a), Q(i, a), acc);
    diag[a] = acc;
  }
  int best = 0;
  float dbest = diag[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) { const bool gt = diag[k] > dbest; best = gt ? k : best; dbest = gt ? diag[k] : dbest; }
  float qb[7];                                     // q_i[best]
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    float v = Q(i, 0);
#pragma unroll
    for (int k = 1; k < 8; ++k) v = (best == k) ? Q(i, k) : v;
    qb[i] = v;
  }
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    float acc = (best == a) ? 1.0f : 0.0f;
#pragma unroll
    for (int i = 0; i < 7; ++i) acc = ffma(-Q(i, a), qb[i], acc);
    r[a] = acc;
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) {                    // once more against the seven: the column carries their rounding
    float d = 0.0f;
#pragma unroll
    for (int a = 0; a < 8; ++a) d = ffma(r[a], Q(i, a), d);
#pragma unroll
    for (int a = 0; a < 8; ++a) r[a] = ffma(-d, Q(i, a), r[a]);
  }
  float n = 0.0f;
#pragma unroll
  for (int a = 0; a < 8; ++a) n = ffma(r[a], r[a], n);
  const float rn = frsq(n);
#pragma unroll
  for (int a = 0; a < 8; ++a) r[a] *= rn;
}
WM_HD void embed_tile_one_small(const float (&x)[8][8], const float (&bb)[8][8], const float (&sw)[8],
                                const float (&alpha_k)[8], float (&sc)[8], float (&out)[8][8]) {
  // three 8 x 8 arrays live at a time (x, B, V): u_i = b_i / |b_i| stays folded into the weights
  float v[8][8];                                   // v[i][c]
  float rs[8];                                     // 1 / |b_i|
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float n = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r) n = ffma(bb[r][i], bb[r][i], n);
    rs[i] = frsq(fmaxf(n, 1e-30f));
    sc[i] = n * rs[i];
  }
  float u7[8];
  complement_of_seven([&](const int i, const int a) { return bb[a][i] * rs[i]; }, u7);
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const float r2 = rs[i] * rs[i];                // v_i = X^T b_i / s_i^2
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float acc = 0.0f;
#pragma unroll
      for (int r = 0; r < 8; ++r) acc = ffma(x[r][c], bb[r][i], acc);
      v[i][c] = acc * r2;
    }
  }
  complement_of_seven([&](const int i, const int a) { return v[i][a]; }, v[7]);
  {
    double d = 0.0;                                // sigma_8 >= 0: u_8^T X v_8 must not be negative (float64: see above)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      double t = 0.0;
#pragma unroll
      for (int c = 0; c < 8; ++c) t += (double)x[r][c] * (double)v[7][c];
      d += (double)u7[r] * t;
    }
    const float sgn = (d < 0.0) ? -1.0f : 1.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) v[7][c] *= sgn;
  }
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float acc = ffma(alpha_k[7] * sw[7] * u7[r], v[7][c], x[r][c]);
#pragma unroll
      for (int i = 0; i < 7; ++i) acc = ffma(alpha_k[i] * sw[i] * rs[i] * bb[r][i], v[i][c], acc);
      out[r][c] = acc;
    }
}

// ---- any rank from 2 to 6: the same construction with more than one missing pair ------------------------------
// Ranks i with s_i > 1e-5 s_1 take u_i, v_i from B as above; every other rank gets a pair (u_j, v_j) from the orthogonal
// complements of what is there so far, one vector at a time (largest diagonal entry of the current projector, orthogonalised
// once more, normalised).  More than one missing direction per side: the reference's completion is arbitrary (LAPACK's
// choice of a basis of the null spaces) and so is this one; what holds whatever the choice - svd(Yw) = Sc + alpha Sw,
// Sc = the tile's singular values, the injected energy - is what the tests check.  u[i][r], v[i][c] hold zero vectors for
// the ranks not filled yet, so every sum runs over all eight slots.
WM_HD void complete_next(const float (&q)[8][8], float (&r)[8]) {
  float diag[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    float acc = 1.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = ffma(-q[i][a], q[i][a], acc);
    diag[a] = acc;
  }
  int best = 0;
  float dbest = diag[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) { const bool gt = diag[k] > dbest; best = gt ? k : best; dbest = gt ? diag[k] : dbest; }
#pragma unroll
  for (int a = 0; a < 8; ++a) r[a] = (best == a) ? 1.0f : 0.0f;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float d = 0.0f;
#pragma unroll
      for (int a = 0; a < 8; ++a) d = ffma(r[a], q[i][a], d);
#pragma unroll
      for (int a = 0; a < 8; ++a) r[a] = ffma(-d, q[i][a], r[a]);
    }
  float n = 0.0f;
#pragma unroll
  for (int a = 0; a < 8; ++a) n = ffma(r[a], r[a], n);
  const float rn = frsq(n);
#pragma unroll
  for (int a = 0; a < 8; ++a) r[a] *= rn;
}
WM_HD void embed_tile_from_b(const float (&x)[8][8], const float (&bb)[8][8], const float (&sw)[8],
                             const float (&alpha_k)[8], float (&sc)[8], float (&out)[8][8]) {
  float u[8][8], v[8][8];
  bool good[8];
  float n0 = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float n = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r) n = ffma(bb[r][i], bb[r][i], n);
    if (i == 0) n0 = n;
    const float rs = frsq(fmaxf(n, 1e-30f));
    sc[i] = n * rs;
    good[i] = n > SIGMA_RATIO_MIN2 * n0 && n > 0.0f;
    const float g = good[i] ? rs : 0.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r) u[i][r] = bb[r][i] * g;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float acc = 0.0f;
#pragma unroll
      for (int r = 0; r < 8; ++r) acc = ffma(x[r][c], u[i][r], acc);
      v[i][c] = acc * g;                           // X^T u_i / s_i  (0 for the ranks to be completed)
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (!good[j]) {
      float ru[8], rv[8];
      complete_next(u, ru);
      complete_next(v, rv);
#pragma unroll
      for (int a = 0; a < 8; ++a) { u[j][a] = ru[a]; v[j][a] = rv[a]; }
    }
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float acc = x[r][c];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = ffma(alpha_k[i] * sw[i] * u[i][r], v[i][c], acc);
      out[r][c] = acc;
    }
}

WM_HD void add_completion(float (&a)[8][8], const float scale) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) a[r][c] = ffma(scale, COMPLETION_PATTERN[r][c], a[r][c]);
}

// the same on the packed form (rows 2 rp, 2 rp + 1 of column c in one v2f): what the literal chain uses, so that the
// pattern is added in the layout the iteration works in (added to a[r][c] the compiler pairs neighbouring COLUMNS
// and re-pairs them through scratch memory)
WM_HD void add_completion_pk(v2f (&b)[4][8], const float scale) {
#pragma unroll
  for (int rp = 0; rp < 4; ++rp)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const v2f pt = {COMPLETION_PATTERN[2 * rp][c], COMPLETION_PATTERN[2 * rp + 1][c]};
      b[rp][c] = fma2(splat2(scale), pt, b[rp][c]);
    }
}

// ---- packed one-sided Jacobi WITH V: A and V stacked as one 16-row matrix ----
// The same rotation (jacobi_rot_pk's two-rsq angle) is applied to the 4 row pairs
// of A and the 4 row pairs of V; dot products and norms come from the A half only.
template <int CHECK>
WM_HD void jacobi_rot_pk_v(v2f (&a)[4][8], v2f (&v)[4][8], float (&n2)[8], const int p, const int q,
                           bool& notconv) {
  v2f gv = a[0][p] * a[0][q];
#pragma unroll
  for (int rp = 1; rp < 4; ++rp) gv = fma2(a[rp][p], a[rp][q], gv);
  const float g = gv[0] + gv[1];
  const float al = n2[p], be = n2[q];
  if (CHECK) notconv = notconv || (g * g > JAC_CONV2 * (al * be));
  const float tau = be - al;
  const float ta = fabsf(tau) + 1e-18f;
  const float g2 = g + g;
  const float ih = frsq(ffma(g2, g2, ta * ta));
  const float x = ffma(0.5f * ta, ih, 0.5f);
  const float rx = frsq(x);
  const float c0 = x * rx;
  const float s0 = (g * ih) * rx;
  const bool sw = tau > 0.0f;
  const float C = sw ? s0 : c0, Sn = sw ? c0 : s0;
  const float w = fabsf((s0 * rx) * g);
  n2[p] = fmaxf(al, be) + w;
  n2[q] = fminf(al, be) - w;
  const v2f Cv = splat2(C), Sv = splat2(Sn);
#pragma unroll
  for (int rp = 0; rp < 4; ++rp) {
    const v2f X = a[rp][p], Y = a[rp][q];
    a[rp][p] = fma2(Cv, X, Sv * Y);
    a[rp][q] = fma2(Cv, Y, -(Sv * X));
  }
#pragma unroll
  for (int rp = 0; rp < 4; ++rp) {
    const v2f X = v[rp][p], Y = v[rp][q];
    v[rp][p] = fma2(Cv, X, Sv * Y);
    v[rp][q] = fma2(Cv, Y, -(Sv * X));
  }
}

// B = A V (columns orthogonal, sorted by norm), V accumulated from the identity.
// n2 = |b_i|^2, vn2 = |v_i|^2 (1 up to the drift of v_rsq_f32, carried so that it
// cancels in sigma_i = |b_i| / |v_i|).  Column norms are recomputed before every
// sweep: this is the path for tiles whose trailing columns are ~1e-8 of the leading one.
#if defined(__HIPCC__) && !defined(WM_NO_ASM_JACOBI) && !defined(WM_NO_ASM_JACOBI_V)
#include "wm_jacobi_v_gfx950.inc"      // generated gfx950 stream of the iteration below (tools/gen_jacobi_asm.py)
#endif
WM_HD int jacobi_cols_pk_v(v2f (&a)[4][8], v2f (&v)[4][8], float (&n2)[8], float (&vn2)[8]) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(WM_NO_ASM_JACOBI) && !defined(WM_NO_ASM_JACOBI_V)
  return jacobi_cols_v_gfx950(a, v, n2, vn2, JAC_CONV2);
#else
#pragma unroll
  for (int rp = 0; rp < 4; ++rp)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      v2f e = {(2 * rp == c) ? 1.0f : 0.0f, (2 * rp + 1 == c) ? 1.0f : 0.0f};
      v[rp][c] = e;
    }
  // A tile that has converged (one of its own sweeps saw nothing to rotate) is frozen: its lane
  // sits out (exec mask) the extra sweeps its wave neighbours need.  The fallback kernel groups
  // tiles in the (atomic, run-to-run varying) order of its work list; with the freeze a tile's
  // result does not depend on which tiles share its wave.
  int sweep = 0;
  bool more = true, active = true;
  while (more && sweep < JAC_MAX_SWEEPS) {
    if (active) {
      col_norms2_pk(a, n2);
      bool notconv = false;
#pragma unroll
      for (int p = 0; p < 7; ++p)
#pragma unroll
        for (int q = p + 1; q < 8; ++q) jacobi_rot_pk_v<1>(a, v, n2, p, q, notconv);
      active = notconv;
    }
    ++sweep;
    more = wave_any(active);
  }
  col_norms2_pk(a, n2);
  col_norms2_pk(v, vn2);
  return more ? -sweep : sweep;
#endif
}

// literal chain on a (possibly) rank-deficient tile: dct2 -> (+delta P) -> svd
// with V -> U diag(S + alpha Sw) V^T -> (-delta P) -> idct2
WM_HD int embed_tile_completed(float (&a)[8][8], const float (&sw)[8], const float (&alpha_k)[8],
                               float (&sc)[8]) {
  v2f b[4][8], v[4][8];
  float n2[8], vn2[8];
  dct8x8_to_pk(a, b);
  add_completion_pk(b, COMPLETION_DELTA);
  const int sweeps = jacobi_cols_pk_v(b, v, n2, vn2);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float nb = fsqrt(n2[i]), nv = fsqrt(vn2[i]);
    const float sig = nb * frcp(nv);                      // sigma_i = |b_i| / |v_i|
    sc[i] = sig;
    const float sp = ffma(alpha_k[i], sw[i], sig);        // S_[:K] = Sc[:K] + alpha*Sw[:K]
    const float den = nb * nv;
    const float f = (den > 0.0f) ? sp * frcp(den) : 0.0f; // sigma'_i / (|b_i| |v_i|)
#pragma unroll
    for (int rp = 0; rp < 4; ++rp) b[rp][i] = b[rp][i] * splat2(f);
  }
  // Cw = sum_i (b_i f_i) v_i^T   ==  U diag(S_) V^T ; row pair rp, column c
  v2f cw[4][8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int rp = 0; rp < 4; ++rp) {
      v2f acc = b[rp][0] * splat2(v[c >> 1][0][c & 1]);
#pragma unroll
      for (int i = 1; i < 8; ++i) acc = fma2(b[rp][i], splat2(v[c >> 1][i][c & 1]), acc);
      const v2f pt = {COMPLETION_PATTERN[2 * rp][c], COMPLETION_PATTERN[2 * rp + 1][c]};
      cw[rp][c] = fma2(splat2(-COMPLETION_DELTA), pt, acc);
    }
  idct8x8_from_pk(cw, a);
  return sweeps;
}

// ---- sigma only (extract / detect): tile -> singular values -----------------
WM_HD int sigma_tile(float (&a)[8][8], float (&s)[8]) {
  float n2[8], vn2[8];
  dct8x8(a);
  const int sweeps = jacobi_svd8<false>(a, a /*unused*/, n2, vn2);
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = fsqrt(n2[i]);
  return sweeps;
}

// ---- full SVD of a float tile (watermark side): U, S, Vt --------------------
// u[r][i], vt[i][c]; columns with sigma == 0 get u_i = 0.
WM_HD int svd_tile(float (&a)[8][8], float (&s)[8], float (&vt)[8][8], const bool complete = false) {
  v2f b[4][8], v[4][8];
  float n2[8], vn2[8];
  dct8x8_to_pk(a, b);
  if (complete) add_completion_pk(b, COMPLETION_DELTA);
  const int sweeps = jacobi_cols_pk_v(b, v, n2, vn2);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float rb = (n2[i] > 0.0f) ? frsq(n2[i]) : 0.0f;
    const float rv = frsq(vn2[i]);
    s[i] = fsqrt(n2[i]) * rv;
#pragma unroll
    for (int rp = 0; rp < 4; ++rp) {                      // U = B / |b_i|
      const v2f u = b[rp][i] * splat2(rb);
      a[2 * rp][i] = u[0];
      a[2 * rp + 1][i] = u[1];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) vt[i][c] = v[c >> 1][i][c & 1] * rv;   // Vt = (V / |v_i|)^T
  }
  return sweeps;
}

// ---- extract: Wm_hat = Uw diag(sw_hat) Vwt, then IDCT (a8 + a9) -------------
// s_cw/sc: stego and stored host singular values; inv_alpha = 1/max(alpha,1e-8);
// keep[i] = 1 for i < K else 0.  out <- idct(Uw diag(sw_hat) Vwt).
WM_HD void extract_tile(const float (&s_cw)[8], const float (&sc)[8], const float inv_alpha,
                        const float (&keep)[8], const float (&uw)[8][8],
                        const float (&vwt)[8][8], float (&out)[8][8]) {
  float sh[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) sh[i] = (s_cw[i] - sc[i]) * inv_alpha * keep[i];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    float us[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) us[i] = uw[r][i] * sh[i];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float s = us[0] * vwt[0][c];
#pragma unroll
      for (int i = 1; i < 8; ++i) s = ffma(us[i], vwt[i][c], s);
      out[r][c] = s;
    }
  }
  idct8x8(out);
}

// ---- the same with PIXEL-domain factors -------------------------------------
// idct2(Uw diag(s) Vwt) = (D^T Uw) diag(s) (Vwt D): with Ux = D^T Uw and Vxt = Vwt D
// prepared once per watermark (factors_to_pixel) the per-frame work is the rank-8 product
// alone - no IDCT - and it packs over column pairs.
WM_HD void factors_to_pixel(float (&u)[8][8], float (&vt)[8][8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c)     // Ux = D^T Uw: inverse transform along the row index
    idct8(u[0][c], u[1][c], u[2][c], u[3][c], u[4][c], u[5][c], u[6][c], u[7][c]);
#pragma unroll
  for (int i = 0; i < 8; ++i)     // Vxt = Vwt D: inverse transform along the column index
    idct8(vt[i][0], vt[i][1], vt[i][2], vt[i][3], vt[i][4], vt[i][5], vt[i][6], vt[i][7]);
}

WM_HD void extract_tile_px(const float (&s_cw)[8], const float (&sc)[8], const float inv_alpha,
                           const float (&keep)[8], const float (&ux)[8][8],
                           const float (&vxt)[8][8], float (&out)[8][8]) {
  float sh[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) sh[i] = (s_cw[i] - sc[i]) * inv_alpha * keep[i];
  v2f vs[8][4];                    // diag(sh) Vxt, packed over column pairs
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int cp = 0; cp < 4; ++cp) {
      const v2f v = {vxt[i][2 * cp], vxt[i][2 * cp + 1]};
      vs[i][cp] = v * splat2(sh[i]);
    }
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int cp = 0; cp < 4; ++cp) {
      v2f acc = splat2(ux[r][0]) * vs[0][cp];
#pragma unroll
      for (int i = 1; i < 8; ++i) acc = fma2(splat2(ux[r][i]), vs[i][cp], acc);
      out[r][2 * cp] = acc[0];
      out[r][2 * cp + 1] = acc[1];
    }
}

// ---- texture-masked strength ("Texture-masked strength") ----------
// A tile's gain is a function of its COVER singular values alone, so embed, extract and detect agree on it with no side
// information beyond the Sc every tile-mode meta already holds.  r = sqrt(s_2^2 + .. + s_8^2) is what the best rank-1 fit
// of the tile leaves over (Frobenius units over 64 pixels); g = clamp((r - lo) / (hi - lo), 0, 1), all in float32, the
// squares summed in index order by fused multiply-adds.  The embed adds alpha * G * sigma_w with G = (1, g, .., g): the leading
// component (the brightness shift every tile shares) stays uniform.  sqrtf and the division are the correctly rounded ones
// (not v_sqrt_f32 / frcp, which are good to an ulp), so this function gives the same g for the same float32 sc on host and
// device, and a tile on the edge of `cut` is carried by both or by neither.  (A restatement that sums the squares in another
// order, as NumPy does, can differ in the last bit of r.)
WM_HD float mask_gain(const float (&sc)[8], const float lo, const float hi) {
  float r2 = 0.0f;
#pragma unroll
  for (int i = 1; i < 8; ++i) r2 = ffma(sc[i], sc[i], r2);
  const float g = (sqrtf(r2) - lo) / (hi - lo);
  return fminf(fmaxf(g, 0.0f), 1.0f);
}

// a tile carries its i >= 2 values iff g >= cut (0 < cut <= 1, so a carried tile has g > 0)
WM_HD bool mask_carried(const float g, const float cut) { return g >= cut; }

// G o sigma_w: what the unchanged embed is fed for a masked tile
WM_HD void mask_sigma_w(const float g, float (&sw)[8]) {
#pragma unroll
  for (int i = 1; i < 8; ++i) sw[i] *= g;
}

// The extract's keep[] with the rule folded in: 1 for the leading value, 1 / g for the others of a carried tile, 0 for
// those of a tile that is not carried, and 0 from K on.  Returns whether the tile is carried.
WM_HD bool mask_keep(const float (&sc)[8], const float lo, const float hi, const float cut, const int K, float (&keep)[8]) {
  const float g = mask_gain(sc, lo, hi);
  const bool carried = mask_carried(g, cut);
  const float inv_g = carried ? 1.0f / g : 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) keep[i] = (i < K) ? (i == 0 ? 1.0f : inv_g) : 0.0f;
  return carried;
}

// ---- blind payload: sigma_1 quantisation ("Blind payload"; include/wmhip.h) ----------
// A tile carries one bit in the parity of its leading singular value on the lattice {k delta}: bit 0 on the even points,
// bit 1 on the odd ones.  The decoder needs delta and nothing of the cover.
// PAYLOAD_BIAS: the embed kernel clips and TRUNCATES to uint8, which takes half a gray level off each of the 64 pixels on
// average, and sigma_1 of a natural tile is close to 8 x its mean: 64 * 0.5 / 8 = 4.  The embed aims that much above the
// lattice point so that the stored tile lands on it.
constexpr float PAYLOAD_BIAS = 4.0f;
constexpr float PAYLOAD_SIGMA_MAX = 2040.0f;   // 8 * 255: sigma_1 of a white tile
constexpr float PAYLOAD_DELTA_MIN = 8.0f, PAYLOAD_DELTA_MAX = 512.0f;

WM_HD bool payload_delta_ok(const float delta) { return delta >= PAYLOAD_DELTA_MIN && delta <= PAYLOAD_DELTA_MAX; }   // (NaN fails)

// What sigma_1 of the stego tile is aimed at, q + PAYLOAD_BIAS: q the point of {2 k delta + bit * delta} nearest to s_1
// (ties to even, as rintf), one step down where the aim would lie above a white tile, then up until it leaves s_2 at least
// delta behind - sigma_1 stays the leading value (q >= s_1 - 3 delta and s_2 <= s_1: at most 2 steps; the loop allows 3).
// All in float32; the product 2 delta * k + bit * delta is ONE fused multiply-add, so host and device agree for every delta
// (for a delta with few mantissa bits - 8, 16, 24 .. - the product is exact and a separate multiply and add give the same).
// The rule's last two steps, shared with the dithered form: the cap under a white tile, then the climb above s_2 + delta
WM_HD float payload_lift(float q, const float (&s)[8], const float delta) {
  const float two_d = 2.0f * delta;
  if (q + PAYLOAD_BIAS > PAYLOAD_SIGMA_MAX) q -= two_d;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (q < s[1] + delta) q += two_d;
  return q + PAYLOAD_BIAS;
}

WM_HD float payload_target(const float (&s)[8], const int bit, const float delta) {
  const float two_d = 2.0f * delta, b = bit ? delta : 0.0f;
  return payload_lift(ffma(two_d, rintf((s[0] - b) / two_d), b), s, delta);
}

// The sigma_w row the unchanged embed is fed with alpha = 1, K = 1: (target - s_1, 0, .., 0)
WM_HD void payload_sigma_w(const float (&s)[8], const int bit, const float delta, float (&sw)[8]) {
  sw[0] = payload_target(s, bit, delta) - s[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) sw[i] = 0.0f;
}

// ---- keyed dither ("Keyed dither"; include/wmhip.h) ----------
// Every tile's lattice is shifted by a secret offset d in [0, 2 delta), from the tile's 16-bit dither word u (the caller's
// keyed table): d = float(u) * (delta * 2^-15).  The step delta * 2^-15 is exact; the product is ONE float32 multiply,
// rounded on its own - the value passes through an empty asm statement so that no compiler contracts it into the add or the
// subtraction that follows, and host, device and a NumPy restatement agree bit for bit.  u = 0 gives d = +0 and, through
// the forms below, today's results to the bit (b + 0 = b, s_1 - 0 = s_1).
WM_HD float payload_dither(const uint16_t u, const float delta) {
  float d = (float)u * (delta * (1.0f / 32768.0f));
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(d));
#elif defined(__GNUC__)
  asm("" : "+m"(d));
#endif
  return d;
}

// payload_target on the shifted lattice {2 k delta + bit * delta + d}: b' = bit * delta + d is one float32 add, the lattice
// point one fused multiply-add as above; the cap and the climb are unchanged.
WM_HD float payload_target(const float (&s)[8], const int bit, const float delta, const float d) {
  const float two_d = 2.0f * delta, b = (bit ? delta : 0.0f) + d;
  return payload_lift(ffma(two_d, rintf((s[0] - b) / two_d), b), s, delta);
}

WM_HD void payload_sigma_w(const float (&s)[8], const int bit, const float delta, const float d, float (&sw)[8]) {
  sw[0] = payload_target(s, bit, delta, d) - s[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) sw[i] = 0.0f;
}

// The decoder's soft value of a stego tile: +1 on a bit-0 lattice point, -1 on a bit-1 point, linear in between (0 half
// way).  The multiply by the float32 reciprocal of 2 delta is the one place a compiler could not change the result of: x -
// floor(x) is exact, and the doublings are exact, so 2 f - 1 and 2 |.| - 1 round the same fused or not.  The host build and a
// NumPy restatement agree bit for bit; so does the device where 1 / (2 delta) is a power of two (the default 16 among them).
// For any other delta the device compiler contracts x - floor(x) into one fused multiply-add on the unrounded product, and m
// lies within 4 * 2^-19 of the restatement's (tests/test_gpu_payload_dither.py) - far inside the sigma bar, in both forms.
WM_HD float payload_metric(const float s1, const float inv_2delta) {
  const float x = s1 * inv_2delta;
  const float f = x - floorf(x);
  return 2.0f * fabsf(2.0f * f - 1.0f) - 1.0f;
}

// Crop resynchronisation (include/wmhip.h; DESIGN.md, "Crop resynchronisation"): the metric as an integer vote, -32768 ..
// 32768.  m * 2^15 is exact in float32 and rintf rounds ties to even, as np.rint does; everything the grid search does with the
// votes - sums of |vote| per phase, per-bit sums per placement - is integer arithmetic, the same on the device and in NumPy.
WM_HD int32_t payload_vote(const float m) { return (int32_t)rintf(m * 32768.0f); }

// The same of a tile whose lattice is shifted by d: x = (s_1 - d) * (1 / (2 delta)), one subtraction and one multiply
WM_HD float payload_metric(const float s1, const float inv_2delta, const float d) {
  return payload_metric(s1 - d, inv_2delta);
}

// ---- Channel code of the blind payload (include/wmhip.h, "channel code"): rate 1/2, constraint length 7,
// generators 171 / 133 octal, zero tail.  Integers throughout, so the device kernel (k_payload_viterbi), this header's scalar
// decoder in a host build and the NumPy restatement (tests/payload_code_refs.py) give the same bits.  State s = the register's
// low 6 bits; the register that enters new state s' from predecessor p_b = (s' >> 1) | (b << 5) is r_b = s' | (b << 6).
constexpr int K7_TAIL = 6;                     // zero bits behind the frame
constexpr int K7_STATES = 64;
constexpr int K7_MAX_STEPS = 1 << 18;          // n_info + K7_TAIL: every metric then stays inside (-2^30 - 2^29, 2^29]
constexpr int32_t K7_LLR_MAX = 1024;           // |L| after the clamp on load
constexpr int32_t K7_PM_FLOOR = -(1 << 30);    // the start metric of every state but 0
constexpr unsigned K7_G0 = 0171u, K7_G1 = 0133u;

WM_HD int k7_parity(const unsigned x) { return __builtin_popcount(x) & 1; }
WM_HD int32_t k7_clamp(const int32_t L) { return L < -K7_LLR_MAX ? -K7_LLR_MAX : L > K7_LLR_MAX ? K7_LLR_MAX : L; }
// The sign of generator g's output on the b = 0 branch into new state s: +1 for a coded 0, -1 for a coded 1.  Both generators
// contain bits 0 and 6, so the b = 1 branch has the opposite sign on both outputs: bm_1 = -bm_0.
WM_HD int32_t k7_sign(const int s, const unsigned g) { return 1 - 2 * k7_parity((unsigned)s & g); }
// The b = 0 branch metric into a state with signs (g0, g1) under the step's clamped pair (L0, L1)
WM_HD int32_t k7_branch(const int32_t g0, const int32_t g1, const int32_t L0, const int32_t L1) {
  return (g0 < 0 ? -L0 : L0) + (g1 < 0 ? -L1 : L1);
}
// Add-compare-select of one state: pm0 / pm1 the metrics of its predecessors p_0 / p_1, bm the b = 0 branch metric.  b = 1 iff
// its candidate is strictly larger; ties go to b = 0.
WM_HD int32_t k7_acs(const int32_t pm0, const int32_t pm1, const int32_t bm, int& b) {
  const int32_t c0 = pm0 + bm, c1 = pm1 - bm;
  b = c1 > c0;
  return b ? c1 : c0;
}
// One traceback step from state s under decision word d: the info bit of the step is s & 1 (read before the call)
WM_HD int k7_back(const int s, const uint64_t d) { return (s >> 1) | ((int)((d >> s) & 1u) << 5); }

// The whole decoder of one codeword in scalar form: what the kernel computes, for the host harness (tests/
// payload_code_harness.cpp).  llr: 2 (n_info + 6) values; info: n_info bytes of 0 / 1; decisions: n_info + 6 words.
inline int32_t k7_decode_scalar(const int32_t* llr, const int n_info, uint8_t* info, uint64_t* decisions) {
  const int n_steps = n_info + K7_TAIL;
  int32_t pm[K7_STATES], nw[K7_STATES];
  for (int s = 0; s < K7_STATES; ++s) pm[s] = s ? K7_PM_FLOOR : 0;
  for (int t = 0; t < n_steps; ++t) {
    const int32_t L0 = k7_clamp(llr[2 * t]), L1 = k7_clamp(llr[2 * t + 1]);
    uint64_t d = 0;
    for (int s = 0; s < K7_STATES; ++s) {
      int b;
      nw[s] = k7_acs(pm[s >> 1], pm[(s >> 1) | 32], k7_branch(k7_sign(s, K7_G0), k7_sign(s, K7_G1), L0, L1), b);
      d |= (uint64_t)b << s;
    }
    for (int s = 0; s < K7_STATES; ++s) pm[s] = nw[s];
    decisions[t] = d;
  }
  int s = 0;
  for (int t = n_steps - 1; t >= 0; --t) {
    if (t < n_info) info[t] = (uint8_t)(s & 1);
    s = k7_back(s, decisions[t]);
  }
  return pm[0];
}

}  // namespace wm
