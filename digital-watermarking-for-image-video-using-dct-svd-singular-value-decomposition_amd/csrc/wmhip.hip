// libwmhip.so - gfx950 kernels + C ABI (include/wmhip.h) of the tile-mode
// DCT-SVD watermark hot path.
//
// Execution model: ONE 8x8 TILE PER LANE.  A wave64 owns 64 consecutive tiles
// (row-major tile order); every load/store instruction of a wave touches
// 64 x 8 B = 512 contiguous bytes of one image row (coalesced), and the whole
// DCT -> one-sided Jacobi SVD -> perturb -> reconstruct -> IDCT -> quantise
// chain runs out of VGPRs with compile-time register indices: no LDS round
// trips, no cross-lane shuffles, no divergence (the sweep loop is
// wave-uniform).  The path is VALU-bound (~10^4 FMA-class instructions per
// tile against 3 B per pixel); see DESIGN.md for the roofline.
//
// The sigma pass (tile load, sigma-only Jacobi stream, k_sigma_pass and its launcher) is in wm_tile_pass.h, which this unit
// shares with the blind payload's, wm_payload.hip; no kernel of that unit is compiled here.
//
//   python ../../tools/gen_jacobi_asm.py --write     (writes wm_jacobi_sigma_gfx950.inc, which is generated and not committed)
//   hipcc -O3 --offload-arch=gfx950 -shared -fPIC -o libwmhip.so wmhip.hip wm_payload.hip wm_ref.hip wm_pixel.hip \
//         wm_route.hip wm_enhance.hip wm_resample.hip                          (what build() runs; __graft_entry__.py)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>

#include "wm_internal.h"
#include "wm_tile_math.h"
#include "wm_tile_pass.h"

using namespace wmi;

namespace wmi {

thread_local char g_err[512] = "";

int set_err(int code, const char* fmt, const char* a, const char* b) {
  snprintf(g_err, sizeof(g_err), fmt, a, b);
  return code;
}

int grow(wm_ctx* ctx, void** buf, size_t* have, size_t bytes, const char* what) {
  if (bytes <= *have) return WM_OK;
  if (*buf) {
    WM_HIP(hipStreamSynchronize(ctx->stream));
    WM_HIP(hipFree(*buf));
    *buf = nullptr; *have = 0;
  }
  const size_t mb = (size_t)1 << 20;
  const size_t want = (bytes + mb - 1) / mb * mb;
  if (hipMalloc(buf, want) != hipSuccess) {
    (void)hipGetLastError();
    *buf = nullptr;
    return set_err(WM_ERR_NOMEM, "hipMalloc failed for %s", what);
  }
  *have = want;
  return WM_OK;
}

}  // namespace wmi

namespace {

constexpr int N_SUMS = 5;          // detect: sum a, b, ab, aa, bb

// The full-V form of the generated Jacobi stream (the embed's; the sigma-only form and what is said about both are in
// wm_tile_pass.h)
#if !defined(WM_NO_ASM_JACOBI)
#include "wm_jacobi_gfx950.inc"
#endif

// ---------------------------------------------------------------------------
// tile I/O (per lane), behind the loads of wm_tile_pass.h
// ---------------------------------------------------------------------------
// the store side of the one byte path (load_px4 / load_px8)
template <bool ALIGNED>
__device__ __forceinline__ void store_px4(uint8_t* __restrict__ q, const uint32_t w) {
  if (ALIGNED) { *reinterpret_cast<uint32_t*>(q) = w; return; }
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = (uint8_t)(w >> (8 * i));
}
template <bool ALIGNED>
__device__ __forceinline__ void store_px8(uint8_t* __restrict__ q, const uint32_t lo, const uint32_t hi) {
  if (ALIGNED) *reinterpret_cast<uint2*>(q) = make_uint2(lo, hi);
  else { store_px4<false>(q, lo); store_px4<false>(q + 4, hi); }
}

template <bool ALIGNED>
__device__ __forceinline__ void load_tile_u8(const uint8_t* __restrict__ p, const size_t stride, float (&a)[8][8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    uint32_t lo, hi;
    load_px8<ALIGNED>(p + r * stride, lo, hi);
    a[r][0] = (float)(lo & 0xffu); a[r][1] = (float)((lo >> 8) & 0xffu);
    a[r][2] = (float)((lo >> 16) & 0xffu); a[r][3] = (float)(lo >> 24);
    a[r][4] = (float)(hi & 0xffu); a[r][5] = (float)((hi >> 8) & 0xffu);
    a[r][6] = (float)((hi >> 16) & 0xffu); a[r][7] = (float)(hi >> 24);
  }
}

template <bool ALIGNED>
__device__ __forceinline__ void store_tile_u8(uint8_t* __restrict__ p, const size_t stride, const float (&a)[8][8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint32_t lo = wm::quant_u8(a[r][0]) | (wm::quant_u8(a[r][1]) << 8) |
                        (wm::quant_u8(a[r][2]) << 16) | (wm::quant_u8(a[r][3]) << 24);
    const uint32_t hi = wm::quant_u8(a[r][4]) | (wm::quant_u8(a[r][5]) << 8) |
                        (wm::quant_u8(a[r][6]) << 16) | (wm::quant_u8(a[r][7]) << 24);
    store_px8<ALIGNED>(p + r * stride, lo, hi);
  }
}

// one 4-pixel word per row (half a tile)
template <bool ALIGNED>
__device__ __forceinline__ void load_words(const uint8_t* __restrict__ p, const size_t stride, uint32_t (&w)[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) w[r] = load_px4<ALIGNED>(p + r * stride);
}
template <bool ALIGNED>
__device__ __forceinline__ void store_words(uint8_t* __restrict__ p, const size_t stride, const uint32_t (&w)[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) store_px4<ALIGNED>(p + r * stride, w[r]);
}

template <bool VEC>
__device__ __forceinline__ void load_row8_f32(const float* __restrict__ p, float (&row)[8]) {
  if (VEC) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    const float4 y = *reinterpret_cast<const float4*>(p + 4);
    row[0] = x.x; row[1] = x.y; row[2] = x.z; row[3] = x.w;
    row[4] = y.x; row[5] = y.y; row[6] = y.z; row[7] = y.w;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) row[i] = p[i];
  }
}

// 8x8 float matrix stored contiguously (tile-major meta arrays: 256 B per tile)
__device__ __forceinline__ void load_mat_f32(const float* __restrict__ p, float (&m)[8][8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) load_row8_f32<true>(p + r * 8, m[r]);
}
__device__ __forceinline__ void store_mat_f32(float* __restrict__ p, const float (&m)[8][8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) store_row8_f32<true>(p + r * 8, m[r]);
}

// The same pair of matrices for the 64 consecutive tiles of a tile group, staged in LDS for a workgroup whose waves all
// work on THAT group (k_extract_tiles<SH>: one wave per plane, the planes share the factors).  The group's matrices are
// one contiguous block of 16 KB per array.  load_mat_f32 reads such a block 16 B per lane at a 256 B stride - 64 cache lines
// per instruction, an eighth of each used - once per wave, and the wave then waits for it with nothing else to do.  Here
// the workgroup's threads read both blocks once, consecutive threads consecutive 16 B (an instruction covers 8 whole
// lines), and leave them in LDS at a pitch of 16 + 1 float4 per tile; every wave then picks up its lanes' own tiles with
// ds_read_b128 (the pitch is odd: the 16 lanes of a read group start on 16 different banks of 4).  The fetch is issued
// before the wave's Jacobi iteration, so its latency is spent there, and the factors cross the vector L1 once per
// workgroup, not once per wave.  `last` is the last tile of the group that exists (63, less in a plane's last group): the
// loads clamp to it, so nothing behind the arrays is read.
constexpr int SH_WAVES = 4;                                      // waves (planes) of a workgroup that shares a staged group
constexpr int STAGE_PITCH4 = 17;                                 // float4 per tile and matrix in LDS
constexpr int STAGE_MAT4 = WAVE * STAGE_PITCH4;                  // one array's block
constexpr int STAGE_LOADS = 2 * WAVE * 16 / (SH_WAVES * WAVE);   // float4 per thread: 2 blocks of 64 x 16
typedef float stage4 __attribute__((ext_vector_type(4)));       // (a native vector: arrays of it stay in registers)
// thread `tid` of the SH_WAVES * 64: its pieces of both blocks, global -> registers ...
__device__ __forceinline__ void stage_fetch(const float* __restrict__ ublk, const float* __restrict__ vblk, const int last,
                                            const int tid, stage4 (&raw)[STAGE_LOADS]) {
#pragma unroll
  for (int i = 0; i < STAGE_LOADS; ++i) {
    const int q = i * (SH_WAVES * WAVE) + tid, r = q & (WAVE * 16 - 1);      // float4 q of the 2 x 1024; r within its block
    const float* blk = (q < WAVE * 16) ? ublk : vblk;                        // (uniform per i: a block is STAGE_LOADS / 2 rounds)
    raw[i] = *reinterpret_cast<const stage4*>(blk + (size_t)min(r >> 4, last) * 64 + (r & 15) * 4);
  }
}
// ... and registers -> LDS (a __syncthreads() of the workgroup goes between this and stage_read)
__device__ __forceinline__ void stage_put(stage4* __restrict__ lds, const int tid, const stage4 (&raw)[STAGE_LOADS]) {
#pragma unroll
  for (int i = 0; i < STAGE_LOADS; ++i) {
    const int q = i * (SH_WAVES * WAVE) + tid, r = q & (WAVE * 16 - 1);
    lds[(q < WAVE * 16 ? 0 : STAGE_MAT4) + (r >> 4) * STAGE_PITCH4 + (r & 15)] = raw[i];
  }
}
// the lane's own tile's matrix out of one array's block
__device__ __forceinline__ void stage_read(const stage4* __restrict__ blk, const int lane, float (&m)[8][8]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const stage4 v = blk[lane * STAGE_PITCH4 + k];
    m[k / 2][(k & 1) * 4 + 0] = v.x; m[k / 2][(k & 1) * 4 + 1] = v.y;
    m[k / 2][(k & 1) * 4 + 2] = v.z; m[k / 2][(k & 1) * 4 + 3] = v.w;
  }
}

// Plane-fastest, XCD-aware order for kernels whose planes SHARE per-tile inputs (the frames of a
// clip share Ux / Vxt: 512 B per tile).  Workgroups are dealt round-robin over the 8 XCDs, so
// b and b + 8 share an L2 (observed placement - it only affects speed, never results).  XCD x
// walks tile groups x, x + 8, ... and, for each group, all planes back to back: the group's
// shared inputs come from HBM once and are served to the other planes by that XCD's L2, instead
// of once per plane (grid (groups, planes): 66 MB of factors re-fetched 32 times at 32 x 4K).
constexpr unsigned N_XCD = 8;
struct GroupPlane { unsigned grp; size_t plane; };
__device__ __forceinline__ GroupPlane group_plane_planefast(const unsigned n_planes) {
  const unsigned b = blockIdx.x, x = b % N_XCD, k = b / N_XCD;
  return {x + N_XCD * (k / n_planes), k % n_planes};
}
inline dim3 tile_grid_planefast(const Geom& g, int n_planes) {
  const size_t groups = ((size_t)g.n_tiles + WAVE - 1) / WAVE;
  const size_t per_xcd = (groups + N_XCD - 1) / N_XCD;
  return dim3((unsigned)(per_xcd * N_XCD * (size_t)n_planes), 1, 1);
}

// ---------------------------------------------------------------------------
// K1  fused embed   (a1 a2 a3 a4 a5 a6 a7; sigma_c side output)
// ---------------------------------------------------------------------------
// Fast path (k_embed_tiles): packed, V-free, pixel-domain (wm_tile_math.h identities (1),(2)).  Flat / rank-deficient
// tiles are left untouched there, appended to the flagged-tile lists and redone by k_embed_fallback (kinds 0-2) and
// k_embed_one_small (kind 3).
//
// The flagged-tile lists.  A flagged tile's id is plane * n_tiles + t; its kind says how it is redone:
//   0  the literal chain with orthonormal completion (wm::embed_tile_completed)
//   1  constant tiles: closed form (wm::embed_tile_constant)
//   2  rank-1 tiles that are not constant: closed form (wm::embed_tile_rank1)
//   3  every other flagged tile - one singular value out of reach or rank 2 .. 6: completed from the fast kernel's B
//      (wm::embed_tile_one_small / embed_tile_from_b), which is kept beside the id
// Each kind is split into FB_SUB sub-lists with a counter of their own, and a wave of the fast kernel appends to sub-list
// (blockIdx.x % FB_SUB), wave-aggregated: one atomic per wave and kind.  (One counter per kind serialised the whole launch
// on content made of such tiles: 16 200 same-address atomics at ~12 ns each were 189 of the fast kernel's 189 us on an
// all-flat 8 x 4K batch, HISTORY.md round 3.)  Three arrays hold them, sized by wm_embed_tiles_u8_dev:
//   fb_list  3 * FB_SUB * fb_cap + FB_SUB * fb_cap3 ids.  Sub-list s of kind k < 3 starts at (k * FB_SUB + s) * fb_cap and
//            cannot overflow: fb_cap is the tile count of all waves that map to one sub-list.  Sub-list s of kind 3 starts
//            at 3 * FB_SUB * fb_cap + s * fb_cap3.
//   fb_cnt   FB_KINDS * FB_SUB counters, FB_PAD ints (one 128-byte line) apart: sub-list s of kind k counts in
//            fb_cnt[(k * FB_SUB + s) * FB_PAD].  Zeroed before every launch.
//   fb_b     64 floats (B as 4 x 8 row pairs) per kind-3 slot: entry j of sub-list s at (s * fb_cap3 + j) * 64.
// Kind 3 is the only one that can overflow (fb_cap3 = fb_cap / 16, at least 64: B costs 256 bytes per tile).  Its counter
// still counts every tile that asked; a tile whose slot is >= fb_cap3 goes to kind 0 instead, and the readers clamp the
// count to fb_cap3.
constexpr unsigned FB_SUB = 64;    // sub-lists per kind (one per lane of the readers' scan)
constexpr unsigned FB_PAD = 32;    // ints between two sub-list counters
constexpr unsigned FB_KINDS = 4;
constexpr int EMBED_WAVES = 3;     // waves per SIMD the launch bounds of k_embed_tiles ...
constexpr int FALLBACK_WAVES = 2;  // ... and k_embed_fallback ask for

__device__ __forceinline__ size_t fb_counter(const unsigned l) { return (size_t)l * FB_PAD; }      // of sub-list l = kind * FB_SUB + s

// Writer: reserves entries of sub-list l = kind * FB_SUB + sub for the wave's flagged lanes with one atomic, then has each
// flagged lane store(l, base, rank) its tile: entry base + rank of the sub-list is that lane's.  store says whether it took
// the entry (kind 3 does not from fb_cap3 on); the result is true for the lanes whose tile is now listed.
template <typename Store>
__device__ __forceinline__ bool fb_reserve(int* __restrict__ fb_cnt, const unsigned kind, const unsigned sub, const bool flag,
                                           const Store& store) {
  const unsigned long long dmask = __builtin_amdgcn_ballot_w64(flag);
  if (dmask == 0ull) return flag;      // (false)
  const unsigned lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const unsigned leader = (unsigned)__builtin_ctzll(dmask);
  const unsigned l = kind * FB_SUB + sub;
  int base = 0;
  if (lane == leader) base = atomicAdd(fb_cnt + fb_counter(l), (int)__builtin_popcountll(dmask));
  base = __builtin_amdgcn_readlane(base, leader);
  return flag && store(l, base, (unsigned)__builtin_popcountll(dmask & ((1ull << lane) - 1ull)));
}

// Readers: one tile per lane, a fixed grid striding a kind's items (the counts are only known on the device).  The
// sub-lists' counts are scanned in the wave (lane l holds sub-list l); the sub-list that owns item `it` is found by a
// 6-step search over the lanes' prefix sums.
struct FlaggedTile {
  size_t plane;
  int t, ty, tx;
  size_t off;      // of the tile in host / stego
  size_t slot;     // of the entry within its kind (kind 3: in fb_b)
};
struct FbWalk {
  const uint32_t* __restrict__ fb_list;
  uint32_t fb_cap, fb_cap3;
  int pre[FB_KINDS], total[FB_KINDS];

  __device__ __forceinline__ FbWalk(const uint32_t* __restrict__ fb_list_, const int* __restrict__ fb_cnt,
                                    const uint32_t fb_cap_, const uint32_t fb_cap3_)
      : fb_list(fb_list_), fb_cap(fb_cap_), fb_cap3(fb_cap3_) {
    static_assert(FB_SUB == WAVE, "one sub-list per lane");
#pragma unroll
    for (int k = 0; k < (int)FB_KINDS; ++k) {
      int c = fb_cnt[fb_counter(k * FB_SUB + threadIdx.x)];
      if (k == 3) c = min(c, (int)fb_cap3);
      int incl = c;
#pragma unroll
      for (int o = 1; o < WAVE; o <<= 1) { const int v = __shfl_up(incl, o, WAVE); if ((int)threadIdx.x >= o) incl += v; }
      pre[k] = incl - c;
      total[k] = __shfl(incl, WAVE - 1, WAVE);
    }
  }
  // The lane's tile of the wave's items it0 .. it0 + 63 of kind k (it0 < total[k], wave-uniform: the shuffles need every
  // lane); false for the lanes past the last item.
  __device__ __forceinline__ bool item(const int k, const int it0, const Geom& g, FlaggedTile& tl) const {
    const int it = min(it0 + (int)threadIdx.x, total[k] - 1);
    int sub = 0;
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) { const int p = __shfl(pre[k], sub + o, WAVE); if (p <= it) sub += o; }
    const int j = it - __shfl(pre[k], sub, WAVE);
    if (it0 + (int)threadIdx.x >= total[k]) return false;
    tl.slot = (size_t)sub * (k == 3 ? fb_cap3 : fb_cap) + j;
    const uint32_t id = fb_list[(size_t)k * FB_SUB * fb_cap + tl.slot];
    tl.plane = id / (uint32_t)g.n_tiles;
    tl.t = (int)(id % (uint32_t)g.n_tiles);
    tl.ty = tl.t / g.nbx;
    tl.tx = tl.t - tl.ty * g.nbx;
    tl.off = STRIDED_TILE((size_t)0, g, tl.plane, tl.ty, tl.tx);
    return true;
  }
};

__device__ __forceinline__ void fill_alpha_k(const float alpha, const int K, float (&alpha_k)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) alpha_k[i] = (i < K) ? alpha : 0.0f;
}

// what a redone tile leaves: its Sc, its stego pixels and, with YW, the unquantised pixels
template <bool ALIGNED, bool YW>
__device__ __forceinline__ void finish_flagged(const Geom& g, const FlaggedTile& tl, float* __restrict__ sigma_c, uint8_t* stego,
                                               float* __restrict__ yw, const float (&sc)[8], const float (&a)[8][8]) {
  store_row8_f32<true>(sigma_c + (tl.plane * g.n_tiles + tl.t) * 8, sc);
  store_tile_u8<ALIGNED>(stego + tl.off, g.row_stride, a);
  if (YW) {
    float* o = DENSE_TILE(yw, g, tl.plane, tl.ty, tl.tx);
#pragma unroll
    for (int r = 0; r < 8; ++r) store_row8_f32<false>(o + (size_t)r * g.W, a[r]);
  }
}

template <bool ALIGNED, bool YW>
__device__ __forceinline__ void embed_group(
    const uint8_t* host, const float* __restrict__ sigma_w,
    uint8_t* stego, float* __restrict__ sigma_c, float* __restrict__ yw,
    const Geom& g, const size_t sw_plane_stride, const float alpha, const int K,
    int* __restrict__ status, uint32_t* __restrict__ fb_list, int* __restrict__ fb_cnt, const uint32_t fb_cap,
    float* __restrict__ fb_b, const uint32_t fb_cap3,
    const int t, const int ty, const int tx, const size_t plane) {
  const size_t off = STRIDED_TILE((size_t)0, g, plane, ty, tx);
  const unsigned fb_sub = blockIdx.x % FB_SUB;
  auto append_kind = [&](const bool flag, const unsigned kind) {
    fb_reserve(fb_cnt, kind, fb_sub, flag, [&](const unsigned l, const int base, const unsigned rank) {
      fb_list[(size_t)l * fb_cap + base + rank] = (uint32_t)(plane * g.n_tiles + t);
      return true;
    });
  };
  wm::v2f a[4][8];
  float n2[8];
  int sweeps;
  bool cst;
  int r1;
  {
    wm::RawTile raw;
    load_raw<ALIGNED>(host + off, g.row_stride, raw);
    // A wave of constant tiles only (letterbox bars, flat backgrounds) has nothing to iterate on: all of them are
    // rank-deficient and go to kind 1.  A constant tile in a mixed wave rides the iteration along and goes to the same list.
    // (the 16-word comparison only if some tile of the wave passes a two-word test: textured content pays 3 instructions)
    cst = false;
    if (__builtin_amdgcn_ballot_w64(raw.lo[0] == raw.hi[0] && raw.lo[0] == raw.hi[7]) != 0ull) cst = wm::raw_is_constant(raw);
    // rank-1 tiles that are not constant (edges of flat rectangles, rules and their crossings) are kind 2.  The exact test
    // (64 integer products) only runs if some tile of the wave passes three 2x2 minors: textured waves pay ~15 instructions.
    r1 = 0;
    if (__builtin_amdgcn_ballot_w64(!cst && wm::raw_rank1_pretest(raw)) != 0ull && !cst && wm::raw_is_rank1(raw)) r1 = 1;
    if (__builtin_amdgcn_ballot_w64(!cst && r1 == 0) == 0ull) {      // nothing in this wave needs the iteration
      append_kind(cst, 1);
      append_kind(r1 != 0, 2);
      return;
    }
#if !defined(WM_NO_ASM_JACOBI)
    // behind the LQ prelude: sweeps 1-3 run untested, the 4th is the first that can be the last (no wave of the study
    // passes the test after three, tools/skip_study.cpp lq) and already skips the pairs that are below JAC_SKIP2
    sweeps = jacobi_cols_gfx950(raw.lo, raw.hi, a, n2, wm::JAC_CONV2, wm::JAC_SKIP2, 4, 3) ? -1 : 1;
#else
    sweeps = wm::embed_jacobi_pk(raw, a, n2);
#endif
  }
  // Only B (64 VGPRs) crosses the sweep loop; everything else is (re)loaded when it is used
  // and stored as soon as it is final, so that the kernel fits 128 VGPRs (4 waves per SIMD):
  // watermark sigma -> coefficients -> Sc out; then the two 4-column halves of the tile one
  // after the other, each re-reading its row words (L2) and writing its stego words.
  asm volatile("" ::: "memory");
  float e[8];
  bool deficient;
  {
    float sw[8], sc[8], alpha_k[8];
    load_row8_f32<true>(sigma_w + plane * sw_plane_stride + (size_t)t * 8, sw);
    fill_alpha_k(alpha, K, alpha_k);
    wm::embed_coeffs_pk(n2, sw, alpha_k, e, sc, deficient);
    deficient = deficient || cst || r1 != 0;   // (constant and rank-1 tiles always are: sigma_8 = 0)
    // flagged tiles are left untouched: stego may alias host (in-place embedding) and the
    // list kernels must still read the original pixels; they also write their Sc
    if (!deficient) store_row8_f32<true>(sigma_c + (plane * g.n_tiles + t) * 8, sc);
  }
  // kind 3 takes THIS B along, so that k_embed_one_small needs no Jacobi with V; a full sub-list sends the tile to kind 0
  bool one_small = deficient && !cst && r1 == 0;
  one_small = fb_reserve(fb_cnt, 3, fb_sub, one_small, [&](const unsigned, const int base, const unsigned rank) {
    const unsigned j = (unsigned)base + rank;
    if (j >= fb_cap3) return false;
    const size_t slot = (size_t)fb_sub * fb_cap3 + j;
    fb_list[(size_t)3 * FB_SUB * fb_cap + slot] = (uint32_t)(plane * g.n_tiles + t);
    wm::v2f* dstb = reinterpret_cast<wm::v2f*>(fb_b + slot * 64);
#pragma unroll
    for (int rp = 0; rp < 4; ++rp)
#pragma unroll
      for (int c = 0; c < 8; ++c) dstb[rp * 8 + c] = a[rp][c];
    return true;
  });
  append_kind(deficient && !cst && r1 == 0 && !one_small, 0);
  append_kind(cst, 1);
  append_kind(r1 != 0, 2);
  if (sweeps < 0) atomicOr(status, 1);
  float* ywp = YW ? DENSE_TILE(yw, g, plane, ty, tx) : nullptr;
#pragma nounroll
  for (int half = 0; half < 2; ++half) {      // a real loop: one half's registers at a time
    uint32_t w[8], ow[8];
    load_words<ALIGNED>(host + off + 4 * half, g.row_stride, w);
    wm::embed_half_pk<YW>(w, a, e, ow, YW ? ywp + 4 * half : nullptr, (size_t)g.W);
    if (!deficient) store_words<ALIGNED>(stego + off + 4 * half, g.row_stride, ow);
    asm volatile("" ::: "memory");
  }
}

// One wave per workgroup and one workgroup per (tile group, plane): 64 800 workgroups per
// 32 x 4K launch.  A persistent grid (CUs x resident waves, grid-stride over the work) was
// measured 4 % SLOWER in the same process (profiles/r02_embed_variants.md): the dispatcher's
// dynamic placement balances waves that need 4 against waves that need 5 sweeps, a fixed
// stride does not.
template <bool ALIGNED, bool YW>
__global__ __launch_bounds__(WAVE, EMBED_WAVES) void k_embed_tiles(
    const uint8_t* host, const float* __restrict__ sigma_w,
    uint8_t* stego, float* __restrict__ sigma_c, float* __restrict__ yw,
    const Geom g, const unsigned n_groups, const size_t sw_plane_stride,
    const float alpha, const int K, int* __restrict__ status, uint32_t* __restrict__ fb_list, int* __restrict__ fb_cnt,
    const uint32_t fb_cap, float* __restrict__ fb_b, const uint32_t fb_cap3) {
  const unsigned w = blockIdx.x;
  const unsigned plane = w / n_groups, grp = w - plane * n_groups;
  const int t = (int)(grp * WAVE + threadIdx.x);
  if (t >= g.n_tiles) return;
  const int ty = t / g.nbx, tx = t - ty * g.nbx;
  embed_group<ALIGNED, YW>(host, sigma_w, stego, sigma_c, yw, g, sw_plane_stride, alpha, K, status, fb_list, fb_cnt, fb_cap, fb_b, fb_cap3,
                           t, ty, tx, (size_t)plane);
}

// Kinds 0, 1 and 2 of the flagged-tile lists, one walk after the other.
template <bool ALIGNED, bool YW>
__global__ __launch_bounds__(WAVE, FALLBACK_WAVES) void k_embed_fallback(
    const uint8_t* host, const float* __restrict__ sigma_w,
    uint8_t* stego, float* __restrict__ sigma_c, float* __restrict__ yw,
    const Geom g, const size_t sw_plane_stride, const float alpha, const int K,
    int* __restrict__ status, const uint32_t* __restrict__ fb_list, const int* __restrict__ fb_cnt, const uint32_t fb_cap,
    const float* __restrict__ fb_b, const uint32_t fb_cap3) {
  float alpha_k[8];
  fill_alpha_k(alpha, K, alpha_k);
  const FbWalk walk(fb_list, fb_cnt, fb_cap, fb_cap3);
  for (int it0 = blockIdx.x * WAVE; it0 < walk.total[0]; it0 += gridDim.x * WAVE) {
    FlaggedTile tl;
    float a[8][8], sw[8], sc[8];
    if (!walk.item(0, it0, g, tl)) continue;
    load_tile_u8<ALIGNED>(host + tl.off, g.row_stride, a);
    load_row8_f32<true>(sigma_w + tl.plane * sw_plane_stride + (size_t)tl.t * 8, sw);
    if (wm::embed_tile_completed(a, sw, alpha_k, sc) < 0) atomicOr(status, 1);
    finish_flagged<ALIGNED, YW>(g, tl, sigma_c, stego, yw, sc, a);
  }
  for (int it0 = blockIdx.x * WAVE; it0 < walk.total[1]; it0 += gridDim.x * WAVE) {
    FlaggedTile tl;
    float a[8][8], sw[8], sc[8];
    if (!walk.item(1, it0, g, tl)) continue;
    const float v0 = (float)host[tl.off];                    // every pixel of the tile has this value
    load_row8_f32<true>(sigma_w + tl.plane * sw_plane_stride + (size_t)tl.t * 8, sw);
    // the table is a compile-time constant when the wave's tiles are all black or none of them is (bit-identical
    // to the general form, which adds 0 * the other table)
    const unsigned long long bm = __builtin_amdgcn_ballot_w64(v0 == 0.0f);
    if (bm == 0ull) wm::embed_tile_constant_t<1>(v0, sw, alpha_k, sc, a);
    else if (bm == __builtin_amdgcn_ballot_w64(true)) wm::embed_tile_constant_t<0>(v0, sw, alpha_k, sc, a);
    else wm::embed_tile_constant(v0, sw, alpha_k, sc, a);
    finish_flagged<ALIGNED, YW>(g, tl, sigma_c, stego, yw, sc, a);
  }
  for (int it0 = blockIdx.x * WAVE; it0 < walk.total[2]; it0 += gridDim.x * WAVE) {
    FlaggedTile tl;
    float a[8][8], sw[8], sc[8];
    if (!walk.item(2, it0, g, tl)) continue;
    load_tile_u8<ALIGNED>(host + tl.off, g.row_stride, a);
    load_row8_f32<true>(sigma_w + tl.plane * sw_plane_stride + (size_t)tl.t * 8, sw);
    wm::embed_tile_rank1(a, sw, alpha_k, sc, a);
    finish_flagged<ALIGNED, YW>(g, tl, sigma_c, stego, yw, sc, a);
  }
}

// Kind 3 of the flagged-tile lists in a kernel of its own, one wave per SIMD: three 8 x 8 arrays and a float64 bilinear
// form need 314-362 registers; inside k_embed_fallback they pushed the literal chain's 202-228 VGPRs into scratch.
template <bool ALIGNED, bool YW>
__global__ __launch_bounds__(WAVE, 1) void k_embed_one_small(
    const uint8_t* host, const float* __restrict__ sigma_w,
    uint8_t* stego, float* __restrict__ sigma_c, float* __restrict__ yw,
    const Geom g, const size_t sw_plane_stride, const float alpha, const int K,
    int* __restrict__ status, const uint32_t* __restrict__ fb_list, const int* __restrict__ fb_cnt, const uint32_t fb_cap,
    const float* __restrict__ fb_b, const uint32_t fb_cap3) {
  float alpha_k[8];
  fill_alpha_k(alpha, K, alpha_k);
  const FbWalk walk(fb_list, fb_cnt, fb_cap, fb_cap3);
  for (int it0 = blockIdx.x * WAVE; it0 < walk.total[3]; it0 += gridDim.x * WAVE) {
    FlaggedTile tl;
    if (!walk.item(3, it0, g, tl)) continue;
    float a[8][8], bb[8][8], sw[8], sc[8];
    load_tile_u8<ALIGNED>(host + tl.off, g.row_stride, a);
    const wm::v2f* srcb = reinterpret_cast<const wm::v2f*>(fb_b + tl.slot * 64);
#pragma unroll
    for (int rp = 0; rp < 4; ++rp)
#pragma unroll
      for (int c = 0; c < 8; ++c) { const wm::v2f v = srcb[rp * 8 + c]; bb[2 * rp][c] = v[0]; bb[2 * rp + 1][c] = v[1]; }
    load_row8_f32<true>(sigma_w + tl.plane * sw_plane_stride + (size_t)tl.t * 8, sw);
    float n6 = 0.0f, n0 = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r) { n6 = __builtin_fmaf(bb[r][6], bb[r][6], n6); n0 = __builtin_fmaf(bb[r][0], bb[r][0], n0); }
    // one missing pair: its joint sign is defined (float64 inside); more than one: any orthonormal completion
    const bool one = n6 > wm::SIGMA_RATIO_MIN2 * n0;
    if (wm::wave_any(one)) { if (one) wm::embed_tile_one_small(a, bb, sw, alpha_k, sc, a); }
    if (wm::wave_any(!one)) { if (!one) wm::embed_tile_from_b(a, bb, sw, alpha_k, sc, a); }
    finish_flagged<ALIGNED, YW>(g, tl, sigma_c, stego, yw, sc, a);
  }
}

// copy the rows/columns no tile covers (H % 8, W % 8) from host to stego,
// and into yw as float
__global__ void k_copy_border(const uint8_t* host, uint8_t* stego,
                              float* __restrict__ yw, const int H, const int W, const int Hb,
                              const int Wb, const size_t row_stride, const size_t plane_stride) {
  const size_t plane = blockIdx.y;
  const int n_right = (W - Wb) * Hb;            // right strip: rows [0,Hb) cols [Wb,W)
  const int n_bottom = (H - Hb) * W;            // bottom strip: rows [Hb,H) all cols
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_right + n_bottom;
       i += gridDim.x * blockDim.x) {
    int r, c;
    if (i < n_right) { r = i / (W - Wb); c = Wb + i % (W - Wb); }
    else { const int j = i - n_right; r = Hb + j / W; c = j % W; }
    const size_t o = plane * plane_stride + (size_t)r * row_stride + c;
    const uint8_t px = host[o];
    if (stego != host) stego[o] = px;
    if (yw) yw[plane * (size_t)H * W + (size_t)r * W + c] = (float)px;
  }
}

// ---------------------------------------------------------------------------
// K2  sigma pass (k_sigma_pass, wm_tile_pass.h): the watermark side's epilogues
// ---------------------------------------------------------------------------
// sigma only
struct EpiSigma {
  float* __restrict__ sigma;
  __device__ __forceinline__ void operator()(const wm::RawTile&, const float (&s)[8], size_t, int, const size_t ti) const {
    store_row8_f32<true>(sigma + ti * 8, s);
  }
};

// The masked embed's gain (wm_tile_math.h, mask_gain): the tile's cover singular values -> g, and G o sigma_w of the
// tile to a dense [plane][tile][8] array that the unchanged embed launches are then fed with a per-plane stride; with
// `gain`, g itself to [plane][tile].  sigma_w may be shared by the planes (sw_plane_stride 0); without sw_eff only g is left.
// `black` (optional, [plane][tile]): 1 for a tile whose 64 pixels are 0 - see k_embed_black.
struct EpiMask {
  const float* __restrict__ sigma_w;
  float* __restrict__ sw_eff;
  float* __restrict__ gain;
  uint8_t* __restrict__ black;
  size_t sw_plane_stride;
  float lo, hi;
  __device__ __forceinline__ void operator()(const wm::RawTile& raw, const float (&s)[8], const size_t plane, const int t,
                                             const size_t ti) const {
    float sw[8];
    const float gn = wm::mask_gain(s, lo, hi);
    if (sw_eff) {
      load_row8_f32<true>(sigma_w + plane * sw_plane_stride + (size_t)t * 8, sw);
      wm::mask_sigma_w(gn, sw);
      store_row8_f32<true>(sw_eff + ti * 8, sw);
    }
    if (gain) gain[ti] = gn;
    if (black) black[ti] = (wm::raw_is_constant(raw) && raw.lo[0] == 0u) ? 1 : 0;
  }
};

// ---------------------------------------------------------------------------
// K3  full SVD of float tiles (watermark side)
// ---------------------------------------------------------------------------
template <bool VECF>
__global__ __launch_bounds__(WAVE, 2) void k_svd_tiles(const float* __restrict__ planes,
                                                   float* __restrict__ U, float* __restrict__ S,
                                                   float* __restrict__ Vt, const Geom g,
                                                   int* __restrict__ status) {
  int t, ty, tx;
  if (!tile_coords(g, t, ty, tx)) return;
  const size_t plane = blockIdx.y;
  const float* p = STRIDED_TILE(planes, g, plane, ty, tx);
  float a[8][8], s[8], vt[8][8];
#pragma unroll
  for (int r = 0; r < 8; ++r) load_row8_f32<VECF>(p + (size_t)r * g.row_stride, a[r]);
  if (wm::svd_tile(a, s, vt) < 0) atomicOr(status, 1);
  const size_t ti = plane * g.n_tiles + t;
  const bool deficient = !(s[7] > 1e-5f * s[0]);
  if (!deficient) {
    store_row8_f32<true>(S + ti * 8, s);
    store_mat_f32(U + ti * 64, a);
    store_mat_f32(Vt + ti * 64, vt);
  }
  // rank-deficient watermark tiles: redo with the completion pattern so that Uw
  // stays a full orthonormal basis (rare: wave-uniform branch, nothing kept live across it)
  if (wm::wave_any(deficient)) {
    asm volatile("" ::: "memory");
#pragma unroll
    for (int r = 0; r < 8; ++r) load_row8_f32<VECF>(p + (size_t)r * g.row_stride, a[r]);
    if (wm::svd_tile(a, s, vt, true) < 0) atomicOr(status, 1);
    if (deficient) {
      store_row8_f32<true>(S + ti * 8, s);
      store_mat_f32(U + ti * 64, a);
      store_mat_f32(Vt + ti * 64, vt);
    }
  }
}

// ---------------------------------------------------------------------------
// K2+K4  fused extract
// ---------------------------------------------------------------------------
// MM: the wave also leaves the {min, max} of its 4 096 outputs (order-preserving uint form) in mm[plane][tile group]: the
// min-max pass of the normalise that follows the unscramble (single:221) costs nothing extra then.  Lanes past the last tile
// of a partial wave recompute the last tile (every lane takes part in the reduction) and store nothing.
// MASK: the texture-masked rule (wm_tile_math.h, mask_keep) folded into keep[] - 1 / g and the carried test from the sc
// that is in registers anyway.  A template flag: the unmasked forms compile to what they were.
// SH: the planes SHARE the factors (uv_plane_stride 0, the frames of a clip).  A workgroup is then SH_WAVES waves, wave w
// taking plane SH_WAVES * slot + w of one tile group, and the group's factors reach the waves through LDS (stage_fetch ..
// stage_read above) instead of once per wave from global memory.  The walk is the plane-fastest one over the plane SLOTS.
// A wave whose plane does not exist (n_planes % SH_WAVES) helps with the fetch and leaves.  Each wave still works on the
// 64 tiles of one plane, in the same lanes: its arithmetic, the Jacobi stream's wave-wide tests included, is that of the
// one-wave form.  Without SH (one plane, or factors per plane) the workgroup is one wave and loads its own factors.
struct MaskParams { float lo, hi, cut; };
template <bool ALIGNED, bool VECF, bool PX, bool MM, bool MASK, bool SH>
__global__ __launch_bounds__(SH ? SH_WAVES * WAVE : WAVE, 3) void k_extract_tiles(
    const uint8_t* __restrict__ stego, const float* __restrict__ sigma_c,
    const float* __restrict__ Uw, const float* __restrict__ Vwt, float* __restrict__ out,
    const Geom g, const unsigned n_planes, const size_t uv_plane_stride, const float inv_alpha, const int K,
    int* __restrict__ status, unsigned* __restrict__ mm, const MaskParams mk) {
  __shared__ stage4 stage[SH ? 2 * STAGE_MAT4 : 1];
  const int lane = threadIdx.x & (WAVE - 1);
  const GroupPlane gp = group_plane_planefast(SH ? (n_planes + SH_WAVES - 1) / SH_WAVES : n_planes);
  const size_t plane = SH ? gp.plane * SH_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE) : gp.plane;
  if ((size_t)gp.grp * WAVE >= (size_t)g.n_tiles) return;                 // uniform in the workgroup: a padding group
  if (SH) {
    stage4 fetched[STAGE_LOADS];
    stage_fetch(Uw + (size_t)gp.grp * WAVE * 64, Vwt + (size_t)gp.grp * WAVE * 64,
                min((int)WAVE, g.n_tiles - (int)(gp.grp * WAVE)) - 1, threadIdx.x, fetched);
    stage_put(stage, threadIdx.x, fetched);
    __syncthreads();                                                     // the only one: the waves part here
    if (plane >= n_planes) return;
  }
  int t = (int)(gp.grp * WAVE) + lane;
  bool valid = true;
  if (MM) {
    valid = t < g.n_tiles;
    t = valid ? t : g.n_tiles - 1;
  } else if (t >= g.n_tiles) return;
  const int ty = t / g.nbx, tx = t - ty * g.nbx;
  wm::RawTile raw;
  float a[8][8], s[8], sc[8], keep[8];
  load_raw<ALIGNED>(STRIDED_TILE(stego, g, plane, ty, tx), g.row_stride, raw);
  if (sigma_tile_dev(raw, s) < 0) atomicOr(status, 1);
  load_row8_f32<true>(sigma_c + (plane * g.n_tiles + t) * 8, sc);
  if (MASK) wm::mask_keep(sc, mk.lo, mk.hi, mk.cut, K, keep);
  else {
#pragma unroll
    for (int i = 0; i < 8; ++i) keep[i] = (i < K) ? 1.0f : 0.0f;
  }
  float uw[8][8], vwt[8][8];
  if (SH) {
    stage_read(stage, lane, uw);
    stage_read(stage + STAGE_MAT4, lane, vwt);
  } else {
    const size_t mi = (plane * uv_plane_stride + (size_t)t) * 64;
    load_mat_f32(Uw + mi, uw);
    load_mat_f32(Vwt + mi, vwt);
  }
  if (PX) wm::extract_tile_px(s, sc, inv_alpha, keep, uw, vwt, a);
  else wm::extract_tile(s, sc, inv_alpha, keep, uw, vwt, a);
  float* o = DENSE_TILE(out, g, plane, ty, tx);
  if (valid) {
#pragma unroll
    for (int r = 0; r < 8; ++r) store_row8_f32<VECF>(o + (size_t)r * g.W, a[r]);
  }
  if (MM) {
    float lo = a[0][0], hi = a[0][0];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int c = 0; c < 8; ++c) { lo = fminf(lo, a[r][c]); hi = fmaxf(hi, a[r][c]); }
    unsigned ulo = f2ord(lo), uhi = f2ord(hi);
#pragma unroll
    for (int o_ = 32; o_ > 0; o_ >>= 1) { ulo = min(ulo, (unsigned)__shfl_down(ulo, o_, WAVE)); uhi = max(uhi, (unsigned)__shfl_down(uhi, o_, WAVE)); }
    if (lane == 0) {
      const size_t groups = ((size_t)g.n_tiles + WAVE - 1) / WAVE, pair = plane * groups + gp.grp;
      mm[2 * pair] = ulo; mm[2 * pair + 1] = uhi;
    }
  }
}

// out[i] = sum over planes z (ascending, deterministic) of in[z][i]: the frames of a clip carry the
// same watermark, their estimates are averaged (video extract) - on the device, so that one plane
// instead of n crosses PCIe
__global__ __launch_bounds__(256) void k_sum_planes(const float* __restrict__ in, const size_t plane_elems, const int n,
                                                   float* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < plane_elems; i += (size_t)gridDim.x * blockDim.x) {
    float acc = 0.0f;
    for (int z = 0; z < n; ++z) acc += in[(size_t)z * plane_elems + i];
    out[i] = acc;
  }
}

// per-watermark preparation for the PX extract: Ux = D^T Uw, Vxt = Vwt D (in place allowed)
__global__ __launch_bounds__(WAVE) void k_factors_to_pixel(const float* Uw, const float* Vwt, float* Ux, float* Vxt,
                                                          const size_t n_tiles) {
  const size_t t = (size_t)blockIdx.x * WAVE + threadIdx.x;
  if (t >= n_tiles) return;
  float u[8][8], vt[8][8];
  load_mat_f32(Uw + t * 64, u);
  load_mat_f32(Vwt + t * 64, vt);
  wm::factors_to_pixel(u, vt);
  store_mat_f32(Ux + t * 64, u);
  store_mat_f32(Vxt + t * 64, vt);
}

// ---------------------------------------------------------------------------
// K4  reconstruct only:  Uw diag(sw_hat) Vwt -> idct
// ---------------------------------------------------------------------------
template <bool VECF>
__global__ __launch_bounds__(WAVE, 3) void k_reconstruct_tiles(
    const float* __restrict__ Uw, const float* __restrict__ sw_hat,
    const float* __restrict__ Vwt, float* __restrict__ out, const Geom g) {
  int t, ty, tx;
  if (!tile_coords(g, t, ty, tx)) return;
  const size_t plane = blockIdx.y;
  const size_t ti = plane * g.n_tiles + t;
  float sh[8], zero[8], one[8], uw[8][8], vwt[8][8], a[8][8];
  load_row8_f32<true>(sw_hat + ti * 8, sh);
#pragma unroll
  for (int i = 0; i < 8; ++i) { zero[i] = 0.0f; one[i] = 1.0f; }
  load_mat_f32(Uw + ti * 64, uw);
  load_mat_f32(Vwt + ti * 64, vwt);
  wm::extract_tile(sh, zero, 1.0f, one, uw, vwt, a);   // (sh - 0) * 1 * 1
  float* o = DENSE_TILE(out, g, plane, ty, tx);
#pragma unroll
  for (int r = 0; r < 8; ++r) store_row8_f32<VECF>(o + (size_t)r * g.W, a[r]);
}

// ---------------------------------------------------------------------------
// K2+K5  fused detect: per-wave partial sums, then one block per plane
// ---------------------------------------------------------------------------
// MASK: the texture-masked rule - the five sums run over the leading value of every tile and the other seven of carried
// tiles only, those scaled by 1 / g (wm_tile_math.h, mask_keep with K = 8); a sixth partial counts the values taken.
template <bool ALIGNED, bool MASK>
__global__ __launch_bounds__(WAVE, 3) void k_detect_tiles(
    const uint8_t* __restrict__ stego, const float* __restrict__ sigma_c,
    const float* __restrict__ sigma_w, double* __restrict__ partials, const Geom g,
    const size_t sw_plane_stride, const float inv_alpha, int* __restrict__ status, const MaskParams mk) {
  constexpr int NS = N_SUMS + (MASK ? 1 : 0);
  int t, ty, tx;
  const size_t plane = blockIdx.y;
  double acc[NS] = {};
  if (tile_coords(g, t, ty, tx)) {
    wm::RawTile raw;
    float s[8], sc[8], sw[8];
    load_raw<ALIGNED>(STRIDED_TILE(stego, g, plane, ty, tx), g.row_stride, raw);
    if (sigma_tile_dev(raw, s) < 0) atomicOr(status, 1);
    load_row8_f32<true>(sigma_c + (plane * g.n_tiles + t) * 8, sc);
    load_row8_f32<true>(sigma_w + plane * sw_plane_stride + (size_t)t * 8, sw);
    if (MASK) {
      float keep[8];
      const bool carried = wm::mask_keep(sc, mk.lo, mk.hi, mk.cut, 8, keep);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i > 0 && !carried) continue;
        const double x = (double)sw[i];
        const double y = (double)((s[i] - sc[i]) * inv_alpha * keep[i]);
        acc[0] += x; acc[1] += y; acc[2] += x * y; acc[3] += x * x; acc[4] += y * y;
      }
      acc[N_SUMS] = carried ? 8.0 : 1.0;
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const double x = (double)sw[i];
        const double y = (double)((s[i] - sc[i]) * inv_alpha);
        acc[0] += x; acc[1] += y; acc[2] += x * y; acc[3] += x * x; acc[4] += y * y;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = wave_sum(acc[k]);
  if (threadIdx.x == 0) {
    double* o = partials + (plane * gridDim.x + blockIdx.x) * NS;
#pragma unroll
    for (int k = 0; k < NS; ++k) o[k] = acc[k];
  }
}

// MASK: the number of values comes from the sixth partial sum instead of n_vals
template <bool MASK>
__global__ __launch_bounds__(256) void k_detect_finalize(const double* __restrict__ partials,
                                                        double* __restrict__ scores,
                                                        const int n_waves, double n_vals) {
  constexpr int NS = N_SUMS + (MASK ? 1 : 0);
  __shared__ double sm[4][NS];
  const size_t plane = blockIdx.x;
  double acc[NS] = {};
  for (int w = threadIdx.x; w < n_waves; w += blockDim.x) {
    const double* p = partials + (plane * n_waves + w) * NS;
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] += p[k];
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = wave_sum(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) sm[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = sm[0][k] + sm[1][k] + sm[2][k] + sm[3][k];
    if (MASK) n_vals = s[N_SUMS];
    double score = 0.0;
    if (n_vals > 0) {
      // _nc (single:284-289): mean-removed correlation, +1e-8 in the denominator
      const double cov = s[2] - s[0] * s[1] / n_vals;
      double va = s[3] - s[0] * s[0] / n_vals;
      double vb = s[4] - s[1] * s[1] / n_vals;
      va = va > 0 ? va : 0;
      vb = vb > 0 ? vb : 0;
      score = cov / (sqrt(va) * sqrt(vb) + 1e-8);
    }
    scores[plane] = score;
  }
}

// A black cover tile is the zero matrix: it has no leading singular vector of its own, and the embed's closed form for
// constant tiles gives it those of a fixed noise pattern, half of whose pixels clip at 0 - sigma_1 of the stored tile lands
// far from what was aimed at (the payload's lattice point; the masked rule's alpha sw_1, which then reads back a third
// short).  The embeds with a derived sigma_w take the flat vector instead (what np.linalg.svd returns for a zero matrix:
// U = V = I, the DC term): the tile becomes the constant a0 sw_eff[0] / 8, a0 = alpha_k[0] (the payload: 1, and sw_eff[0]
// = q + c there, s_1 being 0; the masked embed: alpha, or 0 for K = 0).  Runs after the unchanged embed launches and
// rewrites only the tiles flagged by the sigma pass; stego and yw are addressed as the embed does.
template <bool ALIGNED>
__global__ __launch_bounds__(WAVE) void k_embed_black(uint8_t* __restrict__ stego, float* __restrict__ yw,
                                                  const float* __restrict__ sw_eff, const uint8_t* __restrict__ black,
                                                  const Geom g, const float a0) {
  int t, ty, tx;
  if (!tile_coords(g, t, ty, tx)) return;
  const size_t plane = blockIdx.y;
  const size_t i = plane * g.n_tiles + t;
  if (!black[i]) return;
  const float v = (a0 * sw_eff[i * 8]) * 0.125f;
  const uint32_t w = wm::quant_u8(v) * 0x01010101u;
  uint8_t* p = STRIDED_TILE(stego, g, plane, ty, tx);
#pragma unroll
  for (int r = 0; r < 8; ++r) store_px8<ALIGNED>(p + r * g.row_stride, w, w);
  if (yw) {
    float* o = DENSE_TILE(yw, g, plane, ty, tx);
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int c = 0; c < 8; ++c) o[(size_t)r * g.W + c] = v;
  }
}

// ---------------------------------------------------------------------------
// host-side argument checking / launch helpers (check_plane_args and embed_derived_dev: below, in wmi)
// ---------------------------------------------------------------------------
inline bool f32_vec_ok(const void* p, size_t row_stride_elems, size_t plane_stride_elems) {
  return (((uintptr_t)p) & 15u) == 0 && (row_stride_elems & 3u) == 0 && (plane_stride_elems & 3u) == 0;
}

// the texture-masked rule's parameters (include/wmhip.h): 0 <= lo < hi, both finite; 0 < cut <= 1
int check_mask(const float lo, const float hi, const float cut) {
  if (!(isfinite(lo) && isfinite(hi) && lo >= 0.0f && lo < hi)) return set_err(WM_ERR_BADARG, "mask needs finite 0 <= lo < hi");
  if (!(cut > 0.0f && cut <= 1.0f)) return set_err(WM_ERR_BADARG, "mask needs 0 < cut <= 1");
  return WM_OK;
}

// ---- host-pointer wrappers: what the embeds share (beside embed_round_trip, wm_internal.h) ----------------------
// Counts are 0 where there is no tile: the host pointer of such an array may be NULL, and nothing is copied.
size_t n_sigma_w(size_t nt, int n_planes, size_t sigma_w_plane_stride) {
  return !nt ? 0 : sigma_w_plane_stride ? (size_t)(n_planes - 1) * sigma_w_plane_stride + nt * 8 : nt * 8;
}

}  // namespace

// The two host functions that wm_payload.hip calls here (declared in wm_internal.h)
namespace wmi {

int check_plane_args(const wm_ctx* ctx, const void* p, int n_planes, int H, int W, int row_stride,
                     size_t plane_stride) {
  WM_TRY(wmi::use_ctx(ctx));
  if (n_planes < 0 || H < 0 || W < 0) return set_err(WM_ERR_BADARG, "negative size");
  if (!p && n_planes > 0 && H > 0 && W > 0) return set_err(WM_ERR_BADARG, "plane pointer is NULL");
  if (n_planes > 65535) return set_err(WM_ERR_BADARG, "n_planes > 65535");
  if (row_stride < W) return set_err(WM_ERR_BADARG, "row_stride < W");
  if (n_planes > 1 && plane_stride < (size_t)row_stride * (size_t)(H > 0 ? H - 1 : 0) + (size_t)W)
    return set_err(WM_ERR_BADARG, "plane_stride smaller than one plane");
  return WM_OK;
}

// The masked and the payload embed, behind the caller's plane and rule checks: `pass(eff, black)` enqueues the sigma pass
// that leaves a [plane][tile][8] sigma_w and the [plane][tile] black flags in the context's grow-only workspace, then the
// unchanged embed launches are fed the sigma_w with a per-plane stride and k_embed_black redoes the flagged tiles.  The
// sigma pass reads the host planes before anything writes (one stream), so stego may alias host.  `missing`: the message if
// an input that the tiles need is NULL, else nullptr.
int embed_derived_dev(wm_ctx* ctx, const uint8_t* host, uint8_t* stego, float* sigma_c, float* yw, int n_planes, int H, int W,
                      int row_stride, size_t plane_stride, float alpha, int K, const char* missing,
                      const std::function<int(float*, uint8_t*)>& pass) {
  if (!stego) return set_err(WM_ERR_BADARG, "stego is NULL");           // (before the sigma pass is enqueued)
  if (K < 0 || K > 8) return set_err(WM_ERR_BADARG, "K must be in 0..8");
  const size_t nt8 = (size_t)(H / 8) * (size_t)(W / 8) * 8;
  float* eff = nullptr;
  uint8_t* black = nullptr;
  if (n_planes > 0 && nt8 > 0) {
    if (missing) return set_err(WM_ERR_BADARG, "%s", missing);
    WM_TRY(staged(ctx, &ctx->sigma_ws, &ctx->sigma_ws_bytes, "derived sigma_w", [&](Carve& cv) {
      eff = cv.take<float>((size_t)n_planes * nt8);
      black = cv.take<uint8_t>((size_t)n_planes * (nt8 / 8));
    }));
    WM_TRY(pass(eff, black));
  }
  WM_TRY(wm_embed_tiles_u8_dev(ctx, host, eff, stego, sigma_c, yw, n_planes, H, W, row_stride, plane_stride, nt8, alpha, K));
  if (black) {
    const Geom g = make_geom(H, W, row_stride, plane_stride);
    const dim3 grid = tile_grid(g, n_planes), block(WAVE);
    with_bools([&](auto A) {
      hipLaunchKernelGGL((k_embed_black<A.value>), grid, block, 0, ctx->stream, stego, yw, (const float*)eff,
                         (const uint8_t*)black, g, K > 0 ? alpha : 0.0f);
    }, u8_aligned(host, stego, row_stride, plane_stride));
    WM_HIP(hipGetLastError());
  }
  return WM_OK;
}

}  // namespace wmi

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int wm_abi_version(void) { return WM_ABI_VERSION; }
const char* wm_last_error(void) { return wmi::g_err; }

int wm_device_count(int* n_out) {
  if (!n_out) return set_err(WM_ERR_BADARG, "n_out is NULL");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
  *n_out = n;
  return WM_OK;
}

int wm_create(int device, void* stream, wm_ctx** ctx_out) {
  if (!ctx_out) return set_err(WM_ERR_BADARG, "ctx_out is NULL");
  *ctx_out = nullptr;
  int n = 0;
  WM_HIP(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return set_err(WM_ERR_BADARG, "device index out of range");
  WM_HIP(hipSetDevice(device));
  wm_ctx* ctx = new (std::nothrow) wm_ctx();
  if (!ctx) return set_err(WM_ERR_NOMEM, "host allocation failed");
  ctx->device = device;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->n_cu = cus;
    else (void)hipGetLastError();
  }
  if (stream) {
    ctx->stream = (hipStream_t)stream;
  } else {
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete ctx; return set_err(WM_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    ctx->owns_stream = true;
  }
  hipError_t e = hipMalloc((void**)&ctx->d_status, 4 * sizeof(int));   // [0] sticky kernel status (the flagged-tile counters live behind fb_list)
  if (e == hipSuccess) e = hipMemsetAsync(ctx->d_status, 0, 4 * sizeof(int), ctx->stream);
  for (int i = 0; i < N_EVENTS && e == hipSuccess; ++i) e = hipEventCreate(&ctx->ev[i]);
  if (e != hipSuccess) { wm_destroy(ctx); return set_err(WM_ERR_HIP, "context setup: %s", hipGetErrorString(e)); }
  *ctx_out = ctx;
  return WM_OK;
}

int wm_destroy(wm_ctx* ctx) {
  if (!ctx) return WM_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (int i = 0; i < N_EVENTS; ++i) if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
  for (int i = 0; i < wm_ctx::MAX_AUX; ++i) {
    if (ctx->aux_stream[i]) { (void)hipStreamSynchronize(ctx->aux_stream[i]); (void)hipStreamDestroy(ctx->aux_stream[i]); }
    if (ctx->ev_fork[i]) (void)hipEventDestroy(ctx->ev_fork[i]);
    if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]);
  }
  if (ctx->d_status) (void)hipFree(ctx->d_status);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->partials) (void)hipFree(ctx->partials);
  if (ctx->fb_list) (void)hipFree(ctx->fb_list);
  if (ctx->ref_ws) (void)hipFree(ctx->ref_ws);
  if (ctx->ref_ws2) (void)hipFree(ctx->ref_ws2);
  if (ctx->route_tmp) (void)hipFree(ctx->route_tmp);
  if (ctx->extract_f32) (void)hipFree(ctx->extract_f32);
  if (ctx->sigma_ws) (void)hipFree(ctx->sigma_ws);
  if (ctx->resample_ws) (void)hipFree(ctx->resample_ws);
  for (int i = 0; i < wm_ctx::MAX_PAIR_TABS; ++i) if (ctx->pair_tab[i]) (void)hipFree(ctx->pair_tab[i]);
  for (int i = 0; i < wm_ctx::MAX_PAIR_TABS; ++i) {
    if (ctx->hier_dev[i]) (void)hipFree(ctx->hier_dev[i]);
    if (ctx->hier_host[i]) wmi::hier_host_free(ctx->hier_host[i]);
  }
  if (ctx->hier_ws) (void)hipFree(ctx->hier_ws);
  for (int i = 0; i < 2; ++i) if (ctx->dct_mat[i]) (void)hipFree(ctx->dct_mat[i]);
  if (ctx->enh_ws) (void)hipFree(ctx->enh_ws);
  if (ctx->enh_tab) (void)hipFree(ctx->enh_tab);
  if (ctx->owns_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return WM_OK;
}

int wm_sync(wm_ctx* ctx) {
  WM_TRY(wmi::use_ctx(ctx));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  return WM_OK;
}

int wm_check_status(wm_ctx* ctx) {
  WM_TRY(wmi::use_ctx(ctx));
  int st = 0;
  WM_HIP(hipMemcpyAsync(&st, ctx->d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  WM_HIP(hipStreamSynchronize(ctx->stream));
  if (st != 0) {
    WM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
    return set_err(WM_ERR_NOCONV, "SVD did not converge");
  }
  return WM_OK;
}

int wm_malloc(wm_ctx* ctx, size_t bytes, void** dptr_out) {
  if (!ctx || !dptr_out) return set_err(WM_ERR_BADARG, "NULL argument");
  WM_HIP(hipSetDevice(ctx->device));
  *dptr_out = nullptr;
  if (hipMalloc(dptr_out, bytes ? bytes : 1) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(WM_ERR_NOMEM, "hipMalloc failed");
  }
  return WM_OK;
}

int wm_free(wm_ctx* ctx, void* dptr) {
  WM_TRY(wmi::use_ctx(ctx));
  if (dptr) { WM_HIP(hipStreamSynchronize(ctx->stream)); WM_HIP(hipFree(dptr)); }
  return WM_OK;
}

int wm_memcpy_h2d(wm_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
  if (!ctx || (bytes && (!dst_dev || !src_host))) return set_err(WM_ERR_BADARG, "NULL argument");
  if (bytes) WM_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  return WM_OK;
}

int wm_memcpy_d2h(wm_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes) {
  if (!ctx || (bytes && (!dst_host || !src_dev))) return set_err(WM_ERR_BADARG, "NULL argument");
  if (bytes) {
    WM_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
  }
  return WM_OK;
}

int wm_memset(wm_ctx* ctx, void* dst_dev, int value, size_t bytes) {
  if (!ctx || (bytes && !dst_dev)) return set_err(WM_ERR_BADARG, "NULL argument");
  if (bytes) WM_HIP(hipMemsetAsync(dst_dev, value, bytes, ctx->stream));
  return WM_OK;
}

int wm_event_record(wm_ctx* ctx, int slot) {
  if (!ctx || slot < 0 || slot >= N_EVENTS) return set_err(WM_ERR_BADARG, "bad event slot");
  WM_HIP(hipEventRecord(ctx->ev[slot], ctx->stream));
  return WM_OK;
}

int wm_event_elapsed_ms(wm_ctx* ctx, int slot_start, int slot_stop, float* ms_out) {
  if (!ctx || !ms_out || slot_start < 0 || slot_start >= N_EVENTS || slot_stop < 0 || slot_stop >= N_EVENTS)
    return set_err(WM_ERR_BADARG, "bad event slot");
  WM_HIP(hipEventSynchronize(ctx->ev[slot_stop]));
  WM_HIP(hipEventElapsedTime(ms_out, ctx->ev[slot_start], ctx->ev[slot_stop]));
  return WM_OK;
}

// ---- K1 --------------------------------------------------------------------
int wm_embed_tiles_u8_dev(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego,
                          float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                          size_t plane_stride, size_t sigma_w_plane_stride, float alpha, int K) {
  WM_TRY(check_plane_args(ctx, host, n_planes, H, W, row_stride, plane_stride));
  if (!stego) return set_err(WM_ERR_BADARG, "stego is NULL");
  if (K < 0 || K > 8) return set_err(WM_ERR_BADARG, "K must be in 0..8");
  if (n_planes == 0 || H == 0 || W == 0) return WM_OK;
  const Geom g = make_geom(H, W, row_stride, plane_stride);
  if (g.n_tiles > 0) {
    if (!sigma_w || !sigma_c) return set_err(WM_ERR_BADARG, "sigma_w / sigma_c is NULL");
    if ((((uintptr_t)sigma_w | (uintptr_t)sigma_c) & 15u) || (sigma_w_plane_stride & 3u))
      return set_err(WM_ERR_BADARG, "sigma arrays must be 16-byte aligned");
    const bool al = u8_aligned(host, stego, row_stride, plane_stride);
    const dim3 block(WAVE);
    const unsigned n_groups = (unsigned)((g.n_tiles + WAVE - 1) / WAVE);
    const size_t n_work_sz = (size_t)n_groups * (size_t)n_planes;
    if (n_work_sz > 0x7fffffffull) return set_err(WM_ERR_BADARG, "more than 2^31 tile groups in one call");
    const dim3 grid((unsigned)n_work_sz);
    const size_t n_all = (size_t)g.n_tiles * (size_t)n_planes;
    if (n_all > 0x7fffffffull) return set_err(WM_ERR_BADARG, "more than 2^31 tiles in one call");   // ids are uint32, the device-side count an int
    const size_t n_waves = (n_all + WAVE - 1) / WAVE;
    // the flagged-tile lists (layout: above k_embed_tiles); a sub-list of kinds 0-2 holds at most the tiles of the waves that
    // map to it
    const size_t cap = (n_work_sz + FB_SUB - 1) / FB_SUB * WAVE;
    if (cap > 0x7fffffffull) return set_err(WM_ERR_BADARG, "more than 2^31 tiles in one call");
    // kind 3 keeps its tiles' B (256 bytes each): its sub-lists hold cap / 16 entries (>= 64), the rest goes to kind 0
    const size_t cap3 = std::max<size_t>(WAVE, cap / 16);
    const size_t n_cnt = (size_t)FB_KINDS * FB_SUB * FB_PAD;
    uint32_t* fb; int* fb_cnt; float* fb_b;
    WM_TRY(staged(ctx, &ctx->fb_list, &ctx->fb_bytes, "fallback lists", [&](Carve& cv) {
      fb = cv.take<uint32_t>((size_t)3 * FB_SUB * cap + (size_t)FB_SUB * cap3);
      fb_cnt = cv.take<int>(n_cnt);
      fb_b = cv.take<float>((size_t)FB_SUB * cap3 * 64);
    }));
    const uint32_t fb_cap3 = (uint32_t)cap3;
    WM_HIP(hipMemsetAsync(fb_cnt, 0, n_cnt * sizeof(int), ctx->stream));
    const uint32_t fb_cap = (uint32_t)cap;
    const dim3 fgrid((unsigned)(n_waves < 2048 ? n_waves : 2048));
    with_bools([&](auto A, auto Y) {
      hipLaunchKernelGGL((k_embed_tiles<A.value, Y.value>), grid, block, 0, ctx->stream, host, sigma_w, stego,
                         sigma_c, yw, g, n_groups, sigma_w_plane_stride, alpha, K,
                         ctx->d_status, fb, fb_cnt, fb_cap, fb_b, fb_cap3);
      hipLaunchKernelGGL((k_embed_fallback<A.value, Y.value>), fgrid, block, 0, ctx->stream, host, sigma_w,
                         stego, sigma_c, yw, g, sigma_w_plane_stride, alpha, K, ctx->d_status, fb,
                         fb_cnt, fb_cap, fb_b, fb_cap3);
      hipLaunchKernelGGL((k_embed_one_small<A.value, Y.value>), fgrid, block, 0, ctx->stream, host, sigma_w,
                         stego, sigma_c, yw, g, sigma_w_plane_stride, alpha, K, ctx->d_status, fb,
                         fb_cnt, fb_cap, fb_b, fb_cap3);
    }, al, yw != nullptr);
    WM_HIP(hipGetLastError());
  }
  const int Hb = (H / 8) * 8, Wb = (W / 8) * 8;
  if ((Hb != H || Wb != W) && (stego != host || yw)) {
    const int n = (W - Wb) * Hb + (H - Hb) * W;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)n_planes);
    hipLaunchKernelGGL(k_copy_border, grid, dim3(256), 0, ctx->stream, host, stego, yw, H, W, Hb, Wb,
                       (size_t)row_stride, plane_stride);
    WM_HIP(hipGetLastError());
  }
  return WM_OK;
}

// ---- K2 --------------------------------------------------------------------
int wm_sigma_tiles_u8_dev(wm_ctx* ctx, const uint8_t* planes, float* sigma, int n_planes, int H,
                          int W, int row_stride, size_t plane_stride) {
  WM_TRY(check_plane_args(ctx, planes, n_planes, H, W, row_stride, plane_stride));
  const char* bad = (!sigma || ((uintptr_t)sigma & 15u)) ? "sigma is NULL or not 16-byte aligned" : nullptr;
  return sigma_pass(ctx, planes, n_planes, H, W, row_stride, plane_stride, bad, EpiSigma{sigma});
}

// ---- K2 + gain, masked K1 ----------------------------------------------------
static int mask_sigma_w_dev(wm_ctx* ctx, const uint8_t* planes, const float* sigma_w, float* sigma_w_eff, float* gain,
                           uint8_t* black, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                           size_t sigma_w_plane_stride, float lo, float hi) {
  WM_TRY(check_plane_args(ctx, planes, n_planes, H, W, row_stride, plane_stride));
  WM_TRY(check_mask(lo, hi, 1.0f));
  const char* bad = (!sigma_w != !sigma_w_eff) ? "sigma_w and sigma_w_eff go together"
                    : (!sigma_w_eff && !gain) ? "neither sigma_w_eff nor gain is asked for"
                    : ((((uintptr_t)sigma_w | (uintptr_t)sigma_w_eff) & 15u) || (sigma_w_plane_stride & 3u))
                        ? "sigma_w / sigma_w_eff is not 16-byte aligned"
                    : ((uintptr_t)gain & 3u) ? "gain is not 4-byte aligned" : nullptr;
  return sigma_pass(ctx, planes, n_planes, H, W, row_stride, plane_stride, bad,
                    EpiMask{sigma_w, sigma_w_eff, gain, black, sigma_w_plane_stride, lo, hi});
}

int wm_mask_sigma_w_tiles_u8_dev(wm_ctx* ctx, const uint8_t* planes, const float* sigma_w, float* sigma_w_eff, float* gain,
                                 int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                 size_t sigma_w_plane_stride, float lo, float hi) {
  return mask_sigma_w_dev(ctx, planes, sigma_w, sigma_w_eff, gain, nullptr, n_planes, H, W, row_stride, plane_stride,
                          sigma_w_plane_stride, lo, hi);
}

// ---- K1 fed with a sigma_w derived from the cover (embed_derived_dev): the masked embed (the payload's: wm_payload.hip) ----
int wm_embed_tiles_masked_u8_dev(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego, float* sigma_c,
                                 float* yw, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                 size_t sigma_w_plane_stride, float alpha, int K, float lo, float hi) {
  WM_TRY(check_plane_args(ctx, host, n_planes, H, W, row_stride, plane_stride));
  WM_TRY(check_mask(lo, hi, 1.0f));
  return embed_derived_dev(ctx, host, stego, sigma_c, yw, n_planes, H, W, row_stride, plane_stride, alpha, K,
                           (!sigma_w || !sigma_c) ? "sigma_w / sigma_c is NULL" : nullptr, [&](float* eff, uint8_t* black) {
    return mask_sigma_w_dev(ctx, host, sigma_w, eff, nullptr, black, n_planes, H, W, row_stride, plane_stride,
                            sigma_w_plane_stride, lo, hi);
  });
}

// ---- K3 --------------------------------------------------------------------
int wm_svd_tiles_f32_dev(wm_ctx* ctx, const float* planes, float* U, float* S, float* Vt,
                         int n_planes, int H, int W, int row_stride, size_t plane_stride) {
  WM_TRY(check_plane_args(ctx, planes, n_planes, H, W, row_stride, plane_stride));
  const Geom g = make_geom(H, W, row_stride, plane_stride);
  if (n_planes == 0 || g.n_tiles == 0) return WM_OK;
  if (!U || !S || !Vt || (((uintptr_t)U | (uintptr_t)S | (uintptr_t)Vt) & 15u))
    return set_err(WM_ERR_BADARG, "U/S/Vt is NULL or not 16-byte aligned");
  const dim3 grid = tile_grid(g, n_planes), block(WAVE);
  with_bools([&](auto V) {
    hipLaunchKernelGGL((k_svd_tiles<V.value>), grid, block, 0, ctx->stream, planes, U, S, Vt, g, ctx->d_status);
  }, f32_vec_ok(planes, (size_t)row_stride, plane_stride));
  WM_HIP(hipGetLastError());
  return WM_OK;
}

// ---- K2+K4 -----------------------------------------------------------------
static int extract_tiles_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                             const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                             size_t plane_stride, size_t uv_plane_stride, float alpha, int K, bool px, unsigned* mm = nullptr,
                             const MaskParams* mask = nullptr) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  if (mask) WM_TRY(check_mask(mask->lo, mask->hi, mask->cut));
  if (!out) return set_err(WM_ERR_BADARG, "out is NULL");
  if (K < 0 || K > 8) return set_err(WM_ERR_BADARG, "K must be in 0..8");
  if (n_planes == 0 || H == 0 || W == 0) return WM_OK;
  const Geom g = make_geom(H, W, row_stride, plane_stride);
  if ((H % 8) || (W % 8))
    WM_HIP(hipMemsetAsync(out, 0, (size_t)n_planes * g.HW * sizeof(float), ctx->stream));
  if (g.n_tiles == 0) return WM_OK;
  if (!sigma_c || !Uw || !Vwt || (((uintptr_t)sigma_c | (uintptr_t)Uw | (uintptr_t)Vwt) & 15u))
    return set_err(WM_ERR_BADARG, "sigma_c/Uw/Vwt is NULL or not 16-byte aligned");
  if (uv_plane_stride != 0 && uv_plane_stride != (size_t)g.n_tiles)
    return set_err(WM_ERR_BADARG, "uv_plane_stride must be 0 (shared) or n_tiles");
  const float inv_alpha = 1.0f / fmaxf(alpha, 1e-8f);
  const bool al = u8_aligned(stego, stego, row_stride, plane_stride);
  const bool vf = f32_vec_ok(out, (size_t)W, g.HW);
  if ((((size_t)g.n_tiles + WAVE - 1) / WAVE + N_XCD) * (size_t)n_planes > 0x7fffffffull)
    return set_err(WM_ERR_BADARG, "more than 2^31 tile groups in one call");
  // planes that share their factors go SH_WAVES to a workgroup, which stages a tile group's factors once (k_extract_tiles<SH>)
  const bool sh = uv_plane_stride == 0 && n_planes >= 2;
  const dim3 grid = tile_grid_planefast(g, sh ? (n_planes + SH_WAVES - 1) / SH_WAVES : n_planes), block(sh ? SH_WAVES * WAVE : WAVE);
  const MaskParams mk = mask ? *mask : MaskParams{0.0f, 1.0f, 1.0f};
  with_bools([&](auto P, auto A, auto V, auto M, auto T, auto S) {
    hipLaunchKernelGGL((k_extract_tiles<A.value, V.value, P.value, M.value, T.value, S.value>), grid, block, 0, ctx->stream, stego,
                       sigma_c, Uw, Vwt, out, g, (unsigned)n_planes, uv_plane_stride, inv_alpha, K, ctx->d_status, mm, mk);
  }, px, al, vf, mm != nullptr, mask != nullptr, sh);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

int wm_extract_tiles_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                            const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                            size_t plane_stride, size_t uv_plane_stride, float alpha, int K) {
  return extract_tiles_dev(ctx, stego, sigma_c, Uw, Vwt, out, n_planes, H, W, row_stride, plane_stride,
                           uv_plane_stride, alpha, K, false);
}

int wm_extract_tiles_px_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Ux,
                               const float* Vxt, float* out, int n_planes, int H, int W, int row_stride,
                               size_t plane_stride, size_t uv_plane_stride, float alpha, int K) {
  return extract_tiles_dev(ctx, stego, sigma_c, Ux, Vxt, out, n_planes, H, W, row_stride, plane_stride,
                           uv_plane_stride, alpha, K, true);
}

int wm_extract_tiles_masked_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                                   const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                                   size_t plane_stride, size_t uv_plane_stride, float alpha, int K, float lo, float hi, float cut) {
  const MaskParams mk{lo, hi, cut};
  return extract_tiles_dev(ctx, stego, sigma_c, Uw, Vwt, out, n_planes, H, W, row_stride, plane_stride,
                           uv_plane_stride, alpha, K, false, nullptr, &mk);
}

int wm_extract_tiles_px_masked_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Ux,
                                      const float* Vxt, float* out, int n_planes, int H, int W, int row_stride,
                                      size_t plane_stride, size_t uv_plane_stride, float alpha, int K, float lo, float hi, float cut) {
  const MaskParams mk{lo, hi, cut};
  return extract_tiles_dev(ctx, stego, sigma_c, Ux, Vxt, out, n_planes, H, W, row_stride, plane_stride,
                           uv_plane_stride, alpha, K, true, nullptr, &mk);
}

// single:203-222 per plane in one call: sigma + rank-8 product (K2+K4) -> routed unscramble -> min-max normalise -> uint8.
// The float estimate lives in a grow-only buffer of the context; the min / max come out of the extract kernel itself.
static int extract_unscrambled_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw, const float* Vwt,
                                   const wm_route* route, uint8_t* out, int n_planes, int H, int W, int row_stride,
                                   size_t plane_stride, size_t uv_plane_stride, float alpha, int K, int px, int do_norm,
                                   const MaskParams* mask) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  if (!out || !route) return set_err(WM_ERR_BADARG, "out / route is NULL");
  if (n_planes == 0 || H == 0 || W == 0) return WM_OK;
  const size_t n = (size_t)H * W;
  const Geom g = make_geom(H, W, row_stride, plane_stride);
  const size_t groups = ((size_t)g.n_tiles + WAVE - 1) / WAVE;
  float* w; unsigned* mm;      // the estimate, then one {min, max} pair per plane and tile group (k_extract_tiles<MM> writes grp < groups only)
  WM_TRY(staged(ctx, &ctx->extract_f32, &ctx->extract_f32_bytes, "extract staging", [&](Carve& cv) {
    w = cv.take<float>((size_t)n_planes * n);
    mm = cv.take<unsigned>((size_t)n_planes * groups * 2);
  }));
  const bool use_mm = do_norm && g.n_tiles > 0;
  WM_TRY(extract_tiles_dev(ctx, stego, sigma_c, Uw, Vwt, w, n_planes, H, W, row_stride, plane_stride, uv_plane_stride, alpha, K,
                           px != 0, use_mm ? mm : nullptr, mask));
  // pixels outside the tile grid (H % 8, W % 8) are zeros of the estimate: they take part in the min / max
  return wmi::route_unpermute_normalize(ctx, w, route, out, n, n_planes, do_norm, use_mm ? mm : nullptr, (unsigned)groups,
                                        ((H % 8) || (W % 8)) ? 1 : 0);
}

int wm_extract_unscrambled_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw, const float* Vwt,
                                  const wm_route* route, uint8_t* out, int n_planes, int H, int W, int row_stride,
                                  size_t plane_stride, size_t uv_plane_stride, float alpha, int K, int px, int do_norm) {
  return extract_unscrambled_dev(ctx, stego, sigma_c, Uw, Vwt, route, out, n_planes, H, W, row_stride, plane_stride,
                                 uv_plane_stride, alpha, K, px, do_norm, nullptr);
}

int wm_extract_unscrambled_masked_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                                         const float* Vwt, const wm_route* route, uint8_t* out, int n_planes, int H, int W,
                                         int row_stride, size_t plane_stride, size_t uv_plane_stride, float alpha, int K, int px,
                                         int do_norm, float lo, float hi, float cut) {
  const MaskParams mk{lo, hi, cut};
  return extract_unscrambled_dev(ctx, stego, sigma_c, Uw, Vwt, route, out, n_planes, H, W, row_stride, plane_stride,
                                 uv_plane_stride, alpha, K, px, do_norm, &mk);
}

int wm_tile_factors_to_pixel_dev(wm_ctx* ctx, const float* Uw, const float* Vwt, float* Ux, float* Vxt,
                                 size_t n_tiles) {
  WM_TRY(wmi::use_ctx(ctx));
  if (n_tiles == 0) return WM_OK;
  if (!Uw || !Vwt || !Ux || !Vxt || (((uintptr_t)Uw | (uintptr_t)Vwt | (uintptr_t)Ux | (uintptr_t)Vxt) & 15u))
    return set_err(WM_ERR_BADARG, "factor arrays are NULL or not 16-byte aligned");
  if (n_tiles > ((size_t)1 << 31)) return set_err(WM_ERR_BADARG, "too many tiles");
  hipLaunchKernelGGL(k_factors_to_pixel, dim3((unsigned)((n_tiles + WAVE - 1) / WAVE)), dim3(WAVE), 0, ctx->stream,
                     Uw, Vwt, Ux, Vxt, n_tiles);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

// ---- K4 --------------------------------------------------------------------
int wm_reconstruct_tiles_dev(wm_ctx* ctx, const float* Uw, const float* sw_hat, const float* Vwt,
                             float* out, int n_planes, int H, int W) {
  WM_TRY(wmi::use_ctx(ctx));
  if (n_planes < 0 || H < 0 || W < 0 || n_planes > 65535) return set_err(WM_ERR_BADARG, "bad size");
  if (!out) return set_err(WM_ERR_BADARG, "out is NULL");
  if (n_planes == 0 || H == 0 || W == 0) return WM_OK;
  const Geom g = make_geom(H, W, W, (size_t)H * W);
  if ((H % 8) || (W % 8))
    WM_HIP(hipMemsetAsync(out, 0, (size_t)n_planes * g.HW * sizeof(float), ctx->stream));
  if (g.n_tiles == 0) return WM_OK;
  if (!Uw || !sw_hat || !Vwt || (((uintptr_t)Uw | (uintptr_t)sw_hat | (uintptr_t)Vwt) & 15u))
    return set_err(WM_ERR_BADARG, "Uw/sw_hat/Vwt is NULL or not 16-byte aligned");
  const dim3 grid = tile_grid(g, n_planes), block(WAVE);
  with_bools([&](auto V) {
    hipLaunchKernelGGL((k_reconstruct_tiles<V.value>), grid, block, 0, ctx->stream, Uw, sw_hat, Vwt, out, g);
  }, f32_vec_ok(out, (size_t)W, g.HW));
  WM_HIP(hipGetLastError());
  return WM_OK;
}

// ---- K2+K5 -----------------------------------------------------------------
static int detect_tiles_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c,
                            const float* sigma_w, double* scores, int n_planes, int H, int W,
                            int row_stride, size_t plane_stride, size_t sigma_w_plane_stride,
                            float alpha, const MaskParams* mask) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  if (mask) WM_TRY(check_mask(mask->lo, mask->hi, mask->cut));
  const int ns = N_SUMS + (mask ? 1 : 0);
  const MaskParams mk = mask ? *mask : MaskParams{0.0f, 1.0f, 1.0f};
  if (!scores) return set_err(WM_ERR_BADARG, "scores is NULL");
  if (n_planes == 0) return WM_OK;
  const Geom g = make_geom(H, W, row_stride, plane_stride);
  const int n_waves = (g.n_tiles + WAVE - 1) / WAVE;
  if (g.n_tiles > 0) {
    if (!sigma_c || !sigma_w || (((uintptr_t)sigma_c | (uintptr_t)sigma_w) & 15u) ||
        (sigma_w_plane_stride & 3u))
      return set_err(WM_ERR_BADARG, "sigma_c/sigma_w is NULL or not 16-byte aligned");
    WM_TRY(grow(ctx, &ctx->partials, &ctx->partials_bytes,
                (size_t)n_planes * n_waves * ns * sizeof(double), "detect partial sums"));
    const float inv_alpha = 1.0f / fmaxf(alpha, 1e-8f);
    const dim3 grid = tile_grid(g, n_planes), block(WAVE);
    with_bools([&](auto A, auto T) {
      hipLaunchKernelGGL((k_detect_tiles<A.value, T.value>), grid, block, 0, ctx->stream, stego, sigma_c, sigma_w,
                         (double*)ctx->partials, g, sigma_w_plane_stride, inv_alpha, ctx->d_status, mk);
    }, u8_aligned(stego, stego, row_stride, plane_stride), mask != nullptr);
    WM_HIP(hipGetLastError());
  }
  with_bools([&](auto T) {
    hipLaunchKernelGGL((k_detect_finalize<T.value>), dim3((unsigned)n_planes), dim3(256), 0, ctx->stream,
                       (const double*)ctx->partials, scores, n_waves, (double)g.n_tiles * 8.0);
  }, mask != nullptr && g.n_tiles > 0);
  WM_HIP(hipGetLastError());
  return WM_OK;
}

int wm_detect_tiles_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c,
                           const float* sigma_w, double* scores, int n_planes, int H, int W,
                           int row_stride, size_t plane_stride, size_t sigma_w_plane_stride,
                           float alpha) {
  return detect_tiles_dev(ctx, stego, sigma_c, sigma_w, scores, n_planes, H, W, row_stride, plane_stride,
                          sigma_w_plane_stride, alpha, nullptr);
}

int wm_detect_tiles_masked_u8_dev(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                                  double* scores, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                                  size_t sigma_w_plane_stride, float alpha, float lo, float hi, float cut) {
  const MaskParams mk{lo, hi, cut};
  return detect_tiles_dev(ctx, stego, sigma_c, sigma_w, scores, n_planes, H, W, row_stride, plane_stride,
                          sigma_w_plane_stride, alpha, &mk);
}

// ===========================================================================
// host-pointer wrappers: H2D, kernels, D2H, sync.  Convenience for callers
// without their own device allocator; the throughput path is *_dev.
// ===========================================================================

static int embed_tiles_host(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego,
                            float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                            size_t plane_stride, size_t sigma_w_plane_stride, float alpha, int K, const MaskParams* mask) {
  WM_TRY(check_plane_args(ctx, host, n_planes, H, W, row_stride, plane_stride));
  if (!stego) return set_err(WM_ERR_BADARG, "stego is NULL");
  if (n_planes == 0 || H == 0 || W == 0) return WM_OK;
  const size_t nt = (size_t)(H / 8) * (W / 8);
  if (nt > 0 && (!sigma_w || !sigma_c)) return set_err(WM_ERR_BADARG, "sigma_w / sigma_c is NULL");
  return embed_round_trip(ctx, host, sigma_w, n_sigma_w(nt, n_planes, sigma_w_plane_stride), stego, sigma_c, yw, n_planes, H, W,
                          row_stride, plane_stride, [&](uint8_t* d_host, float* d_sw, uint8_t* d_stego, float* d_sc, float* d_yw) {
    return mask ? wm_embed_tiles_masked_u8_dev(ctx, d_host, d_sw, d_stego, d_sc, d_yw, n_planes, H, W, row_stride, plane_stride,
                                               sigma_w_plane_stride, alpha, K, mask->lo, mask->hi)
                : wm_embed_tiles_u8_dev(ctx, d_host, d_sw, d_stego, d_sc, d_yw, n_planes, H, W, row_stride, plane_stride,
                                        sigma_w_plane_stride, alpha, K);
  });
}

int wm_embed_tiles_u8(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego,
                      float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                      size_t plane_stride, size_t sigma_w_plane_stride, float alpha, int K) {
  return embed_tiles_host(ctx, host, sigma_w, stego, sigma_c, yw, n_planes, H, W, row_stride, plane_stride,
                          sigma_w_plane_stride, alpha, K, nullptr);
}

int wm_embed_tiles_masked_u8(wm_ctx* ctx, const uint8_t* host, const float* sigma_w, uint8_t* stego,
                             float* sigma_c, float* yw, int n_planes, int H, int W, int row_stride,
                             size_t plane_stride, size_t sigma_w_plane_stride, float alpha, int K, float lo, float hi) {
  const MaskParams mk{lo, hi, 1.0f};
  return embed_tiles_host(ctx, host, sigma_w, stego, sigma_c, yw, n_planes, H, W, row_stride, plane_stride,
                          sigma_w_plane_stride, alpha, K, &mk);
}

int wm_mask_sigma_w_tiles_u8(wm_ctx* ctx, const uint8_t* planes, const float* sigma_w, float* sigma_w_eff, float* gain,
                             int n_planes, int H, int W, int row_stride, size_t plane_stride,
                             size_t sigma_w_plane_stride, float lo, float hi) {
  WM_TRY(check_plane_args(ctx, planes, n_planes, H, W, row_stride, plane_stride));
  const size_t nt = (size_t)(H / 8) * (W / 8);
  if (n_planes == 0 || nt == 0) return WM_OK;
  if (!sigma_w != !sigma_w_eff) return set_err(WM_ERR_BADARG, "sigma_w and sigma_w_eff go together");
  uint8_t* d_p; float *d_sw, *d_eff, *d_g;
  return staged_call(ctx, [&](Carve& cv) {
    d_p = cv.in(plane_span(n_planes, H, row_stride, plane_stride, W), planes);
    d_sw = sigma_w ? cv.in(n_sigma_w(nt, n_planes, sigma_w_plane_stride), sigma_w) : nullptr;
    d_eff = sigma_w ? cv.out((size_t)n_planes * nt * 8, sigma_w_eff) : nullptr;
    d_g = gain ? cv.out((size_t)n_planes * nt, gain) : nullptr;
  }, [&] {
    return wm_mask_sigma_w_tiles_u8_dev(ctx, d_p, d_sw, d_eff, d_g, n_planes, H, W, row_stride, plane_stride,
                                        sigma_w_plane_stride, lo, hi);
  });
}

int wm_sigma_tiles_u8(wm_ctx* ctx, const uint8_t* planes, float* sigma, int n_planes, int H, int W,
                      int row_stride, size_t plane_stride) {
  WM_TRY(check_plane_args(ctx, planes, n_planes, H, W, row_stride, plane_stride));
  const size_t nt = (size_t)(H / 8) * (W / 8);
  if (n_planes == 0 || nt == 0) return WM_OK;
  if (!sigma) return set_err(WM_ERR_BADARG, "sigma is NULL");
  uint8_t* d_p; float* d_s;
  return staged_call(ctx, [&](Carve& cv) {
    d_p = cv.in(plane_span(n_planes, H, row_stride, plane_stride, W), planes);
    d_s = cv.out((size_t)n_planes * nt * 8, sigma);
  }, [&] { return wm_sigma_tiles_u8_dev(ctx, d_p, d_s, n_planes, H, W, row_stride, plane_stride); });
}

int wm_svd_tiles_f32(wm_ctx* ctx, const float* planes, float* U, float* S, float* Vt, int n_planes,
                     int H, int W, int row_stride, size_t plane_stride) {
  WM_TRY(check_plane_args(ctx, planes, n_planes, H, W, row_stride, plane_stride));
  const size_t nt = (size_t)(H / 8) * (W / 8);
  if (n_planes == 0 || nt == 0) return WM_OK;
  if (!U || !S || !Vt) return set_err(WM_ERR_BADARG, "U/S/Vt is NULL");
  const size_t n_m = (size_t)n_planes * nt * 64;
  float *d_p, *d_U, *d_V, *d_S;
  return staged_call(ctx, [&](Carve& cv) {
    d_p = cv.in(plane_span(n_planes, H, row_stride, plane_stride, W), planes);
    d_U = cv.out(n_m, U);
    d_V = cv.out(n_m, Vt);
    d_S = cv.out((size_t)n_planes * nt * 8, S);
  }, [&] { return wm_svd_tiles_f32_dev(ctx, d_p, d_U, d_S, d_V, n_planes, H, W, row_stride, plane_stride); });
}

static int extract_tiles_host(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                              const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                              size_t plane_stride, size_t uv_plane_stride, float alpha, int K, bool sum_planes,
                              const MaskParams* mask = nullptr) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  if (!out) return set_err(WM_ERR_BADARG, "out is NULL");
  if (n_planes == 0 || H == 0 || W == 0) return WM_OK;
  const size_t nt = (size_t)(H / 8) * (W / 8);
  if (nt > 0 && (!sigma_c || !Uw || !Vwt)) return set_err(WM_ERR_BADARG, "sigma_c/Uw/Vwt is NULL");
  const size_t n_uv = (uv_plane_stride ? (size_t)n_planes : (size_t)1) * nt * 64;
  const size_t hw = (size_t)H * W, n_out = (size_t)n_planes * hw;
  uint8_t* d_p; float *d_sc, *d_U, *d_V, *d_o, *d_sum;
  return staged_call(ctx, [&](Carve& cv) {
    d_p = cv.in(plane_span(n_planes, H, row_stride, plane_stride, W), stego);
    d_sc = cv.in((size_t)n_planes * nt * 8, sigma_c);
    d_U = cv.in(n_uv, Uw);
    d_V = cv.in(n_uv, Vwt);
    d_o = cv.take<float>(n_out);
    d_sum = cv.take<float>(hw);
    if (sum_planes) cv.down(out, d_sum, hw);
    else cv.down(out, d_o, n_out);
  }, [&]() -> int {
    if (mask) WM_TRY(wm_extract_tiles_masked_u8_dev(ctx, d_p, d_sc, d_U, d_V, d_o, n_planes, H, W, row_stride, plane_stride,
                                                    uv_plane_stride, alpha, K, mask->lo, mask->hi, mask->cut));
    else WM_TRY(wm_extract_tiles_u8_dev(ctx, d_p, d_sc, d_U, d_V, d_o, n_planes, H, W, row_stride, plane_stride,
                                        uv_plane_stride, alpha, K));
    if (sum_planes) {
      const size_t g = (hw + 255) / 256;
      hipLaunchKernelGGL(k_sum_planes, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, ctx->stream, d_o, hw, n_planes, d_sum);
      WM_HIP(hipGetLastError());
    }
    return WM_OK;
  });
}

int wm_extract_tiles_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                        const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                        size_t plane_stride, size_t uv_plane_stride, float alpha, int K) {
  return extract_tiles_host(ctx, stego, sigma_c, Uw, Vwt, out, n_planes, H, W, row_stride, plane_stride,
                            uv_plane_stride, alpha, K, false);
}

int wm_extract_tiles_sum_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                            const float* Vwt, float* out_sum, int n_planes, int H, int W, int row_stride,
                            size_t plane_stride, size_t uv_plane_stride, float alpha, int K) {
  return extract_tiles_host(ctx, stego, sigma_c, Uw, Vwt, out_sum, n_planes, H, W, row_stride, plane_stride,
                            uv_plane_stride, alpha, K, true);
}

int wm_extract_tiles_masked_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                               const float* Vwt, float* out, int n_planes, int H, int W, int row_stride,
                               size_t plane_stride, size_t uv_plane_stride, float alpha, int K, float lo, float hi, float cut) {
  const MaskParams mk{lo, hi, cut};
  return extract_tiles_host(ctx, stego, sigma_c, Uw, Vwt, out, n_planes, H, W, row_stride, plane_stride,
                            uv_plane_stride, alpha, K, false, &mk);
}

int wm_extract_tiles_sum_masked_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* Uw,
                                   const float* Vwt, float* out_sum, int n_planes, int H, int W, int row_stride,
                                   size_t plane_stride, size_t uv_plane_stride, float alpha, int K, float lo, float hi, float cut) {
  const MaskParams mk{lo, hi, cut};
  return extract_tiles_host(ctx, stego, sigma_c, Uw, Vwt, out_sum, n_planes, H, W, row_stride, plane_stride,
                            uv_plane_stride, alpha, K, true, &mk);
}

int wm_reconstruct_tiles(wm_ctx* ctx, const float* Uw, const float* sw_hat, const float* Vwt,
                         float* out, int n_planes, int H, int W) {
  WM_TRY(wmi::use_ctx(ctx));
  if (n_planes < 0 || H < 0 || W < 0) return set_err(WM_ERR_BADARG, "negative size");
  if (!out) return set_err(WM_ERR_BADARG, "out is NULL");
  if (n_planes == 0 || H == 0 || W == 0) return WM_OK;
  const size_t nt = (size_t)(H / 8) * (W / 8);
  if (nt > 0 && (!Uw || !sw_hat || !Vwt)) return set_err(WM_ERR_BADARG, "Uw/sw_hat/Vwt is NULL");
  const size_t n_m = (size_t)n_planes * nt * 64;
  float *d_U, *d_V, *d_s, *d_o;
  return staged_call(ctx, [&](Carve& cv) {
    d_U = cv.in(n_m, Uw);
    d_V = cv.in(n_m, Vwt);
    d_s = cv.in((size_t)n_planes * nt * 8, sw_hat);
    d_o = cv.out((size_t)n_planes * H * W, out);
  }, [&] { return wm_reconstruct_tiles_dev(ctx, d_U, d_s, d_V, d_o, n_planes, H, W); }, /* sync_only: no SVD, no status */ true);
}

static int detect_tiles_host(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                             double* scores, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                             size_t sigma_w_plane_stride, float alpha, const MaskParams* mask) {
  WM_TRY(check_plane_args(ctx, stego, n_planes, H, W, row_stride, plane_stride));
  if (!scores) return set_err(WM_ERR_BADARG, "scores is NULL");
  if (n_planes == 0) return WM_OK;
  const size_t nt = (size_t)(H / 8) * (W / 8);
  if (nt > 0 && (!sigma_c || !sigma_w)) return set_err(WM_ERR_BADARG, "sigma_c/sigma_w is NULL");
  const size_t span = plane_span(n_planes, H, row_stride, plane_stride, W);
  uint8_t* d_p; float *d_sc, *d_sw; double* d_scores;
  return staged_call(ctx, [&](Carve& cv) {
    d_p = cv.take<uint8_t>(span ? span : 1);      // (planes without a sample still get a pointer the _dev form accepts)
    cv.up(d_p, stego, span);
    d_sc = cv.in((size_t)n_planes * nt * 8, sigma_c);
    d_sw = cv.in(n_sigma_w(nt, n_planes, sigma_w_plane_stride), sigma_w);
    d_scores = cv.out((size_t)n_planes, scores);
  }, [&] {
    return mask ? wm_detect_tiles_masked_u8_dev(ctx, d_p, d_sc, d_sw, d_scores, n_planes, H, W, row_stride, plane_stride,
                                                sigma_w_plane_stride, alpha, mask->lo, mask->hi, mask->cut)
                : wm_detect_tiles_u8_dev(ctx, d_p, d_sc, d_sw, d_scores, n_planes, H, W, row_stride, plane_stride,
                                         sigma_w_plane_stride, alpha);
  });
}

int wm_detect_tiles_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                       double* scores, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                       size_t sigma_w_plane_stride, float alpha) {
  return detect_tiles_host(ctx, stego, sigma_c, sigma_w, scores, n_planes, H, W, row_stride, plane_stride,
                           sigma_w_plane_stride, alpha, nullptr);
}

int wm_detect_tiles_masked_u8(wm_ctx* ctx, const uint8_t* stego, const float* sigma_c, const float* sigma_w,
                              double* scores, int n_planes, int H, int W, int row_stride, size_t plane_stride,
                              size_t sigma_w_plane_stride, float alpha, float lo, float hi, float cut) {
  const MaskParams mk{lo, hi, cut};
  return detect_tiles_host(ctx, stego, sigma_c, sigma_w, scores, n_planes, H, W, row_stride, plane_stride,
                           sigma_w_plane_stride, alpha, &mk);
}

}  // extern "C"
