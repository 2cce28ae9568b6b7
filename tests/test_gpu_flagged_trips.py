"""The second trip of the flagged-tile walks of k_embed_fallback (csrc/wmhip.hip: `it0 += gridDim.x * WAVE` on a grid of at most
2048 waves, kinds 0, 1 and 2): more than 131 072 flagged tiles of one kind in one call.

Geometry (tests/test_loop_trips.py, which holds the shapes against the caps): planes of 2752 x 3072 = 132 096 tiles = 2064 full
waves whose tile t is palette[t % 64], with per-tile sigma_w rows laid out the same way.  Every wave of the fast kernel then
holds the same 64 tiles in the same lanes as the one wave of an 8 x 512 plane that holds the palette once, so every tile of
the large call must equal the small call's tile t % 64 - byte for byte in stego, bit for bit in sigma_c and yw - wherever the
walk picks it up (that a redone tile does not depend on its partners in the list is what
test_gpu_parity.py::test_fallback_tiles_do_not_depend_on_their_wave_partners asserts).  The calls go through
wm_embed_tiles_u8_dev on buffers of the test's own: sigma_c and yw are prefilled with NaN and stego with a tile pattern that
no expected tile equals (asserted), so a tile the walk never reached shows up on its own.

Kind 0 is reached through overflow: two planes of exactly-rank-7 tiles ask for 264 192 kind-3 entries, the sub-lists keep
64 * 260 and 247 552 tiles go to the literal chain - two trips.  A tile may then come out in its kind-3 or its kind-0 form.

Left out on purpose: the second trip of kind 3 itself (k_embed_one_small).  Its lists are clamped to 64 * fb_cap3 entries, so it
needs more than 2.1 million rank-deficient, non-rank-1 tiles in one call: over 130 MB of input, not a test of a few seconds."""
import numpy as np
import pytest

import test_loop_trips as lt

pytestmark = pytest.mark.gpu

ALPHA = 0.15
U32 = np.uint32
# what an unreached stego tile keeps: the same 8 x 8 bytes in every tile, no two rows or columns alike
PREFILL = ((np.arange(8)[:, None] * 29 + np.arange(8)[None, :] * 5 + 41) % 251).astype(np.uint8)


class _Bufs:
    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes):
        p = self.ctx.malloc(int(nbytes))
        self.ptrs.append(p)
        return p

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        self.ctx.h2d(p, arr)
        return p

    def nans(self, n_floats):
        p = self.alloc(4 * n_floats)
        self.ctx.memset(p, 0xFF, 4 * n_floats)                             # 0xFFFFFFFF: a NaN
        return p

    def close(self):
        self.ctx.sync()
        for p in reversed(self.ptrs):
            self.ctx.free(p)


def _tiles(a, n, H, W):
    """[n, H, W] -> [n * tiles, 64], tiles row-major within a plane"""
    return np.ascontiguousarray(a.reshape(n, H // 8, 8, W // 8, 8).transpose(0, 1, 3, 2, 4)).reshape(-1, 64)


def _embed(ctx, palette, shape, n=1, in_place=False):
    """wm_embed_tiles_u8_dev on n periodic planes of the palette -> per tile (stego [N, 64] uint8, sigma_c [N, 8], yw [N, 64] as
    uint32 bit patterns), N = n * tiles"""
    H, W = shape
    nt = (H // 8) * (W // 8)
    planes = np.broadcast_to(lt.periodic_plane(palette, H, W), (n, H, W))
    sw = lt.periodic_plane(lt.sigma_w_rows(), H, W)
    b = _Bufs(ctx)
    try:
        d_host, d_sw = b.put(planes), b.put(sw)
        d_stego = d_host if in_place else b.put(np.tile(PREFILL, (n, H // 8, W // 8)))
        d_sc, d_yw = b.nans(n * nt * 8), b.nans(n * H * W)
        ctx.embed_tiles_u8_dev(d_host, d_sw, d_stego, d_sc, d_yw, n, H, W, W, H * W, 0, ALPHA, 8)
        ctx.check_status()
        stego, sc, yw = np.empty((n, H, W), np.uint8), np.empty((n * nt, 8), np.float32), np.empty((n, H, W), np.float32)
        ctx.d2h(stego, d_stego); ctx.d2h(sc, d_sc); ctx.d2h(yw, d_yw)
        ctx.sync()
        ctx.check_status()
    finally:
        b.close()
    return _tiles(stego, n, H, W), sc.view(U32), _tiles(yw.view(U32), n, H, W)


def _same_as(got, want):
    """per tile: stego, sigma_c and yw all equal to the palette entry's (got [N, ..], want [64, ..]; N a multiple of 64)"""
    ok = np.ones(got[0].shape[0], bool)
    for g, w in zip(got, want):
        ok &= (g.reshape(-1, 64, g.shape[1]) == w[None]).all(axis=2).reshape(-1)
    return ok


def _no_tile_is_the_prefill(small, palette, in_place):
    assert not (small[0] == PREFILL.reshape(1, 64)).all(axis=1).any()      # an unreached stego tile cannot pass for a result
    if in_place:                                                           # ... there it keeps the host's tile instead
        assert not (small[0] == palette.reshape(64, 64)).all(axis=1).any()
    assert not np.isnan(small[1].view(np.float32)).any() and not np.isnan(small[2].view(np.float32)).any()


def _check_every_tile(ctx, palette, in_place=False):
    small = _embed(ctx, palette, lt.FLAGGED_SMALL)
    _no_tile_is_the_prefill(small, palette, in_place)
    big = _embed(ctx, palette, lt.FLAGGED_PLANE, in_place=in_place)
    assert big[0].shape[0] == 132096 > lt.FLAGGED_TRIP
    ok = _same_as(big, small)
    bad = np.flatnonzero(~ok)
    nan_sc = int(np.isnan(big[1].view(np.float32)).any(axis=1).sum())
    print(f"{bad.size} of {ok.size} tiles differ from the small call's (first {bad[:4].tolist()}, last {bad[-4:].tolist()}), "
          f"{nan_sc} tiles with the NaN prefill in sigma_c")
    assert bad.size == 0


def test_constant_tiles_black_and_grey_in_one_wave(gpu_ctx):
    """kind 1, embed_tile_constant's general form: 132 096 constant tiles, black and grey side by side"""
    _check_every_tile(gpu_ctx, lt.constant_palettes()[0])


def test_black_tiles_only(gpu_ctx):
    """kind 1, every lane black: embed_tile_constant_t<0>"""
    _check_every_tile(gpu_ctx, lt.constant_palettes()[1])


def test_constant_tiles_in_place(gpu_ctx):
    """stego aliases host: the constant tiles are read after the fast kernel has had the buffer"""
    _check_every_tile(gpu_ctx, lt.constant_palettes()[0], in_place=True)


def test_rank_1_tiles(gpu_ctx):
    """kind 2: outer products, edges of flat rectangles, equal rows and equal columns"""
    _check_every_tile(gpu_ctx, lt.rank1_palette())


def test_rank_7_tiles_overflow_into_the_literal_chain(gpu_ctx):
    """Kind 0 through overflow.  The tiles of each palette entry take at most two values: the small call's (kind 3, nothing
    overflows there) and the one a 1024 x 1024 plane of the same periodic content gives to the tiles its sub-lists sent to
    kind 0 within one trip.  Every distinct value is held to the bars of
    test_gpu_parity.py::test_one_small_singular_value_tiles_on_gpu: svd(yw) within 1e-4 sigma_1 of sort(sc + alpha sw), sigma_c
    against float64 LAPACK by (|sc - s| - 4 * 2^-14) / sigma_1 < 1e-5, stego == clip(yw) truncated, no NaN left."""
    palette = lt.rank7_palette()
    small = _embed(gpu_ctx, palette, lt.FLAGGED_SMALL)
    _no_tile_is_the_prefill(small, palette, False)
    medium = _embed(gpu_ctx, palette, lt.RANK7_MEDIUM)
    in3 = _same_as(medium, small)
    assert 0 < in3.sum() < in3.size                                        # the medium plane holds both forms
    # the kind-0 form of each entry: what the medium plane's overflowed tiles of that entry hold, all alike
    entry = np.arange(medium[0].shape[0]) % 64
    first = np.array([np.flatnonzero(~in3 & (entry == e))[0] if (~in3 & (entry == e)).any() else -1 for e in range(64)])
    assert (first >= 0).all(), "a palette entry without an overflowed tile in the medium plane"
    chain = tuple(m[first] for m in medium)
    in0 = _same_as(medium, chain)
    assert (in3 | in0).all(), f"{int((~(in3 | in0)).sum())} tiles of the medium plane hold a third value"
    forms_differ = not (in3 & in0).any()
    # the large call
    big = _embed(gpu_ctx, palette, lt.FLAGGED_PLANE, n=lt.RANK7_PLANES)
    assert big[0].shape[0] == 264192
    b3, b0 = _same_as(big, small), _same_as(big, chain)
    bad = np.flatnonzero(~(b3 | b0))
    nan_sc = int(np.isnan(big[1].view(np.float32)).any(axis=1).sum())
    print(f"{int(b3.sum())} tiles in their kind-3 form, {int((b0 & ~b3).sum())} in their kind-0 form (expected {lt.RANK7_KIND0}), "
          f"{bad.size} in neither (first {bad[:4].tolist()}, last {bad[-4:].tolist()}), {nan_sc} tiles with the NaN prefill in sigma_c")
    assert bad.size == 0
    if forms_differ:
        assert int(b0.sum()) == lt.RANK7_KIND0 and int(b3.sum()) == 264192 - lt.RANK7_KIND0
    else:
        assert int((b0 & ~b3).sum()) <= lt.RANK7_KIND0
    assert not np.isnan(big[1].view(np.float32)).any() and not np.isnan(big[2].view(np.float32)).any()
    # the (at most 128) distinct values against the existing bars
    sw = lt.sigma_w_rows().astype(np.float64)
    s_true = np.linalg.svd(palette.astype(np.float64), compute_uv=False)
    for name, (st, sc, yw) in (("kind 3", small), ("kind 0", chain)):
        sc, yw = sc.view(np.float32), yw.view(np.float32).reshape(64, 8, 8)
        got = np.linalg.svd(yw.astype(np.float64), compute_uv=False)
        want = np.sort(sc.astype(np.float64) + ALPHA * sw, axis=-1)[:, ::-1]
        e_yw = float(np.max(np.abs(got - want) / want[:, :1]))
        e_sc = float(np.max((np.abs(sc - s_true) - 4 * 2.0 ** -14) / s_true[:, :1]))
        print(f"{name}: svd(yw) off by {e_yw:.2e} sigma_1 (bar 1e-4), sigma_c off by {e_sc:.2e} sigma_1 (bar 1e-5)")
        assert np.isfinite(yw).all() and e_yw < 1e-4 and e_sc < 1e-5
        assert np.array_equal(st.reshape(64, 8, 8), np.clip(yw, 0, 255).astype(np.uint8))
