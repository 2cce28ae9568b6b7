"""GPU: the route kernels (csrc/wm_route.hip), the fused min / max of the one-call extract, and the normalise, squared-
difference and SSIM kernels of csrc/wm_pixel.hip at their edges, against the plain references of tests/pixel_refs.py.

Routes run permutations a uniform shuffle never produces (cells of 0, 1, S and n mod S elements), odd plane sizes on
several planes (plane bases at odd byte offsets), offset pointers through the C ABI, the block limit and the index-pass
fallback above it, and a long-lived context whose route cache and staging rotate.  Bytes and floats equal NumPy's.
The one-call extract is held to NumPy on the device's own float estimate, with estimates whose only other extremum is the
zero border of a ragged plane.  Normalise is exact against oracle.normalize_minmax; wm_sqdiff_u8_dev is an exact integer;
SSIM is compared with a float64 restatement on flat, saturated and two-level content, where float32 moments are weakest."""
import ctypes as C

import numpy as np
import pytest

import pixel_refs as pr
from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

S = pr.S
vp = C.c_void_p
GUARD = 32
FILL = 0xA5


class _Buf:
    """device bytes at `off` bytes past a 16-byte aligned address, between two guard zones that must keep their fill"""

    def __init__(self, c, nbytes, off=0):
        self.c, self.nbytes, self.off = c, nbytes, off
        self.total = nbytes + off + 2 * GUARD
        self.base = c.malloc(self.total)
        assert self.base % 16 == 0
        c.memset(self.base, FILL, self.total)
        self.p = self.base + GUARD + off

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == self.nbytes
        self.c.h2d(self.p, arr)
        return self

    def get(self, dtype):
        raw = np.empty(self.total, np.uint8)
        self.c.d2h(raw, self.base)
        lo = GUARD + self.off
        assert (raw[:lo] == FILL).all() and (raw[lo + self.nbytes:] == FILL).all(), "written outside the buffer"
        return raw[lo:lo + self.nbytes].copy().view(dtype)

    def free(self):
        self.c.free(self.base)


def _planes(rng, n_pl, n):
    """float planes of different offset and scale (every plane has its own min / max), values on both sides of 0..255"""
    x = rng.normal(20, 80, (n_pl, n)) * rng.uniform(0.2, 3, (n_pl, 1)) + rng.uniform(-40, 40, (n_pl, 1))
    return x.astype(np.float32)


def _want_unscrambled(x, idx, norm):
    return np.stack([pr.normalize_u8(pr.unscramble(x[z], idx), norm) for z in range(x.shape[0])])


def _want_scrambled(g, idx):
    return np.stack([pr.scramble(g[z], idx) for z in range(g.shape[0])])


# ---- 1. routes against NumPy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pr.ROUTE_SIZES)
def test_routes_of_non_uniform_permutations_equal_numpy(gpu_ctx, n):
    """flat[idx] and inv[idx] = arange; flat[inv] for every builder of pixel_refs at this size, do_norm 0 and 1, on 1, 2
    and 3 planes.  With odd n the planes after the first start at odd byte offsets (uint8) and 4-byte-only aligned
    addresses (float): the unaligned arms of k_route_p2, k_route_ga and k_minmax_planes on multi-block planes."""
    c = gpu_ctx
    rng = np.random.default_rng(n)
    for name, idx in pr.permutations_for(n):
        assert c.route_dev(idx) is not None
        for n_pl in (1, 2, 3):
            x = _planes(rng, n_pl, n)
            for norm in (True, False):
                got = c.unpermute_normalize_u8(x.reshape(n_pl, 1, n), idx, norm).reshape(n_pl, n)
                assert np.array_equal(got, _want_unscrambled(x, idx, norm)), (name, n_pl, norm)
            g = rng.integers(0, 256, (n_pl, n), dtype=np.uint8)
            got = c.permute_planes(g.reshape(n_pl, 1, n), idx).reshape(n_pl, n)
            assert got.dtype == np.float32 and np.array_equal(got, _want_scrambled(g, idx)), (name, n_pl)


@pytest.mark.parametrize("n", [3 * S + 5, 2 * S + 16, 17])
def test_routes_with_offset_pointers_through_the_c_abi(gpu_ctx, n):
    """src and dst 1 to 15 bytes (uint8) and 4, 8, 12 bytes (float) past their allocation's 16-byte alignment, two planes;
    the guard zones either side of the destination keep their fill"""
    c = gpu_ctx
    rng = np.random.default_rng(n + 1)
    perms = pr.permutations_for(n)
    n_pl = 2
    for k, off8 in enumerate(range(1, 16)):
        offf = (4, 8, 12)[k % 3]
        name, idx = perms[k % len(perms)]
        route = c.route_dev(idx)
        x = _planes(rng, n_pl, n)
        g = rng.integers(0, 256, (n_pl, n), dtype=np.uint8)
        src = _Buf(c, x.nbytes, offf).put(x); dst = _Buf(c, n_pl * n, off8)
        s8 = _Buf(c, g.nbytes, off8).put(g); df = _Buf(c, n_pl * n * 4, offf)
        try:
            norm = k % 2
            c._call("wm_unpermute_normalize_u8_dev", vp(src.p), vp(route), vp(dst.p), n, n_pl, norm)
            assert np.array_equal(dst.get(np.uint8).reshape(n_pl, n), _want_unscrambled(x, idx, norm)), (name, off8, offf)
            c._call("wm_permute_u8_f32_routed_dev", vp(s8.p), vp(route), vp(df.p), n, n_pl)
            assert np.array_equal(df.get(np.float32).reshape(n_pl, n), _want_scrambled(g, idx)), (name, off8, offf)
        finally:
            for b in (src, dst, s8, df):
                b.free()


def test_route_block_limit_and_the_index_pass_above_it(hostapi):
    """n = 2048 * S (2^26) is the largest plane a route takes: it is created and both directions equal NumPy.  One element
    more: wm_route_create_dev refuses, route_dev is None, and the host wrappers still equal NumPy through the index pass."""
    n = hostapi.Context.ROUTE_MAX_N
    assert n == 2048 * S == 1 << 26
    rng = np.random.default_rng(26)
    idx = rng.permutation(n)
    with hostapi.Context(0) as c:
        assert c.route_dev(idx) is not None
        x = rng.normal(30, 70, n).astype(np.float32)
        got = c.unpermute_normalize_u8(x.reshape(2048, S), idx, True)
        assert np.array_equal(got.ravel(), pr.normalize_u8(pr.unscramble(x, idx)))
        g = rng.integers(0, 256, n, dtype=np.uint8)
        got = c.permute_planes(g.reshape(2048, S), idx)
        assert np.array_equal(got.ravel(), pr.scramble(g, idx))
    # n + 1: the new element trades places with element 0
    idx1 = np.append(idx, n)
    idx1[0], idx1[n] = idx1[n], idx1[0]
    del idx
    x = np.append(x, np.float32(-55.5)); g = np.append(g, np.uint8(201))
    with hostapi.Context(0) as c:
        r = vp()
        with pytest.raises(ValueError, match="too large for a route"):
            c._call("wm_route_create_dev", vp(c.index_dev(idx1)), n + 1, C.byref(r))
        assert not r.value
        assert c.route_dev(idx1) is None
        got = c.unpermute_normalize_u8(x.reshape(1, n + 1), idx1, True)
        assert np.array_equal(got.ravel(), pr.normalize_u8(pr.unscramble(x, idx1)))
        got = c.permute_planes(g.reshape(1, n + 1), idx1)
        assert np.array_equal(got.ravel(), pr.scramble(g, idx1))


def test_route_bad_arguments(gpu_ctx):
    c = gpu_ctx
    n = S + 1
    idx = pr.perm_rotation(n, 1)
    route = c.route_dev(idx)
    other = c.route_dev(pr.perm_rotation(n + 1, 1))
    x = _planes(np.random.default_rng(0), 1, n)
    src = _Buf(c, x.nbytes).put(x); dst = _Buf(c, n); s8 = _Buf(c, n).put(np.zeros(n, np.uint8)); df = _Buf(c, 4 * n)
    try:
        for r in (other, None):                                                  # a route of another size; a NULL route
            with pytest.raises(ValueError):
                c._call("wm_unpermute_normalize_u8_dev", vp(src.p), vp(r), vp(dst.p), n, 1, 1)
            with pytest.raises(ValueError):
                c._call("wm_permute_u8_f32_routed_dev", vp(s8.p), vp(r), vp(df.p), n, 1)
        c._call("wm_unpermute_normalize_u8_dev", vp(src.p), vp(route), vp(dst.p), n, 0, 1)      # no planes: OK, nothing written
        c._call("wm_permute_u8_f32_routed_dev", vp(s8.p), vp(route), vp(df.p), n, 0)
        assert (dst.get(np.uint8) == FILL).all() and (df.get(np.uint8) == FILL).all()
        c._call("wm_unpermute_normalize_u8_dev", vp(src.p), vp(route), vp(dst.p), n, 1, 0)      # and the context still works
        assert np.array_equal(dst.get(np.uint8), _want_unscrambled(x, idx, False)[0])
    finally:
        for b in (src, dst, s8, df):
            b.free()


def _extract_inputs(c, rng, H, W, n_pl):
    stego = rng.integers(0, 256, (n_pl, H, W), dtype=np.uint8)
    U, _, Vt = c.svd_tiles(rng.integers(0, 256, (H, W)).astype(np.float32))
    sc = (c.sigma_tiles(stego) * rng.uniform(0.9, 1.0, (n_pl, H // 8, W // 8, 8))).astype(np.float32)
    return stego, sc, U, Vt


def test_route_cache_rotation_and_staging_reuse(gpu_ctx, hostapi):
    """Indices A, B, C taken in the order A B C A B on one context: its two-entry index / route cache evicts, destroys the
    route and rebuilds it; plane sizes go small, large, small, so the grow-only route and extract staging grows and is
    reused; routed permute, routed unpermute and the one-call extract interleave.  Every result equals a fresh context's."""
    rng = np.random.default_rng(41)
    cases = {"A": (40, 56, 3, pr.perm_multiply(40 * 56)),
             "B": (360, 641, 1, rng.permutation(360 * 641)),
             "C": (129, 255, 2, pr.perm_fill_last_block(129 * 255))}
    data = {}
    for key, (H, W, n_pl, idx) in cases.items():
        data[key] = (_planes(rng, n_pl, H * W).reshape(n_pl, H, W), rng.integers(0, 256, (n_pl, H, W), dtype=np.uint8),
                     _extract_inputs(gpu_ctx, rng, H, W, n_pl))

    def run(ctx, key, step):
        H, W, n_pl, idx = cases[key]
        x, g, (stego, sc, U, Vt) = data[key]
        ops = [lambda: ctx.permute_planes(g, idx), lambda: ctx.unpermute_normalize_u8(x, idx, True),
               lambda: ctx.extract_tiles_unscrambled_u8(stego, sc, U, Vt, 0.15, 8, idx, True),
               lambda: ctx.unpermute_normalize_u8(x, idx, False)]
        return [ops[(step + j) % 4]() for j in range(4)]           # the same calls in a different order at every step

    for step, key in enumerate("ABCAB"):
        got = run(gpu_ctx, key, step)
        with hostapi.Context(0) as fresh:
            want = run(fresh, key, step)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), (step, key)
        H, W, n_pl, idx = cases[key]                               # ... and both are NumPy's
        x, g, _ = data[key]
        mine = dict(zip([(step + j) % 4 for j in range(4)], got))
        assert np.array_equal(mine[0].reshape(n_pl, -1), _want_scrambled(g.reshape(n_pl, -1), idx))
        assert np.array_equal(mine[1].reshape(n_pl, -1), _want_unscrambled(x.reshape(n_pl, -1), idx, True))


# ---- 2. the one-call extract against a host reference ----------------------------------------------------------------
EXTRACT_GEOMETRIES = [
    (8, 8, 1), (8, 9, 1), (15, 15, 2), (7, 40, 1), (40, 7, 2),               # one tile; one tile and a border; no tile
    (56, 72, 1), (64, 64, 1), (40, 104, 1),                                  # 63, 64, 65 tiles on full planes ...
    (59, 75, 2), (66, 67, 1), (43, 105, 3),                                  # ... and on ragged ones
    (200, 328, 3), (203, 331, 3),                                            # 1025 tiles: 17 wave groups per plane, 3 planes
]


@pytest.mark.parametrize("geom", EXTRACT_GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}x{g[2]}")
def test_one_call_extract_equals_numpy_on_the_devices_own_estimate(gpu_ctx, geom):
    """wm_extract_unscrambled_u8_dev against NumPy on the float estimate the device itself computed
    (wm_extract_tiles[_px]_u8_dev): unscramble, normalize_minmax in float32, clip, truncate - the route, the min / max
    fused into k_extract_tiles and the normalise with no tolerance; the SVD's rounding is on both sides.

    Single-entry factors with sigma_c = sigma / 2 and K = 1 make every tile one constant of the factor's sign, so on a
    ragged plane 0 - the border outside the tile grid - is the minimum (or the maximum) and nothing else supplies it.  On
    flat stego planes all tiles carry the same constant v: the grid comes out 255 and the border 0 (negative sign: grid 0,
    border 255) - up to the last byte, because float32 v * float32(255 / v) may round just below 255 (then the reference
    itself says 254; the test checks what the reference says before it relies on it)."""
    H, W, n_pl = geom
    c = gpu_ctx
    n = H * W; nby, nbx = H // 8, W // 8; nt = nby * nbx
    ragged = bool(H % 8 or W % 8)
    rng = np.random.default_rng(n)
    idx = rng.permutation(n) if n % 2 else pr.perm_multiply(n)
    route = c.route_dev(idx)
    m = pr.grid_mask(H, W).ravel()
    flat = np.stack([np.full((H, W), v, np.uint8) for v in (200, 64, 131)[:n_pl]])
    d_w = c.malloc(n_pl * n * 4); d_b = c.malloc(n_pl * n)
    d_u = c.malloc(max(nt, 1) * 256); d_v = c.malloc(max(nt, 1) * 256); d_ux = c.malloc(max(nt, 1) * 256); d_vx = c.malloc(max(nt, 1) * 256)
    d_st = c.malloc(n_pl * n); d_sc = c.malloc(max(n_pl * nt, 1) * 32)
    exact_255 = 0
    try:
        for kind, stego in (("flat", flat), ("noise", rng.integers(1, 256, (n_pl, H, W), dtype=np.uint8))):
            c.h2d(d_st, stego)
            if nt:
                sigma = c.sigma_tiles(stego)
                assert (sigma[..., 0] > 0).all()
                c.h2d(d_sc, (0.5 * sigma).astype(np.float32))
            for sign in (1.0, -1.0):
                if nt:
                    U, V = pr.single_entry_factors(nby, nbx, sign)
                    c.h2d(d_u, U); c.h2d(d_v, V)
                    c.tile_factors_to_pixel_dev(d_u, d_v, d_ux, d_vx, nt)
                for px in (0, 1):
                    fu, fv = (d_ux, d_vx) if px else (d_u, d_v)
                    (c.extract_tiles_px_u8_dev if px else c.extract_tiles_u8_dev)(d_st, d_sc, fu, fv, d_w, n_pl, H, W, W, n, 0, 0.15, 1)
                    w = np.empty((n_pl, n), np.float32); c.d2h(w, d_w)
                    assert not w[:, ~m].any()
                    assert (np.sign(w[:, m]) == sign).all()                       # 0 is an extremum only through the border
                    for norm in (1, 0):
                        c.memset(d_b, FILL, n_pl * n)
                        c._call("wm_extract_unscrambled_u8_dev", vp(d_st), vp(d_sc), vp(fu), vp(fv), vp(route), vp(d_b), n_pl, H, W, W, n, 0,
                                0.15, 1, px, norm)
                        got = np.empty((n_pl, n), np.uint8); c.d2h(got, d_b)
                        want = _want_unscrambled(w, idx, bool(norm))
                        assert np.array_equal(got, want), (kind, sign, px, norm)
                        if not (norm and ragged):
                            continue
                        back = want[:, idx]                                       # the normalised bytes in the estimate's own layout
                        if nt == 0:
                            assert not back.any()
                            continue
                        tiles, border = back[:, m], back[:, ~m]                   # the reference itself, before it is relied on:
                        if sign > 0:                                              # the zero border is the minimum ...
                            assert not border.any() and (tiles.max(axis=1) >= 254).all(), (kind, sign, px)
                        else:                                                     # ... or the maximum
                            assert (border >= 254).all() and (tiles.min(axis=1) == 0).all(), (kind, sign, px)
                        if kind == "flat":                                        # one value on the grid: 255 (or a rounding below) / 0
                            hi = tiles if sign > 0 else border
                            assert (tiles >= 254).all() if sign > 0 else not tiles.any()
                            assert all(np.unique(p).size == 1 for p in hi)
                            exact_255 += int((hi == 255).all(axis=1).sum())
                            assert np.array_equal(got[:, idx], back)
            c.check_status()
        if nt == 0:
            assert not got.any()
    finally:
        for d in (d_w, d_b, d_u, d_v, d_ux, d_vx, d_st, d_sc):
            c.free(d)
    print(f"extract {H}x{W}x{n_pl}: flat planes whose reference pattern is exactly 255 / 0: {exact_255}")


# ---- 3. normalise, exact ----------------------------------------------------------------------------------------------
NORM_LENGTHS = list(range(1, 10)) + [1023, 1024, 1025, 4 * 256 * 513 + 3, 2160 * 3840]


def _extreme_positions(n):
    """where a lost element shows: first, last, the tail after the last float4, the first and last elements of the last
    min-max partial block (k_minmax launches min(512, ceil((n / 4 + 1) / 256)) blocks of 256 float4 lanes)"""
    n_part = min(512, (n // 4 + 1 + 255) // 256)
    cand = {0, n - 1, n // 2, (n // 4) * 4, (n // 4) * 4 - 1, 4 * 256 * (n_part - 1), 4 * 256 * (n_part - 1) + 1023, 4 * 256 * n_part - 1}
    return sorted(p for p in cand if 0 <= p < n)


@pytest.mark.parametrize("n", NORM_LENGTHS)
def test_normalise_is_exact_at_every_length(gpu_ctx, n):
    """gpu_ctx.normalize_u8 and the routed form equal uint8(clip(oracle.normalize_minmax(x), 0, 255)) byte for byte:
    NormQ is the reference's arithmetic (the scale through float64, the rest float32, nothing an FMA could contract).
    The minimum and the maximum sit, in turn, at every position where a tail or a fold of the partial pairs could lose
    them.  Finite input only: what cv2.normalize does with NaN / Inf is not part of this contract."""
    c = gpu_ctx
    rng = np.random.default_rng(n)
    base = rng.normal(40, 90, n).astype(np.float32)
    pos = _extreme_positions(n)
    idx = pr.perm_identity(n) if n < 10 else (pr.perm_multiply(n) if n < 100000 else rng.permutation(n))
    for k, p_hi in enumerate(pos):
        x = base.copy()
        p_lo = pos[(k + 1) % len(pos)]
        x[p_lo] = -1234.5
        x[p_hi] = 2345.25                                       # p_hi == p_lo for n = 1: range 0
        want = pr.normalize_u8(x)
        assert np.array_equal(c.normalize_u8(x, True), want), (n, p_hi, p_lo)
        if k < 3 or n < 2000:
            got = c.unpermute_normalize_u8(x[idx].reshape(1, n), idx, True).ravel()      # unscramble(scramble(x)) = x
            assert np.array_equal(got, want), (n, p_hi, p_lo)
    assert np.array_equal(c.normalize_u8(base, True), pr.normalize_u8(base))
    assert np.array_equal(c.normalize_u8(base, False), pr.normalize_u8(base, False))


NORM_VALUES = {
    "all-negative": [-900.0, -3.25, -17.0, -3.25001, -899.9],
    "all-equal": [7.5] * 6,
    "signed-zeros": [-0.0, 0.0, 0.0, -0.0],
    "range-below-epsilon": [0.0, 2.0e-16, 1.0e-16],
    "range-above-epsilon": [0.0, 2.5e-16, 1.0e-16, 2.4e-16],
    "range-at-epsilon": [-1.0e-16, 1.3e-16, 0.0],
    "denormal-range": [0.0, 1.0e-40, 5.0e-41, -1.0e-42],
    "denormal-minimum": [1.0e-40, 1.0, 0.5, 3.0e-39],
    "huge": [-1.0e30, 1.0e30, 0.0, 3.3e29, -9.9e29, 2.0 ** 100, -2.0 ** 100],
    "overflowing-range": [-3.0e38, 3.0e38],
    "overflowing-range-with-middle": [-3.0e38, 3.0e38, 0.0, 1.0e38, -2.9e38],
}


@pytest.mark.parametrize("name", list(NORM_VALUES))
def test_normalise_is_exact_on_edge_values(gpu_ctx, name):
    """the same equality on ranges where the arithmetic is at its limits; (-3e38, 3e38): the float32 subtraction
    overflows to inf and the reference's own arithmetic gives 255 there.  Non-finite INPUT is out of scope."""
    c = gpu_ctx
    vals = np.array(NORM_VALUES[name], np.float32)
    assert np.isfinite(vals).all()
    rng = np.random.default_rng(len(name))
    for n in (len(vals), 7, 1024, 5000):
        if n < len(vals):
            continue
        x = np.resize(vals, n)
        if n > len(vals):                                       # the same min and max, the rest spread between them
            lo, hi = float(vals.min()), float(vals.max())
            mid = (lo / 2 + hi / 2) + rng.uniform(-0.5, 0.5, n) * (hi / 2 - lo / 2) * 2 * 0.999
            x = mid.astype(np.float32); x[: len(vals)] = vals
            x = rng.permutation(x)
            assert x.min() == vals.min() and x.max() == vals.max()
        want = pr.normalize_u8(x)
        assert np.array_equal(c.normalize_u8(x, True), want), (name, n)
        idx = pr.perm_reversal(n)
        assert np.array_equal(c.unpermute_normalize_u8(x.reshape(1, n), idx, True).ravel(), want[::-1]), (name, n)
    if name.startswith("overflowing"):
        assert c.normalize_u8(vals[:2], True).tolist() == [0, 255]


def test_normalise_dev_output_offsets_and_input_alignment(gpu_ctx):
    """wm_normalize_u8_dev with `out` 1, 2 and 3 bytes past a 4-byte boundary (the scalar arm of k_normalize_u8: no packed
    stores), and its refusal of a float plane that is not 16-byte aligned"""
    c = gpu_ctx
    rng = np.random.default_rng(5)
    for n in (1, 5, 1027, 70001):
        x = rng.normal(100, 120, n).astype(np.float32)
        x[n - 1] = 900.0; x[0] = min(x[0], -300.0)
        src = _Buf(c, x.nbytes).put(x)
        try:
            for off in (0, 1, 2, 3):
                for norm in (1, 0):
                    dst = _Buf(c, n, off)
                    c._call("wm_normalize_u8_dev", vp(src.p), n, norm, vp(dst.p))
                    got = dst.get(np.uint8); dst.free()
                    assert np.array_equal(got, pr.normalize_u8(x, bool(norm))), (n, off, norm)
        finally:
            src.free()
    src = _Buf(c, 4 * 64 + 16).put(np.zeros(68, np.float32)); dst = _Buf(c, 64)
    try:
        with pytest.raises(ValueError, match="16-byte aligned"):
            c._call("wm_normalize_u8_dev", vp(src.p + 4), 64, 1, vp(dst.p))
        assert (dst.get(np.uint8) == FILL).all()
    finally:
        src.free(); dst.free()


# ---- 4. squared differences, exact ----------------------------------------------------------------------------------
def _ssd_dev(c, d_a, d_b, n, d_out):
    c.memset(d_out, FILL, 8)
    c._call("wm_sqdiff_u8_dev", vp(d_a), vp(d_b), n, vp(d_out))
    v = np.zeros(1, np.uint64); c.d2h(v, d_out)
    return int(v[0])


SQDIFF_LENGTHS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 16 * 256 * 2048 + 16 * 3 + 5]     # the last: past grid_for's cap of 2048 blocks


@pytest.mark.parametrize("n", SQDIFF_LENGTHS)
def test_sqdiff_is_an_exact_integer(gpu_ctx, n):
    """wm_sqdiff_u8_dev against NumPy in int64, equal as integers: random pairs, and one differing byte (difference 255)
    placed first, last, in the tail behind the last 16-byte group, and at either end of the last 16-byte group"""
    c = gpu_ctx
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, n, dtype=np.uint8); b = rng.integers(0, 256, n, dtype=np.uint8)
    d_a = c.malloc(n + 16); d_b = c.malloc(n + 16); d_o = c.malloc(8)
    try:
        if n:
            c.h2d(d_a, a); c.h2d(d_b, b)
        want = int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
        assert _ssd_dev(c, d_a, d_b, n, d_o) == want
        assert _ssd_dev(c, d_b, d_a, n, d_o) == want
        if n:
            assert _ssd_dev(c, d_a, d_a, n, d_o) == 0
        n16 = n // 16 * 16
        for p in sorted(q for q in {0, n - 1, n16, n16 - 1, n16 - 16, n16 + (n % 16) // 2} if 0 <= q < n):
            b1 = a.copy(); b1[p] = 0 if a[p] > 127 else 255
            c.h2d(d_b, b1)
            d = int(a[p]) - int(b1[p])
            assert _ssd_dev(c, d_a, d_b, n, d_o) == d * d, (n, p)
    finally:
        c.free(d_a); c.free(d_b); c.free(d_o)


def test_sqdiff_past_32_bits_and_psnr_extremes(gpu_ctx):
    """all 0 against all 255 at 2160 x 3840 x 3: 1.6e12, past 2^32; psnr on that pair and on ONE differing LSB in an 8K plane"""
    c = gpu_ctx
    n = 2160 * 3840 * 3
    zeros = np.zeros(n, np.uint8); white = np.full(n, 255, np.uint8)
    d_a = c.malloc(n); d_b = c.malloc(n); d_o = c.malloc(8)
    try:
        c.h2d(d_a, zeros); c.h2d(d_b, white)
        assert n * 65025 > 1 << 32
        assert _ssd_dev(c, d_a, d_b, n, d_o) == n * 65025
        white[n - 1] = 254; c.h2d(d_b, white)
        assert _ssd_dev(c, d_a, d_b, n, d_o) == (n - 1) * 65025 + 254 * 254
        white[n - 1] = 255
        for bad_a, bad_b in ((1, 0), (0, 1), (8, 0), (0, 15)):                   # unaligned a, unaligned b
            with pytest.raises(ValueError, match="16-byte aligned"):
                c._call("wm_sqdiff_u8_dev", vp(d_a + bad_a), vp(d_b + bad_b), 1024, vp(d_o))
    finally:
        c.free(d_a); c.free(d_b); c.free(d_o)
    z3 = zeros.reshape(2160, 3840, 3); w3 = white.reshape(2160, 3840, 3)
    assert abs(c.psnr(z3, w3) - o.psnr(z3, w3)) < 1e-4
    assert abs(c.psnr(z3, w3)) < 1e-4                                            # mse = 255^2: 0 dB
    a = np.random.default_rng(8).integers(0, 256, (4320, 7680), dtype=np.uint8)
    b = a.copy(); b[4319, 7679] ^= 1
    assert abs(c.psnr(a, b) - o.psnr(a, b)) < 1e-4
    b = a.copy(); b[0, 0] ^= 1
    assert abs(c.psnr(a, b) - o.psnr(a, b)) < 1e-4
    assert c.psnr(a, a) == 99.0


# ---- 5. SSIM where float32 moments are weakest ------------------------------------------------------------------------
SSIM_BAR = 3e-5          # the project's bar (test_gpu_pixel.py); the float32 oracle is within 4e-6 of the float64 form on these inputs


def test_ssim_on_flat_saturated_and_two_level_content(gpu_ctx):
    """k_ssim against the float64 restatement of single:44-57 on content where x^2 + y^2 is near 1.3e5 and the variances
    near 0: white backgrounds, two levels, LSB flips, noise of sigma 0.3 on flat levels - every uint8 / float32
    combination the kernel instantiates"""
    for name, a, b in pr.ssim_pairs(200, 300):
        want = pr.ssim64(a, b)
        for x, y in pr.dtype_combinations(a, b):
            for p, q in ((x, y), (y, x)):
                got = gpu_ctx.ssim(p, q)
                print(f"ssim {name} {p.dtype}/{q.dtype}: got {got:.9f} want {want:.9f} diff {got - want:+.2e}")
                assert abs(got - want) < SSIM_BAR, (name, p.dtype, q.dtype, got, want)


@pytest.mark.parametrize("shape", [(1080, 1920), (2160, 3840)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ssim_on_large_flat_content(gpu_ctx, shape):
    for name, a, b in pr.ssim_large_pairs(*shape):
        want = pr.ssim64(a, b)
        for x, y in pr.dtype_combinations(a, b):
            got = gpu_ctx.ssim(x, y)
            print(f"ssim {shape} {name} {x.dtype}/{y.dtype}: got {got:.9f} want {want:.9f} diff {got - want:+.2e}")
            assert abs(got - want) < SSIM_BAR, (shape, name, x.dtype, y.dtype, got, want)


def _ssim_dev(c, p1, s1, p2, s2, H, W, kind, d_out):
    c._call("wm_ssim_dev", vp(p1), s1, vp(p2), s2, H, W, kind, vp(d_out))
    v = np.zeros(1); c.d2h(v, d_out)
    return float(v[0])


def test_ssim_windows_of_larger_planes(gpu_ctx):
    """wm_ssim_dev on windows: origin at column 3 of a larger uint8 plane (a base pointer that is not 4-byte aligned), two
    different row strides, a float32 window with a stride larger than W - flat bright content and random content"""
    c = gpu_ctx
    rng = np.random.default_rng(31)
    H, W, S1, S2 = 70, 100, 171, 236
    for kind_name in ("flat", "noise"):
        if kind_name == "flat":
            big1 = np.full((H + 2, S1), 255, np.uint8); big1[:, ::17] = 250
            big2 = big1[:, :1].repeat(S2, axis=1).copy(); big2[::9] = 253
            bigf = (np.float32(255) + rng.normal(0, 0.3, (H + 2, S2))).astype(np.float32)
        else:
            big1 = rng.integers(0, 256, (H + 2, S1), dtype=np.uint8); big2 = rng.integers(0, 256, (H + 2, S2), dtype=np.uint8)
            bigf = rng.uniform(0, 255, (H + 2, S2)).astype(np.float32)
        d1 = c.malloc(big1.nbytes); d2 = c.malloc(big2.nbytes); df = c.malloc(bigf.nbytes); ds = c.malloc(8)
        try:
            c.h2d(d1, big1); c.h2d(d2, big2); c.h2d(df, bigf)
            for (r1, c1, r2, c2) in ((0, 3, 0, 0), (1, 3, 2, 5), (2, 1, 1, 3), (0, 0, 1, 2)):
                w1 = big1[r1:r1 + H, c1:c1 + W]; w2 = big2[r2:r2 + H, c2:c2 + W]; wf = bigf[r2:r2 + H, c2:c2 + W]
                got = _ssim_dev(c, d1 + r1 * S1 + c1, S1, d2 + r2 * S2 + c2, S2, H, W, 0, ds)
                assert abs(got - pr.ssim64(w1, w2)) < SSIM_BAR, (kind_name, r1, c1, r2, c2, got)
                got = _ssim_dev(c, d1 + r1 * S1 + c1, S1, df + 4 * (r2 * S2 + c2), S2, H, W, 2, ds)       # uint8 window, float window
                assert abs(got - pr.ssim64(w1, wf)) < SSIM_BAR, (kind_name, r1, c1, r2, c2, got)
                got = _ssim_dev(c, df + 4 * (r2 * S2 + c2), S2, d1 + r1 * S1 + c1, S1, H, W, 1, ds)
                assert abs(got - pr.ssim64(wf, w1)) < SSIM_BAR, (kind_name, r1, c1, r2, c2, got)
                got = _ssim_dev(c, df + 4 * (r2 * S2 + c2), S2, df + 4 * (r1 * S2 + c1), S2, H, W, 3, ds)
                assert abs(got - pr.ssim64(wf, bigf[r1:r1 + H, c1:c1 + W])) < SSIM_BAR, (kind_name, r1, c1, r2, c2, got)
        finally:
            for d in (d1, d2, df, ds):
                c.free(d)


def test_ssim_refuses_planes_of_two_gib(gpu_ctx):
    """((H - 1) * stride + W) * elem >= 2^31 is refused before any launch (the kernel's buffer resources hold 32-bit
    sizes), for either image, uint8 or float32; small buffers suffice"""
    c = gpu_ctx
    d = c.malloc(4096); ds = c.malloc(8)
    try:
        W = 10
        s8 = (1 << 31) - W            # H = 2: (stride + W) * 1 = 2^31
        s32 = (1 << 29) - W           # H = 2: (stride + W) * 4 = 2^31
        for args in ((s8, 16, 0), (16, s8, 0), (s32, 16, 1), (16, s32, 2), (s32, s32, 3), (16, s8 // 2 + 5, 0)):
            s1, s2, kind = args
            H = 2 if args[1] != s8 // 2 + 5 else 3
            with pytest.raises(ValueError, match="2 GiB"):
                c._call("wm_ssim_dev", vp(d), s1, vp(d), s2, H, W, kind, vp(ds))
        x = np.full((2, 16), 255, np.uint8); c.h2d(d, x)                         # and the context still works
        assert abs(_ssim_dev(c, d, 16, d, 16, 2, W, 0, ds) - 1.0) < 1e-6
    finally:
        c.free(d); c.free(ds)
