"""The watermark side on logo-like planes (tests/watermark_planes.py): the tile SVD (K3), the tile reconstruct (K4), the
extract and detect arithmetic isolated from the SVD, and the full-frame watermark SVD, each against float64
scipy.fft / LAPACK.  A scrambled logo's tiles are mostly rank deficient, so K3's wave-uniform second pass (the completion
pattern on the generated V stream) is the NORMAL path here; a blank or sparse logo is a rank-deficient full-frame plane."""
import ctypes as C
import os
import time

import numpy as np
import pytest
from scipy.fft import dctn, idctn

import watermark_planes as wp
from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

TILE_SIZES = [(64, 96), (256, 320), (45, 70)]
PLANE_SIZES = [(40, 56), (56, 40), (72, 72), (200, 328)]
_vp = C.c_void_p


def _idct_tiles(c):
    return idctn(c, axes=(-2, -1), norm="ortho")


def _from_tiles(t, H, W):
    """[nby, nbx, 8, 8] -> (H, W) with zero borders"""
    nby, nbx = t.shape[:2]
    out = np.zeros((H, W), t.dtype)
    out[:8 * nby, :8 * nbx] = t.transpose(0, 2, 1, 3).reshape(8 * nby, 8 * nbx)
    return out


class _Dev:
    """device buffers of one test, freed at the end"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, arr, offset_bytes=0, extra=0):
        arr = np.ascontiguousarray(arr)
        d = self.ctx.malloc(arr.nbytes + offset_bytes + extra + 64)
        self.bufs.append(d)
        self.ctx.h2d(d + offset_bytes, arr)
        return d + offset_bytes

    def empty(self, nbytes):
        d = self.ctx.malloc(nbytes + 64)
        self.bufs.append(d)
        return d

    def get(self, d, shape, dtype):
        out = np.empty(shape, dtype)
        self.ctx.d2h(out, d)
        self.ctx.sync()
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.sync()
        for b in self.bufs:
            self.ctx.free(b)


# =====================================================================================================================
# tile mode: K3
# =====================================================================================================================
@pytest.mark.parametrize("H,W", TILE_SIZES)
def test_tile_svd_of_every_logo_class_against_float64(gpu_ctx, H, W):
    """wm_svd_tiles_f32 through the tile checker (singular values, order, orthonormal U and Vt on EVERY tile, U diag(S) Vt
    against the DCT tile, pixel round trip), twice with identical bytes, the sticky status clean after every class."""
    worst = {}
    for cls in wp.CLASSES:
        p = wp.generate(cls, H, W)
        U, S, Vt = gpu_ctx.svd_tiles(p)
        gpu_ctx.check_status()
        m = wp.check_tiles(p, U, S, Vt)
        U2, S2, Vt2 = gpu_ctx.svd_tiles(p)
        assert U.tobytes() == U2.tobytes() and S.tobytes() == S2.tobytes() and Vt.tobytes() == Vt2.tobytes(), cls
        print(f"tile svd {H}x{W} {cls}: {m}")
        for k in ("dS", "unsorted", "orthU", "orthV", "recon", "roundtrip"):
            worst[k] = max(worst.get(k, -1e9), m[k])
    print(f"tile svd {H}x{W} worst over classes: {worst}")


def test_tile_svd_does_not_depend_on_the_wave_neighbours(gpu_ctx):
    """Tile rows alternate classes (40 tiles per row: most waves of 64 hold full-rank and rank-deficient tiles), and every
    tile's U, S, Vt are the bytes of the same tile decomposed inside a plane of its own class only: the redo branch is
    wave uniform, a tile's result must not depend on who shares its wave."""
    H, W = 96, 320
    mix = ("noise", "white_5pct_black", "binary50", "blank255", "near_singular_tiles", "three_level")
    own = {c: wp.generate(c, H, W) for c in mix}
    plane = np.empty((H, W), np.float32)
    for r in range(H // 8):
        plane[8 * r: 8 * r + 8] = own[mix[r % len(mix)]][8 * r: 8 * r + 8]
    d = wp.deficient_tiles(plane).reshape(-1)
    waves = [d[i: i + 64] for i in range(0, d.size, 64)]
    assert sum(1 for w in waves if w.any() and not w.all()) >= len(waves) - 1
    U, S, Vt = gpu_ctx.svd_tiles(plane)
    wp.check_tiles(plane, U, S, Vt)
    for c in mix:
        Uo, So, Vo = gpu_ctx.svd_tiles(own[c])
        for r in range(H // 8):
            if mix[r % len(mix)] == c:
                assert U[r].tobytes() == Uo[r].tobytes() and S[r].tobytes() == So[r].tobytes() and Vt[r].tobytes() == Vo[r].tobytes(), (c, r)


@pytest.mark.parametrize("cls", ["three_level", "binary50"])
def test_tile_svd_of_strided_unaligned_planes(gpu_ctx, cls):
    """A view with row stride != W at an odd float offset (the VECF = false loads) gives the bytes of the dense copy."""
    H, W, rs, off = 64, 96, 101, 3
    p = wp.generate(cls, H, W)
    nt = (H // 8) * (W // 8)
    wide = np.full((H, rs), -7.0, np.float32)
    wide[:, :W] = p
    with _Dev(gpu_ctx) as dv:
        d_dense = dv.put(p)
        d_view = dv.put(wide, offset_bytes=4 * off)
        outs = []
        for d_in, stride in ((d_dense, W), (d_view, rs)):
            dU, dS, dV = dv.empty(nt * 256), dv.empty(nt * 32), dv.empty(nt * 256)
            gpu_ctx.svd_tiles_f32_dev(d_in, dU, dS, dV, 1, H, W, stride, H * stride)
            gpu_ctx.check_status()
            outs.append((dv.get(dU, (H // 8, W // 8, 8, 8), np.float32), dv.get(dS, (H // 8, W // 8, 8), np.float32),
                         dv.get(dV, (H // 8, W // 8, 8, 8), np.float32)))
    assert (d_view & 15) != 0
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    wp.check_tiles(p, *outs[1])


def test_tile_svd_of_a_batch_equals_the_single_calls(gpu_ctx):
    H, W = 64, 96
    planes = np.stack([wp.generate(c, H, W) for c in ("noise", "white_5pct_black", "three_level")])
    Ub, Sb, Vb = gpu_ctx.svd_tiles(planes)
    gpu_ctx.check_status()
    for z in range(3):
        U, S, Vt = gpu_ctx.svd_tiles(planes[z])
        assert U.tobytes() == Ub[z].tobytes() and S.tobytes() == Sb[z].tobytes() and Vt.tobytes() == Vb[z].tobytes()


# =====================================================================================================================
# tile mode: K4  wm_reconstruct_tiles
# =====================================================================================================================
def _k4_ref(U, sh, Vt, H, W):
    rec = (U.astype(np.float64) * sh.astype(np.float64)[..., None, :]) @ Vt.astype(np.float64)
    return _from_tiles(_idct_tiles(rec), H, W)


def _orth_tiles(rng, nby, nbx):
    q, _ = np.linalg.qr(rng.normal(size=(2, nby, nbx, 8, 8)))
    return q[0].astype(np.float32), np.ascontiguousarray(np.swapaxes(q[1], -1, -2)).astype(np.float32)


@pytest.mark.parametrize("H,W", [(64, 96), (45, 70), (43, 68)])
def test_k4_with_orthonormal_factors_against_float64(gpu_ctx, H, W):
    rng = np.random.default_rng(H * W)
    nby, nbx = H // 8, W // 8
    U, Vt = _orth_tiles(rng, nby, nbx)
    sh = np.sort(rng.uniform(0, 2000, (nby, nbx, 8)).astype(np.float32), axis=-1)[..., ::-1].copy()
    out = gpu_ctx.reconstruct_tiles(U, sh, Vt, H, W)
    want = _k4_ref(U, sh, Vt, H, W)
    err = np.abs(out - want).max()
    print(f"K4 orthonormal {H}x{W}: max error {err:.3e} at max|s| {sh.max():.1f}")
    assert err <= 2e-6 * float(np.abs(sh).max()) + 1e-6
    # border rows / columns outside the tile grid are exactly 0 (W % 4 != 0: scalar stores; W % 4 == 0: vector stores)
    assert not out[8 * nby:].any() and not out[:, 8 * nbx:].any()


def test_k4_with_arbitrary_finite_factors(gpu_ctx):
    """random, non-orthonormal factors of norm ~3: the f32 FMA chain's bound with margin 4,
    2e-6 * sum_i |s_i| |u_i|_inf |v_i|_inf per tile"""
    H, W = 64, 96
    rng = np.random.default_rng(5)
    nby, nbx = H // 8, W // 8
    U = rng.normal(0, 3 / np.sqrt(8), (nby, nbx, 8, 8)).astype(np.float32)
    Vt = rng.normal(0, 3 / np.sqrt(8), (nby, nbx, 8, 8)).astype(np.float32)
    sh = rng.normal(0, 500, (nby, nbx, 8)).astype(np.float32)
    out = gpu_ctx.reconstruct_tiles(U, sh, Vt, H, W)
    want = _k4_ref(U, sh, Vt, H, W)
    bound = 2e-6 * (np.abs(sh) * np.abs(U).max(-2) * np.abs(Vt).max(-1)).sum(-1)          # [nby, nbx]
    err = np.abs(wp.to_tiles(out) - wp.to_tiles(want)).max((-1, -2))
    print(f"K4 arbitrary factors: worst error / bound {float((err / bound).max()):.3f}, worst error {float(err.max()):.3e}")
    assert (err <= bound).all()


def test_k4_value_edges(gpu_ctx):
    H, W = 16, 24
    rng = np.random.default_rng(6)
    U, Vt = _orth_tiles(rng, 2, 3)
    sh = np.zeros((2, 3, 8), np.float32)
    assert not gpu_ctx.reconstruct_tiles(U, sh, Vt, H, W).any()                    # s = 0: exactly 0
    sh[0, 0] = [1e6, -1e6, 3, -2, 0, 0, 1e-3, -1e-3]
    sh[0, 1] = [-5, -4, -3, -2, -1, -0.5, -0.25, -0.125]
    sh[1, 2] = [1e6, 0, 0, 0, 0, 0, 0, 0]
    out = gpu_ctx.reconstruct_tiles(U, sh, Vt, H, W)
    want = _k4_ref(U, sh, Vt, H, W)
    t_err = np.abs(wp.to_tiles(out) - wp.to_tiles(want)).max((-1, -2))
    assert (t_err <= 2e-6 * np.abs(sh).max(-1) + 1e-6).all(), t_err
    assert not wp.to_tiles(out)[0, 2].any() and not wp.to_tiles(out)[1, 0].any()   # tiles whose estimates are all 0


def test_k4_batches_and_planes_smaller_than_a_tile(gpu_ctx):
    H, W = 24, 40
    rng = np.random.default_rng(7)
    for n in (1, 5):
        q = [_orth_tiles(rng, 3, 5) for _ in range(n)]
        U = np.stack([a for a, _ in q]); Vt = np.stack([b for _, b in q])
        sh = rng.uniform(-300, 300, (n, 3, 5, 8)).astype(np.float32)
        out = gpu_ctx.reconstruct_tiles(U, sh, Vt, H, W)
        assert out.shape == (n, H, W)
        for z in range(n):
            assert np.abs(out[z] - _k4_ref(U[z], sh[z], Vt[z], H, W)).max() <= 2e-6 * 300 + 1e-6
            one = gpu_ctx.reconstruct_tiles(U[z], sh[z], Vt[z], H, W)
            assert one.tobytes() == out[z].tobytes()
    # H or W < 8: no tile at all -> all zeros, WM_OK
    for (h, w) in ((7, 40), (24, 5), (3, 3)):
        e = np.empty((0,), np.float32)
        out = np.full((2, h, w), 9.0, np.float32)
        rc = gpu_ctx.lib.wm_reconstruct_tiles(gpu_ctx._h, _vp(e.ctypes.data), _vp(e.ctypes.data), _vp(e.ctypes.data),
                                              _vp(out.ctypes.data), 2, h, w)
        assert rc == 0 and not out.any()


@pytest.mark.parametrize("H,W", [(64, 96), (45, 70)])
def test_k4_round_trip_of_the_tile_svd_gives_the_logo_back(gpu_ctx, H, W):
    """rint(reconstruct_tiles(*svd_tiles(x))) == x on the full tiles of every class"""
    for cls in wp.CLASSES:
        p = wp.generate(cls, H, W)
        U, S, Vt = gpu_ctx.svd_tiles(p)
        back = gpu_ctx.reconstruct_tiles(U, S, Vt, H, W)
        assert np.array_equal(np.rint(wp.to_tiles(back)), wp.to_tiles(p)), cls
        assert np.abs(wp.to_tiles(back) - wp.to_tiles(p)).max() <= 2e-3, cls


def test_k4_raw_abi_refuses_bad_arguments(gpu_ctx, hostapi):
    lib, h = gpu_ctx.lib, gpu_ctx._h
    with _Dev(gpu_ctx) as dv:
        dU, dV, dS, dO = dv.empty(4096), dv.empty(4096), dv.empty(4096), dv.empty(4096)
        f = lib.wm_reconstruct_tiles_dev
        assert f(h, _vp(dU), _vp(dS), _vp(dV), _vp(dO), 1, 16, 16) == hostapi.WM_OK
        gpu_ctx.sync()
        assert f(h, _vp(dU), _vp(dS), _vp(dV), None, 1, 16, 16) == hostapi.WM_ERR_BADARG
        for n, hh, ww in ((-1, 16, 16), (1, -16, 16), (1, 16, -16), (65536, 16, 16)):
            assert f(h, _vp(dU), _vp(dS), _vp(dV), _vp(dO), n, hh, ww) == hostapi.WM_ERR_BADARG
        for bad in ((dU + 4, dS, dV), (dU, dS + 8, dV), (dU, dS, dV + 4), (None, dS, dV), (dU, None, dV), (dU, dS, None)):
            assert f(h, *[_vp(x) if x else None for x in bad], _vp(dO), 1, 16, 16) == hostapi.WM_ERR_BADARG
        gpu_ctx.sync()
    gpu_ctx.check_status()


# =====================================================================================================================
# tile mode: extract and detect arithmetic, isolated from the SVD
# =====================================================================================================================
def _stego(H, W, seed=9):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def _logo_factors(gpu_ctx, H, W, cls):
    U, S, Vt = gpu_ctx.svd_tiles(wp.generate(cls, H, W))
    return U, S, Vt


@pytest.mark.parametrize("per_plane", [False, True])
def test_extract_of_a_stego_against_its_own_sigma_is_exactly_zero(gpu_ctx, per_plane):
    """sc = sigma_tiles(stego): both kernels call the same sigma_tile_dev, (s - sc) is exactly 0 for every K"""
    H, W = 64, 96
    st = np.stack([_stego(H, W, 9), _stego(H, W, 10)])
    st[1, :16] = 200                                                   # flat tiles too
    sc = gpu_ctx.sigma_tiles(st)
    f = [_logo_factors(gpu_ctx, H, W, c) for c in ("binary50", "white_5pct_black")]
    U = np.stack([a[0] for a in f]) if per_plane else f[0][0]
    Vt = np.stack([a[2] for a in f]) if per_plane else f[0][2]
    for K in range(9):
        for alpha in (0.15, 1e-3):
            assert not gpu_ctx.extract_tiles(st, sc, U, Vt, alpha, K).any(), (K, alpha)


@pytest.mark.parametrize("cls", ["binary50", "three_level", "white_5pct_black"])
def test_extract_of_one_unit_estimate_is_the_outer_product(gpu_ctx, cls):
    """sc = sigma - alpha e_k: the output is idct2(u_k v_k^T) times the float32 value of (s - sc) / alpha;
    for K <= k it is exactly 0"""
    H, W, alpha = 64, 96, 0.15
    st = _stego(H, W)
    s = gpu_ctx.sigma_tiles(st)
    U, _, Vt = _logo_factors(gpu_ctx, H, W, cls)
    inv = np.float32(1.0) / np.float32(max(alpha, 1e-8))
    worst = 0.0
    for k in range(8):
        sc = s.copy()
        sc[..., k] = s[..., k] - np.float32(alpha)
        y = ((s[..., k] - sc[..., k]) * inv).astype(np.float64)                       # as the kernel computes it
        assert np.abs(y - 1).max() < 1e-2
        want = _idct_tiles(y[..., None, None] * U[..., :, k, None].astype(np.float64) * Vt[..., None, k, :].astype(np.float64))
        out = gpu_ctx.extract_tiles(st, sc, U, Vt, alpha, 8)
        e = float(np.abs(wp.to_tiles(out) - want).max())
        worst = max(worst, e)
        assert e <= 2e-6, (k, e)
        for K in range(k + 1):
            assert not gpu_ctx.extract_tiles(st, sc, U, Vt, alpha, K).any(), (k, K)
    print(f"extract unit estimate {cls}: worst error {worst:.3e}")


def test_extract_alpha_guard(gpu_ctx):
    """alpha = 0 and 1e-9 are max(alpha, 1e-8): the bytes of alpha = 1e-8"""
    H, W = 32, 48
    st = _stego(H, W)
    s = gpu_ctx.sigma_tiles(st)
    sc = s - np.float32(1e-4) * s                                       # small differences: finite after / 1e-8
    U, _, Vt = _logo_factors(gpu_ctx, H, W, "binary50")
    ref = gpu_ctx.extract_tiles(st, sc, U, Vt, 1e-8, 8)
    assert np.isfinite(ref).all() and ref.any()
    for a in (0.0, 1e-9):
        assert gpu_ctx.extract_tiles(st, sc, U, Vt, a, 8).tobytes() == ref.tobytes()


@pytest.mark.parametrize("cls", ["binary50", "white_5pct_black", "unscrambled_logo"])
def test_extract_with_pixel_domain_factors(gpu_ctx, cls):
    """wm_tile_factors_to_pixel_dev + wm_extract_tiles_px_u8_dev against float64 (D^T U) diag (Vt D)"""
    H, W, alpha = 64, 96, 0.15
    nt = (H // 8) * (W // 8)
    st = _stego(H, W)
    s = gpu_ctx.sigma_tiles(st)
    rng = np.random.default_rng(3)
    sc = (s - np.float32(alpha) * rng.uniform(0, 255, s.shape).astype(np.float32)).astype(np.float32)
    U, _, Vt = _logo_factors(gpu_ctx, H, W, cls)
    inv = np.float32(1.0) / np.float32(alpha)
    y = ((s - sc) * inv).astype(np.float64)
    want = _idct_tiles((U.astype(np.float64) * y[..., None, :]) @ Vt.astype(np.float64))
    with _Dev(gpu_ctx) as dv:
        dU, dV, dst, dsc = dv.put(U), dv.put(Vt), dv.put(st), dv.put(sc)
        dUx, dVx, dout = dv.empty(nt * 256), dv.empty(nt * 256), dv.empty(H * W * 4)
        gpu_ctx.tile_factors_to_pixel_dev(dU, dV, dUx, dVx, nt)
        gpu_ctx.extract_tiles_px_u8_dev(dst, dsc, dUx, dVx, dout, 1, H, W, W, H * W, 0, alpha, 8)
        gpu_ctx.check_status()
        out = dv.get(dout, (H, W), np.float32)
        Ux = dv.get(dUx, U.shape, np.float32)
    D = dctn(np.eye(8), axes=0, norm="ortho")                                   # D @ x = dct(x)
    assert np.abs(Ux - D.T @ U.astype(np.float64)).max() < 2e-6
    e = float(np.abs(wp.to_tiles(out) - want).max())
    print(f"extract px {cls}: error {e:.3e} at max|y| {np.abs(y).max():.1f}")
    assert e <= 2e-6 * float(np.abs(y).max()) + 1e-6


def _nc64(x, y):
    """the reference's two-pass normalised correlation in float64"""
    x = np.asarray(x, np.float64).ravel(); y = np.asarray(y, np.float64).ravel()
    x = x - x.mean(); y = y - y.mean()
    return float((x * y).sum() / (np.sqrt((x * x).sum()) * np.sqrt((y * y).sum()) + 1e-8))


def _detect_inputs(gpu_ctx, H, W, alpha, seed=1):
    st = _stego(H, W, seed)
    s = gpu_ctx.sigma_tiles(st)
    rng = np.random.default_rng(seed + 100)
    sw = np.sort(rng.uniform(0, 2000, s.shape).astype(np.float32), axis=-1)[..., ::-1].copy()
    sc = (s - np.float32(alpha) * (sw + rng.normal(0, 200, s.shape).astype(np.float32))).astype(np.float32)
    inv = np.float32(1.0) / np.float32(max(alpha, 1e-8))
    y = (s - sc) * inv                                                  # float32, as the kernel computes it
    return st, s, sc, sw, y


@pytest.mark.parametrize("H,W", [(8, 8), (8 * 7, 8 * 9), (64, 64), (8 * 5, 8 * 13), (64, 96)])
def test_detect_against_the_float64_two_pass_correlation(gpu_ctx, H, W):
    """n_tiles = 1, 63, 64, 65 and 96: well-conditioned vectors, 1e-9 absolute"""
    alpha = 0.15
    st, s, sc, sw, y = _detect_inputs(gpu_ctx, H, W, alpha)
    got = gpu_ctx.detect_tiles(st, sc, sw, alpha)[0]
    want = _nc64(sw, y)
    print(f"detect {H}x{W}: |score - float64| = {abs(got - want):.3e}")
    assert abs(got - want) <= 1e-9
    # edges: a constant sigma_w, sc == s -> exactly 0
    assert gpu_ctx.detect_tiles(st, sc, np.full_like(sw, 37.0), alpha)[0] == 0.0
    assert gpu_ctx.detect_tiles(st, s, sw, alpha)[0] == 0.0


def test_detect_without_tiles_is_zero(gpu_ctx):
    st = _stego(7, 40)
    e = np.zeros((0, 5, 8), np.float32)
    assert gpu_ctx.detect_tiles(st, e, e, 0.15)[0] == 0.0


def test_detect_conditioning(gpu_ctx):
    """sigma_w with mean / std up to 1e4: the kernel's sums are one-pass (float64); the existing 1e-4 bar"""
    H, W, alpha = 64, 96, 0.15
    st, s, sc, sw, y = _detect_inputs(gpu_ctx, H, W, alpha)
    worst = 0.0
    for ratio in (1e1, 1e2, 1e3, 1e4):
        swr = (sw / np.float32(sw.std()) + np.float32(ratio)).astype(np.float32)       # std 1, mean = ratio
        got = gpu_ctx.detect_tiles(st, sc, swr, alpha)[0]
        worst = max(worst, abs(got - _nc64(swr, y)))
    print(f"detect conditioning: worst |score - float64| = {worst:.3e}")
    assert worst <= 1e-4


def test_detect_of_more_planes_than_the_finalize_block_has_threads(gpu_ctx):
    H, W, alpha, n = 24, 40, 0.15, 300
    st = np.random.default_rng(2).integers(0, 256, (n, H, W), dtype=np.uint8)
    s = gpu_ctx.sigma_tiles(st)
    rng = np.random.default_rng(3)
    sw = rng.uniform(0, 2000, s.shape).astype(np.float32)                       # per-plane sigma_w
    sc = (s - np.float32(alpha) * (sw + rng.normal(0, 300, s.shape).astype(np.float32))).astype(np.float32)
    y = (s - sc) * (np.float32(1.0) / np.float32(alpha))
    got = gpu_ctx.detect_tiles(st, sc, sw, alpha)
    want = np.array([_nc64(sw[z], y[z]) for z in range(n)])
    assert np.abs(got - want).max() <= 1e-9
    got1 = gpu_ctx.detect_tiles(st, sc, sw[0], alpha)                           # shared sigma_w
    assert np.abs(got1 - np.array([_nc64(sw[0], y[z]) for z in range(n)])).max() <= 1e-9


def test_detect_of_one_8k_plane(gpu_ctx):
    """518 400 tiles = 8 100 wave partials: every partial of every wave of the finalize block counts"""
    H, W, alpha = 4320, 7680, 0.15
    st = np.random.default_rng(4).integers(0, 256, (1, H, W), dtype=np.uint8)
    s = gpu_ctx.sigma_tiles(st)
    rng = np.random.default_rng(5)
    sw = np.sort(rng.uniform(0, 2000, s.shape).astype(np.float32), axis=-1)[..., ::-1].copy()
    sc = (s - np.float32(alpha) * (sw + rng.normal(0, 200, s.shape).astype(np.float32))).astype(np.float32)
    y = (s - sc) * (np.float32(1.0) / np.float32(alpha))
    got = gpu_ctx.detect_tiles(st, sc, sw, alpha)[0]                            # sw [1, nby, nbx, 8]: per-plane stride
    want = _nc64(sw, y)
    print(f"detect 8K: |score - float64| = {abs(got - want):.3e}")
    assert abs(got - want) <= 1e-9


# =====================================================================================================================
# full-frame mode: wm_ref_svd_f32 / wm_ref_svd_planes_f32
# =====================================================================================================================
@pytest.mark.parametrize("apply_dct", [True, False])
@pytest.mark.parametrize("H,W", PLANE_SIZES)
def test_fullframe_svd_of_every_logo_class_against_float64(gpu_ctx, H, W, apply_dct):
    """56x40 is the transposed path (U is the long side); L is not a multiple of 32 in any of these.  Orthonormality over
    ALL L columns / rows: a rank-deficient plane (blank, sparse, zero, unscrambled) must come back with a completed basis."""
    failed = []
    for cls in wp.CLASSES:
        p = wp.generate(cls, H, W)
        U, S, Vt = gpu_ctx.ref_svd(p, apply_dct=apply_dct)
        try:
            m = wp.check_plane(p, U, S, Vt, apply_dct=apply_dct)
            print(f"full-frame svd {H}x{W} dct={int(apply_dct)} {cls}: {m}")
        except AssertionError as e:
            print(f"full-frame svd {H}x{W} dct={int(apply_dct)} {cls}: FAILED {e}")
            failed.append((cls, str(e)))
    assert not failed, failed


@pytest.mark.parametrize("H,W", [(24, 40), (6, 10), (40, 24), (10, 6)])
def test_fullframe_svd_of_small_planes(gpu_ctx, H, W):
    for cls in ("noise", "binary50", "blank255"):
        for apply_dct in (True, False):
            p = wp.generate(cls, H, W)
            m = wp.check_plane(p, *gpu_ctx.ref_svd(p, apply_dct=apply_dct), apply_dct=apply_dct)
            print(f"full-frame svd {H}x{W} dct={int(apply_dct)} {cls}: {m}")


@pytest.mark.parametrize("cls", ["noise", "sparse_marks"])
def test_fullframe_svd_of_a_strided_plane(gpu_ctx, cls):
    H, W, rs = 72, 100, 117
    p = wp.generate(cls, H, W)
    wide = np.full((H, rs), -3.0, np.float32)
    wide[:, :W] = p
    L = min(H, W)
    U = np.empty((H, L), np.float32); S = np.empty(L, np.float32); Vt = np.empty((L, W), np.float32)
    gpu_ctx._call("wm_ref_svd_f32", _vp(wide.ctypes.data), _vp(U.ctypes.data), _vp(S.ctypes.data), _vp(Vt.ctypes.data),
                  H, W, rs, 1)
    wp.check_plane(p, U, S, Vt)
    U1, S1, V1 = gpu_ctx.ref_svd(p)
    assert S.tobytes() == S1.tobytes() and U.tobytes() == U1.tobytes() and Vt.tobytes() == V1.tobytes()


@pytest.mark.parametrize("H,W", [(72, 100), (100, 72)])
def test_fullframe_svd_of_a_colour_logo_with_constant_channels(gpu_ctx, H, W):
    """three planes per batch, noise | sparse_marks | zero: each passes the checker, S as the single-plane call's"""
    planes = np.stack([wp.generate(c, H, W) for c in ("noise", "sparse_marks", "zero")])
    for apply_dct in (True, False):
        Ub, Sb, Vb = gpu_ctx.ref_svd_planes(planes, apply_dct=apply_dct)
        for z in range(3):
            wp.check_plane(planes[z], Ub[z], Sb[z], Vb[z], apply_dct=apply_dct)
            _, S1, _ = gpu_ctx.ref_svd(planes[z], apply_dct=apply_dct)
            s1 = max(float(S1[0]), 1e-30)
            assert np.abs(S1 - Sb[z]).max() <= (2e-6 * s1 if S1[0] > 1e-6 else 1e-6)


@pytest.mark.parametrize("cls", ["white_5pct_black", "blank255"])
def test_fullframe_svd_at_1080p(gpu_ctx, cls):
    """full rank with sigma_1 / sigma_L ~ 600, and rank 1; wall time printed (DESIGN 9.3 states 28 ms on noise)"""
    p = wp.generate(cls, 1080, 1920)
    gpu_ctx.ref_svd(p)                                                  # workspaces, DCT bases
    t0 = time.perf_counter()
    U, S, Vt = gpu_ctx.ref_svd(p)
    ms = 1e3 * (time.perf_counter() - t0)
    m = wp.check_plane(p, U, S, Vt)
    print(f"full-frame svd 1080p {cls}: {ms:.1f} ms, {m}")


@pytest.mark.parametrize("cls", ["binary50", "sparse_marks"])
@pytest.mark.parametrize("H,W", [(64, 96), (96, 64), (128, 128)])
def test_fullframe_round_trip_with_the_devices_own_factors(gpu_ctx, cls, H, W):
    """ref_embed then ref_extract with the device's own factors of a logo, held against oracle.extract_plane fed the same
    stego and factors (2e-3 of the range and correlation > 0.98, as test_fullframe_watermark_svd_and_extract asks), at
    the reference's band K = max(8, int(0.6 L)) and at the full band K = L.
    Correlation with the LOGO itself is held only where the reference arithmetic reaches 0.98 at all: the float64 oracle
    alone, on these inputs, gives 0.9986 for binary50 at 128x128 with K = L, but 0.97 there with K = 0.6 L, 0.76-0.81 on
    the 64x96 / 96x64 planes (single:214-218 keep the L x L corner only) and a negative value for sparse_marks (its
    estimate is a constant plus 40 marks)."""
    alpha = 0.15
    host = np.random.default_rng(1234).integers(0, 256, (H, W), dtype=np.uint8)
    wys = wp.generate(cls, H, W)
    U, S, Vt = gpu_ctx.ref_svd(wys, apply_dct=True)
    L = min(H, W)
    for kfrac in (0.6, 1.0):
        K = o.k_of(L, kfrac, 8)
        st, sc, _ = gpu_ctx.ref_embed(host, S, alpha, K)
        w = gpu_ctx.ref_extract(st, sc, U, Vt, alpha, K)
        wo = o.extract_plane(st.astype(np.float32), sc, U, Vt, alpha, kfrac, H, W, None)
        c_o = np.corrcoef(w[:L, :L].ravel(), wo[:L, :L].ravel())[0, 1]
        c_logo = np.corrcoef(w.ravel(), wys.ravel())[0, 1]
        print(f"round trip {cls} {H}x{W} K={K}: |w - oracle| / max = {np.abs(w - wo).max() / np.abs(wo).max():.3e}, "
              f"corr with the oracle {c_o:.5f}, with the logo {c_logo:.4f}")
        assert np.abs(w - wo).max() < 2e-3 * np.abs(wo).max()
        assert c_o > 0.98
        if cls == "binary50" and H == W and K == L:
            assert c_logo > 0.98


def _full_k_estimate(U, S, Vt, K, H, W):
    """what a lossless channel would return: idct2 of the rank-K part of the logo's DCT plane"""
    L = min(H, W)
    s = np.zeros(L); s[:K] = S[:K]
    full = np.zeros((H, W))
    full[:L, :L] = (U[:L, :L].astype(np.float64) * s) @ Vt[:L, :L].astype(np.float64)
    return idctn(full, norm="ortho")


@pytest.mark.parametrize("cls", wp.CLASSES)
def test_fullframe_f16_and_f32_reconstruct_agree_on_the_devices_factors(gpu_ctx, monkeypatch, cls):
    """wm_ref_reconstruct_f32 on the device's own factors of each class (128x192: the split-f16 products are eligible)
    under WM_RF_FINAL_F16=1 and =0, both against float64 at the bar of tests/test_gpu_f16_products.py (2e-6 of the range)"""
    H, W = 128, 192
    p = wp.generate(cls, H, W)
    U, S, Vt = gpu_ctx.ref_svd(p, apply_dct=True)
    sh = S if S.max() > 0 else np.ones_like(S)
    want = _full_k_estimate(U, sh, Vt, len(sh), H, W)
    scale = max(float(np.abs(want).max()), 1e-300)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("WM_RF_FINAL_F16", flag)
        out[flag] = gpu_ctx.ref_reconstruct(U, sh, Vt, H, W)
        e = float(np.abs(out[flag] - want).max()) / scale
        print(f"reconstruct {cls} WM_RF_FINAL_F16={flag}: {e:.3e}")
        assert e <= 2e-6, (cls, flag, e)


# =====================================================================================================================
# the drop-in on logos
# =====================================================================================================================
@pytest.mark.parametrize("tile", [8, None])
@pytest.mark.parametrize("color", [False, True])
def test_dropin_on_logos(gpu_ctx, tile, color):
    """a gray binary50 logo / a colour logo whose B and G planes are zero: embed -> extract -> detect do not raise, the
    meta's factors are orthonormal, the extract is the oracle's extract of the same stego and meta"""
    import dct_svd_core_secure as core
    H, W = 64, 96
    rng = np.random.default_rng(8)
    cover = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    logo = wp.generate("binary50", H, W).astype(np.uint8)
    # the drop-in scrambles the logo itself: hand it the unscrambled picture, a half-black half-white plane
    logo = np.sort(logo.reshape(-1)).reshape(H, W)
    if color:
        wm = np.zeros((H, W, 3), np.uint8); wm[..., 2] = logo
    else:
        wm = np.stack([logo] * 3, axis=-1)
    r = core.embed_arrays(cover, wm, "pw", bytes(8), alpha=0.12, color=color, tile=tile)
    meta = r["meta"]
    pairs = [("UWb", "VWbt"), ("UWg", "VWgt"), ("UWr", "VWrt")] if color else [("Uw", "Vwt")]
    bar = 1e-5
    for un, vn in pairs:
        U = np.asarray(meta[un], np.float64); Vt = np.asarray(meta[vn], np.float64)
        n = U.shape[-1]
        assert np.isfinite(U).all() and np.isfinite(Vt).all()
        assert np.abs(np.swapaxes(U, -1, -2) @ U - np.eye(n)).max() < bar, (un, tile)
        assert np.abs(Vt @ np.swapaxes(Vt, -1, -2) - np.eye(n)).max() < bar, (vn, tile)
    ex = core.extract_arrays(r["stego"], meta, "pw", True)
    ex_o = o.extract_arrays(r["stego"], meta, "pw", True, tile, 8)
    assert ex.shape == ex_o.shape
    if color:
        # the estimate of a ZERO watermark plane is the rounding noise of (S_cw - Sc) / alpha, min-max normalised to 0..255
        # (single:269-274): nothing the two implementations could agree on.  The channel that carries the logo is compared.
        ex, ex_o = ex[..., 2], ex_o[..., 2]
    if tile == 8:
        assert np.mean(np.abs(ex.astype(int) - ex_o.astype(int)) > 1) < 2e-2
    else:
        assert np.mean(np.abs(ex.astype(int) - ex_o.astype(int)) > 2) < 5e-2
    ok, score = core.detect_arrays(r["stego"], meta)
    assert np.isfinite(score)
