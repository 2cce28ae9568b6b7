"""Tiles and waves shared by tests/test_jacobi_scaled_rotation.py and tests/test_gpu_scaled_rotation.py: the four content
kinds of tools/conv_study.cpp (noise, natural, JPEG-quantised, posterised) and waves built around the wave-uniform swap
branch of the scaled rotations."""
import numpy as np

KINDS = ("noise", "natural", "quantised", "posterised")

_QT = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.float64).reshape(8, 8)
_C = np.array([[(0.5 if u else np.sqrt(0.125)) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


def _smooth(rng, n):
    yy, xx = np.mgrid[0:8, 0:8]
    b0 = rng.uniform(20, 220, (n, 1, 1)); gx = rng.uniform(-4, 4, (n, 1, 1)); gy = rng.uniform(-4, 4, (n, 1, 1))
    cxy = rng.uniform(-0.25, 0.25, (n, 1, 1))
    return b0 + gx * xx + gy * yy + cxy * xx * yy + rng.normal(0, 2.0, (n, 8, 8))


def tiles(kind, n, seed):
    """n uint8 tiles [n, 8, 8] of one content kind"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (n, 8, 8), dtype=np.uint8)
    v = _smooth(rng, n)
    if kind == "posterised":                                    # 16 grey levels
        v = 16 * np.floor(v / 16) + 8
    if kind == "quantised":                                     # JPEG-like round trip: 8x8 DCT, luminance table at quality 50
        p = np.clip(v, 0, 255).astype(np.uint8).astype(np.float64) - 128.0
        d = _QT * np.rint(np.einsum("ur,nrc,vc->nuv", _C, p, _C) / _QT)
        v = np.rint(np.einsum("ur,nuv,vc->nrc", _C, d, _C) + 128.0)
    return np.clip(v, 0, 255).astype(np.uint8)


def one_late_swap_wave():
    """63 smooth tiles with steep, well-separated spectra and, in lane 17, a block-diagonal tile whose singular values
    come in near-equal pairs (diag(A, A) with one pixel nudged): in the third sweep that lane alone still wants a swap."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:8, 0:8]
    t = np.zeros((64, 8, 8))
    for i in range(64):
        t[i] = (rng.uniform(40, 200) + rng.uniform(-6, 6) * xx + rng.uniform(-6, 6) * yy + rng.uniform(-.25, .25) * xx * yy
                + rng.normal(0, 3.5, (8, 8)))
    w = np.clip(t, 0, 255).astype(np.uint8)
    a = rng.integers(0, 256, (4, 4))
    d = np.zeros((8, 8), np.int64); d[:4, :4] = a; d[4:, 4:] = a; d[7, 7] = min(255, d[7, 7] + 1)
    w[17] = d
    return w


def every_lane_swaps_wave():
    """64 row permutations of one noise tile: the same column Gram matrix in every lane, so where one lane wants the swap
    all 64 do"""
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (8, 8), dtype=np.uint8)
    return np.stack([base[rng.permutation(8)] for _ in range(64)])


def degenerate_wave():
    """zero, flat and rank-1 tiles between full-rank ones"""
    rng = np.random.default_rng(13)
    w = rng.integers(0, 256, (64, 8, 8), dtype=np.uint8)
    for k in range(0, 64, 4):
        w[k] = 0 if k % 12 == 0 else 200 if k % 12 == 4 else np.outer(rng.integers(1, 16, 8), rng.integers(1, 16, 8))
    return w


def plane_of(tile_stack, nby, nbx, H=None, W=None, fill=77):
    """the first nby * nbx tiles laid out row-major on an H x W plane (ragged border of `fill` when H, W exceed the tiles)"""
    H, W = H or 8 * nby, W or 8 * nbx
    p = np.full((H, W), fill, np.uint8)
    p[:8 * nby, :8 * nbx] = tile_stack[:nby * nbx].reshape(nby, nbx, 8, 8).transpose(0, 2, 1, 3).reshape(8 * nby, 8 * nbx)
    return p
