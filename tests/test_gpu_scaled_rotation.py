"""The tile kernels on the stream with scaled rotations (csrc/wm_jacobi_gfx950.inc) against oracle/wm_oracle.py: embed,
sigma pass and extract on a 64 x 64 plane (one full wave) and on a 75 x 139 one (72 x 136 of tiles: two full waves, a
partial third, and a ragged border), on the four content kinds of tools/conv_study.cpp and on the waves built around the
wave-uniform swap branch (tests/scaled_rotation_inputs.py).  Bars: stego within 1 LSB, singular values within 1e-4
sigma_1, extract within the 2e-2 of tests/test_gpu_parity.py, status clean."""
import os
import sys

import numpy as np
import pytest

from oracle import wm_oracle as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scaled_rotation_inputs as inp  # noqa: E402

pytestmark = pytest.mark.gpu

ALPHA = 0.15
SHAPES = {"64x64": (8, 8, 64, 64), "75x139": (9, 17, 75, 139)}          # (tile rows, tile columns, H, W)


def _stack(name, n):
    """n tiles of a content kind, or the named 64-tile wave repeated (the partial wave then holds its first lanes)"""
    if name in inp.KINDS:
        return inp.tiles(name, n, 50 + inp.KINDS.index(name))
    w = {"one_late_swap": inp.one_late_swap_wave, "every_lane_swaps": inp.every_lane_swaps_wave}[name]()
    return np.concatenate([w] * ((n + 63) // 64))[:n]


_WM = {}


def _watermark(H, W):
    if (H, W) not in _WM:
        wys = np.random.default_rng(4321).integers(0, 256, (H, W)).astype(np.float32)
        _WM[H, W] = (wys,) + tuple(o.watermark_decompose(wys, 8))
    return _WM[H, W]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", list(inp.KINDS) + ["one_late_swap", "every_lane_swaps"])
def test_embed_sigma_extract_against_the_oracle(gpu_ctx, name, shape):
    nby, nbx, H, W = SHAPES[shape]
    host = inp.plane_of(_stack(name, nby * nbx), nby, nbx, H, W)
    wys, Uo, So, Vto = _watermark(H, W)
    ref = o.embed_plane(host.astype(np.float32), wys, ALPHA, 0.6, 8, wm_svd=(Uo, So, Vto))
    stego, sc, yw = gpu_ctx.embed_tiles(host, So, ALPHA, K=8, want_yw=True)
    rel = lambda a, b: float(np.max(np.abs(a.reshape(-1, 8) - b.reshape(-1, 8)) / np.maximum(b.reshape(-1, 8)[:, :1], 1e-30)))
    T = lambda x: x[:8 * nby, :8 * nbx].reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3)
    d = T(np.abs(stego.astype(np.int32) - ref["stego"].astype(np.int32))).max(axis=(2, 3))           # per tile
    # The oracle's stego is defined where the tile's singular vectors are: s_8 > 1e-9 s_1 and no two singular values
    # within 1e-4 s_1 of each other (the definition of test_gpu_parity.py::test_random_scenes_every_tile_class; JPEG-
    # quantised and posterised content is rich in the other kind).  Every other tile is held to what the reference
    # guarantees whatever vectors it picks: svd(Yw) = Sc + alpha Sw, to the 5e-4 sigma_1 of that test.
    S = np.linalg.svd(T(host).astype(np.float64), compute_uv=False)
    gaps = np.min(-np.diff(S, axis=-1) / np.maximum(S[..., :1], 1e-30), axis=-1)
    unique = (S[..., 7] > 1e-9 * S[..., 0]) & (gaps > 1e-4)
    got = np.linalg.svd(T(yw).astype(np.float64), compute_uv=False)
    want = np.sort(sc.astype(np.float64) + ALPHA * So.astype(np.float64), axis=-1)[..., ::-1]
    sig = gpu_ctx.sigma_tiles(ref["stego"])
    sref = o.stego_sigma(ref["stego"].astype(np.float32), 8)
    w = gpu_ctx.extract_tiles(ref["stego"], ref["Sc"], Uo, Vto, ALPHA, K=8)
    wo = o.extract_plane(ref["stego"].astype(np.float32), ref["Sc"], Uo, Vto, ALPHA, 0.6, H, W, 8)
    print(f"{name} {shape}: {int(unique.sum())} of {unique.size} tiles with unique vectors, stego max "
          f"{int(d[unique].max()) if unique.any() else 0} LSB on them ({int(d.max())} on all), Sc {rel(sc, ref['Sc']):.2e} "
          f"sigma_1, svd(Yw) {float(np.max(np.abs(got - want) / np.maximum(want[..., :1], 1.0))):.2e} sigma_1, sigma pass "
          f"{rel(sig, sref):.2e} sigma_1, extract max |diff| {float(np.abs(w - wo).max()):.2e}")
    assert not unique.any() or d[unique].max() <= 1
    assert np.isfinite(yw).all() and np.array_equal(stego[:8 * nby, :8 * nbx], np.clip(yw, 0, 255).astype(np.uint8)[:8 * nby, :8 * nbx])
    assert np.max(np.abs(got - want) / np.maximum(want[..., :1], 1.0)) < 5e-4
    assert np.array_equal(stego[8 * nby:], host[8 * nby:]) and np.array_equal(stego[:, 8 * nbx:], host[:, 8 * nbx:])
    assert rel(sc, ref["Sc"]) < 1e-4
    assert rel(sig, sref) < 1e-4
    assert np.abs(w - wo).max() < 2e-2
    gpu_ctx.check_status()
