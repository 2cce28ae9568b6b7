"""The logo-like watermark planes of tests/watermark_planes.py and its float64 checkers, without a GPU:
the generators are what they claim (ranks, shares of rank-deficient tiles), float32 LAPACK - the reference's own
arithmetic - meets every bar of both checkers, the CPU build of the tile arithmetic (tests/host_harness.cpp) meets the
tile bars on every class, and the generated V stream (tools/emu_jacobi_asm.py) decomposes a wave that mixes full-rank and
rank-deficient logo tiles, with and without the completion pattern."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import __graft_entry__ as ge
import watermark_planes as wp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TILE_SIZES = [(64, 96), (256, 320), (45, 70)]
PLANE_SIZES = [(40, 56), (56, 40), (72, 72), (200, 328)]


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("cls", wp.CLASSES)
def test_generators_are_seeded_integer_planes(cls):
    a = wp.generate(cls, 40, 56, seed=3)
    assert a.dtype == np.float32 and a.shape == (40, 56)
    assert np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() <= 255
    assert np.array_equal(a, wp.generate(cls, 40, 56, seed=3))
    if cls not in ("blank255", "zero", "unscrambled_logo", "antialiased"):
        assert not np.array_equal(a, wp.generate(cls, 40, 56, seed=4))


def test_generated_levels():
    n = 256 * 320
    g = lambda c: wp.generate(c, 256, 320)
    assert set(np.unique(g("binary50"))) == {0, 255} and np.sum(g("binary50") == 0) == n // 2
    assert np.sum(g("white_5pct_black") == 0) == round(0.05 * n) and np.sum(g("white_5pct_black") == 255) == n - round(0.05 * n)
    assert np.array_equal(g("black_5pct_white") == 255, g("black_5pct_white") != 0) and np.sum(g("black_5pct_white") == 255) == round(0.05 * n)
    v, c = np.unique(g("three_level"), return_counts=True)
    assert list(v) == [0, 128, 255] and np.allclose(c / n, [0.1, 0.1, 0.8], atol=1e-4)
    assert set(np.unique(g("two_adjacent"))) == {254, 255}
    assert len(np.unique(g("antialiased"))) > 32
    assert np.sum(g("sparse_marks") != 255) == 40
    assert (g("blank255") == 255).all() and not g("zero").any()


@pytest.mark.parametrize("H,W", PLANE_SIZES + [(24, 40), (6, 10)])
def test_plane_ranks(H, W):
    L = min(H, W)
    for cls in ("noise", "binary50", "three_level"):
        if H * W >= 40 * 56:
            assert wp.plane_rank(wp.generate(cls, H, W)) == L, cls
    for cls in ("white_5pct_black", "black_5pct_white"):        # small planes have rows without a single mark: rank deficient
        r = wp.plane_rank(wp.generate(cls, H, W))
        assert r == L if (H, W) == (200, 328) else min(L, H * W // 40) // 3 < r <= L, (cls, r)
    assert wp.plane_rank(wp.generate("blank255", H, W)) == 1
    assert wp.plane_rank(wp.generate("zero", H, W)) == 0
    r = wp.plane_rank(wp.generate("sparse_marks", H, W))
    assert r <= 41 and (r < L or L <= 41)
    assert wp.plane_rank(wp.generate("unscrambled_logo", H, W)) <= 3


def test_1080p_ranks():
    """a white 1080p logo with 40 dark pixels: rank 40 or 41 of 1080; the 5 % logo is full rank with a wide spectrum"""
    assert wp.plane_rank(wp.generate("sparse_marks", 1080, 1920)) in (40, 41)
    s = np.linalg.svd(wp.generate("white_5pct_black", 1080, 1920).astype(np.float64), compute_uv=False)
    assert s[-1] > 1e-9 * s[0] and 100 < s[0] / s[-1] < 1e5


# share of tiles the kernels must complete (s8 <= 1e-5 s1), per class: measured 0.43-0.50 / 0.74-0.78 / 0.98-1.00 /
# 0.35; loose brackets, so that a changed generator cannot silently turn the GPU tests back into noise tests
SHARES = {"noise": (0.0, 0.01), "binary50": (0.35, 0.60), "three_level": (0.65, 0.88), "white_5pct_black": (0.95, 1.0),
          "black_5pct_white": (0.95, 1.0), "two_adjacent": (0.25, 0.60), "sparse_marks": (0.9, 1.0), "blank255": (1.0, 1.0),
          "zero": (1.0, 1.0), "unscrambled_logo": (1.0, 1.0), "antialiased": (0.0, 1.0), "near_singular_tiles": (0.0, 0.01)}


@pytest.mark.parametrize("H,W", [(256, 320), (512, 512)])
def test_share_of_rank_deficient_tiles(H, W):
    got = {}
    for cls in wp.CLASSES:
        share = float(wp.deficient_tiles(wp.generate(cls, H, W)).mean())
        got[cls] = share
        lo, hi = SHARES[cls]
        assert lo <= share <= hi, (cls, share)
    print(got)


def test_near_singular_tiles_are_full_rank_and_near_singular():
    p = wp.generate("near_singular_tiles", 64, 96)
    s = wp.tile_svals64(p)[wp.near_singular_mask(64, 96)]
    r = s[:, 7] / s[:, 0]
    # the DCT is orthogonal: the tile's own ratio
    assert (r >= 1e-5 * (1 - 1e-9)).all() and (r <= 1e-3 * (1 + 1e-9)).all() and len(r) >= 30


# ---- the reference alone meets every bar -------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", TILE_SIZES)
def test_float32_lapack_meets_the_tile_bars(H, W):
    for cls in wp.CLASSES:
        p = wp.generate(cls, H, W)
        m = wp.check_tiles(p, *wp.lapack_f32_tiles(p), completed_by_pattern=False)
        assert max(m["orthU"], m["orthV"]) < 2e-6 and m["recon"] < 1e-6 and m["dS"] < 1e-6, (cls, m)


@pytest.mark.parametrize("apply_dct", [True, False])
@pytest.mark.parametrize("H,W", PLANE_SIZES + [(24, 40), (6, 10)])
def test_float32_lapack_meets_the_plane_bars(H, W, apply_dct):
    for cls in wp.CLASSES:
        p = wp.generate(cls, H, W)
        m = wp.check_plane(p, *wp.lapack_f32_plane(p, apply_dct), apply_dct=apply_dct)
        assert max(m["orthU"], m["orthV"]) < 5e-6 and m["recon"] < 2e-6 and m["dS"] < 1e-6, (cls, m)


@pytest.mark.parametrize("cls", ["white_5pct_black", "blank255", "sparse_marks"])
def test_float32_lapack_meets_the_plane_bars_at_1080p(cls):
    p = wp.generate(cls, 1080, 1920)
    m = wp.check_plane(p, *wp.lapack_f32_plane(p))
    assert max(m["orthU"], m["orthV"]) < 1e-5, m


# ---- the CPU build of the tile arithmetic ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hh():
    return C.CDLL(ge.build_host_harness())


def _hh_svd(hh, p):
    H, W = p.shape
    nby, nbx = H // 8, W // 8
    U = np.empty((nby, nbx, 8, 8), np.float32); S = np.empty((nby, nbx, 8), np.float32); Vt = np.empty((nby, nbx, 8, 8), np.float32)
    p = np.ascontiguousarray(p)
    hh.hh_svd_tiles_f32(vp(p), vp(U), vp(S), vp(Vt), H, W, W)
    return U, S, Vt


@pytest.mark.parametrize("H,W", TILE_SIZES + [(512, 512)])
def test_cpu_build_of_the_tile_svd_meets_the_tile_bars(hh, H, W):
    worst = {}
    for cls in wp.CLASSES:
        p = wp.generate(cls, H, W)
        m = wp.check_tiles(p, *_hh_svd(hh, p))
        for k in ("dS", "unsorted", "orthU", "orthV", "recon", "roundtrip"):
            worst[k] = max(worst.get(k, -1e9), m[k])
    print((H, W), worst)


# ---- the generated V stream --------------------------------------------------------------------------------------
def _completion_pattern():
    text = open(os.path.join(ROOT, "digital-watermarking-for-image-video-using-dct-svd-singular-value-decomposition_amd",
                             "csrc", "wm_tile_math.h")).read()
    body = text.split("COMPLETION_PATTERN[8][8] = {", 1)[1].split("};", 1)[0]
    v = np.array([float(x) for x in re.findall(r"[-+]\d+\.\d+", body)], np.float32)
    assert v.size == 64
    return v.reshape(8, 8)


def _logo_wave():
    """64 DCT tiles drawn from the logo classes: full-rank and rank-deficient ones in one wave"""
    tiles = []
    for cls in ("noise", "binary50", "three_level", "white_5pct_black", "two_adjacent", "unscrambled_logo", "zero",
                "near_singular_tiles"):
        t = wp.to_tiles(wp.generate(cls, 64, 64)).reshape(-1, 8, 8)
        tiles += list(t[:: len(t) // 8][:8])
    t = np.stack(tiles).astype(np.float32)
    from scipy.fft import dctn
    return dctn(t, axes=(-2, -1), norm="ortho").astype(np.float32)


@pytest.mark.parametrize("with_pattern", [False, True])
def test_generated_v_stream_on_a_wave_of_logo_tiles(with_pattern):
    import emu_jacobi_asm as emu
    t = _logo_wave()
    ref0 = np.linalg.svd(t.astype(np.float64), compute_uv=False)
    deficient = ref0[:, 7] <= 1e-5 * ref0[:, 0]
    assert 16 <= deficient.sum() <= 48                               # the wave mixes both kinds
    if with_pattern:
        t = (t + np.float32(wp.DELTA) * _completion_pattern()).astype(np.float32)
    b, v, n2, vn2, more, sweeps = emu.run_v(t, 1e-7)
    assert not np.any(more) and 3 <= sweeps <= 9
    assert all(np.isfinite(x).all() for x in (b, v, n2, vn2))
    ref = np.linalg.svd(t.astype(np.float64), compute_uv=False)
    s = np.sqrt(np.maximum(n2, 0)) / np.sqrt(vn2)
    scale = np.maximum(ref[:, :1], 1e-30)
    assert np.max(np.abs(s - ref) / scale) < 2e-6
    assert np.all(np.diff(s, axis=1) <= 2e-6 * scale)                                   # descending (de Rijk)
    t64, v64 = t.astype(np.float64), v.astype(np.float64)
    assert np.max(np.abs(np.einsum("nrk,nkc->nrc", t64, v64) - b) / np.maximum(scale[:, :, None], 1.0)) < 2e-6   # B = A V
    assert np.max(np.abs(np.einsum("nkc,nkd->ncd", v64, v64) - np.eye(8))) < 1e-5         # V orthogonal
    gram = np.einsum("nrc,nrd->ncd", b.astype(np.float64), b.astype(np.float64))
    off = np.abs(gram - gram * np.eye(8)).max(axis=(1, 2))
    assert np.max(off / np.maximum(ref[:, 0] ** 2, 1e-30)) < 1e-6
    # a lane's result does not depend on its wave neighbours
    k = int(np.nonzero(deficient)[0][0])
    b1, v1, n21, _, _, _ = emu.run_v(t[k:k + 1], 1e-7)
    assert np.array_equal(b1[0], b[k]) and np.array_equal(v1[0], v[k]) and np.array_equal(n21[0], n2[k])
