"""The tile kernels behind the LQ prelude of the Jacobi stream, on the GPU against the NumPy oracle, at the bars of
test_gpu_parity.py: shapes that end a wave on a single lane, fill whole waves, and take the byte path with a ragged
border; noise, smooth, half-flat and checkerboard planes (the flagged-tile kinds must still produce their closed forms)."""
import ctypes as C

import numpy as np
import pytest

from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

SIGMA_RTOL = 1e-4          # test_gpu_parity.py
ALPHA = 0.15


def _planes(H, W, rng):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([
        rng.integers(0, 256, (H, W)),
        np.clip(128 + 70 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 40 * np.sin((xx + 2 * yy) / 91.0) + rng.normal(0, 2, (H, W)), 0, 255),
        np.where(xx < (W // 16) * 8, 200, rng.integers(0, 256, (H, W))),
        (yy + xx) % 2 * 255,
    ]).astype(np.uint8)


def _rel_sigma(a, b):
    a = a.reshape(-1, 8); b = b.reshape(-1, 8)
    return float(np.max(np.abs(a - b) / np.maximum(b[:, :1], 1e-30)))


@pytest.mark.parametrize("H,W,strided", [(8, 520, False), (64, 512, False), (67, 515, True)],
                         ids=["8x520", "64x512", "67x515-unaligned"])
def test_tile_kernels_behind_the_lq_prelude(gpu_ctx, H, W, strided):
    rng = np.random.default_rng(31)
    Hb, Wb = H // 8 * 8, W // 8 * 8
    dense = _planes(H, W, rng)
    wys = rng.integers(0, 256, (H, W)).astype(np.float32)
    Uo, So, Vto = o.watermark_decompose(wys, 8)
    n = dense.shape[0]
    if strided:                                     # base offset and row stride odd: the byte path of every kernel
        big = rng.integers(0, 256, (n, H + 5, W + 12), dtype=np.uint8)
        big[:, 3:3 + H, 5:5 + W] = dense
        rs, ps, off = W + 12, (H + 5) * (W + 12), 3 * (W + 12) + 5
        out_big = np.full_like(big, 7)
        sc = np.empty((n, (H // 8) * (W // 8), 8), np.float32)
        yw = np.zeros((n, H, W), np.float32)          # the ragged border is not written
        vp = lambda a, o_=0: C.c_void_p(a.ctypes.data + o_)
        sw = np.ascontiguousarray(So.reshape(-1, 8))
        gpu_ctx._call("wm_embed_tiles_u8", vp(big, off), vp(sw), vp(out_big, off), vp(sc), vp(yw), n, H, W, rs, ps, 0, ALPHA, 8)
        stego_view = out_big[:, 3:3 + H, 5:5 + W]
        stego = np.ascontiguousarray(stego_view)
        mask = np.ones_like(big, bool); mask[:, 3:3 + H, 5:5 + W] = False
        assert np.all(out_big[mask] == 7)
        sc = sc.reshape(n, H // 8, W // 8, 8)
    else:
        stego, sc, yw = gpu_ctx.embed_tiles(dense, So, ALPHA, want_yw=True)
        stego_view = stego
    gpu_ctx.check_status()                          # WM_OK: no wave hit the sweep bound
    assert np.isfinite(yw).all() and np.isfinite(sc).all()
    assert np.array_equal(stego[:, Hb:], dense[:, Hb:]) and np.array_equal(stego[:, :, Wb:], dense[:, :, Wb:])
    for p in range(n):
        ref = o.embed_plane(dense[p].astype(np.float32), wys, ALPHA, 0.6, 8, wm_svd=(Uo, So, Vto))
        S = ref["Sc"].astype(np.float64)
        # singular values: every tile, flagged ones included (their completion adds up to 4 * 2^-14)
        assert np.max((np.abs(sc[p] - S) - 4 * 2.0 ** -14) / np.maximum(S[..., :1], 1.0)) < 1e-5, p
        ok = S[..., 7] / np.maximum(S[..., 0], 1e-30) > 1e-5          # tiles the fast kernel keeps
        if ok.any():
            assert _rel_sigma(sc[p][ok], ref["Sc"][ok]) < SIGMA_RTOL, p
            m = np.zeros((H, W), bool); m[:Hb, :Wb] = np.kron(ok, np.ones((8, 8), bool))
            d = np.abs(stego[p].astype(int) - ref["stego"].astype(int))
            assert d[m].max() <= 1, p
        if p in (0, 1):
            assert ok.mean() > 0.5, p
        # flagged tiles (flat half, checkerboard, near-singular smooth tiles): the reference's completion is arbitrary;
        # what holds whatever the choice is svd(Yw) = Sc + alpha Sw, and the stego is the truncated Yw
        T = o.to_tiles(yw[p, :Hb, :Wb].astype(np.float64)).reshape(-1, 8, 8)
        want = np.sort(sc[p].reshape(-1, 8).astype(np.float64) + ALPHA * So.reshape(-1, 8), axis=1)[:, ::-1]
        got = np.linalg.svd(T, compute_uv=False)
        assert np.max(np.abs(got - want) / np.maximum(want[:, :1], 1.0)) < 5e-4, p
        assert np.array_equal(stego[p, :Hb, :Wb], np.clip(yw[p, :Hb, :Wb], 0, 255).astype(np.uint8)), p
    # sigma-only kernels on the stego, against the oracle on the same bytes
    sig = gpu_ctx.sigma_tiles(stego_view)
    w = gpu_ctx.extract_tiles(stego_view, sc, Uo, Vto, ALPHA)
    scores = gpu_ctx.detect_tiles(stego_view, sc, So, ALPHA)
    gpu_ctx.check_status()
    assert np.all(w[:, Hb:] == 0) and np.all(w[:, :, Wb:] == 0)
    for p in range(n):
        sref = o.stego_sigma(stego[p].astype(np.float32), 8)
        assert _rel_sigma(sig[p], sref) < SIGMA_RTOL, p
        wo = o.extract_plane(stego[p].astype(np.float32), sc[p], Uo, Vto, ALPHA, 0.6, H, W, 8)
        assert np.abs(w[p] - wo).max() < 2e-2, p
        sh = (sref - sc[p]) / ALPHA
        if np.std(sh) < 1e-2:                        # NC of a constant vector is 0 / 0
            assert abs(scores[p]) < 1.0 + 1e-9
        else:
            assert abs(scores[p] - o.detect_plane(stego[p].astype(np.float32), sc[p], So, ALPHA, 8)) < (1e-4 if p < 2 else 2e-3), p
