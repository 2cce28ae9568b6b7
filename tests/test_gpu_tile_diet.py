"""The tile kernels on the trimmed streams - the prelude's row norms from the raw bytes (csrc/wm_jacobi_gfx950.inc)
and the sigma-only stream whose columns stay scaled to the end, with
1 / c^2 from one v_rcp_f32 (csrc/wm_jacobi_sigma_gfx950.inc) - against oracle/wm_oracle.py.
Shapes: 8 x 8 (one tile), 64 x 96 (one full wave and a half), 52 x 83 (ragged); K in {3, 8}; noise, smooth, flat plus
gradient, and the tiles that want a swap inside a tested sweep (tests/tile_diet_inputs.py).
Bars: stego within 1 LSB of the oracle where the tile's singular vectors are defined (elsewhere the reference's invariant
svd(Yw) = Sc + alpha Sw, as in tests/test_gpu_scaled_rotation.py), sigma_c within 1e-4 sigma_1, extract with pixel-domain
factors within the 2e-2 of test_gpu_parity.py::test_extract_with_pixel_domain_factors, in-place embed equal to
out-of-place, two identical calls equal bytes, device status 0; the sigma pass hands out the very bits extract works
with, and detect's score is the one those bits give.
Two stated departures from bars that were asked of this test as "1 LSB on all content" and "detect bit for bit":
* A flat tile, a pure gradient and a circulant have zero or repeated singular values, so their singular vectors - and with
  them the oracle's stego, which adds alpha Sw along LAPACK's arbitrary choice of them - are not defined: kernel and oracle
  differ by up to 49 grey levels there (flat_gradient; 11 on the circulant lanes), as they did before these streams
  (k_embed_tiles returns the bytes it returned).  Such tiles are held to what the reference guarantees whatever vectors it
  picks, svd(Yw) = Sc + alpha Sw to 5e-4 sigma_1, the rule of tests/test_gpu_scaled_rotation.py and
  test_gpu_parity.py::test_random_scenes_every_tile_class; the 1 LSB bar holds on every tile with unique vectors.
* Detect hands out one float64 score per plane, reduced on the device in an order of its own, not its sigma: it cannot be
  compared bit for bit with anything on the host.  It is held to the score the sigma pass's bits give (1e-6, one float32
  rounding per value) and to equal bytes over two calls; sigma pass against extract IS bit for bit."""
import os
import sys

import numpy as np
import pytest

from oracle import wm_oracle as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scaled_rotation_inputs as inp  # noqa: E402
import tile_diet_inputs as diet       # noqa: E402

pytestmark = pytest.mark.gpu

ALPHA = 0.15
SHAPES = {"8x8": (1, 1, 8, 8), "64x96": (8, 12, 64, 96), "52x83": (6, 10, 52, 83)}     # (tile rows, tile columns, H, W)
CONTENT = ("noise", "smooth", "flat_gradient", "late_swap")


def _tiles(name, n):
    if name == "noise":
        return inp.tiles("noise", n, 61)
    if name == "smooth":
        return inp.tiles("natural", n, 62)
    if name == "late_swap":
        w = diet.late_swap_wave()
        return np.concatenate([w] * ((n + 63) // 64))[:n]
    rng = np.random.default_rng(63)                         # flat tiles and pure gradients, alternating (rank 1 and 2)
    xx = np.arange(8)[None, None, :]
    t = rng.integers(10, 120, (n, 1, 1)) + (np.arange(n)[:, None, None] % 2) * rng.integers(1, 16, (n, 1, 1)) * xx
    return np.broadcast_to(t, (n, 8, 8)).astype(np.uint8)


_REF = {}


def _case(name, shape, K):
    """host plane, watermark factors and the oracle's embed: computed once per case, shared by the tests, left unchanged"""
    if (name, shape, K) not in _REF:
        nby, nbx, H, W = SHAPES[shape]
        host = inp.plane_of(_tiles(name, nby * nbx), nby, nbx, H, W)
        wys = np.random.default_rng(4321).integers(0, 256, (H, W)).astype(np.float32)
        Uo, So, Vto = o.watermark_decompose(wys, 8)
        ref = o.embed_plane(host.astype(np.float32), wys, ALPHA, 0.0, 8, k_floor=K, wm_svd=(Uo, So, Vto))
        _REF[name, shape, K] = (host, Uo, So, Vto, ref)
    return _REF[name, shape, K]


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", CONTENT)
def test_embed_and_extract_against_the_oracle(gpu_ctx, name, shape, K):
    nby, nbx, H, W = SHAPES[shape]
    host, Uo, So, Vto, ref = _case(name, shape, K)
    stego, sc, yw = gpu_ctx.embed_tiles(host, So, ALPHA, K=K, want_yw=True)
    rel = lambda a, b: float(np.max(np.abs(a.reshape(-1, 8) - b.reshape(-1, 8)) / np.maximum(b.reshape(-1, 8)[:, :1], 1e-30)))
    T = lambda x: x[:8 * nby, :8 * nbx].reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3)
    d = T(np.abs(stego.astype(np.int32) - ref["stego"].astype(np.int32))).max(axis=(2, 3))
    S = np.linalg.svd(T(host).astype(np.float64), compute_uv=False)
    gaps = np.min(-np.diff(S, axis=-1) / np.maximum(S[..., :1], 1e-30), axis=-1)
    unique = (S[..., 7] > 1e-9 * S[..., 0]) & (gaps > 1e-4)
    got = np.linalg.svd(T(yw).astype(np.float64), compute_uv=False)
    aK = np.where(np.arange(8) < K, ALPHA, 0.0)
    want = np.sort(sc.astype(np.float64) + aK * So.astype(np.float64), axis=-1)[..., ::-1]
    inv = float(np.max(np.abs(got - want) / np.maximum(want[..., :1], 1.0)))
    print(f"{name} {shape} K={K}: {int(unique.sum())} of {unique.size} tiles with unique vectors, stego max "
          f"{int(d[unique].max()) if unique.any() else 0} LSB on them ({int(d.max())} on all), sigma_c {rel(sc, ref['Sc']):.2e} "
          f"sigma_1, svd(Yw) {inv:.2e} sigma_1")
    assert not unique.any() or d[unique].max() <= 1
    assert rel(sc, ref["Sc"]) < 1e-4
    assert np.isfinite(yw).all() and inv < 5e-4
    assert np.array_equal(stego[8 * nby:], host[8 * nby:]) and np.array_equal(stego[:, 8 * nbx:], host[:, 8 * nbx:])
    # two identical calls, and the embed in place, give the same bytes
    stego2, sc2, _ = gpu_ctx.embed_tiles(host, So, ALPHA, K=K)
    assert stego2.tobytes() == stego.tobytes() and sc2.tobytes() == sc.tobytes()
    nt = nby * nbx
    dev = {k: gpu_ctx.malloc(n) for k, n in dict(p=host.nbytes, sw=nt * 32, sc=nt * 32, U=nt * 256, V=nt * 256,
                                                 out=H * W * 4, st=host.nbytes).items()}
    try:
        gpu_ctx.h2d(dev["p"], host); gpu_ctx.h2d(dev["sw"], np.ascontiguousarray(So, np.float32))
        gpu_ctx.embed_tiles_u8_dev(dev["p"], dev["sw"], dev["p"], dev["sc"], None, 1, H, W, W, H * W, 0, ALPHA, K)
        inplace, sc3 = np.empty_like(host), np.empty((nt, 8), np.float32)
        gpu_ctx.d2h(inplace, dev["p"]); gpu_ctx.d2h(sc3, dev["sc"])
        assert inplace.tobytes() == stego.tobytes() and sc3.tobytes() == sc.tobytes()
        # extract with pixel-domain factors, on the oracle's stego
        gpu_ctx.h2d(dev["st"], ref["stego"]); gpu_ctx.h2d(dev["sc"], np.ascontiguousarray(ref["Sc"], np.float32).reshape(nt, 8))
        gpu_ctx.h2d(dev["U"], np.ascontiguousarray(Uo.reshape(nt, 8, 8), np.float32))
        gpu_ctx.h2d(dev["V"], np.ascontiguousarray(Vto.reshape(nt, 8, 8), np.float32))
        gpu_ctx.tile_factors_to_pixel_dev(dev["U"], dev["V"], dev["U"], dev["V"], nt)
        outs = []
        for _ in range(2):
            gpu_ctx.extract_tiles_px_u8_dev(dev["st"], dev["sc"], dev["U"], dev["V"], dev["out"], 1, H, W, W, H * W, 0, ALPHA, K)
            w = np.empty((H, W), np.float32); gpu_ctx.d2h(w, dev["out"]); outs.append(w)
        gpu_ctx.check_status()
    finally:
        for q in dev.values():
            gpu_ctx.free(q)
    wo = o.extract_plane(ref["stego"].astype(np.float32), ref["Sc"], Uo, Vto, ALPHA, 0.0, H, W, 8, k_floor=K)
    print(f"    extract (px) max |diff| {float(np.abs(outs[0] - wo).max()):.2e}")
    assert np.abs(outs[0] - wo).max() < 2e-2
    assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", CONTENT)
def test_sigma_pass_extract_and_detect_share_their_sigma(gpu_ctx, name, shape):
    """The three reach the iteration through one device function.  Extract with identity factors, sigma_c = 0, alpha = 1
    and K = 8 writes diag(sigma) into every tile (products with 1 and sums with 0 are exact): the sigma pass must hand
    out those bits.  Detect forms (sigma - sigma_c) / alpha per value in float32 (one rounding of 6e-8, and its own
    choice between a division and a product with 1 / alpha) and reduces over the tiles in float64 in an order of its
    own: its score is held to the one the sigma pass's values give, to 1e-6."""
    nby, nbx, H, W = SHAPES[shape]
    host, Uo, So, Vto, ref = _case(name, shape, 8)
    st = ref["stego"]
    nt = nby * nbx
    sig = gpu_ctx.sigma_tiles(st)
    assert sig.tobytes() == gpu_ctx.sigma_tiles(st).tobytes()
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(8, dtype=np.float32), (nt, 8, 8)))
    dev = {k: gpu_ctx.malloc(n) for k, n in dict(st=st.nbytes, sc=nt * 32, U=nt * 256, V=nt * 256, out=H * W * 4).items()}
    try:
        gpu_ctx.h2d(dev["st"], st); gpu_ctx.h2d(dev["sc"], np.zeros((nt, 8), np.float32))
        gpu_ctx.h2d(dev["U"], eye); gpu_ctx.h2d(dev["V"], eye)
        gpu_ctx.extract_tiles_px_u8_dev(dev["st"], dev["sc"], dev["U"], dev["V"], dev["out"], 1, H, W, W, H * W, 0, 1.0, 8)
        w = np.empty((H, W), np.float32); gpu_ctx.d2h(w, dev["out"])
        gpu_ctx.check_status()
    finally:
        for q in dev.values():
            gpu_ctx.free(q)
    tiles = w[:8 * nby, :8 * nbx].reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3)
    diag = np.ascontiguousarray(np.diagonal(tiles, axis1=2, axis2=3))
    assert diag.tobytes() == np.ascontiguousarray(sig.reshape(nby, nbx, 8)).tobytes()
    scores = gpu_ctx.detect_tiles(st, ref["Sc"], So, ALPHA)
    assert scores.tobytes() == gpu_ctx.detect_tiles(st, ref["Sc"], So, ALPHA).tobytes()
    score = float(scores[0])
    sw_hat = (sig.astype(np.float32).reshape(-1) - np.asarray(ref["Sc"], np.float32).reshape(-1)) / np.float32(ALPHA)
    a64, b64 = np.asarray(So, np.float64).reshape(-1), sw_hat.astype(np.float64)
    a64, b64 = a64 - a64.mean(), b64 - b64.mean()
    want = float(a64 @ b64 / (np.linalg.norm(a64) * np.linalg.norm(b64) + 1e-8))      # oracle.nc, in float64
    sref = o.stego_sigma(st.astype(np.float32), 8)
    rel = float(np.max(np.abs(sig.reshape(-1, 8) - sref.reshape(-1, 8)) / np.maximum(sref.reshape(-1, 8)[:, :1], 1e-30)))
    print(f"{name} {shape}: sigma pass {rel:.2e} sigma_1 from the oracle, detect {score:.9f} (from the sigma pass {want:.9f})")
    assert rel < 1e-4
    assert abs(score - want) < 1e-6
    gpu_ctx.check_status()
