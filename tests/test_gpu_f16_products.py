"""The full-frame extract's finalisation (Uw[:L,:L] diag(sw_hat) Vwt[:L,:L], zero-padded, inverse DCT) on the split-f16
k_hgemm (WM_RF_FINAL_F16=1, the default) and on the f32 k_sgemm (=0), against a float64 NumPy reference, where split-f16
arithmetic goes wrong: estimates far from 1 (f16's range and its subnormal lo parts), factors that are not orthonormal,
ragged shapes and truncation lengths, unaligned device pointers, batches whose planes differ in scale, and the embed's
switch between the two products.  The bar is 2e-6 of the reference's range (at 4K 5e-6 for the f32 products, see
test_4k_plane for the f16 ones); wherever the f16 path must not be taken, the two flags give the same bits."""
import numpy as np
import pytest
from scipy.fft import idctn

pytestmark = pytest.mark.gpu

BAR = 2e-6
SCALE_EXPS = (-40, -24, -12, -6, 0, 8, 14, 15, 16, 24, 40)


def _orth(rng, n, k):
    q, _ = np.linalg.qr(rng.normal(size=(n, k)))
    return q.astype(np.float32)


def _factors(rng, H, W):
    """float32 QR factors shaped like the meta's: Uw [H, Lm] with orthonormal columns, Vwt [Lm, W] with orthonormal rows."""
    Lm = min(H, W)
    return _orth(rng, H, Lm), np.ascontiguousarray(_orth(rng, W, Lm).T)


def _spectrum(rng, n):
    """Decaying estimates of both signs, max |.| exactly 1."""
    s = np.exp(-np.linspace(0.0, 6.0, n)) * rng.choice([-1.0, 1.0], n)
    s[0] = 1.0
    return s.astype(np.float32)


def _ref(Uw, sh, Vwt, H, W):
    """float64: idctn(pad(Uw[:L,:L] diag(sh) Vwt[:L,:L]), norm="ortho"), L = len(sh)."""
    L = sh.size
    full = np.zeros((H, W))
    if L:
        full[:L, :L] = (Uw[:L, :L].astype(np.float64) * sh.astype(np.float64)) @ Vwt[:L, :L].astype(np.float64)
    return idctn(full, type=2, norm="ortho")


def _err(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want))) / max(float(np.max(np.abs(want))), 1e-300)


def _flags(monkeypatch, fn):
    """fn() under WM_RF_FINAL_F16=1 and =0 (the library reads it per call)."""
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("WM_RF_FINAL_F16", flag)
        out[flag] = fn()
    return out["1"], out["0"]


def _f16_shape(H, W):
    return H % 4 == 0 and W % 4 == 0 and min(H, W) % 4 == 0


@pytest.mark.parametrize("H,W", [(128, 192), (200, 328)])
def test_estimate_scale_both_ways(gpu_ctx, monkeypatch, H, W):
    """max |sw_hat| from 2^-40 to 2^40: within the bar on both paths, and exactly scale invariant -
    reconstruct(sh 2^k) == reconstruct(sh) 2^k bit for bit, which needs a power-of-two normalisation in both directions."""
    rng = np.random.default_rng(H + W)
    Uw, Vwt = _factors(rng, H, W)
    base = _spectrum(rng, min(H, W))
    want = _ref(Uw, base, Vwt, H, W)
    runs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("WM_RF_FINAL_F16", flag)
        runs[flag] = {k: gpu_ctx.ref_reconstruct(Uw, np.ldexp(base, k), Vwt, H, W) for k in SCALE_EXPS}
    for flag, got in runs.items():
        for k in SCALE_EXPS:
            assert np.isfinite(got[k]).all(), (flag, k)
            assert _err(got[k], want * 2.0 ** k) <= BAR, (flag, k, _err(got[k], want * 2.0 ** k))
            assert np.array_equal(got[k], np.ldexp(got[0], k)), (flag, k)
    # orthonormal factors on an aligned shape do take the f16 products
    assert not np.array_equal(runs["1"][0], runs["0"][0])


@pytest.mark.parametrize("H,W", [(128, 192), (200, 328)])
def test_factors_that_are_not_orthonormal(gpu_ctx, monkeypatch, H, W):
    """Uw or Vwt scaled by 2^j, normal(0, 1) factors and rank-one factors with unit rows / columns (whose product's columns
    reach sqrt(L) times its entries): finite, and within the bar or bit-identical to the f32 products (fell back)."""
    rng = np.random.default_rng(7 * H + W)
    Lm = min(H, W)
    Uw, Vwt = _factors(rng, H, W)
    cases = {}
    for j in (-8, -4, 4, 8):
        cases[f"Uw*2^{j}"] = (np.ldexp(Uw, j), Vwt)
        cases[f"Vwt*2^{j}"] = (Uw, np.ldexp(Vwt, j))
    cases["normal"] = (rng.normal(0, 1, (H, Lm)).astype(np.float32), rng.normal(0, 1, (Lm, W)).astype(np.float32))
    cases["rank-one"] = (np.full((H, Lm), 1 / np.sqrt(Lm), np.float32), np.full((Lm, W), 1 / np.sqrt(Lm), np.float32))
    base = _spectrum(rng, Lm)
    for name, (U, V) in cases.items():
        for smax in (1e-3, 30.0, 1e4):
            sh = (np.ones(Lm, np.float32) if name == "rank-one" else base) * np.float32(smax)
            a, b = _flags(monkeypatch, lambda: gpu_ctx.ref_reconstruct(U, sh, V, H, W))
            assert np.isfinite(a).all() and np.isfinite(b).all(), (name, smax)
            want = _ref(U, sh, V, H, W)
            assert _err(b, want) <= BAR, (name, smax, _err(b, want))
            assert _err(a, want) <= BAR or np.array_equal(a, b), (name, smax, _err(a, want))


SHAPES = [(4, 388), (388, 4), (8, 30), (30, 8), (32, 36), (36, 130), (130, 36), (30, 126), (124, 252), (252, 124),
          (126, 128), (128, 126), (130, 132), (132, 260), (260, 132), (252, 388), (388, 260)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_and_truncation_lengths(gpu_ctx, monkeypatch, H, W):
    """Ragged 128-tiles and 32-chunks, odd truncation lengths (k_hgemm's partial 16-byte loads), shapes whose strides rule
    the f16 products out (same bits as the f32 ones there)."""
    rng = np.random.default_rng(H * 1000 + W)
    Lm = min(H, W)
    Uw, Vwt = _factors(rng, H, W)
    base = _spectrum(rng, Lm) * np.float32(300.0)
    for Lx in sorted({L for L in (1, 2, 31, 32, 33, Lm - 1, Lm) if 1 <= L <= Lm}):
        sh = base[:Lx]
        a, b = _flags(monkeypatch, lambda: gpu_ctx.ref_reconstruct(Uw, sh, Vwt, H, W))
        want = _ref(Uw, sh, Vwt, H, W)
        assert _err(a, want) <= BAR and _err(b, want) <= BAR, (Lx, _err(a, want), _err(b, want))
        if not _f16_shape(H, W):
            assert np.array_equal(a, b), Lx


def test_4k_plane(gpu_ctx, monkeypatch):
    """The f32 products hold 5e-6 at 4K.  The split-f16 ones do not: their error grows with the corner length (2e-6 of the
    range at Lx = 32 and at 128 x 192, 1e-5 at 1080p, 3.7e-5 here), with orthonormal factors and unchanged by the operand
    scaling; 6e-5 pins that figure until the accumulation is fixed."""
    H, W = 2160, 3840
    rng = np.random.default_rng(2160)
    Uw, Vwt = _factors(rng, H, W)
    sh = _spectrum(rng, H) * np.float32(5e3)
    a, b = _flags(monkeypatch, lambda: gpu_ctx.ref_reconstruct(Uw, sh, Vwt, H, W))
    want = _ref(Uw, sh, Vwt, H, W)
    assert np.isfinite(a).all()
    assert _err(b, want) <= 5e-6, _err(b, want)
    assert _err(a, want) <= 6e-5, _err(a, want)


def test_unaligned_device_factors(gpu_ctx, monkeypatch):
    """Uw / Vwt 4 bytes past a 16-byte boundary cannot feed k_hgemm's 16-byte loads: the f32 products, bit for bit, and the
    aligned call's result within the bar.  (The flag also switches sigma's own product, so the f32 products are formed from
    the estimates of the same sigma by the host entry point under WM_RF_FINAL_F16=0.)"""
    c = gpu_ctx
    n, H, W, alpha = 2, 128, 192, 0.1
    L = min(H, W)
    rng = np.random.default_rng(44)
    Uw, Vwt = _factors(rng, H, W)
    stegos = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    sig = c.ref_sigma_planes(stegos)
    sc = (sig - np.float32(alpha) * (_spectrum(rng, L) * np.float32(50.0))).astype(np.float32)
    ptrs = []
    try:
        d_st = c.malloc(stegos.nbytes); ptrs.append(d_st); c.h2d(d_st, stegos)
        d_sc = c.malloc(sc.nbytes); ptrs.append(d_sc); c.h2d(d_sc, sc)
        d_u = c.malloc(Uw.nbytes + 16); ptrs.append(d_u)
        d_v = c.malloc(Vwt.nbytes + 16); ptrs.append(d_v)
        d_out = c.malloc(n * H * W * 4); ptrs.append(d_out)
        assert d_u % 16 == 0 and d_v % 16 == 0

        def run(off):
            c.h2d(d_u + off, Uw); c.h2d(d_v + off, Vwt)
            c.ref_extract_planes_u8_dev(d_st, d_sc, d_u + off, d_v + off, d_out, n, H, W, W, H * W, alpha, L)
            out = np.empty((n, H, W), np.float32); c.d2h(out, d_out)
            return out
        monkeypatch.setenv("WM_RF_FINAL_F16", "1")
        a4, a0 = run(4), run(0)
        est = ((c.ref_sigma_planes(stegos) - sc) / np.float32(alpha)).astype(np.float32)
        monkeypatch.setenv("WM_RF_FINAL_F16", "0")
        for p in range(n):
            assert np.array_equal(a4[p], c.ref_reconstruct(Uw, est[p], Vwt, H, W)), p
        assert _err(a4, a0.astype(np.float64)) <= BAR
        assert not np.array_equal(a0, a4)               # the aligned call did take the f16 products
    finally:
        for p in ptrs:
            c.free(p)


def test_batched_extract_scales_each_plane(gpu_ctx, monkeypatch):
    """Extract runs the same sigma on the same batch as ref_sigma_planes (under the same flag: it switches sigma's product
    too): sigma_c = that sigma gives exactly zero estimates and an exactly zero plane.  sigma_c = sigma - alpha t, with t on
    scales 1e4, 1 and 1e-3 in one batch, gives estimates known in float32; every plane within the bar of its own range
    (one scale for the batch loses the small plane)."""
    n, H, W, alpha = 3, 128, 192, 0.1
    L = min(H, W)
    K = int(0.6 * L)
    rng = np.random.default_rng(55)
    Uw, Vwt = _factors(rng, H, W)
    stegos = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    t = np.stack([_spectrum(rng, L) * np.float32(s) for s in (1e4, 1.0, 1e-3)])
    for flag in ("1", "0"):
        monkeypatch.setenv("WM_RF_FINAL_F16", flag)
        sig = gpu_ctx.ref_sigma_planes(stegos)
        assert np.all(gpu_ctx.ref_extract_planes(stegos, sig, Uw, Vwt, alpha, K) == 0.0), flag
        sc = (sig - np.float32(alpha) * t).astype(np.float32)
        est = ((sig - sc) / np.float32(max(alpha, 1e-8))).astype(np.float32)      # the host's single:212-213 arithmetic
        est[:, K:] = 0.0
        out = gpu_ctx.ref_extract_planes(stegos, sc, Uw, Vwt, alpha, K)
        for p in range(n):
            want = _ref(Uw, est[p], Vwt, H, W)
            assert _err(out[p], want) <= BAR, (flag, p, _err(out[p], want))


@pytest.mark.parametrize("target", [3e4 * (1 - 2.0 ** -12), 3e4 * (1 + 2.0 ** -12), 1e-6])
def test_embed_product_switch(gpu_ctx, monkeypatch, target):
    """The embed's U diag(alpha sw) V^T takes the split-f16 product while alpha max(sw) < 3e4: just below, just above and far
    below that switch the two flags agree (stego 1 LSB on at most 2e-3 of the pixels, Yw 2e-2 grey levels)."""
    H, W = 200, 328
    L = min(H, W)
    K = int(0.6 * L)
    alpha = np.float32(0.15)
    rng = np.random.default_rng(66)
    hosts = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
    top = np.float32(target / np.float64(alpha))
    sw = np.sort(rng.uniform(0.0, 1.0, L).astype(np.float32) * top)[::-1].copy()
    sw[0] = top
    assert (np.float64(alpha) * np.float64(sw[0]) < 3e4) == (target < 3e4)
    a, b = _flags(monkeypatch, lambda: gpu_ctx.ref_embed_planes(hosts, sw, float(alpha), K, want_yw=True))
    d = np.abs(a[0].astype(int) - b[0].astype(int))
    assert d.max() <= 1 and np.mean(d != 0) <= 2e-3
    assert np.max(np.abs(a[2] - b[2])) < 2e-2
    assert np.max(np.abs(a[1] - b[1])) < 1e-6 * b[1].max()
