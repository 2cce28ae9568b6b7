"""Texture-masked strength: the seeded test hosts and the expected values, composed from the unchanged oracle
(oracle/wm_oracle.py) and the rule as include/wmhip.h states it.  Shared by tests/test_mask.py (CPU) and
tests/test_gpu_mask.py; nothing here touches the product.

The rule, for a tile with cover singular values s_1 >= .. >= s_8 (float32) and parameters lo, hi, cut:
    r = sqrt(s_2^2 + .. + s_8^2);  g = clamp((r - lo) / (hi - lo), 0, 1);  G = (1, g, .., g)
    embed    s'_i = s_i + alpha * G_i * sw_i for i < K
    carried  g >= cut
    extract  sw_hat_1 = (s~_1 - s_1) / max(alpha, 1e-8); sw_hat_i = (s~_i - s_i) / (max(alpha, 1e-8) * g) for i >= 2 on
             carried tiles, 0 on the others; then sw_hat_i = 0 for i >= K
    detect   NC over the i = 1 values of all tiles and the i >= 2 values of carried tiles
"""
import functools

import numpy as np

from oracle import wm_oracle as o

MASK = (8.0, 64.0, 0.25)
ALPHA = 0.12
STDS = np.array([0, 0.6, 1.2, 2.5, 5, 10, 20, 40])
HOSTS = ((72, 100, 1), (72, 100, 2), (64, 64, 3))          # 108 tiles (a partial wave, ragged right edge) / one wave


def host(H: int, W: int, seed: int) -> np.ndarray:
    """A ramp whose 8x8 tiles carry noise of std STDS[(3 ty + tx) % 8]: every regime of the gain in one small image."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    nby, nbx = (H + 7) // 8, (W + 7) // 8
    s = STDS[(np.arange(nby)[:, None] * 3 + np.arange(nbx)[None, :]) % 8]
    s = np.kron(s, np.ones((8, 8)))[:H, :W]
    x = 90 + 0.4 * xx + 0.2 * yy + rng.normal(0, 1, (H, W)) * s
    return np.clip(np.round(x), 0, 255).astype(np.uint8)


def gain(Sc, lo, hi):
    """(g [...], G [..., 8]) of cover singular values Sc [..., 8], float32"""
    Sc = np.asarray(Sc, np.float32)
    r = np.sqrt((Sc[..., 1:] ** 2).sum(-1, dtype=np.float32))
    g = np.clip((r - np.float32(lo)) / np.float32(np.float32(hi) - np.float32(lo)), 0, 1).astype(np.float32)
    G = np.ones(Sc.shape, np.float32)
    G[..., 1:] = g[..., None]
    return g, G


def keep(Sc, lo, hi, cut, K=8):
    """(carried [...], keep [..., 8]): what sw_hat = (s~ - s) / max(alpha, 1e-8) is multiplied by"""
    g, _ = gain(Sc, lo, hi)
    carried = g >= np.float32(cut)
    k = np.zeros(np.shape(Sc), np.float32)
    k[..., 0] = 1.0
    with np.errstate(divide="ignore"):
        k[..., 1:] = np.where(carried, np.float32(1.0) / g, np.float32(0.0))[..., None]
    k[..., K:] = 0.0
    return carried, k


def check_preconditions(Sc, mask=MASK):
    """What lets every tile of a test host take part in every comparison (asserted on the oracle's values)."""
    lo, hi, cut = mask
    g, _ = gain(Sc, lo, hi)
    full = Sc[..., 7] > 1e-5 * Sc[..., 0]
    regimes = ((g == 0).sum(), ((g > 0) & (g < cut)).sum(), ((g >= cut) & (g < 1)).sum(), (g == 1).sum())
    assert min(regimes) >= 9, regimes
    assert full[g > 0].all()
    assert np.abs(g - np.float32(cut)).min() > 1e-5
    return regimes


@functools.lru_cache(maxsize=None)
def watermark(H: int, W: int, seed: int = 9):
    """(wy_s, Uw, Sw, Vwt) of a seeded noise watermark, decomposed once"""
    wy_s = np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.float32)
    return (wy_s,) + tuple(o.watermark_decompose(wy_s, 8))


@functools.lru_cache(maxsize=None)
def cover_sigma(H: int, W: int, seed: int):
    return o.stego_sigma(host(H, W, seed).astype(np.float32), 8)


def embed_ref(Y, wm, alpha=ALPHA, mask=MASK):
    """oracle.embed_plane with G o Sw; mask None: the uniform oracle.  wm = (wy_s, Uw, Sw, Vwt)."""
    wy_s, Uw, Sw, Vwt = wm
    Yf = Y.astype(np.float32)
    if mask is None:
        return o.embed_plane(Yf, wy_s, alpha, tile=8, wm_svd=(Uw, Sw, Vwt))
    _, G = gain(o.stego_sigma(Yf, 8), mask[0], mask[1])
    return o.embed_plane(Yf, wy_s, alpha, tile=8, wm_svd=(Uw, (Sw * G).astype(np.float32), Vwt))


def sw_hat_ref(stego, Sc, alpha, mask, K=8):
    """(carried, sw_hat [nby, nbx, 8]) by the rule, sigma of the stego from the oracle"""
    S_cw = o.stego_sigma(stego.astype(np.float32), 8)
    carried, k = keep(Sc, *mask, K=K)
    return carried, ((S_cw - Sc) / np.float32(max(alpha, 1e-8)) * k).astype(np.float32)


def extract_ref(stego, Sc, Uw, Vwt, alpha, mask, K=8):
    """from_tiles(_idct_tiles(Uw diag(sw_hat) Vwt)): the scrambled estimate, float32 [H, W]"""
    _, sh = sw_hat_ref(stego, Sc, alpha, mask, K)
    out = np.zeros(stego.shape, np.float32)
    o.from_tiles(o._idct_tiles(np.matmul(Uw * sh[..., None, :], Vwt).astype(np.float32)), out)
    return out


def detect_ref(stego, Sc, Sw, alpha, mask):
    carried, sh = sw_hat_ref(stego, Sc, alpha, mask)
    m = np.ones(Sw.shape, bool)
    m[..., 1:] = carried[..., None]
    return o.nc(Sw[m], sh[m])


def to_u8(x, normalize=True):
    return np.clip(o.normalize_minmax(x) if normalize else x, 0, 255).astype(np.uint8)


# ---- planes of the test hosts' regimes for batched cases ------------------------------------------------------------
def planes_of(H: int, W: int, n: int) -> np.ndarray:
    """n <= 3 planes with the test hosts' tile statistics: the seeded hosts of that size, then mirror images of the first
    (a mirrored tile has the singular values of the tile it mirrors, so the preconditions carry over)."""
    seeds = [s for h, w, s in HOSTS if (h, w) == (H, W)]
    base = [host(H, W, s) for s in seeds]
    extra = [base[0][:, ::-1], base[0][::-1]]
    return np.ascontiguousarray(np.stack((base + extra)[:n]))


def rel_sigma(a, b) -> float:
    a = a.reshape(-1, 8); b = b.reshape(-1, 8)
    return float(np.max(np.abs(a - b) / np.maximum(b[:, :1], 1e-30)))


def embed_figures(ctx, planes, wms, alpha=ALPHA, mask=MASK) -> dict:
    """Device embed of uint8 planes [n, H, W] against the oracle, uniform and masked: per variant the worst plane's
    sigma_rel (Sc against the oracle's, relative to s_1), max_lsb, share (of differing pixels) and max_dyw (|Yw - Yw_oracle|).
    wms: one (wy_s, Uw, Sw, Vwt) shared by the planes, or a list of one per plane."""
    shared = isinstance(wms, tuple)
    Sw = wms[2] if shared else np.stack([w[2] for w in wms])
    out = {}
    for name, m in (("uniform", None), ("masked", mask)):
        st, sc, yw = ctx.embed_tiles(planes, Sw, alpha, K=8, want_yw=True, mask=m)
        fig = dict(sigma_rel=0.0, max_lsb=0, share=0.0, max_dyw=0.0)
        for p in range(planes.shape[0]):
            ref = embed_ref(planes[p], wms if shared else wms[p], alpha, m)
            d = np.abs(st[p].astype(np.int32) - ref["stego"].astype(np.int32))
            fig["sigma_rel"] = max(fig["sigma_rel"], rel_sigma(sc[p], ref["Sc"]))
            fig["max_lsb"] = max(fig["max_lsb"], int(d.max()))
            fig["share"] = max(fig["share"], float(np.mean(d != 0)))
            fig["max_dyw"] = max(fig["max_dyw"], float(np.abs(yw[p] - ref["Yw"]).max()))
        out[name] = fig
    return out
