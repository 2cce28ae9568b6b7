"""Texture-masked strength: the seeded test hosts and the expected values, composed from the unchanged oracle
(oracle/wm_oracle.py) and the rule as include/wmhip.h states it.  Shared by tests/test_mask.py (CPU) and
tests/test_gpu_mask.py / tests/test_gpu_mask_edges.py; nothing here touches the product.

The rule, for a tile with cover singular values s_1 >= .. >= s_8 (float32) and parameters lo, hi, cut:
    r = sqrt(s_2^2 + .. + s_8^2);  g = clamp((r - lo) / (hi - lo), 0, 1);  G = (1, g, .., g)
    embed    s'_i = s_i + alpha * G_i * sw_i for i < K
    carried  g >= cut
    extract  sw_hat_1 = (s~_1 - s_1) / max(alpha, 1e-8); sw_hat_i = (s~_i - s_i) / (max(alpha, 1e-8) * g) for i >= 2 on
             carried tiles, 0 on the others; then sw_hat_i = 0 for i >= K
    detect   NC over the i = 1 values of all tiles and the i >= 2 values of carried tiles
"""
import functools
import math
from fractions import Fraction

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


# ---- the rule with every operation rounded once to float32 (wm_tile_math.h, mask_gain) ------------------------------
# lo, hi, cut: the default, a low ramp with a small cut (1 / g up to 20), a narrow ramp with cut = 1, a very large hi
RULES = ((8.0, 64.0, 0.25), (0.0, 16.0, 0.05), (2.0, 2.5, 1.0), (8.0, 3.0e38, 0.25))


def _rn32(x: Fraction) -> np.float32:
    """a non-negative rational rounded to the nearest float32, ties to even"""
    if x == 0:
        return np.float32(0.0)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1                                                              # 2^e <= x < 2^(e + 1)
    q = max(e - 23, -149)                                                   # the exponent of one ulp (subnormals: 2^-149)
    return np.float32(math.ldexp(round(x / Fraction(2) ** q), q))          # round(): half to even, an integer <= 2^24


def gain_exact(Sc, lo, hi) -> np.ndarray:
    """g [...] of cover singular values Sc [..., 8] exactly as mask_gain states it: the seven squares added in index order,
    each step RN32(s_i^2 + acc) - one fused multiply-add - in rational arithmetic; sqrt, the subtraction and the division are
    NumPy's float32 operations, which are correctly rounded."""
    Sc = np.asarray(Sc, np.float32)
    rows = Sc.reshape(-1, 8)
    r2 = np.empty(rows.shape[0], np.float32)
    for n, row in enumerate(rows):
        acc = np.float32(0.0)
        for i in range(1, 8):
            s = Fraction(float(row[i]))
            acc = _rn32(s * s + Fraction(float(acc)))
        r2[n] = acc
    g = (np.sqrt(r2) - np.float32(lo)) / (np.float32(hi) - np.float32(lo))
    return np.minimum(np.maximum(g, np.float32(0.0)), np.float32(1.0)).astype(np.float32).reshape(Sc.shape[:-1])


def carried_exact(Sc, lo, hi, cut) -> np.ndarray:
    return gain_exact(Sc, lo, hi) >= np.float32(cut)


def _gain_chain64(Sc, lo, hi):
    """gain_exact's chain with each step computed in float64 and then rounded to float32: a fast stand-in (the double
    rounding is wrong about once in 2^29 steps) that near_cut_rows only SEARCHES with - what it returns is confirmed by
    gain_exact."""
    Sc = np.asarray(Sc, np.float32).astype(np.float64)
    acc = np.zeros(Sc.shape[:-1], np.float32)
    for i in range(1, 8):
        acc = (Sc[..., i] * Sc[..., i] + acc.astype(np.float64)).astype(np.float32)
    g = (np.sqrt(acc) - np.float32(lo)) / (np.float32(hi) - np.float32(lo))
    return np.clip(g, 0, 1).astype(np.float32)


def edge_rows() -> np.ndarray:
    """all-zero, r = lo, r = hi, far above hi, g = 0.5, a tiny r, and a decaying spectrum (for the default rule)"""
    rows = np.zeros((7, 8), np.float32)
    rows[1, :2] = (500, 8); rows[2, :2] = (500, 64); rows[3] = (900, 300, 100, 100, 100, 100, 100, 100)
    rows[4, :2] = (500, 36); rows[5, :2] = (500, 1e-3); rows[6] = (1000, 20, 15, 10, 8, 5, 3, 1)
    return rows


N_NEAR, N_NEAR_SPLIT = 128, 72


@functools.lru_cache(maxsize=None)
def near_cut_rows(lo, hi, cut, seed=17) -> np.ndarray:
    """128 descending Sc rows with s_1 = 500 on the edge of `cut` (a rule with cut < 1):
      * rows 0-2: (500, r, 0, ..) with r such that g is exactly cut, then r one float32 below and one above (the square
        root of a rounded square is exact, so r is s_2 itself);
      * N_NEAR_SPLIT multi-component rows that carried_exact and the pairwise-summing keep() put on different sides;
      * the rest multi-component rows on which the two agree, all within 3e-7 of cut.
    The multi-component rows are random descending 7-vectors scaled to the r of row 0 and rounded to float32."""
    lo32, hi32, cut32 = np.float32(lo), np.float32(hi), np.float32(cut)
    r_eq = np.float32(lo32 + cut32 * (hi32 - lo32))
    for _ in range(64):                                                     # walk to the r whose g is cut itself
        g = (r_eq - lo32) / (hi32 - lo32)
        if g == cut32:
            break
        r_eq = np.nextafter(r_eq, np.float32(np.inf if g < cut32 else 0.0), dtype=np.float32)
    assert (r_eq - lo32) / (hi32 - lo32) == cut32, "no float32 r gives g = cut for this rule"
    single = np.zeros((3, 8), np.float32)
    single[:, 0] = 500.0
    single[:, 1] = (r_eq, np.nextafter(r_eq, np.float32(0.0)), np.nextafter(r_eq, np.float32(np.inf)))
    rng = np.random.default_rng(seed)
    v = -np.sort(-rng.uniform(0.05, 1.0, (8192, 7)), axis=-1)
    v *= float(r_eq) / np.linalg.norm(v, axis=-1, keepdims=True)
    cand = np.concatenate([np.full((v.shape[0], 1), 500.0), v], axis=-1).astype(np.float32)
    split = (_gain_chain64(cand, lo, hi) >= cut32) != keep(cand, lo, hi, cut)[0]
    a, b = cand[split][:N_NEAR_SPLIT], cand[~split][:N_NEAR - 3 - N_NEAR_SPLIT]
    rows = np.concatenate([single, a, b])
    assert rows.shape == (N_NEAR, 8) and np.all(np.diff(rows, axis=-1) <= 0)
    g = gain_exact(rows, lo, hi)
    ce = g >= cut32
    assert g[0] == cut32 and g[1] < cut32 and g[2] > cut32
    assert np.all(ce[3:3 + N_NEAR_SPLIT] != keep(a, lo, hi, cut)[0]) and np.all(ce[3 + N_NEAR_SPLIT:] == keep(b, lo, hi, cut)[0])
    assert np.abs(g.astype(np.float64) - float(cut32)).max() < 3e-7
    assert min(int(ce.sum()), int((~ce).sum())) >= 16
    rows.setflags(write=False)
    return rows


def sw_hat_with(S_cw, Sc, alpha, g, carried, K=8):
    """the rule's sw_hat [..., 8] from given stego singular values, gain and carried set (float64 inside)"""
    k = np.zeros(np.shape(Sc), np.float64)
    k[..., 0] = 1.0
    with np.errstate(divide="ignore"):
        k[..., 1:] = np.where(carried, 1.0 / g.astype(np.float64), 0.0)[..., None]
    k[..., K:] = 0.0
    return ((S_cw.astype(np.float64) - Sc.astype(np.float64)) / max(alpha, 1e-8) * k).astype(np.float32)


def detect_with(S_cw, Sc, Sw, alpha, g, carried) -> float:
    """NC over the i = 1 values of all tiles and the i >= 2 values of the given carried set"""
    sh = sw_hat_with(S_cw, Sc, alpha, g, carried)
    m = np.ones(Sw.shape, bool)
    m[..., 1:] = carried[..., None]
    return o.nc(Sw[m], sh[m])


def near_cut_case(lo, hi, cut):
    """near_cut_rows as the sigma_c [8, 16, 8] of a 64 x 128 plane, a seeded noise plane as the stego (s~_2 - sc_2 is in
    the hundreds), the seeded watermark's Sw, and the detect score of the restatement with carried_exact and with the
    pairwise-summing keep(): (sigma_c, stego, Sw, score_exact, score_pairwise)"""
    sc = near_cut_rows(lo, hi, cut).reshape(8, 16, 8)
    stego = np.random.default_rng(41).integers(0, 256, (64, 128), dtype=np.uint8)
    Sw = watermark(64, 128)[2]
    S = o.stego_sigma(stego.astype(np.float32), 8)
    g = gain_exact(sc, lo, hi)
    gp, _ = gain(sc, lo, hi)
    return (sc, stego, Sw, detect_with(S, sc, Sw, ALPHA, g, g >= np.float32(cut)),
            detect_with(S, sc, Sw, ALPHA, gp, gp >= np.float32(cut)))


# ---- hosts of the edge tests: black and constant tiles, flagged tiles with g > 0 ------------------------------------
def constant_batch() -> np.ndarray:
    """five 64 x 64 planes: black, white, constant 128, host(64, 64, 3), black with one textured tile (row 3, column 5)"""
    p = np.zeros((5, 64, 64), np.uint8)
    p[1] = 255; p[2] = 128; p[3] = host(64, 64, 3)
    p[4, 24:32, 40:48] = np.random.default_rng(23).integers(0, 256, (8, 8), dtype=np.uint8)
    p.setflags(write=False)
    return p


def constant_tiles(Y: np.ndarray) -> np.ndarray:
    """bool [nby, nbx]: tiles whose 64 pixels are equal"""
    t = o.to_tiles(Y)
    return t.max((-1, -2)) == t.min((-1, -2))


def handmade_plane() -> np.ndarray:
    """64 x 64: noise tiles with hand-made rank classes between them, one class per tile row of odd columns - two equal
    rows of noise (rank 7), rank-2 and rank-4 products of noise factors, constant (v > 0), rank-1 non-constant - and in
    the last three tile rows the near-deficient and exactly rank-7 tiles of test_host_harness._one_small_tiles."""
    from test_host_harness import _one_small_tiles
    rng = np.random.default_rng(29)
    t = rng.integers(0, 256, (64, 8, 8), dtype=np.uint8)

    def product(rank):                                                      # integer factors: the rank is exact
        top = int(np.sqrt(255 // rank))
        return (rng.integers(0, top + 1, (8, rank)) @ rng.integers(0, top + 1, (rank, 8))).astype(np.uint8)

    for k in range(1, 40, 2):
        cls = (k // 2) % 5
        if cls == 0:
            t[k, 5] = t[k, 2]
        elif cls == 1:
            t[k] = product(2)
        elif cls == 2:
            t[k] = product(4)
        elif cls == 3:
            t[k] = 40 + 5 * k
        else:
            t[k] = np.outer(rng.integers(1, 16, 8), rng.integers(1, 16, 8))
    near, r7 = _one_small_tiles(n_want=8)
    for k, x in zip(range(41, 64, 2), near + r7[:4]):
        t[k] = x
    p = np.ascontiguousarray(t.reshape(8, 8, 8, 8).transpose(0, 2, 1, 3).reshape(64, 64))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def flagged_hosts() -> dict:
    """name -> uint8 plane: quantised, posterised and natural content of tests/scaled_rotation_inputs.py at 64 x 64 (one
    wave) and 72 x 100 (9 x 12 tiles, a partial wave and a ragged right edge), and the hand-made plane"""
    import scaled_rotation_inputs as inp
    out = {}
    for kind in ("quantised", "posterised", "natural"):
        tl = inp.tiles(kind, 108, 50 + inp.KINDS.index(kind))
        for name, plane in ((f"{kind}_64x64", inp.plane_of(tl, 8, 8)), (f"{kind}_72x100", inp.plane_of(tl, 9, 12, 72, 100))):
            plane.setflags(write=False)
            out[name] = plane
    out["handmade_64x64"] = handmade_plane()
    return out


@functools.lru_cache(maxsize=None)
def flagged_sigma(name: str) -> np.ndarray:
    """the oracle's Sc of a flagged host"""
    return o.stego_sigma(flagged_hosts()[name].astype(np.float32), 8)
