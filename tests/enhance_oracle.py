"""NumPy restatement of the reference's extract post-processing chain.  TEST INFRASTRUCTURE ONLY: the product never
imports this file (tests/test_capi.py::test_product_does_not_import_the_oracle holds the same rule for wm_oracle).

What it restates (citations into the reference, ``single`` = app_dct_svd_single.py):

* gray   single:223-227, 88-96:  ``cv2.fastNlMeansDenoising(wy, None, 7, 7, 21)`` then ``_enhance_gray``
  (CLAHE clip 2.0 on 8x8 tiles, then ``addWeighted(e, 1.25, GaussianBlur(e, (0, 0), 1.0), -0.25, 0)``);
* colour single:275-277, 98-110: ``cv2.fastNlMeansDenoisingColored(out, None, 3, 3, 7, 21)`` (LBGR -> Lab, NL-means on L
  and on the interleaved ab pair, Lab -> LBGR) then ``_enhance_color`` (CLAHE on the Y of YCrCb, unsharp with 0.15).

The definitions are OpenCV 4.x's 8-bit algorithms as this project understands them.  OpenCV
cannot run where this suite runs, so bit parity with OpenCV itself is UNPINNED, like the rest of the project's parity
(VERDICT row c).  What IS pinned is the device against this file: every step is integer or f32 with no fused operations,
so the HIP kernels (csrc/wm_enhance.hip, csrc/wm_enhance_math.h) must match it bit for bit.
"""
from __future__ import annotations

import numpy as np

from oracle.wm_oracle import bgr_to_ycrcb, ycrcb_to_bgr

F32 = np.float32
TEMPLATE, SEARCH = 7, 21
BLUR_TAPS = np.array([1, 14, 62, 102, 62, 14, 1], np.int64)      # GaussianBlur sigma 1, 8-bit: 8 fractional bits


# ---- borders -----------------------------------------------------------------------------------------------------
def reflect101(p: np.ndarray, n: int) -> np.ndarray:
    """borderInterpolate(BORDER_REFLECT_101), repeated until the index lands inside (borders wider than the image)."""
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def pad101(img: np.ndarray, top: int, bottom: int, left: int, right: int) -> np.ndarray:
    H, W = img.shape[:2]
    ri = reflect101(np.arange(-top, H + bottom), H)
    ci = reflect101(np.arange(-left, W + right), W)
    return img[ri][:, ci]


# ---- NL-means ----------------------------------------------------------------------------------------------------
def nlm_fpm(search: int = SEARCH) -> int:
    return (2 ** 31 - 1) // (search * search * 255)


def nlm_shift(template: int = TEMPLATE) -> int:
    s = 0
    while (1 << s) < template * template:
        s += 1
    return s


def nlm_weights(h: float, channels: int, template: int = TEMPLATE, search: int = SEARCH) -> np.ndarray:
    """Non-zero prefix of the weight table indexed by ad = ssd >> shift, plus one trailing 0 (int64)."""
    fpm = nlm_fpm(search)
    shift = nlm_shift(template)
    mult = (1 << shift) / (template * template)
    h2 = float(F32(h) * F32(h))
    n_all = int(255 * 255 * channels / mult + 1)
    ad = np.arange(n_all, dtype=np.float64)
    w = np.rint(fpm * np.exp(-(ad * mult) / (h2 * channels))).astype(np.int64)
    w[w < 0.001 * fpm] = 0
    n = int(np.argmax(w == 0)) if (w == 0).any() else n_all
    return np.concatenate([w[:n], [0]]).astype(np.int64)


def nlmeans(img: np.ndarray, h: float, template: int = TEMPLATE, search: int = SEARCH) -> np.ndarray:
    """fastNlMeansDenoising on u8 [H, W] (1 channel) or [H, W, 2] (2 interleaved channels), L2 distance."""
    img = np.asarray(img, np.uint8)
    x = img[..., None] if img.ndim == 2 else img
    H, W, ch = x.shape
    tr, sr = template // 2, search // 2
    B = sr + tr
    ext = pad101(x, B, B, B, B).astype(np.int64)
    lut = nlm_weights(h, ch, template, search)
    n_nz = len(lut) - 1
    shift = nlm_shift(template)
    Ht, Wt = H + 2 * tr, W + 2 * tr                    # template-extended output region
    cen = ext[sr:sr + Ht, sr:sr + Wt]
    est = np.zeros((H, W, ch), np.int64)
    wsum = np.zeros((H, W), np.int64)
    for dy in range(-sr, sr + 1):
        for dx in range(-sr, sr + 1):
            nb = ext[sr + dy:sr + dy + Ht, sr + dx:sr + dx + Wt]
            d = ((cen - nb) ** 2).sum(axis=2)
            c = np.cumsum(np.cumsum(np.pad(d, ((1, 0), (1, 0))), axis=0), axis=1)
            ssd = c[template:, template:] - c[:-template, template:] - c[template:, :-template] + c[:-template, :-template]
            w = lut[np.minimum(ssd >> shift, n_nz)]
            wsum += w
            est += w[..., None] * ext[B + dy:B + dy + H, B + dx:B + dx + W]
    out = (est + (wsum // 2)[..., None]) // wsum[..., None]
    out = out.astype(np.uint8)
    return out[..., 0] if img.ndim == 2 else out


# ---- CLAHE -------------------------------------------------------------------------------------------------------
def clahe_padded(H: int, W: int, tiles_x: int = 8, tiles_y: int = 8):
    if W % tiles_x == 0 and H % tiles_y == 0:
        return H, W
    return H + tiles_y - H % tiles_y, W + tiles_x - W % tiles_x


def clahe_clip_count(clip_limit: float, tile_total: int) -> int:
    """clip_limit * total / 256 (in double), at least 1, saturated at INT_MAX: a count at or above the tile's pixel
    count clips nothing, so a huge clip equals clip <= 0 (OpenCV's int cast is undefined there)."""
    if not clip_limit > 0:
        return 0
    c = float(clip_limit) * tile_total / 256
    if c >= 2 ** 31 - 1:
        return 2 ** 31 - 1
    return max(int(c), 1)


def clahe_clip_hist(hist: np.ndarray, clip: int) -> np.ndarray:
    hist = np.asarray(hist, np.int64).copy()
    if clip <= 0:
        return hist
    clipped = int(np.maximum(hist - clip, 0).sum())
    hist = np.minimum(hist, clip)
    batch = clipped // 256
    residual = clipped - batch * 256
    hist += batch
    if residual:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            hist[i] += 1
            i += step
            residual -= 1
    return hist


def sat_u8(v) -> np.ndarray:
    return np.clip(np.rint(np.asarray(v, F32)), 0, 255).astype(np.uint8)


def clahe_luts(img: np.ndarray, clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8) -> np.ndarray:
    """[tiles_y, tiles_x, 256] u8 LUTs over the padded image."""
    H, W = img.shape
    Hp, Wp = clahe_padded(H, W, tiles_x, tiles_y)
    src = pad101(img, 0, Hp - H, 0, Wp - W)
    th, tw = Hp // tiles_y, Wp // tiles_x
    total = th * tw
    clip = clahe_clip_count(float(F32(clip_limit)), total)      # the C ABI takes clip_limit as a float
    scale = F32(255.0 / total)
    luts = np.empty((tiles_y, tiles_x, 256), np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            t = src[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            hist = clahe_clip_hist(np.bincount(t.ravel(), minlength=256), clip)
            luts[ty, tx] = sat_u8(np.cumsum(hist).astype(F32) * scale)
    return luts


def clahe_axis(n: int, inv_t: np.float32, tiles: int):
    tf = np.arange(n).astype(F32) * inv_t - F32(0.5)
    fl = np.floor(tf)
    a = (tf - fl).astype(F32)
    i1 = fl.astype(np.int64)
    return np.maximum(i1, 0), np.minimum(i1 + 1, tiles - 1), a, (F32(1.0) - a).astype(F32)


def clahe(img: np.ndarray, clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8) -> np.ndarray:
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    Hp, Wp = clahe_padded(H, W, tiles_x, tiles_y)
    th, tw = Hp // tiles_y, Wp // tiles_x
    luts = clahe_luts(img, clip_limit, tiles_x, tiles_y)
    tx1, tx2, xa, xa1 = clahe_axis(W, F32(1.0) / F32(tw), tiles_x)
    ty1, ty2, ya, ya1 = clahe_axis(H, F32(1.0) / F32(th), tiles_y)
    lut = luts.astype(F32)
    v = img.astype(np.int64)
    l11 = lut[ty1[:, None], tx1[None, :], v]
    l12 = lut[ty1[:, None], tx2[None, :], v]
    l21 = lut[ty2[:, None], tx1[None, :], v]
    l22 = lut[ty2[:, None], tx2[None, :], v]
    top = (l11 * xa1[None, :]).astype(F32) + (l12 * xa[None, :]).astype(F32)
    bot = (l21 * xa1[None, :]).astype(F32) + (l22 * xa[None, :]).astype(F32)
    res = (top * ya1[:, None]).astype(F32) + (bot * ya[:, None]).astype(F32)
    return sat_u8(res)


# ---- unsharp -----------------------------------------------------------------------------------------------------
def blur_u8(img: np.ndarray) -> np.ndarray:
    """GaussianBlur(img, (0, 0), 1.0) on u8, reflect-101, per channel: (sum_r k_r (sum_c k_c p) + 2^15) >> 16."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    ext = pad101(img, 3, 3, 3, 3).astype(np.int64)
    rows = sum(BLUR_TAPS[k] * ext[:, k:k + W] for k in range(7))
    acc = sum(BLUR_TAPS[k] * rows[k:k + H] for k in range(7))
    return ((acc + 32768) >> 16).astype(np.uint8)


def unsharp(img: np.ndarray, amount: float) -> np.ndarray:
    alpha = F32(1.0 + float(F32(amount)))
    beta = F32(-float(F32(amount)))
    blur = blur_u8(img)
    t = (img.astype(F32) * alpha).astype(F32)
    u = (blur.astype(F32) * beta).astype(F32)
    return sat_u8(t + u)


# ---- Lab (8-bit, linear RGB, D65) --------------------------------------------------------------------------------
def lab_tables():
    """RGB2Lab_b's cube-root table (2^15 fixed point, 3072 entries) and its XYZ rows x 2^12 / white, for B, G, R bytes."""
    i = np.arange(3072)
    x = i.astype(F32) * (F32(1.0) / (F32(255.0) * F32(8.0)))
    lin = (x * F32(7.787)).astype(np.float64) + 0.13793103448275862
    cb = np.cbrt(x.astype(np.float64)).astype(F32).astype(np.float64)
    f = np.where(x < F32(0.008856), lin, cb)
    tab = np.clip(np.rint(32768.0 * f), 0, 65535).astype(np.int64)
    m = np.array([0.412453, 0.357580, 0.180423, 0.212671, 0.715160, 0.072169, 0.019334, 0.119193, 0.950227])
    wp = np.array([0.950456, 1.0, 1.088754])
    C = np.empty(9, np.int64)
    for r in range(3):
        C[r * 3 + 2] = int(np.rint(4096.0 * m[r * 3] / wp[r]))
        C[r * 3 + 1] = int(np.rint(4096.0 * m[r * 3 + 1] / wp[r]))
        C[r * 3 + 0] = int(np.rint(4096.0 * m[r * 3 + 2] / wp[r]))
    return tab, C


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def bgr_to_lab(bgr: np.ndarray) -> np.ndarray:
    tab, C = lab_tables()
    s = bgr.astype(np.int64) * 8
    s0, s1, s2 = s[..., 0], s[..., 1], s[..., 2]
    fX = tab[_descale(s0 * C[0] + s1 * C[1] + s2 * C[2], 12)]
    fY = tab[_descale(s0 * C[3] + s1 * C[4] + s2 * C[5], 12)]
    fZ = tab[_descale(s0 * C[6] + s1 * C[7] + s2 * C[8], 12)]
    Lscale = (116 * 255 + 50) // 100
    Lshift = -((16 * 255 * (1 << 15) + 50) // 100)
    L = _descale(Lscale * fY + Lshift, 15)
    a = _descale(500 * (fX - fY) + 128 * (1 << 15), 15)
    b = _descale(200 * (fY - fZ) + 128 * (1 << 15), 15)
    return np.clip(np.stack([L, a, b], axis=-1), 0, 255).astype(np.uint8)


def lab_inv_coeffs() -> np.ndarray:
    m = np.array([3.240479, -1.53715, -0.498535, -0.969256, 1.875991, 0.041556, 0.055648, -0.204043, 1.057311], F32)
    wp = np.array([0.950456, 1.0, 1.088754], F32)
    C = np.empty(9, F32)
    C[6:9] = m[0:3] * wp
    C[3:6] = m[3:6] * wp
    C[0:3] = m[6:9] * wp
    return C


def lab_to_bgr(lab: np.ndarray) -> np.ndarray:
    C = lab_inv_coeffs()
    li = (lab[..., 0].astype(F32) * (F32(100.0) / F32(255.0))).astype(F32)
    ai = (lab[..., 1].astype(np.int64) - 128).astype(F32)
    bi = (lab[..., 2].astype(np.int64) - 128).astype(F32)
    lthresh = F32(0.008856) * F32(903.3)
    fthresh = F32(7.787) * F32(0.008856) + F32(16.0) / F32(116.0)
    low = li <= lthresh
    y_lo = (li / F32(903.3)).astype(F32)
    fy_lo = (F32(7.787) * y_lo).astype(F32) + F32(16.0) / F32(116.0)
    fy_hi = ((li + F32(16.0)) / F32(116.0)).astype(F32)
    y_hi = ((fy_hi * fy_hi).astype(F32) * fy_hi).astype(F32)
    y = np.where(low, y_lo, y_hi).astype(F32)
    fy = np.where(low, fy_lo, fy_hi).astype(F32)

    def finv(f):
        lo = ((f - F32(16.0) / F32(116.0)).astype(F32) / F32(7.787)).astype(F32)
        hi = ((f * f).astype(F32) * f).astype(F32)
        return np.where(f <= fthresh, lo, hi).astype(F32)
    fx = finv(((ai / F32(500.0)).astype(F32) + fy).astype(F32))
    fz = finv((fy - (bi / F32(200.0)).astype(F32)).astype(F32))

    def row(k):
        v = ((C[k] * fx).astype(F32) + (C[k + 1] * y).astype(F32)).astype(F32) + (C[k + 2] * fz).astype(F32)
        return sat_u8(np.clip(v.astype(F32), F32(0.0), F32(1.0)) * F32(255.0))
    return np.stack([row(0), row(3), row(6)], axis=-1)


# ---- the chains --------------------------------------------------------------------------------------------------
def enhance_gray(wy: np.ndarray) -> np.ndarray:
    """single:223-227 then _enhance_gray (single:88-96)."""
    return unsharp(clahe(nlmeans(wy, 7.0), 2.0), 0.25)


def denoise_color(bgr: np.ndarray) -> np.ndarray:
    """fastNlMeansDenoisingColored(bgr, None, 3, 3, 7, 21)."""
    lab = bgr_to_lab(bgr)
    L = nlmeans(lab[..., 0], 3.0)
    ab = nlmeans(np.ascontiguousarray(lab[..., 1:]), 3.0)
    return lab_to_bgr(np.concatenate([L[..., None], ab], axis=-1))


def enhance_color(bgr: np.ndarray) -> np.ndarray:
    """single:275-277 then _enhance_color (single:98-110)."""
    d = denoise_color(bgr)
    ycc = bgr_to_ycrcb(d).copy()
    ycc[..., 0] = clahe(ycc[..., 0], 2.0)
    return unsharp(ycrcb_to_bgr(ycc), 0.15)


def enhance(img: np.ndarray) -> np.ndarray:
    return enhance_gray(img) if img.ndim == 2 else enhance_color(img)


def nlm_boundary_h(channels: int, cap: int = 2048) -> float:
    """The largest float32 h whose weight table's non-zero prefix fits cap - 1 entries (plus its 0): the kernels keep
    cap = 2048 entries in LDS and refuse any h above this one.  Bisection over float32 bit patterns (the prefix grows
    with h)."""
    def fits(bits):
        return len(nlm_weights(float(np.uint32(bits).view(F32)), channels)) - 1 <= cap - 1
    lo, hi = int(F32(1.0).view(np.uint32)), int(F32(1000.0).view(np.uint32))
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return float(np.uint32(lo).view(F32))
