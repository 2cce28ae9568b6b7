"""Plain references and input builders for the pixel-side edge tests (tests/test_gpu_pixel_edges.py; checked on their own,
without a GPU, by tests/test_pixel_refs.py):

  * permutations that are NOT uniformly random, built so that the cells cnt[a][b] of a route (elements of source block a
    that go to destination block b, blocks of S = 32768) take the values a uniform shuffle never produces: 0, 1, S and
    n mod S;
  * the scramble / unscramble of app_dct_svd_single.py:66-80 as NumPy statements;
  * min-max normalise + clip + uint8 (single:221-222) through oracle.normalize_minmax;
  * SSIM (single:44-57) restated in float64 - same taps, same reflect-101 border, same constants - and the flat, saturated
    and two-level images on which float32 moments are weakest;
  * single-entry tile factors that make every tile of an extract estimate one constant, so that on a ragged plane the zero
    border is the only other value of the min / max."""
import math

import numpy as np
import scipy.ndimage

from oracle import wm_oracle as o

LOG_S = 15
S = 1 << LOG_S


# ---- permutations ----------------------------------------------------------------------------------------------------
def n_blocks(n):
    return (n + S - 1) // S


def perm_identity(n):
    return np.arange(n, dtype=np.int64)


def perm_reversal(n):
    return np.arange(n - 1, -1, -1, dtype=np.int64)


def perm_rotation(n, r):
    """i -> (i + r) mod n"""
    return (np.arange(n, dtype=np.int64) + r) % n


def coprime_above(n, lo=S):
    k = lo + 1
    while math.gcd(k, n) != 1:
        k += 1
    return k


def perm_multiply(n):
    """i -> i * k mod n for the first k > S coprime to n"""
    return (np.arange(n, dtype=np.int64) * coprime_above(n)) % n


def perm_block_transpose(nb):
    """n = nb * S: i -> (i mod nb) * S + i // nb"""
    i = np.arange(nb * S, dtype=np.int64)
    return (i % nb) * S + i // nb


def perm_block_local(n, seed=0):
    """a shuffle inside every block of S elements: nothing leaves its block"""
    rng = np.random.default_rng(seed)
    idx = np.empty(n, np.int64)
    for b0 in range(0, n, S):
        m = min(S, n - b0)
        idx[b0:b0 + m] = b0 + rng.permutation(m)
    return idx


def perm_fill_last_block(n):
    """The first n mod S elements of source block 0 fill the last (partial) block completely; the rest of block 0 and
    every other element go elsewhere: onto the full blocks, rotated by S // 2 + 1.  Needs a partial last block behind
    at least one full block."""
    r = n % S
    last = n - r
    assert r and last >= S
    idx = np.empty(n, np.int64)
    idx[:r] = last + np.arange(r)
    idx[r:] = (np.arange(last, dtype=np.int64) + S // 2 + 1) % last
    return idx


def inverse(idx):
    inv = np.empty_like(idx)
    inv[idx] = np.arange(idx.size, dtype=idx.dtype)
    return inv


def is_bijection(idx):
    n = idx.size
    return idx.shape == (n,) and n > 0 and int(idx.min()) == 0 and int(idx.max()) == n - 1 \
        and np.array_equal(np.bincount(idx, minlength=n), np.ones(n, np.int64))


def cell_counts(idx):
    """cnt[a][b] = elements of source block a = i >> 15 whose destination block is b = idx[i] >> 15"""
    nb = n_blocks(idx.size)
    a = np.arange(idx.size, dtype=np.int64) >> LOG_S
    return np.bincount(a * nb + (idx >> LOG_S), minlength=nb * nb).reshape(nb, nb)


def permutations_for(n):
    """(name, index) of every non-uniform permutation that exists at this size"""
    out = [("identity", perm_identity(n)), ("reversal", perm_reversal(n)), ("rot1", perm_rotation(n, 1)),
           ("rotS-1", perm_rotation(n, S - 1)), ("multiply", perm_multiply(n)), ("block-local", perm_block_local(n, n))]
    if n % S == 0 and n > S:
        out.append(("block-transpose", perm_block_transpose(n // S)))
    if n % S and n > S:
        f = perm_fill_last_block(n)
        out += [("fill-last", f), ("fill-last-inverse", inverse(f))]
    return out


ROUTE_SIZES = (1, 2, 15, 16, 17, S - 1, S, S + 1, 2 * S - 1, 2 * S + 1, 3 * S + 5, 4 * S + 16383, 3 * S)


# ---- scramble / unscramble / normalise -------------------------------------------------------------------------------
def scramble(flat, idx):
    """single:66-72 `_permute`: flat[idx] as float32"""
    return flat[idx].astype(np.float32)


def unscramble(flat, idx):
    """single:74-80 `_unpermute`: inv[idx] = arange; flat[inv]"""
    return flat[inverse(idx)]


def normalize_u8(x, do_norm=True):
    """single:221-222: cv2.normalize(NORM_MINMAX) in float32, clip, truncate"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        v = o.normalize_minmax(x) if do_norm else x
    return np.clip(v, 0, 255).astype(np.uint8)


# ---- the one-call extract: estimates whose only other extremum is the zero border ------------------------------------
def single_entry_factors(nby, nbx, sign):
    """Uw[t][0][0] = sign, Vwt[t][0][0] = 1, all else 0: with K = 1 the estimate of tile t is sign * sw_hat[t][0] in its DC
    coefficient alone, one constant over the tile"""
    U = np.zeros((nby, nbx, 8, 8), np.float32)
    V = np.zeros((nby, nbx, 8, 8), np.float32)
    U[..., 0, 0] = sign
    V[..., 0, 0] = 1.0
    return U, V


def grid_mask(H, W):
    m = np.zeros((H, W), bool)
    m[:H // 8 * 8, :W // 8 * 8] = True
    return m


def constant_grid_estimate(H, W, value):
    """what such an extract leaves on a plane of identical tiles: `value` on the tile grid, zeros outside"""
    w = np.zeros((H, W), np.float32)
    w[grid_mask(H, W)] = value
    return w


# ---- SSIM ------------------------------------------------------------------------------------------------------------
def _blur64(img):
    k = o._gauss_kernel().astype(np.float64)        # the float32 taps the reference hands to its filter
    t = scipy.ndimage.correlate1d(img, k, axis=0, mode="mirror")
    return scipy.ndimage.correlate1d(t, k, axis=1, mode="mirror")


def ssim64(img1, img2):
    """oracle.ssim (single:44-57) with every intermediate in float64"""
    a = np.asarray(img1).astype(np.float64)
    b = np.asarray(img2).astype(np.float64)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    mu1, mu2 = _blur64(a), _blur64(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = _blur64(a * a) - mu1_sq
    s2 = _blur64(b * b) - mu2_sq
    s12 = _blur64(a * b) - mu1_mu2
    num = (2 * mu1_mu2 + C1) * (2 * s12 + C2)
    den = (mu1_sq + mu2_sq + C1) * (s1 + s2 + C2) + 1e-12
    return float(np.mean(num / den))


def logo(H, W):
    """two-level artwork on a white background: a disc, a bar and thin strokes, values 0 and 255 only"""
    yy, xx = np.mgrid[:H, :W]
    img = np.full((H, W), 255, np.uint8)
    r = min(H, W) // 3
    img[(yy - H // 2) ** 2 + (xx - W // 3) ** 2 < r * r] = 0
    img[H // 5:H // 5 + max(H // 20, 1), W // 2:W - W // 10] = 0
    img[:, W - W // 8::7] = 0
    return img


def flip_lsbs(img, count, seed):
    out = img.copy().ravel()
    where = np.random.default_rng(seed).choice(out.size, size=min(count, out.size), replace=False)
    out[where] ^= 1
    return out.reshape(img.shape)


def noisy(level, H, W, seed):
    """float32 plane at a flat level with noise of sigma 0.3 (the float Yw of a gray-mode embed on a flat cover)"""
    return (np.float32(level) + np.random.default_rng(seed).normal(0, 0.3, (H, W))).astype(np.float32)


def ssim_pairs(H, W):
    """(name, img1 uint8, img2 uint8 or float32): content on which x^2 + y^2 is largest and the variances smallest"""
    yy, xx = np.mgrid[:H, :W]
    white = np.full((H, W), 255, np.uint8)
    lg = logo(H, W)
    chk = np.where(((yy // 4) + (xx // 4)) % 2 == 0, 255, 0).astype(np.uint8)
    return [
        ("white-white", white, white.copy()),
        ("white-254", white, np.full((H, W), 254, np.uint8)),
        ("black-white", np.zeros((H, W), np.uint8), white),
        ("logo-logo", lg, lg.copy()),
        ("logo-lsb", lg, flip_lsbs(lg, 40, 5)),
        ("checker-inverse", chk, (255 - chk).astype(np.uint8)),
        ("white-noisy", white, noisy(255, H, W, 11)),
        ("one-noisy", np.full((H, W), 1, np.uint8), noisy(1, H, W, 12)),
        ("mid-noisy", np.full((H, W), 128, np.uint8), noisy(128, H, W, 13)),
    ]


def ssim_large_pairs(H, W):
    """the white-with-noise and logo pairs of ssim_pairs alone (1080p and 4K)"""
    return [p for p in ssim_pairs(H, W) if p[0] in ("white-noisy", "logo-logo", "logo-lsb")]


def dtype_combinations(a, b):
    """every uint8 / float32 combination k_ssim instantiates that represents the pair without changing a value: a uint8
    image also goes in as float32; a float32 image stays float32"""
    out = []
    for x in ((a, a.astype(np.float32)) if a.dtype == np.uint8 else (a,)):
        for y in ((b, b.astype(np.float32)) if b.dtype == np.uint8 else (b,)):
            out.append((x, y))
    return out
