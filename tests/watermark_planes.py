"""Watermark-side inputs and float64 references (no GPU, no project code).

The reference is a LOGO watermarking program: the planes the watermark-side SVDs see are binary, flat, few-level or
nearly blank images whose pixels the keyed permutation shuffles around - not ``rng.integers(0, 256)`` noise.  This
module holds seeded generators of such scrambled planes and two checkers that hold a decomposition (U, S, Vt) to
float64 ``scipy.fft.dctn(norm='ortho')`` + ``np.linalg.svd``:

  check_tiles  - per 8x8 tile  (wm_svd_tiles_f32, the CPU build of the same arithmetic, float32 LAPACK)
  check_plane  - one full-frame plane (wm_ref_svd[_planes]_f32, float32 LAPACK)

Each checker returns the quantities it measured and asserts its bars; the bars are the ones the suite already holds
on noise planes (tests/test_gpu_fullframe.py, tests/test_gpu_parity.py) and, for full-frame orthonormality, the 1e-5
that DESIGN.md 9.3 claims.
"""
from functools import lru_cache

import numpy as np
from scipy.fft import dctn, idctn

DELTA = 2.0 ** -14          # the tile kernels' completion scale (csrc/wm_tile_math.h COMPLETION_DELTA)

CLASSES = ("noise", "binary50", "white_5pct_black", "black_5pct_white", "three_level", "two_adjacent", "antialiased",
           "sparse_marks", "blank255", "zero", "unscrambled_logo", "near_singular_tiles")
# classes whose 8x8 tiles are (almost) all rank deficient / whose full plane is rank deficient
DEFICIENT_PLANE = ("sparse_marks", "blank255", "zero", "unscrambled_logo")


def _seed(cls, H, W, seed):
    return [CLASSES.index(cls), H, W, seed]


def _scramble(img, rng):
    """a seeded permutation of the flat plane, as the oracle's ``permute`` does (flat[idx])"""
    idx = rng.permutation(img.size)
    return img.reshape(-1)[idx].reshape(img.shape)


@lru_cache(maxsize=None)
def _near_singular_pool(n_want=48, seed=5):
    """full-rank uint8 tiles with s8 / s1 in [1e-5, 1e-3] (found among random tiles, as _one_small_tiles of
    tests/test_host_harness.py finds its near-singular ones)"""
    rng = np.random.default_rng(seed)
    found = []
    while len(found) < n_want:
        t = rng.integers(0, 256, (20000, 8, 8)).astype(np.float64)
        s = np.linalg.svd(t, compute_uv=False)
        r = s[:, 7] / s[:, 0]
        found += [x.astype(np.uint8) for x in t[(r >= 1e-5) & (r <= 1e-3)]]
    return np.stack(found[:n_want])


def near_singular_mask(H, W):
    """[nby, nbx] bool: where ``near_singular_tiles`` places its near-singular tiles (every third tile)"""
    nby, nbx = H // 8, W // 8
    return (np.arange(nby * nbx) % 3 == 0).reshape(nby, nbx)


def generate(cls, H, W, seed=0):
    """scrambled plane (H, W) float32 with integer values in 0..255 of the logo class ``cls``"""
    rng = np.random.default_rng(_seed(cls, H, W, seed))
    n = H * W
    if cls == "noise":
        img = rng.integers(0, 256, (H, W))
    elif cls == "binary50":
        img = np.where(np.arange(n) < n // 2, 0, 255).reshape(H, W)
    elif cls == "white_5pct_black":
        img = np.where(np.arange(n) < max(1, round(0.05 * n)), 0, 255).reshape(H, W)
    elif cls == "black_5pct_white":
        img = np.where(np.arange(n) < max(1, round(0.05 * n)), 255, 0).reshape(H, W)
    elif cls == "three_level":
        a, b = round(0.1 * n), round(0.2 * n)
        i = np.arange(n)
        img = np.where(i < a, 0, np.where(i < b, 128, 255)).reshape(H, W)
    elif cls == "two_adjacent":
        img = np.where(np.arange(n) < n // 2, 254, 255).reshape(H, W)
    elif cls == "antialiased":
        yy, xx = np.mgrid[0:H, 0:W]
        f = 127.5 + 127.5 * np.tanh(3.0 * np.sin(xx / (0.11 * W + 1.0) + 0.3) * np.cos(yy / (0.13 * H + 1.0)))
        img = np.clip(np.rint(f), 0, 255).astype(np.int64)
    elif cls == "sparse_marks":
        img = np.full(n, 255)
        img[:min(40, n // 2)] = rng.integers(0, 64, min(40, n // 2))
        img = img.reshape(H, W)
    elif cls == "blank255":
        return np.full((H, W), 255.0, np.float32)
    elif cls == "zero":
        return np.zeros((H, W), np.float32)
    elif cls == "unscrambled_logo":
        img = np.full((H, W), 255)
        img[H // 4: H // 4 + max(1, H // 8), W // 8: W - W // 8] = 0          # a horizontal bar
        img[H // 8: H - H // 8, W // 3: W // 3 + max(1, W // 10)] = 0          # a vertical bar
        return img.astype(np.float32)                                          # NOT scrambled: constant / rank-1 tiles
    elif cls == "near_singular_tiles":
        img = rng.integers(0, 256, (H, W))
        pool = _near_singular_pool()
        m = near_singular_mask(H, W)
        k = 0
        for by, bx in zip(*np.nonzero(m)):
            img[8 * by: 8 * by + 8, 8 * bx: 8 * bx + 8] = pool[k % len(pool)]
            k += 1
        return img.astype(np.float32)                                          # tiles must stay tiles: not scrambled
    else:
        raise KeyError(cls)
    return _scramble(img, rng).astype(np.float32)


# ---- float64 references ------------------------------------------------------------------------------------------
def to_tiles(plane):
    """(H, W) -> [nby, nbx, 8, 8] of the full 8x8 tiles"""
    H, W = plane.shape
    nby, nbx = H // 8, W // 8
    return plane[:8 * nby, :8 * nbx].reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3)


def tile_dct64(plane):
    return dctn(to_tiles(np.asarray(plane, np.float64)), axes=(-2, -1), norm="ortho")


def tile_svals64(plane):
    return np.linalg.svd(tile_dct64(plane), compute_uv=False)


def deficient_tiles(plane):
    """[nby, nbx] bool: the tile's 8th singular value is at most 1e-5 of its first (the kernels' completion criterion)"""
    s = tile_svals64(plane)
    return s[..., 7] <= 1e-5 * s[..., 0]


def plane_rank(plane):
    s = np.linalg.svd(np.asarray(plane, np.float64), compute_uv=False)
    return int(np.sum(s > 1e-9 * max(s[0], 1e-300))) if s[0] > 0 else 0


def lapack_f32_tiles(plane):
    """float32 LAPACK on the float32 DCT tiles: the reference's own arithmetic"""
    C = dctn(to_tiles(np.asarray(plane, np.float32)), axes=(-2, -1), norm="ortho").astype(np.float32)
    return np.linalg.svd(C)


def lapack_f32_plane(plane, apply_dct=True):
    C = dctn(np.asarray(plane, np.float32), norm="ortho").astype(np.float32) if apply_dct else np.asarray(plane, np.float32)
    return np.linalg.svd(C, full_matrices=False)


# ---- checkers ----------------------------------------------------------------------------------------------------
def check_tiles(plane, U, S, Vt, completed_by_pattern=True):
    """U [nby, nbx, 8, 8], S [nby, nbx, 8], Vt [nby, nbx, 8, 8] of the DCT tiles of ``plane`` against float64.
    ``completed_by_pattern``: the decomposition under test completes rank-deficient tiles with delta x pattern (the
    project's tile kernels); float32 LAPACK does not, and then no tile gets the delta allowances."""
    plane = np.asarray(plane, np.float64)
    C = tile_dct64(plane)
    assert U.shape == C.shape and Vt.shape == C.shape and S.shape == C.shape[:-1]
    assert np.isfinite(U).all() and np.isfinite(S).all() and np.isfinite(Vt).all()
    assert (S >= 0).all()
    U64, S64, Vt64 = (np.asarray(a, np.float64) for a in (U, S, Vt))
    s64 = np.linalg.svd(C, compute_uv=False)
    sig1 = np.maximum(s64[..., 0], 1.0)
    comp = (s64[..., 7] <= 1e-5 * s64[..., 0]) & completed_by_pattern
    d = DELTA * comp
    m = {"tiles": int(comp.size), "completed": int(comp.sum())}

    ds = np.abs(S64 - s64).max(-1)
    m["dS"] = float(((ds - 4 * d) / sig1).max())
    assert m["dS"] <= 2e-6, ("singular values", m["dS"])

    up = np.diff(S64, axis=-1).max(-1)                       # S[i+1] - S[i]: how far it is from descending
    m["unsorted"] = float(((up - 4 * DELTA * completed_by_pattern) / sig1).max())
    assert m["unsorted"] <= 2e-6, ("order", m["unsorted"])

    I = np.eye(8)
    m["orthU"] = float(np.abs(np.swapaxes(U64, -1, -2) @ U64 - I).max())
    m["orthV"] = float(np.abs(Vt64 @ np.swapaxes(Vt64, -1, -2) - I).max())
    assert m["orthU"] < 1e-5 and m["orthV"] < 1e-5, ("orthonormality", m["orthU"], m["orthV"])

    rec = (U64 * S64[..., None, :]) @ Vt64
    e = np.abs(rec - C).max((-1, -2))
    m["recon"] = float(((e - d) / sig1).max())
    assert m["recon"] <= 2e-6, ("U diag(S) Vt against the DCT tile", m["recon"])

    px = idctn(rec, axes=(-2, -1), norm="ortho")
    t = to_tiles(plane)
    m["roundtrip"] = float(np.abs(px - t).max())
    assert m["roundtrip"] <= 2e-3, ("pixel round trip", m["roundtrip"])
    assert np.array_equal(np.rint(px), t)
    return m


def check_plane(plane, U, S, Vt, apply_dct=True, orth_bar=None):
    """U [H, L], S [L], Vt [L, W] of dct2(plane) (or of the plane itself) against float64."""
    plane = np.asarray(plane, np.float64)
    H, W = plane.shape
    L = min(H, W)
    C = dctn(plane, norm="ortho") if apply_dct else plane
    assert U.shape == (H, L) and S.shape == (L,) and Vt.shape == (L, W), (U.shape, S.shape, Vt.shape)
    assert np.isfinite(U).all() and np.isfinite(S).all() and np.isfinite(Vt).all()
    if orth_bar is None:
        orth_bar = 1e-5          # DESIGN 9.3's claim; measured <= 5.3e-6 on every class up to 1080p (the suite's noise bars are 1e-4 / 2e-4)
    U64, S64, Vt64 = (np.asarray(a, np.float64) for a in (U, S, Vt))
    s64 = np.linalg.svd(C, compute_uv=False)
    sig1 = float(s64[0])
    m = {"L": L, "rank": int(np.sum(s64 >= 1e-9 * sig1)) if sig1 > 0 else 0}
    assert (np.diff(S64) <= 0).all(), "S is not descending"
    rec = (U64 * S64) @ Vt64
    if sig1 == 0.0:                                           # the zero plane: absolute bars
        m["dS"] = float(np.abs(S64).max())
        m["recon"] = float(np.abs(rec).max())
        assert m["dS"] <= 1e-6 and m["recon"] <= 1e-6, (m["dS"], m["recon"])
    else:
        null = s64 < 1e-9 * sig1
        m["dS"] = float((np.abs(S64 - s64)[~null] / sig1).max())
        m["null"] = float((S64[null] / sig1).max()) if null.any() else 0.0
        assert m["dS"] <= 2e-6, ("singular values", m["dS"])
        assert m["null"] <= 3e-5, ("null singular values", m["null"])
        m["recon"] = float(np.abs(rec - C).max() / sig1)
        assert m["recon"] <= 2e-5, ("U diag(S) Vt against the plane", m["recon"])
    m["orthU"] = float(np.abs(U64.T @ U64 - np.eye(L)).max())
    m["orthV"] = float(np.abs(Vt64 @ Vt64.T - np.eye(L)).max())
    assert m["orthU"] < orth_bar, ("U^T U - I over all L columns", m["orthU"])
    assert m["orthV"] < orth_bar, ("Vt Vt^T - I over all L rows", m["orthV"])
    return m
