"""Blind payload (sigma_1 quantisation): the NumPy restatement of the rule as include/wmhip.h states it, composed from the
unchanged oracle (oracle/wm_oracle.py: to_tiles, _dct_tiles, np.linalg.svd, from_tiles, stego_sigma, embed_plane's clip and
truncation to uint8), the seeded hosts of tests/mask_refs.py and an edge host.  Shared by tests/test_payload.py (CPU) and
tests/test_gpu_payload.py; nothing here touches the product.

    embed   q = 2 delta rint((s_1 - b delta) / (2 delta)) + b delta;  if q + 4 > 2040: q -= 2 delta;
            up to 3 times: if q < s_2 + delta: q += 2 delta;  sigma_w_eff = (q + 4 - s_1, 0, ..), alpha = 1, K = 1
    decode  x = s~_1 * (1 / (2 delta));  f = x - floor(x);  m = 2 |2 f - 1| - 1;  soft[j] = sum of m;  bit = soft < 0
(all float32 but the float64 sums; for the deltas used here - 8, 16, 24, 512 - the product 2 delta * k is exact, so the
rule's fused multiply-add and NumPy's separate multiply and add agree)
"""
import functools

import numpy as np

import mask_refs as mr
from oracle import wm_oracle as o

F = np.float32
BIAS = F(4.0)
SIGMA_MAX = F(2040.0)
DELTA = 16.0
HOSTS = mr.HOSTS                                                            # (72, 100, 1), (72, 100, 2), (64, 64, 3)
EDGE = (16, 64)


def host(H, W, seed):
    return mr.host(H, W, seed)


@functools.lru_cache(maxsize=None)
def edge_host() -> np.ndarray:
    """16 tiles (16 x 64): constants 0, 1, 2, 64, 127, 128, 192, 253, 254, 255; a {0, 40} checkerboard (s_1 = s_2: the
    s_2 + delta loop); a horizontal ramp 36 x and a vertical one; a single 255 pixel on 0; one 255 row over 250; constant 100."""
    yy, xx = np.mgrid[0:8, 0:8]
    tiles = [np.full((8, 8), v) for v in (0, 1, 2, 64, 127, 128, 192, 253, 254, 255)]
    tiles.append(((yy + xx) % 2) * 40)
    tiles.append(36 * xx)
    tiles.append(36 * yy)
    one = np.zeros((8, 8), int); one[3, 5] = 255
    tiles.append(one)
    row = np.full((8, 8), 250); row[0] = 255
    tiles.append(row)
    tiles.append(np.full((8, 8), 100))
    assert len(tiles) == 16
    t = np.stack(tiles).reshape(2, 8, 8, 8).astype(np.uint8)
    out = np.zeros(EDGE, np.uint8)
    o.from_tiles(t, out)
    out.setflags(write=False)
    return out


def all_hosts():
    """[(name, uint8 plane)]: the three seeded hosts and the edge host"""
    return [(f"{H}x{W}s{seed}", host(H, W, seed)) for H, W, seed in HOSTS] + [("edge", edge_host())]


def seeded_bits(n: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)


# ---- the rule --------------------------------------------------------------------------------------------------------
def target(Sc, bit, delta) -> np.ndarray:
    """q + 4 of every tile: Sc [..., 8] float32, bit [...] of 0 / 1 -> float32 [...]"""
    Sc = np.asarray(Sc, F)
    d = F(delta); two = F(2.0) * d
    s1, s2 = Sc[..., 0], Sc[..., 1]
    b = np.where(np.asarray(bit) != 0, d, F(0.0)).astype(F)
    q = (two * np.rint((s1 - b) / two).astype(F) + b).astype(F)
    q = np.where(q + BIAS > SIGMA_MAX, q - two, q).astype(F)
    for _ in range(3):
        q = np.where(q < s2 + d, q + two, q).astype(F)
    return (q + BIAS).astype(F)


def tie_distance(Sc, bit, delta) -> np.ndarray:
    """how far (s_1 - b delta) / (2 delta) is from a half-integer, float64 [...]: 0 is a rounding tie"""
    Sc = np.asarray(Sc, np.float64)
    x = (Sc[..., 0] - np.where(np.asarray(bit) != 0, float(delta), 0.0)) / (2.0 * float(delta))
    return np.abs(x - np.floor(x) - 0.5)


def sigma_w_eff(Sc, bit, delta) -> np.ndarray:
    Sc = np.asarray(Sc, F)
    eff = np.zeros(Sc.shape, F)
    eff[..., 0] = target(Sc, bit, delta) - Sc[..., 0]
    return eff


def metric(s1, delta) -> np.ndarray:
    s1 = np.asarray(s1, F)
    inv = F(1.0) / (F(2.0) * F(delta))
    x = (s1 * inv).astype(F)
    f = (x - np.floor(x)).astype(F)
    return (F(2.0) * np.abs(F(2.0) * f - F(1.0)) - F(1.0)).astype(F)


@functools.lru_cache(maxsize=None)
def _cover_sigma_cached(key):
    name, = key
    return o.stego_sigma(dict(all_hosts())[name].astype(F), 8)


def cover_sigma(name: str) -> np.ndarray:
    return _cover_sigma_cached((name,))


def embed_ref(Y: np.ndarray, tile_bit, delta=DELTA) -> dict:
    """oracle.embed_plane fed the rule's sigma_w rows with alpha = 1, K = 1 (k_of(8, 0, 1) = 1): clip, truncate to uint8.
    tile_bit: [nby, nbx] or flat.  Returns the oracle's dict (stego, Yw, Sc, ..) with eff added."""
    Yf = Y.astype(F)
    Sc = o.stego_sigma(Yf, 8)
    eff = sigma_w_eff(Sc, np.asarray(tile_bit).reshape(Sc.shape[:2]), delta)
    r = o.embed_plane(Yf, None, 1.0, kfrac=0.0, tile=8, k_floor=1, wm_svd=(None, eff, None))
    assert r["K"] == 1
    r["eff"] = eff
    return r


def metric_ref(stego: np.ndarray, delta=DELTA) -> np.ndarray:
    """m of every tile of a uint8 plane, float32 [nby, nbx], sigma from the oracle"""
    return metric(o.stego_sigma(stego.astype(F), 8)[..., 0], delta)


def soft_ref(m_planes, order, offs) -> np.ndarray:
    """float64 [n_bits]: planes ascending, then the bit's tiles in ascending tile index"""
    m = np.asarray(m_planes, F)
    m = m.reshape(-1, order.size) if m.ndim != 2 or m.shape[-1] != order.size else m
    soft = np.zeros(len(offs) - 1, np.float64)
    for j in range(len(offs) - 1):
        for p in range(m.shape[0]):
            soft[j] += m[p, order[offs[j]:offs[j + 1]]].astype(np.float64).sum()
    return soft


def simple_map(n_tiles: int, n_bits: int, seed: int = 5):
    """a seeded tile-to-bit map with the product's structure (a permutation modulo n_bits) and its CSR inverse, without
    the product: (tile_bit_index, order, offs)"""
    perm = np.random.default_rng(seed).permutation(n_tiles)
    tbi = (perm % n_bits).astype(np.int32)
    order = np.argsort(tbi, kind="stable").astype(np.int32)
    offs = np.concatenate([[0], np.cumsum(np.bincount(tbi, minlength=n_bits))]).astype(np.int32)
    return tbi, order, offs


def check_preconditions(delta=DELTA, floor=0.4) -> float:
    """For both bit values every tile of every host decodes correctly with |m| >= floor, on the restatement alone.
    Returns the worst margin."""
    worst = 1.0
    for name, Y in all_hosts():
        for b in (0, 1):
            nt = (Y.shape[0] // 8, Y.shape[1] // 8)
            m = metric_ref(embed_ref(Y, np.full(nt, b, np.uint8), delta)["stego"], delta)
            signed = m if b == 0 else -m
            assert signed.min() >= floor, (name, b, float(signed.min()), np.argwhere(signed < floor).tolist())
            worst = min(worst, float(signed.min()))
    return worst
