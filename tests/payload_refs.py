"""Blind payload (sigma_1 quantisation): the NumPy restatement of the rule as include/wmhip.h states it, composed from the
unchanged oracle (oracle/wm_oracle.py: to_tiles, _dct_tiles, np.linalg.svd, from_tiles, stego_sigma, embed_plane's clip and
truncation to uint8), the seeded hosts of tests/mask_refs.py, an edge host, a host of tiles pinned by clipping, a "document"
page and letterboxed planes.  Shared by tests/test_payload.py (CPU), tests/test_gpu_payload.py and
tests/test_gpu_payload_edges.py; nothing here touches the product.

    embed   q = 2 delta rint((s_1 - b delta) / (2 delta)) + b delta;  if q + 4 > 2040: q -= 2 delta;
            up to 3 times: if q < s_2 + delta: q += 2 delta;  sigma_w_eff = (q + 4 - s_1, 0, ..), alpha = 1, K = 1
    decode  x = s~_1 * (1 / (2 delta));  f = x - floor(x);  m = 2 |2 f - 1| - 1;  soft[j] = sum of m;  bit = soft < 0
(all float32 but the float64 sums; for the deltas used here - 8, 12, 16, 24, 200, 512 - 2 delta * k is an integer below
2^24, exact in float32, so the rule's fused multiply-add and NumPy's separate multiply and add agree)
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


PINNED = (16, 128)
DOCUMENT = (128, 256)
EDGE_DELTAS = (8.0, 12.0, 16.0, 24.0, 200.0, 512.0)


@functools.lru_cache(maxsize=None)
def _pinned_tiles() -> dict:
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:8, 0:8]
    z = lambda: np.zeros((8, 8), int)
    w = lambda: np.full((8, 8), 255)
    tiles = {}
    tiles["checker_0_255"] = ((yy + xx) % 2) * 255
    tiles["checker_255_0"] = ((yy + xx + 1) % 2) * 255
    tiles["half_left_255"] = np.where(xx < 4, 255, 0)
    tiles["half_right_255"] = np.where(xx < 4, 0, 255)
    tiles["half_top_255"] = np.where(yy < 4, 255, 0)
    tiles["half_bottom_255"] = np.where(yy < 4, 0, 255)
    tiles["half_255_200"] = np.where(xx < 4, 255, 200)
    tiles["checker_255_200"] = np.where((yy + xx) % 2 == 0, 255, 200)
    tiles["blockdiag_4_4"] = np.where((yy < 4) == (xx < 4), 255, 0)
    tiles["blockdiag_6_2"] = np.where((yy < 6) == (xx < 6), 255, 0)
    tiles["checker_230_255"] = np.where((yy + xx) % 2 == 0, 230, 255)
    tiles["ramp_200_8x"] = np.minimum(200 + 8 * xx, 255)
    tiles["ramp_200_8y"] = np.minimum(200 + 8 * yy, 255)
    t = w(); t[1:7, 3:5] = 0
    tiles["white_vstroke"] = t
    t = w(); t[5:7, 0:6] = 0
    tiles["white_hstroke"] = t
    t = z(); t[2:5, 4:7] = 255
    tiles["black_white_3x3"] = t
    tiles["noise_200_255_a"] = rng.integers(200, 256, (8, 8))
    tiles["noise_200_255_b"] = rng.integers(200, 256, (8, 8))
    tiles["noise_0_30_a"] = rng.integers(0, 31, (8, 8))
    tiles["noise_0_30_b"] = rng.integers(0, 31, (8, 8))
    tiles["binary_noise_a"] = rng.integers(0, 2, (8, 8)) * 255
    tiles["binary_noise_b"] = rng.integers(0, 2, (8, 8)) * 255
    tiles["rows_255_0"] = np.where(yy % 2 == 0, 255, 0)
    tiles["cols_255_0"] = np.where(xx % 2 == 0, 255, 0)
    tiles["white"] = w()
    t = w(); t[0, 0] = 0
    tiles["white_one_black_pixel"] = t
    tiles["ramp_0_8x"] = np.maximum(8 * xx - 24, 0)
    tiles["diag_255"] = np.where(yy == xx, 255, 0)
    tiles["noise_full_range"] = rng.integers(0, 256, (8, 8))
    tiles["rows_255_250"] = np.where(yy % 2 == 0, 255, 250)
    tiles["corner_255"] = np.where((yy < 4) & (xx < 4), 255, 0)
    tiles["white_frame"] = np.where((yy % 7 == 0) | (xx % 7 == 0), 255, 0)
    assert len(tiles) == 32
    return tiles


def pinned_names() -> tuple:
    return tuple(_pinned_tiles())


@functools.lru_cache(maxsize=None)
def pinned_host() -> np.ndarray:
    """32 tiles (16 x 128), one class each (pinned_names(), row-major), most of them pinned by the clip to 0..255 or by the
    truncation: tiles whose sigma_1 the embed cannot move to its target."""
    t = np.stack(list(_pinned_tiles().values())).reshape(2, 16, 8, 8).astype(np.uint8)
    out = np.zeros(PINNED, np.uint8)
    o.from_tiles(t, out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def document_host(H: int, W: int, seed: int) -> np.ndarray:
    """A white page (255) with H W / 300 short black strokes, 2 pixels wide and 3..10 long, half of them horizontal: text-like
    content whose tiles are white with a few clipped pixels - the case of DESIGN 14's limits."""
    rng = np.random.default_rng(seed)
    out = np.full((H, W), 255, np.uint8)
    for _ in range(H * W // 300):
        y, x, n = int(rng.integers(0, H - 2)), int(rng.integers(0, W - 2)), int(rng.integers(3, 11))
        if rng.integers(0, 2):
            out[y:y + 2, x:x + n] = 0
        else:
            out[y:y + n, x:x + 2] = 0
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def letterbox_planes() -> np.ndarray:
    """Three 72 x 100 planes (9 x 12 tiles and a ragged right edge) of mask_refs.planes_of: plane 0 untouched; plane 1 with
    its top two and bottom two tile rows black; plane 2 with its left three tile columns black.  Black tiles exist only at
    plane > 0, at tile indices that differ from plane to plane."""
    p = mr.planes_of(72, 100, 3).copy()
    p[1, :16] = 0; p[1, 56:] = 0
    p[2, :, :24] = 0
    p.setflags(write=False)
    return p


def black_tiles(Y: np.ndarray) -> np.ndarray:
    """bool [nby, nbx]: tiles all of whose 64 pixels are 0"""
    return o.to_tiles(Y).max((-1, -2)) == 0


def edge_hosts():
    """[(name, uint8 plane)]: all_hosts() and the pinned host"""
    return all_hosts() + [("pinned", pinned_host())]


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


# ---- which tiles have a unique restatement, and which of them vote clearly ------------------------------------------
SIGMA_RTOL = 1e-4                                                           # the project's sigma bar (BASELINE.json)
EDGE_BIT_SEEDS = (0, 1)
EDGE_MAP_SEED = 7
CAP_SEEDED, CAP_EDGE = 0.10, 0.50


def tie_tiles(Sc, bits, delta=DELTA):
    """a rounding tie: (s_1 - b delta) / (2 delta) within the sigma bar of a half-integer - either lattice point is right"""
    return tie_distance(Sc, bits, delta) < SIGMA_RTOL * Sc[..., 0] / (2 * delta)


def degenerate_tiles(Sc):
    """s_1 = s_2 to the sigma bar: the leading singular vector is not unique, the stego is compared in its singular values"""
    return (Sc[..., 0] - Sc[..., 1]) <= SIGMA_RTOL * Sc[..., 0]


def slope_bar(delta) -> float:
    """the sigma bar through the metric's slope: |dm| <= 4 / (2 delta) * (1e-4 * 2040)"""
    return 2 * (SIGMA_RTOL * 2040) / float(delta)


def edge_tile_bits(nt: int, seed: int) -> tuple:
    """(bits [nt], tile_bit [nt], order, offs) of the n_bits = n_tiles cases: seeded bits through simple_map(seed 7)"""
    bits = seeded_bits(nt, seed)
    tbi, order, offs = simple_map(nt, nt, seed=EDGE_MAP_SEED)
    return bits, bits[tbi], order, offs


@functools.lru_cache(maxsize=None)
def _margins_cached(key):
    name, delta, seed = key
    hosts = dict(edge_hosts())
    if name.startswith("letterbox"):
        Y = letterbox_planes()[int(name[-1])]
    else:
        Y = hosts[name]
    return margins_of(Y, edge_tile_bits((Y.shape[0] // 8) * (Y.shape[1] // 8), seed)[1], delta)


def margins_of(Y, tile_bits, delta) -> dict:
    """On the restatement alone, per tile of one plane: signed (the margin, +1 right and -1 wrong), tie, deg, comparable
    (no tie, not degenerate, |m| above the slope bar), with the restatement's stego, its cover sigma and the tile bits."""
    nt = (Y.shape[0] // 8, Y.shape[1] // 8)
    tile_bits = np.asarray(tile_bits, np.uint8).reshape(nt)
    ref = embed_ref(Y, tile_bits, delta)
    m = metric_ref(ref["stego"], delta)
    signed = np.where(tile_bits != 0, -m, m)
    # (a black tile is the zero matrix: s_1 = s_2 = 0, but both np.linalg.svd and the payload embed take the flat vector
    # for it by definition, so its stego is unique and it is not counted as degenerate here)
    black = black_tiles(Y)
    tie, deg = tie_tiles(ref["Sc"], tile_bits, delta), degenerate_tiles(ref["Sc"]) & ~black
    comparable = ~tie & ~deg & (np.abs(m) > slope_bar(delta))
    return dict(signed=signed, m=m, tie=tie, deg=deg, black=black, comparable=comparable, stego=ref["stego"], Yw=ref["Yw"],
                Sc=ref["Sc"], tile_bits=tile_bits)


def margins(name: str, delta: float, seed: int) -> dict:
    """margins_of a named host (edge_hosts(), 'letterbox0..2') under the bits of edge_tile_bits(seed); cached"""
    return _margins_cached((name, float(delta), int(seed)))


DOCUMENT_SEED = 1
DOCUMENT_NONCE = bytes([3] * 8)                                             # with password "pw": see test_payload's document test
DOCUMENT_PAYLOADS = (b"id", b"9 bytes!!", bytes(range(56)))                 # 80 bits, 136 bits, 512 bits = n_tiles


def document_votes(Y, bits, tbi, order, offs, delta=DELTA) -> dict:
    """The restatement's decode of its own embed of ``bits`` under a tile-to-bit map: margins_of(Y, bits[tbi]) with soft
    [n_bits], wrong (bits that decode wrongly) and sure: |soft[j]| exceeds what the bit's non-comparable tiles (2 each) and
    the sigma bar (slope_bar per tile) could move it by - a device that follows the rule decodes a sure bit the same way."""
    r = dict(margins_of(Y, np.asarray(bits)[tbi], delta))
    soft = soft_ref(r["m"].reshape(1, -1), order, offs)
    count = np.diff(offs)
    unsure = np.array([np.count_nonzero(~r["comparable"].ravel()[order[offs[j]:offs[j + 1]]]) for j in range(len(count))])
    r.update(soft=soft, count=count, wrong=(soft < 0) != (np.asarray(bits) != 0),
             sure=np.abs(soft) > 2.0 * unsure + count * slope_bar(delta))
    return r


def left_out_cap(name: str) -> float:
    return CAP_EDGE if name in ("edge", "pinned") else CAP_SEEDED
