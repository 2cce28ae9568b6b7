"""Blind payload with keyed dither: the NumPy restatement of the rule as include/wmhip.h states it, on top of
tests/payload_refs.py (hosts, bars, caps, the dither-free rule) and the unchanged oracle.  Shared by
tests/test_payload_dither.py (CPU), tests/test_gpu_payload_dither.py and tests/test_gpu_payload_dither_edges.py; nothing here
touches the product.

    offset  d = float(u) * (delta * 2^-15)                      one float32 multiply; delta * 2^-15 is exact
    embed   b' = b delta + d;  q = fma(2 delta, rint((s_1 - b') / (2 delta)), b');  then the cap, the climb and the bias
    decode  x = (s~_1 - d) * (1 / (2 delta));  f, m as in payload_refs.metric
d is no integer, so 2 delta k + b' is formed in float64 - exact there for every delta in 8..512 (2 delta k needs at most
24 + 8 bits; b' has 24, and its last bit lies fewer than 53 places below the first bit of 2 delta k) - and rounded once to
float32: the fused multiply-add of the rule.
"""
import functools

import numpy as np

import payload_refs as pr
from oracle import wm_oracle as o

F = pr.F
D = np.float64
U_EDGES = (0, 1, 32767, 32768, 65535)
DELTAS = (8.0, 12.0, 16.0, 16.5, 24.0, 200.0, 512.0)
PASSWORD, NONCE = "pw", bytes([5] * 8)                                       # the product's table in the tests: this key


def offset(u, delta) -> np.ndarray:
    return (np.asarray(u).astype(F) * (F(delta) * F(2.0 ** -15))).astype(F)


def target(Sc, bit, u, delta) -> np.ndarray:
    """q + 4 of every tile: Sc [..., 8] float32, bit [...] of 0 / 1, u [...] uint16 -> float32 [...]"""
    Sc = np.asarray(Sc, F)
    d = F(delta); two = F(2.0) * d
    s1, s2 = Sc[..., 0], Sc[..., 1]
    bp = (np.where(np.asarray(bit) != 0, d, F(0.0)).astype(F) + offset(u, delta)).astype(F)
    k = np.rint(((s1 - bp).astype(F) / two).astype(F)).astype(F)
    q = (D(two) * k.astype(D) + bp.astype(D)).astype(F)
    q = np.where(q + pr.BIAS > pr.SIGMA_MAX, q - two, q).astype(F)
    for _ in range(3):
        q = np.where(q < s2 + d, q + two, q).astype(F)
    return (q + pr.BIAS).astype(F)


def sigma_w_eff(Sc, bit, u, delta) -> np.ndarray:
    Sc = np.asarray(Sc, F)
    eff = np.zeros(Sc.shape, F)
    eff[..., 0] = target(Sc, bit, u, delta) - Sc[..., 0]
    return eff


def metric(s1, u, delta) -> np.ndarray:
    return pr.metric((np.asarray(s1, F) - offset(u, delta)).astype(F), delta)


def tie_distance(Sc, bit, u, delta) -> np.ndarray:
    """how far (s_1 - b') / (2 delta) is from a half-integer, float64 [...]: 0 is a rounding tie"""
    Sc = np.asarray(Sc, D)
    bp = np.where(np.asarray(bit) != 0, float(delta), 0.0) + offset(u, delta).astype(D)
    x = (Sc[..., 0] - bp) / (2.0 * float(delta))
    return np.abs(x - np.floor(x) - 0.5)


def tie_tiles(Sc, bits, u, delta):
    return tie_distance(Sc, bits, u, delta) < pr.SIGMA_RTOL * Sc[..., 0] / (2 * delta)


def embed_ref(Y: np.ndarray, tile_bit, u, delta=pr.DELTA) -> dict:
    """payload_refs.embed_ref on the shifted lattices: u [nby, nbx] or flat"""
    Yf = Y.astype(F)
    Sc = o.stego_sigma(Yf, 8)
    eff = sigma_w_eff(Sc, np.asarray(tile_bit).reshape(Sc.shape[:2]), np.asarray(u).reshape(Sc.shape[:2]), delta)
    r = o.embed_plane(Yf, None, 1.0, kfrac=0.0, tile=8, k_floor=1, wm_svd=(None, eff, None))
    assert r["K"] == 1
    r["eff"] = eff
    return r


def metric_ref(stego: np.ndarray, u, delta=pr.DELTA) -> np.ndarray:
    s1 = o.stego_sigma(stego.astype(F), 8)[..., 0]
    return metric(s1, np.asarray(u).reshape(s1.shape), delta)


def margins_of(Y, tile_bits, u, delta) -> dict:
    """payload_refs.margins_of under dither words u, with keyless added: the dither-free read of the same stego"""
    nt = (Y.shape[0] // 8, Y.shape[1] // 8)
    tile_bits = np.asarray(tile_bits, np.uint8).reshape(nt)
    u = np.asarray(u, np.uint16).reshape(nt)
    ref = embed_ref(Y, tile_bits, u, delta)
    m = metric_ref(ref["stego"], u, delta)
    signed = np.where(tile_bits != 0, -m, m)
    black = pr.black_tiles(Y)
    tie, deg = tie_tiles(ref["Sc"], tile_bits, u, delta), pr.degenerate_tiles(ref["Sc"]) & ~black
    comparable = ~tie & ~deg & (np.abs(m) > pr.slope_bar(delta))
    return dict(signed=signed, m=m, tie=tie, deg=deg, black=black, comparable=comparable, stego=ref["stego"], Yw=ref["Yw"],
                Sc=ref["Sc"], eff=ref["eff"], tile_bits=tile_bits, u=u, keyless=pr.metric_ref(ref["stego"], delta))


def seeded_words(n: int, seed: int = 0) -> np.ndarray:
    """a seeded stand-in table (not the product's)"""
    return np.random.default_rng(1000 + seed).integers(0, 65536, n, dtype=np.uint16)


def named_host(name: str) -> np.ndarray:
    if name.startswith("planes"):
        return pr.mr.planes_of(72, 100, 3)[int(name[-1])]
    return dict(pr.edge_hosts())[name]


@functools.lru_cache(maxsize=None)
def _margins_cached(key):
    name, delta, seed, n_bits = key
    Y = named_host(name)
    nt = (Y.shape[0] // 8) * (Y.shape[1] // 8)
    bits, tile_bit, order, offs = case_bits(nt, n_bits, seed)
    r = margins_of(Y, tile_bit, seeded_words(nt, seed), delta)
    r.update(bits=bits, order=order, offs=offs)
    return r


def case_bits(nt: int, n_bits: int, seed: int):
    """(bits [n_bits], tile_bit [nt], order, offs): seeded bits through payload_refs.simple_map(seed 7)"""
    bits = pr.seeded_bits(n_bits, seed)
    tbi, order, offs = pr.simple_map(nt, n_bits, seed=pr.EDGE_MAP_SEED)
    return bits, bits[tbi], order, offs


def margins(name: str, delta: float, seed: int = 0, n_bits: int = 0) -> dict:
    """margins_of a named host ('72x100s1' .., 'edge', 'pinned', 'planes0..2') under seeded bits and seeded_words(seed);
    n_bits = 0 stands for n_tiles.  Cached, shared and never written to."""
    Y = named_host(name)
    nt = (Y.shape[0] // 8) * (Y.shape[1] // 8)
    return _margins_cached((name, float(delta), int(seed), int(n_bits) or nt))
