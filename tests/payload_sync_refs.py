"""Crop resynchronisation of the blind payload: the NumPy restatement of the rule's four steps as include/wmhip.h states them,
built on tests/payload_refs.py (the oracle's sigma, the metric, embed_ref), and the cases the tests share.  The keyed
tile-to-bit map is the product's own (payload.payload_map under hostglue.derive_key): it is host code the GPU tests do not
question, and the study behind the cases used it.  Nothing here touches the device.

    1 vote    vote = rint(m * 32768) as int32
    2 phase   p = 8 py + px: windows at (py + 8 r, px + 8 c), r < (h - py) // 8, c < (w - px) // 8; sum_p = sum |vote|, the
              winner by sum_p / count_p compared exactly, ties to the smallest p, count 0 does not take part
    3 offset  hist[j] = sum of V[r, c] with T[ty + r, tx + c] == j (int32), score = sum |hist[j]| (int64), the winner the
              largest, ties to the smallest (ty, tx)
    4 decode  soft[j] = hist[j] / 32768, origin = (8 ty - py, 8 tx - px)
"""
import functools
import importlib
from fractions import Fraction

import numpy as np

import __graft_entry__ as ge
import payload_refs as pr
from oracle import wm_oracle as o

P = importlib.import_module(ge.PKG_NAME + ".payload")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")

F = np.float32
PASSWORD = "pw"
NONCE = bytes([3] * 8)
DELTA = 16.0
VOTE_ONE = 32768

# name -> host shape, host seeds, payload, crops (y0, x0, h, w)
CASES = {
    "A": dict(shape=(128, 192), seeds=(1, 2), data=b"id",
              crops=((3, 5, 118, 180), (1, 1, 127, 191), (8, 16, 112, 168), (7, 7, 113, 177), (0, 9, 128, 160), (13, 0, 115, 192))),
    "B": dict(shape=(160, 256), seeds=(1, 3), data=b"id42",
              crops=((11, 21, 120, 200), (40, 56, 120, 200), (5, 3, 150, 250))),
}


def all_cases():
    """[(case, seed, crop)] of every case"""
    return [(c, s, crop) for c, d in CASES.items() for s in d["seeds"] for crop in d["crops"]]


def case_id(c):
    return f"{c[0]}s{c[1]}-" + "x".join(map(str, c[2]))


def key() -> bytes:
    return hg.derive_key(PASSWORD, NONCE)


@functools.lru_cache(maxsize=None)
def case_map(case: str) -> tuple:
    """(bits uint8 [n_bits], tile_bit_index int32 [nby, nbx]) of a case: its framed payload under the keyed map"""
    H, W = CASES[case]["shape"]
    bits = P.payload_frame(CASES[case]["data"])
    tbi = P.payload_map(H // 8, W // 8, key(), bits.size)[0].reshape(H // 8, W // 8)
    tbi.setflags(write=False)
    return bits, tbi


@functools.lru_cache(maxsize=None)
def marked(case: str, seed: int) -> np.ndarray:
    """the restatement's stego plane of a case host (payload_refs.embed_ref under the case's map)"""
    H, W = CASES[case]["shape"]
    bits, tbi = case_map(case)
    st = pr.embed_ref(pr.host(H, W, seed), bits[tbi], DELTA)["stego"]
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def marked_bgr_y(case: str, seed: int) -> np.ndarray:
    """The same through the product's BGR path, on the CPU: the host as a gray BGR stack, Y of BGR2YCrCb, the restatement's
    embed, Y put back, YCrCb2BGR, and Y of the result - the plane the extract reads from the stego that
    embed_payload_arrays returns."""
    H, W = CASES[case]["shape"]
    bits, tbi = case_map(case)
    bgr = np.repeat(pr.host(H, W, seed)[..., None], 3, -1)
    ycc = o.bgr_to_ycrcb(bgr).copy()
    ycc[..., 0] = pr.embed_ref(ycc[..., 0], bits[tbi], DELTA)["stego"]
    y = np.ascontiguousarray(o.bgr_to_ycrcb(o.ycrcb_to_bgr(ycc))[..., 0])
    y.setflags(write=False)
    return y


def crop_of(plane: np.ndarray, crop) -> np.ndarray:
    y0, x0, h, w = crop
    return plane[y0:y0 + h, x0:x0 + w]


# ---- the rule --------------------------------------------------------------------------------------------------------
def vote_of(m) -> np.ndarray:
    return np.rint(np.asarray(m, F) * F(VOTE_ONE)).astype(np.int32)


def phase_shape(h: int, w: int, py: int, px: int) -> tuple:
    return max(h - py, 0) // 8, max(w - px, 0) // 8


def votes_ref(plane: np.ndarray, delta=DELTA) -> list:
    """votes[py][px]: int32 [ny_p, nx_p] of every phase of a uint8 plane, sigma from the oracle"""
    h, w = plane.shape
    out = []
    for py in range(8):
        row = []
        for px in range(8):
            ny, nx = phase_shape(h, w, py, px)
            if ny * nx == 0:
                row.append(np.zeros((ny, nx), np.int32))
            else:
                row.append(vote_of(pr.metric_ref(np.ascontiguousarray(plane[py:py + 8 * ny, px:px + 8 * nx]), delta)))
        out.append(row)
    return out


def phase_sums(votes) -> tuple:
    """(sums int64 [8, 8], counts int64 [8, 8]) of votes[py][px]"""
    sums = np.array([[int(np.abs(v.astype(np.int64)).sum()) for v in row] for row in votes], np.int64)
    counts = np.array([[v.size for v in row] for row in votes], np.int64)
    return sums, counts


def pick_phase_ref(sums, counts):
    best = None
    for p in range(64):
        s, n = int(np.asarray(sums).reshape(-1)[p]), int(np.asarray(counts).reshape(-1)[p])
        if n > 0 and (best is None or Fraction(s, n) > best[1]):
            best = (p, Fraction(s, n))
    return None if best is None else divmod(best[0], 8)


def hist_ref(V, Twin, n_bits: int) -> np.ndarray:
    """int32 [n_bits]: the votes summed per bit under a window of the map; entries outside 0 .. n_bits - 1 skipped"""
    v = np.asarray(V, np.int64).reshape(-1)
    t = np.asarray(Twin, np.int64).reshape(-1)
    ok = (t >= 0) & (t < n_bits)
    h = np.zeros(n_bits, np.int64)
    np.add.at(h, t[ok], v[ok])
    return h.astype(np.int32)                                              # (wraps like the device's int32)


def offset_scores_ref(V, T, n_bits: int) -> np.ndarray:
    V, T = np.asarray(V), np.asarray(T)
    (ny, nx), (nby, nbx) = V.shape, T.shape
    sc = np.zeros((max(nby - ny + 1, 0), max(nbx - nx + 1, 0)), np.int64)
    for ty in range(sc.shape[0]):
        for tx in range(sc.shape[1]):
            sc[ty, tx] = np.abs(hist_ref(V, T[ty:ty + ny, tx:tx + nx], n_bits).astype(np.int64)).sum()
    return sc


def pick_offset_ref(scores):
    best = None
    for ty in range(scores.shape[0]):
        for tx in range(scores.shape[1]):
            if best is None or int(scores[ty, tx]) > best[0]:
                best = (int(scores[ty, tx]), (ty, tx))
    return None if best is None else best[1]


def soft_ref(V, Twin, n_bits: int) -> tuple:
    """(soft float64 [n_bits], count int64 [n_bits]) - and payload_refs.soft_ref is what test_payload_sync holds it to"""
    t = np.asarray(Twin, np.int64).reshape(-1)
    ok = (t >= 0) & (t < n_bits)
    return hist_ref(V, Twin, n_bits).astype(np.float64) / VOTE_ONE, np.bincount(t[ok], minlength=n_bits).astype(np.int64)


def locate_ref(plane: np.ndarray, T: np.ndarray, n_bits: int, delta=DELTA, votes=None) -> dict:
    """The four steps on one plane (``votes``: votes_ref(plane) where the caller has them).  Beside the result: the gaps
    between the winner and the best other candidate - phase_gap in units of mean |m| (sum / (32768 count)), offset_gap in
    score / (32768 tiles), inf where there is no other candidate."""
    votes = votes_ref(plane, delta) if votes is None else votes
    sums, counts = phase_sums(votes)
    py, px = pick_phase_ref(sums, counts)
    mean = np.where(counts > 0, sums / (VOTE_ONE * np.maximum(counts, 1)), -np.inf)
    others = np.delete(mean.reshape(-1), 8 * py + px)
    V = votes[py][px]
    scores = offset_scores_ref(V, T, n_bits)
    place = pick_offset_ref(scores)
    r = dict(votes=votes, sums=sums, counts=counts, phase=(py, px), V=V, scores=scores, place=place,
             phase_gap=float(mean[py, px] - others.max()))
    if place is None:
        return dict(r, valid=False, data=b"", origin=None, offset_gap=float("inf"))
    ty, tx = place
    norm = scores / (VOTE_ONE * float(V.size))
    rest = np.delete(norm.reshape(-1), ty * scores.shape[1] + tx)
    soft, count = soft_ref(V, T[ty:ty + V.shape[0], tx:tx + V.shape[1]], n_bits)
    data, valid = P.payload_unframe(soft < 0)
    return dict(r, soft=soft, count=count, data=data, valid=bool(valid), origin=(8 * ty - py, 8 * tx - px),
                offset_gap=float(norm[ty, tx] - rest.max()) if rest.size else float("inf"))


def check_precondition(r: dict, crop, data: bytes, delta=DELTA) -> None:
    """What a GPU test may rely on, on the restatement alone: the true phase and the true placement win by at least
    4 slope_bar(delta), every bit has a tile in the crop, the decode is valid and equal to the data."""
    y0, x0, h, w = crop
    bar = 4 * pr.slope_bar(delta)
    assert r["origin"] == (y0, x0), (r["origin"], crop)
    assert r["phase"] == ((-y0) % 8, (-x0) % 8), (r["phase"], crop)
    assert r["phase_gap"] >= bar, (r["phase_gap"], bar, crop)
    assert r["offset_gap"] >= bar, (r["offset_gap"], bar, crop)
    assert r["count"].min() >= 1, (int(r["count"].min()), crop)
    assert r["valid"] and r["data"] == data, (r["valid"], r["data"], crop)


@functools.lru_cache(maxsize=None)
def located(case: str, seed: int, crop: tuple) -> dict:
    """locate_ref of a case crop of the restatement's stego; cached, shared by the tests"""
    bits, tbi = case_map(case)
    return locate_ref(crop_of(marked(case, seed), crop), tbi, bits.size)
