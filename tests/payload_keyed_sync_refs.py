"""Keyed crop resynchronisation of the dithered blind payload: the NumPy restatement of the rule's four steps as
include/wmhip.h states them, built on the oracle's sigma, tests/payload_dither_refs.py (the dithered embed and metric) and the
cases of tests/payload_sync_refs.py.  The keyed tile-to-bit map and the dither table are the product's own (payload.payload_map
and payload.dither_table under hostglue.derive_key): host code the GPU tests do not question.  Nothing here touches the device.

    1 scan    p = 8 py + px: windows at (py + 8 r, px + 8 c), r < (h - py) // 8, c < (w - px) // 8; s1[p][r, c] float32
    2 scores  score[p][ty, tx] = sum over the windows of |vote(metric(s1[p][r, c], U[ty + r, tx + c], delta))|, int64
    3 winner  the largest score / count_p compared exactly, ties to the smallest (p, ty, tx), count 0 does not take part
    4 decode  votes of the winner's s1 under its window of U, soft[j] their sums per bit / 32768, origin = (8 ty - py, 8 tx - px)
"""
import functools
from fractions import Fraction

import numpy as np

import payload_dither_refs as pdr
import payload_refs as pr
import payload_sync_refs as sr
from oracle import wm_oracle as o

P = sr.P
F = np.float32
DELTA = sr.DELTA
VOTE_ONE = sr.VOTE_ONE
CASES = sr.CASES
all_cases, case_id, case_map, crop_of, key, phase_shape, vote_of = (sr.all_cases, sr.case_id, sr.case_map, sr.crop_of, sr.key,
                                                                    sr.phase_shape, sr.vote_of)


@functools.lru_cache(maxsize=None)
def case_table(case: str) -> np.ndarray:
    """uint16 [nby, nbx]: the embed's dither table of a case (frame index 0)"""
    H, W = CASES[case]["shape"]
    u = P.dither_table(H // 8, W // 8, key(), 0).reshape(H // 8, W // 8)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def marked(case: str, seed: int, delta: float = DELTA) -> np.ndarray:
    """the restatement's dithered stego plane of a case host"""
    H, W = CASES[case]["shape"]
    bits, tbi = case_map(case)
    st = pdr.embed_ref(pr.host(H, W, seed), bits[tbi], case_table(case), delta)["stego"]
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def marked_bgr_y(case: str, seed: int, delta: float = DELTA) -> np.ndarray:
    """The same through the product's BGR path, on the CPU (payload_sync_refs.marked_bgr_y with the dithered embed): the
    plane the extract reads from the stego that embed_payload_arrays(dither=True) returns."""
    H, W = CASES[case]["shape"]
    bits, tbi = case_map(case)
    bgr = np.repeat(pr.host(H, W, seed)[..., None], 3, -1)
    ycc = o.bgr_to_ycrcb(bgr).copy()
    ycc[..., 0] = pdr.embed_ref(ycc[..., 0], bits[tbi], case_table(case), delta)["stego"]
    y = np.ascontiguousarray(o.bgr_to_ycrcb(o.ycrcb_to_bgr(ycc))[..., 0])
    y.setflags(write=False)
    return y


# ---- the rule --------------------------------------------------------------------------------------------------------
def s1_ref(plane: np.ndarray) -> list:
    """s1[py][px]: float32 [ny_p, nx_p] of every phase of a uint8 plane, sigma from the oracle"""
    h, w = plane.shape
    out = []
    for py in range(8):
        row = []
        for px in range(8):
            ny, nx = phase_shape(h, w, py, px)
            if ny * nx == 0:
                row.append(np.zeros((ny, nx), F))
            else:
                row.append(o.stego_sigma(np.ascontiguousarray(plane[py:py + 8 * ny, px:px + 8 * nx]).astype(F), 8)[..., 0].astype(F))
        out.append(row)
    return out


def votes_ref(s1, u, delta) -> np.ndarray:
    """int32 votes of sigma_1 values under dither words of the same (or a broadcastable) shape"""
    return vote_of(pdr.metric(s1, u, delta))


def keyed_scores_ref(s1, U, delta) -> list:
    """The 64 phases' int64 [nby - ny_p + 1, nbx - nx_p + 1] score grids of a scan s1[py][px] under the table U [nby, nbx];
    [0, 0] for a phase without a window"""
    U = np.asarray(U)
    nby, nbx = U.shape
    out = []
    for p in range(64):
        g = np.asarray(s1[p // 8][p % 8], F)
        ny, nx = g.shape
        if ny * nx == 0 or ny > nby or nx > nbx:
            out.append(np.zeros((0, 0), np.int64))
            continue
        win = np.lib.stride_tricks.sliding_window_view(U, (ny, nx))       # [n_ty, n_tx, ny, nx]
        sc = np.zeros(win.shape[:2], np.int64)
        for ty in range(win.shape[0]):                                     # (a row of placements at a time: bounded memory)
            sc[ty] = np.abs(votes_ref(g[None], win[ty], delta).astype(np.int64)).sum(axis=(1, 2))
        out.append(sc)
    return out


def counts_ref(h: int, w: int) -> list:
    """the 64 phases' window counts"""
    return [int(np.prod(phase_shape(h, w, p // 8, p % 8))) for p in range(64)]


def pick_keyed_ref(scores, counts):
    """((py, px), (ty, tx)) by exact fractions, scanning (p, ty, tx) in ascending order and keeping the first maximum"""
    best = None
    for p in range(64):
        sc = np.asarray(scores[p])
        if counts[p] == 0:
            continue
        for ty in range(sc.shape[0]):
            for tx in range(sc.shape[1]):
                f = Fraction(int(sc[ty, tx]), counts[p])
                if best is None or f > best[0]:
                    best = (f, divmod(p, 8), (ty, tx))
    return None if best is None else best[1:]


def locate_ref(plane: np.ndarray, U: np.ndarray, T: np.ndarray, n_bits: int, delta=DELTA, s1=None) -> dict:
    """The four steps on one plane (``s1``: s1_ref(plane) where the caller has it).  Beside the result: ``top`` = the winner's
    score / (32768 windows), ``runner_up`` = the best other candidate's, gap = their difference (inf without another),
    candidates = how many took part."""
    h, w = plane.shape
    s1 = s1_ref(plane) if s1 is None else s1
    scores, counts = keyed_scores_ref(s1, U, delta), counts_ref(h, w)
    (py, px), (ty, tx) = pick_keyed_ref(scores, counts)
    norm = [sc.astype(np.float64) / (VOTE_ONE * max(n, 1)) for sc, n in zip(scores, counts)]
    flat = np.concatenate([n.reshape(-1) for n in norm])
    at = sum(n.size for n in norm[:8 * py + px]) + ty * norm[8 * py + px].shape[1] + tx
    rest = np.delete(flat, at)
    g = s1[py][px]
    ny, nx = g.shape
    votes = votes_ref(g, U[ty:ty + ny, tx:tx + nx], delta)
    soft, count = sr.soft_ref(votes, T[ty:ty + ny, tx:tx + nx], n_bits)
    data, valid = P.payload_unframe(soft < 0)
    have = count > 0
    return dict(s1=s1, scores=scores, phase=(py, px), place=(ty, tx), votes=votes, soft=soft, count=count,
                data=data, valid=bool(valid), origin=(8 * ty - py, 8 * tx - px), top=float(flat[at]),
                runner_up=float(rest.max()) if rest.size else float("-inf"), candidates=int(flat.size),
                gap=float(flat[at] - rest.max()) if rest.size else float("inf"),
                confidence=float(np.mean(np.abs(soft[have]) / count[have])) if have.any() else 0.0)


def check_precondition(r: dict, crop, data: bytes, delta=DELTA) -> None:
    """What a GPU test may rely on, on the restatement alone: the true phase and the true placement win by at least
    4 slope_bar(delta), every bit has a tile in the crop, the decode is valid and equal to the data."""
    y0, x0, h, w = crop
    bar = 4 * pr.slope_bar(delta)
    assert r["origin"] == (y0, x0), (r["origin"], crop)
    assert r["phase"] == ((-y0) % 8, (-x0) % 8), (r["phase"], crop)
    assert r["gap"] >= bar, (r["gap"], bar, crop)
    assert r["count"].min() >= 1, (int(r["count"].min()), crop)
    assert r["valid"] and r["data"] == data, (r["valid"], r["data"], crop)


@functools.lru_cache(maxsize=None)
def located(case: str, seed: int, crop: tuple, delta: float = DELTA) -> dict:
    """locate_ref of a case crop of the restatement's dithered stego; cached, shared by the tests"""
    bits, tbi = case_map(case)
    return locate_ref(crop_of(marked(case, seed, delta), crop), case_table(case), tbi, bits.size, delta)


@functools.lru_cache(maxsize=None)
def located_bgr(case: str, seed: int, crop: tuple, delta: float = DELTA) -> dict:
    """the same of the BGR-path plane"""
    bits, tbi = case_map(case)
    return locate_ref(crop_of(marked_bgr_y(case, seed, delta), crop), case_table(case), tbi, bits.size, delta)
