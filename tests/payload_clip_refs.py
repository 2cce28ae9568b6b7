"""Clip resynchronisation of the dithered blind payload in a video: the NumPy restatement of the rule's five steps as
include/wmhip.h states them, built on tests/payload_keyed_sync_refs.py (s1_ref, keyed_scores_ref, votes_ref), and the
scenarios the tests share.  Marked frames come from payload_dither_refs.embed_ref under the product's dither_table and
payload_map (host code the GPU tests do not question); unmarked frames are the bare hosts.  Nothing here touches the device.

    1 scan    s1_ref of the first A = min(n_c, anchors fi) clip frames
    2 tables  tables[k] = dither_table(frame k fi); table_of[g][a] = (g + a) // fi where (g + a) % fi == 0, else -1
    3 scores  score[g][p][ty, tx] = sum over the marked anchors of keyed_scores_ref(anchor a, tables[table_of[g][a]]);
              best[g][p] = (max, first row-major argmax), (-1, -1) without a window or a marked anchor
    4 winner  the largest score / (count_p m_g) by exact fractions, scanning (g, p, index) in ascending order
    5 decode  votes of every marked clip frame at the winner's phase under its own table's window, added; soft per bit
"""
import functools
from fractions import Fraction

import numpy as np

import payload_code_refs as cr
import payload_dither_refs as pdr
import payload_keyed_sync_refs as kr
import payload_refs as pr
import payload_sync_refs as sr
from oracle import wm_oracle as o

P = sr.P
F32 = np.float32
DELTA = sr.DELTA
VOTE_ONE = sr.VOTE_ONE
HOST_SEED = 10                                                              # frame f of a host is payload_refs.host(H, W, 10 + f)

# name -> host case (payload_sync_refs.CASES: A 128 x 192 carrying b"id", B 160 x 256 carrying b"id42"), the marked video's
# frames F and frame interval fi, the clip's first frame t0, its frames n_c and its crop (y0, x0, h, w)
SCENARIOS = {
    "A-crop": dict(case="A", F=6, fi=1, t0=2, n_c=3, crop=(3, 5, 118, 180)),
    "A-time": dict(case="A", F=6, fi=1, t0=3, n_c=2, crop=(0, 0, 128, 192)),            # cut in time only
    "A-fi2": dict(case="A", F=7, fi=2, t0=1, n_c=4, crop=(8, 16, 112, 168)),            # starts on an unmarked frame
    "B-crop": dict(case="B", F=5, fi=1, t0=1, n_c=3, crop=(11, 21, 120, 200)),
    "A-48x64": dict(case="A", F=6, fi=1, t0=2, n_c=4, crop=(40, 64, 48, 64)),           # 48 tiles: needs its 4 anchors
    "A-k7": dict(case="A", F=6, fi=1, t0=1, n_c=3, crop=(8, 16, 96, 160), code="k7"),   # 240 of 384 tiles: coded bits without a tile
}
LIMITS = {                                                                  # recorded, not GPU cases (the limits)
    "A-48x64-1anchor": dict(SCENARIOS["A-48x64"], anchors=1),
    "A-24x32-1anchor": dict(case="A", F=6, fi=1, t0=0, n_c=6, crop=(40, 64, 24, 32), anchors=1),
    "A-24x32-6anchors": dict(case="A", F=6, fi=1, t0=0, n_c=6, crop=(40, 64, 24, 32), anchors=6),
}
ANCHORS = 4


def scenario(name: str) -> dict:
    sc = dict(SCENARIOS.get(name) or LIMITS[name])
    sc.setdefault("code", None)
    sc.setdefault("anchors", ANCHORS)
    sc["shape"] = sr.CASES[sc["case"]]["shape"]
    sc["data"] = sr.CASES[sc["case"]]["data"]
    return sc


@functools.lru_cache(maxsize=None)
def case_map(case: str, code) -> tuple:
    """(frame bits, carried bits, tile_bit_index [nby, nbx]) of a case's payload, bare or under the channel code"""
    H, W = sr.CASES[case]["shape"]
    frame = P.payload_frame(sr.CASES[case]["data"])
    carried = cr.encode_ref(frame) if code else frame
    tbi = P.payload_map(H // 8, W // 8, sr.key(), carried.size)[0].reshape(H // 8, W // 8)
    tbi.setflags(write=False)
    return frame, carried, tbi


@functools.lru_cache(maxsize=None)
def frame_table(case: str, f: int) -> np.ndarray:
    """uint16 [nby, nbx]: the dither table of file frame f"""
    H, W = sr.CASES[case]["shape"]
    u = P.dither_table(H // 8, W // 8, sr.key(), f).reshape(H // 8, W // 8)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def host_frame(case: str, f: int) -> np.ndarray:
    H, W = sr.CASES[case]["shape"]
    return pr.host(H, W, HOST_SEED + f)


@functools.lru_cache(maxsize=None)
def marked_frame(case: str, f: int, code) -> np.ndarray:
    """the restatement's dithered stego of file frame f (its own host, its own table)"""
    _, carried, tbi = case_map(case, code)
    st = pdr.embed_ref(host_frame(case, f), carried[tbi], frame_table(case, f), DELTA)["stego"]
    st.setflags(write=False)
    return st


def hosts(name: str) -> np.ndarray:
    """uint8 [F, H, W]: the bare hosts of a scenario's video, what the product's embed is given"""
    sc = scenario(name)
    return np.stack([host_frame(sc["case"], f) for f in range(sc["F"])])


def video(name: str) -> np.ndarray:
    """uint8 [F, H, W]: the restatement's marked video of a scenario"""
    sc = scenario(name)
    return np.stack([marked_frame(sc["case"], f, sc["code"]) if f % sc["fi"] == 0 else host_frame(sc["case"], f)
                     for f in range(sc["F"])])


def cut(frames: np.ndarray, sc: dict) -> np.ndarray:
    """the scenario's clip of a [F, H, W] video"""
    y0, x0, h, w = sc["crop"]
    return np.ascontiguousarray(frames[sc["t0"]:sc["t0"] + sc["n_c"], y0:y0 + h, x0:x0 + w])


# ---- the rule --------------------------------------------------------------------------------------------------------
def table_of_ref(F: int, fi: int, n_c: int, A: int) -> np.ndarray:
    """int32 [F - n_c + 1, A], the literal loops"""
    out = np.full((F - n_c + 1, A), -1, np.int32)
    for g in range(F - n_c + 1):
        for a in range(A):
            if (g + a) % fi == 0:
                out[g, a] = (g + a) // fi
    return out


def summed_scores_ref(s1_scans, tables, table_of, delta) -> list:
    """summed[g] = the 64 phases' int64 score grids of candidate g added over its marked anchors (None without one);
    an entry outside 0 .. n_tables - 1 is skipped as -1 is"""
    pair = {}
    out = []
    for row in np.asarray(table_of):
        acc = None
        for a, t in enumerate(row):
            if not 0 <= t < len(tables):
                continue
            if (a, int(t)) not in pair:
                pair[a, int(t)] = kr.keyed_scores_ref(s1_scans[a], tables[int(t)], delta)
            acc = [x.copy() for x in pair[a, int(t)]] if acc is None else [x + y for x, y in zip(acc, pair[a, int(t)])]
        out.append(acc)
    return out


def best_of(summed) -> np.ndarray:
    """int64 [n_cand, 64, 2]: (max, first row-major argmax) of every candidate's 64 grids; (-1, -1) where there is none"""
    best = np.full((len(summed), 64, 2), -1, np.int64)
    for g, grids in enumerate(summed):
        for p in range(64 if grids is not None else 0):
            sc = np.asarray(grids[p]).reshape(-1)
            if sc.size:
                i = 0
                for j in range(sc.size):                                    # (the literal scan: the first of equals)
                    if sc[j] > sc[i]:
                        i = j
                best[g, p] = (sc[i], i)
    return best


def best_ref(s1_scans, tables, table_of, delta) -> np.ndarray:
    return best_of(summed_scores_ref(s1_scans, tables, table_of, delta))


def pick_clip_ref(best, counts, marked):
    """(g, p, index) by exact fractions, scanning (g, p) in ascending order and keeping the first maximum"""
    win = None
    for g in range(len(best)):
        for p in range(64):
            s, i = int(best[g][p][0]), int(best[g][p][1])
            if s < 0 or i < 0 or counts[p] * marked[g] <= 0:
                continue
            f = Fraction(s, int(counts[p]) * int(marked[g]))
            if win is None or f > win[0]:
                win = (f, g, p, i)
    return None if win is None else win[1:]


def locate_clip_ref(clip: np.ndarray, case: str, F: int, fi: int, code=None, anchors: int = ANCHORS, delta=DELTA) -> dict:
    """The five steps on a clip uint8 [n_c, h, w] of a case's marked video.  Beside the result: top = the winner's score /
    (32768 windows marked anchors), runner_up = the best other (candidate, phase, placement)'s, gap = their difference."""
    n_c, h, w = clip.shape
    H, W = sr.CASES[case]["shape"]
    nby, nbx = H // 8, W // 8
    frame, carried, tbi = case_map(case, code)
    A = min(n_c, anchors * fi)
    table_of = table_of_ref(F, fi, n_c, A)
    tables = [frame_table(case, k * fi) for k in range(-(-F // fi))]
    scans = [kr.s1_ref(clip[a]) for a in range(A)]
    summed = summed_scores_ref(scans, tables, table_of, delta)
    counts = kr.counts_ref(h, w)
    m_g = [int((row >= 0).sum()) for row in table_of]
    best = best_of(summed)
    win = pick_clip_ref(best, counts, m_g)
    if win is None:
        return dict(best=best, first_frame=None)
    t0, p, index = win
    py, px = divmod(p, 8)
    ny, nx = sr.phase_shape(h, w, py, px)
    ty, tx = divmod(index, nbx - nx + 1)
    norm = np.concatenate([grids[q].reshape(-1) / (VOTE_ONE * float(counts[q] * m_g[g]))
                           for g, grids in enumerate(summed) if grids is not None for q in range(64) if counts[q] and grids[q].size])
    top = float(summed[t0][p][ty, tx]) / (VOTE_ONE * float(counts[p] * m_g[t0]))
    rest = np.sort(norm)[::-1]
    assert rest[0] == top
    votes = np.zeros((ny, nx), np.int64)
    n_marked = 0
    for i in range(n_c):
        if (t0 + i) % fi == 0:
            view = np.ascontiguousarray(clip[i, py:py + 8 * ny, px:px + 8 * nx]).astype(F32)
            s1 = o.stego_sigma(view, 8)[..., 0].astype(F32)
            votes += kr.votes_ref(s1, frame_table(case, t0 + i)[ty:ty + ny, tx:tx + nx], delta)
            n_marked += 1
    t = np.asarray(tbi[ty:ty + ny, tx:tx + nx], np.int64).reshape(-1)
    hist = np.zeros(carried.size, np.int64)
    np.add.at(hist, t, votes.reshape(-1))
    soft = hist.astype(np.float64) / VOTE_ONE
    count = np.bincount(t, minlength=carried.size).astype(np.int64)
    got = cr.viterbi_ref(cr.quantise_ref(soft), frame.size)[0] if code else (soft < 0).astype(np.uint8)
    data, valid = P.payload_unframe(got)
    have = count > 0
    return dict(best=best, first_frame=int(t0), phase=(py, px), place=(ty, tx), origin=(8 * ty - py, 8 * tx - px), top=top,
                runner_up=float(rest[1]) if rest.size > 1 else float("-inf"),
                gap=float(top - rest[1]) if rest.size > 1 else float("inf"), candidates=int(norm.size), soft=soft, count=count,
                n_marked=n_marked, data=data, valid=bool(valid),
                confidence=float(np.mean(np.abs(soft[have]) / (count[have] * max(n_marked, 1)))) if have.any() else 0.0)


@functools.lru_cache(maxsize=None)
def located(name: str) -> dict:
    """locate_clip_ref of a scenario's clip of the restatement's video; cached, shared by the tests"""
    sc = scenario(name)
    return locate_clip_ref(cut(video(name), sc), sc["case"], sc["F"], sc["fi"], sc["code"], sc["anchors"])


def is_true(r: dict, sc: dict) -> bool:
    """the winner is the scenario's true (first frame, phase, place)"""
    y0, x0 = sc["crop"][:2]
    return r["first_frame"] == sc["t0"] and r["origin"] == (y0, x0) and r["phase"] == ((-y0) % 8, (-x0) % 8)
