"""Frame resynchronisation of the dithered blind payload in a video: the NumPy restatement of the rule's four steps as
include/wmhip.h states them, built on tests/payload_clip_refs.py (the frames, the tables, best_ref, pick_clip_ref) and
tests/payload_keyed_sync_refs.py (s1_ref, votes_ref), and the scenarios the tests share.  Nothing here touches the device.

    1 geometry  the first A = min(n_c, anchors fi) frames in file order, each alone: best_ref of its scan under all K tables
                (candidate g = table g), pick_clip_ref with one marked anchor; accepted when the winner leads every other
                (candidate, phase) entry by 1 / 10 of full scale, by exact fractions.  The first accepted fixes phase and place.
    2 scores    score[f][k] = sum over the windows of |votes_ref(s1[f], tables[k][ty : ty + ny, tx : tx + nx])|, int64
    3 assign    k* the first maximum of the row, second = max(the best other table, 16384 n_win); accepted when
                (score[k*] - second) / (32768 n_win) >= 1 / 10 by exact fractions; frame_map[f] = k* fi or -1
    4 decode    the accepted frames' votes under their own tables' windows, added; soft per bit; the decode
"""
import functools
from fractions import Fraction

import numpy as np

import payload_clip_refs as cl
import payload_code_refs as cr
import payload_keyed_sync_refs as kr
import payload_refs as pr
import payload_sync_refs as sr
from oracle import wm_oracle as o

P = sr.P
F32 = np.float32
DELTA = sr.DELTA
VOTE_ONE = sr.VOTE_ONE
GAP = Fraction(1, 10)                                                       # the bar of steps 1 and 3
FOREIGN_SEED = 900                                                          # clip entry -1 - i is payload_refs.host(H, W, 900 + i)
ANCHORS = 4

# name -> host case (payload_sync_refs.CASES), the marked video's frames F and frame interval fi, the clip as the file frame of
# every clip frame in clip order (a negative entry: a foreign frame), and the crop (y0, x0, h, w) of every frame
SCENARIOS = {
    "A-drop": dict(case="A", F=12, fi=1, clip=[0, 1, 2, 3, 5, 6, 7, 8, 10, 11], crop=(0, 0, 128, 192)),      # 30 -> 24 fps
    "A-shuffle": dict(case="A", F=8, fi=1, clip=[5, 2, 7, 2, 0], crop=(3, 5, 118, 180)),                     # a repeat among them
    "A-fi2-foreign": dict(case="A", F=9, fi=2, clip=[3, 4, -1, 6, 1, 8], crop=(8, 16, 112, 168)),            # starts on an unmarked frame
    "B-reverse": dict(case="B", F=5, fi=1, clip=[4, 3, 2, 1, 0], crop=(11, 21, 120, 200)),
    "A-k7": dict(case="A", F=6, fi=1, clip=[4, 1, 3], crop=(8, 16, 96, 160), code="k7"),                     # coded bits without a tile
}
LIMITS = {                                                                  # recorded, not GPU cases (the limits)
    "A-48x64": dict(case="A", F=6, fi=1, clip=[5, 2, 0, 3], crop=(40, 64, 48, 64)),      # 48 windows: found, too close to the bar
    "A-24x32": dict(case="A", F=6, fi=1, clip=[5, 2, 0, 3], crop=(40, 64, 24, 32)),      # 12 windows: frames do not name their tables
}


# ---- the kernel's blocks, chunks and caps, restated; SOURCE holds the statement of each in csrc/wm_payload.hip, which
# tests/test_payload_frames.py finds there, so the shapes below cannot drift from what the kernel does
FRAME_FB, FRAME_TB = 8, 8                           # frames and tables of a wave's block
FRAME_CHUNK = 512                                   # windows of a wave's chunk: 8 a lane, so an int32 accumulator stays below 2^18
FRAME_GRID_CAP = 1024                               # table blocks (grid y) and frame blocks (grid z) of a launch
WAVE = 64
SOURCE = [
    "constexpr int FRAME_FB = 8;", "constexpr int FRAME_TB = 8;", "#define WM_FRAME_CHUNK 512", "constexpr int FRAME_CHUNK = WM_FRAME_CHUNK;",
    "constexpr int FRAME_GRID_CAP = 1024;",
    "for (int i = i0 + (int)threadIdx.x; i < i1; i += WAVE)",
    "for (int f0 = blockIdx.z * FRAME_FB; f0 < g.n_frames; f0 += gridDim.z * FRAME_FB)",
    "for (int t0 = blockIdx.y * FRAME_TB; t0 < g.n_tables; t0 += gridDim.y * FRAME_TB)",
    "std::min((n_tables - 1) / FRAME_TB + 1, FRAME_GRID_CAP)", "std::min((n_frames - 1) / FRAME_FB + 1, FRAME_GRID_CAP)",
]
# name -> (n_frames, n_tables, ny, nx, nby, nbx, ty, tx): one shape one past each chunk, cap and loop of the kernel
TRIPS = {
    "lane-0-twice": (3, 3, 5, 13, 6, 15, 1, 2),                             # 65 windows: lane 0 alone goes round its loop again
    "second-chunk-of-one-window": (3, 3, 27, 19, 28, 21, 1, 1),             # 513 windows: the second wave of a row has one
    "a-lane-in-three-chunks": (9, 9, 33, 33, 34, 36, 1, 2),                 # 1089 windows: lane 0 adds 8 + 8 + 2 over three waves
    "table-blocks-past-the-grid": (2, FRAME_TB * FRAME_GRID_CAP + 1, 1, 3, 1, 3, 0, 0),     # 1025 table blocks: block 0 strides
    "frame-blocks-past-the-grid": (FRAME_FB * FRAME_GRID_CAP + 1, 2, 1, 3, 1, 3, 0, 0),     # 1025 frame blocks
}


def scenario(name: str) -> dict:
    sc = dict(SCENARIOS.get(name) or LIMITS[name])
    sc.setdefault("code", None)
    sc.setdefault("anchors", ANCHORS)
    sc["shape"] = sr.CASES[sc["case"]]["shape"]
    sc["data"] = sr.CASES[sc["case"]]["data"]
    # what the search must return: a marked frame's own file index, -1 for an unmarked or a foreign one
    sc["frame_map"] = [f if f >= 0 and f % sc["fi"] == 0 else -1 for f in sc["clip"]]
    return sc


@functools.lru_cache(maxsize=None)
def foreign_frame(case: str, i: int) -> np.ndarray:
    H, W = sr.CASES[case]["shape"]
    return pr.host(H, W, FOREIGN_SEED + i)


def hosts(name: str) -> np.ndarray:
    """uint8 [F, H, W]: the bare hosts of a scenario's video, what the product's embed is given"""
    sc = scenario(name)
    return np.stack([cl.host_frame(sc["case"], f) for f in range(sc["F"])])


def video(name: str) -> np.ndarray:
    """uint8 [F, H, W]: the restatement's marked video of a scenario"""
    sc = scenario(name)
    return np.stack([cl.marked_frame(sc["case"], f, sc["code"]) if f % sc["fi"] == 0 else cl.host_frame(sc["case"], f)
                     for f in range(sc["F"])])


def edit(frames: np.ndarray, sc: dict) -> np.ndarray:
    """the scenario's file of a [F, H, W] video: its frames picked in clip order, foreign ones mixed in, all cropped"""
    y0, x0, h, w = sc["crop"]
    picked = [frames[f] if f >= 0 else foreign_frame(sc["case"], -1 - f) for f in sc["clip"]]
    return np.ascontiguousarray(np.stack(picked)[:, y0:y0 + h, x0:x0 + w])


# ---- the rule --------------------------------------------------------------------------------------------------------
def frame_scores_ref(s1, tables, ny: int, nx: int, ty: int, tx: int, delta) -> np.ndarray:
    """int64 [n_frames, n_tables] of s1 float32 [n_frames, ny, nx] (or any layout that reshapes to it) under tables
    [n_tables, nby, nbx] at the placement (ty, tx)"""
    s1 = np.asarray(s1, F32).reshape(-1, ny, nx)
    out = np.zeros((s1.shape[0], len(tables)), np.int64)
    for k, U in enumerate(tables):
        win = np.asarray(U)[ty:ty + ny, tx:tx + nx]
        assert win.shape == (ny, nx), (win.shape, ny, nx)
        out[:, k] = np.abs(kr.votes_ref(s1, win[None], delta).astype(np.int64)).sum(axis=(1, 2))
    return out


def pick_frames_ref(scores, n_win: int) -> list:
    """the literal loops of step 3, by exact fractions: the table index every row names, or -1"""
    out = []
    for row in np.asarray(scores):
        k = 0
        for j in range(len(row)):                                           # (the first of equals)
            if row[j] > row[k]:
                k = j
        second = Fraction(VOTE_ONE // 2 * n_win)
        for j in range(len(row)):
            if j != k and Fraction(int(row[j])) > second:
                second = Fraction(int(row[j]))
        out.append(k if (Fraction(int(row[k])) - second) / (VOTE_ONE * n_win) >= GAP else -1)
    return out


def frame_gaps(scores, n_win: int) -> np.ndarray:
    """float64 [n_frames]: (the row's maximum - max(its best other entry, the half-scale floor)) / (32768 n_win)"""
    out = []
    for row in np.asarray(scores):
        row = [int(x) for x in row]
        k = row.index(max(row))
        out.append((row[k] - max(row[:k] + row[k + 1:] + [VOTE_ONE // 2 * n_win])) / (VOTE_ONE * n_win))
    return np.asarray(out, np.float64)


def anchor_lead_ref(best, counts, win) -> Fraction:
    """the winner's score / (32768 windows) less the best other (candidate, phase) entry's, an exact fraction (None: no other)"""
    g, p = win[:2]
    top = Fraction(int(best[g][p][0]), int(counts[p]) * VOTE_ONE)
    rest = [Fraction(int(best[e][q][0]), int(counts[q]) * VOTE_ONE) for e in range(len(best)) for q in range(64)
            if (e, q) != (g, p) and best[e][q][0] >= 0 and counts[q] > 0]
    return top - max(rest) if rest else None


def match_frames_ref(clip: np.ndarray, case: str, F: int, fi: int, code=None, anchors: int = ANCHORS, delta=DELTA) -> dict:
    """The four steps on a file uint8 [n_c, h, w] of frames of a case's marked video.  Beside the result: anchor_leads = the
    lead of every tried anchor's winner (floats, in file order; the last one was accepted where ``found``), scores, gaps =
    frame_gaps of them."""
    n_c, h, w = clip.shape
    H, W = sr.CASES[case]["shape"]
    nby, nbx = H // 8, W // 8
    frame, carried, tbi = cl.case_map(case, code)
    K = -(-F // fi)
    tables = [cl.frame_table(case, k * fi) for k in range(K)]
    counts = kr.counts_ref(h, w)
    table_of = np.arange(K, dtype=np.int32)[:, None]
    out = dict(found=False, anchor_leads=[], frame_map=[-1] * n_c, data=b"", valid=False, confidence=0.0, origin=None)
    geometry = None
    for a in range(min(n_c, anchors * fi)):
        best = cl.best_ref([kr.s1_ref(clip[a])], tables, table_of, delta)
        win = cl.pick_clip_ref(best, counts, [1] * K)
        if win is None:
            continue
        lead = anchor_lead_ref(best, counts, win)
        out["anchor_leads"].append(float("inf") if lead is None else float(lead))
        if lead is None or lead >= GAP:
            geometry = win
            break
    if geometry is None:
        return out
    _, p, index = geometry
    py, px = divmod(p, 8)
    ny, nx = sr.phase_shape(h, w, py, px)
    ty, tx = divmod(index, nbx - nx + 1)
    s1 = np.stack([o.stego_sigma(np.ascontiguousarray(clip[i, py:py + 8 * ny, px:px + 8 * nx]).astype(F32), 8)[..., 0].astype(F32)
                   for i in range(n_c)])
    scores = frame_scores_ref(s1, tables, ny, nx, ty, tx, delta)
    named = pick_frames_ref(scores, ny * nx)
    votes = np.zeros((ny, nx), np.int64)
    for i, k in enumerate(named):
        if k >= 0:
            votes += kr.votes_ref(s1[i], tables[k][ty:ty + ny, tx:tx + nx], delta)
    n_acc = sum(k >= 0 for k in named)
    out.update(found=True, phase=(py, px), place=(ty, tx), origin=(8 * ty - py, 8 * tx - px), scores=scores, n_win=ny * nx,
               gaps=frame_gaps(scores, ny * nx), frame_map=[k * fi if k >= 0 else -1 for k in named], n_accepted=n_acc)
    if n_acc == 0:
        return out
    t = np.asarray(tbi[ty:ty + ny, tx:tx + nx], np.int64).reshape(-1)
    hist = np.zeros(carried.size, np.int64)
    np.add.at(hist, t, votes.reshape(-1))
    soft = hist.astype(np.float64) / VOTE_ONE
    count = np.bincount(t, minlength=carried.size).astype(np.int64)
    got = cr.viterbi_ref(cr.quantise_ref(soft), frame.size)[0] if code else (soft < 0).astype(np.uint8)
    data, valid = P.payload_unframe(got)
    have = count > 0
    out.update(soft=soft, count=count, data=data, valid=bool(valid),
               confidence=float(np.mean(np.abs(soft[have]) / (count[have] * n_acc))) if have.any() else 0.0)
    return out


@functools.lru_cache(maxsize=None)
def matched(name: str) -> dict:
    """match_frames_ref of a scenario's file of the restatement's video; cached, shared by the tests"""
    sc = scenario(name)
    return match_frames_ref(edit(video(name), sc), sc["case"], sc["F"], sc["fi"], sc["code"], sc["anchors"])


MARKED_GAP = 0.1 + 2 * pr.slope_bar(DELTA)                                  # what a marked frame (and an accepted anchor) must reach
OTHER_GAP = 0.1 - 2 * pr.slope_bar(DELTA)                                   # what any other frame (and a refused anchor) must stay under


def meets_precondition(r: dict, sc: dict) -> bool:
    """What a GPU test may lean on, on the restatement alone.  The device's sigma_1 may differ from the oracle's within the
    sigma bar, which moves a score / (32768 windows) by at most slope_bar(delta) - the best and the runner-up one each - so a
    gap of at least 0.1 + 2 slope_bar stays above the bar of 0.1 and one of at most 0.1 - 2 slope_bar stays below: the same
    anchors are refused and accepted and the same frames name the same tables."""
    y0, x0 = sc["crop"][:2]
    if not r["found"] or r["origin"] != (y0, x0) or r["phase"] != ((-y0) % 8, (-x0) % 8):
        return False
    if not (all(g <= OTHER_GAP for g in r["anchor_leads"][:-1]) and r["anchor_leads"][-1] >= MARKED_GAP):
        return False
    if r["frame_map"] != sc["frame_map"]:
        return False
    for g, want in zip(r["gaps"], sc["frame_map"]):
        if (want >= 0 and g < MARKED_GAP) or (want < 0 and g > OTHER_GAP):
            return False
    return bool(r["valid"]) and r["data"] == sc["data"]
