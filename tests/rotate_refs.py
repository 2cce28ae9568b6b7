"""Rotation resynchronisation of the blind payload: the NumPy restatement of the integer rotation, the validity test, the score,
the schedule and the winner's rule as include/wmhip.h states them ("rotation resynchronisation"), the float attackers the tests
rotate a stego with, and the restatement's search and decode, built on tests/resample_refs.py (the payload under test, the
oracle's sigma through payload_dither_refs.metric_ref).  The keyed tile-to-bit map, the frame and the dither table are the
product's own (payload.py): host code the GPU tests do not question.  Nothing here touches the device.

    candidate  C = rint(cos theta 2^16), S = rint(sin theta 2^16)
    pixel      X2 = 2 x + 1 - W, Y2 = 2 y + 1 - H;  U = C X2 - S Y2 + (w - 1) 2^16, V = S X2 + C Y2 + (h - 1) 2^16
               x0 = U >> 17, fx = (U >> 9) & 255, the same for y
               row_j = (sum_i K[fx][i] px[clamp(y0 - 1 + j)][clamp(x0 - 1 + i)] + 2^7) >> 8
               out = clip((sum_j K[fy][j] row_j + 2^19) >> 20, 0, 255)
    sense      a stego made by ``rotate_float(marked, deg)`` is restored by theta = +deg
"""
import functools
import math

import numpy as np

import payload_dither_refs as pdr
import resample_refs as rr

P = rr.P
I64 = np.int64
ONE = 1 << 14
COVER = (256, 384, 2)                                                       # mask_refs.host(H, W, seed): 32 x 48 = 1536 tiles
SMALL = (136, 200, 2)                                                       # 17 x 25: two tiles a bit, a limit
DELTA = 32.0
MAX_ANGLE = 8.0
ANGLES = (1.0, 3.0, -7.3)                                                   # degrees
KINDS = ("bilinear", "cubic")
VOTE_ONE = 32768
MARGIN_BAR = 0.102                                                          # the project's 4 sigma bar on a score gap


# ---- the rule --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights_ref() -> np.ndarray:
    """K int16 [256, 4], one phase and one tap at a time"""
    K = np.zeros((256, 4), np.int16)
    for f in range(256):
        iw = [int(np.rint(rr.cubic_ref(f / 256.0 + 1.0 - i) * ONE)) for i in range(4)]
        big = max(range(4), key=lambda k: (iw[k], -k))                      # the largest, the first of equals
        iw[big] += ONE - sum(iw)
        K[f] = iw
    K.setflags(write=False)
    return K


def candidate_ref(theta: float) -> tuple:
    return int(np.rint(math.cos(theta) * 65536.0)), int(np.rint(math.sin(theta) * 65536.0))


def coords_ref(H: int, W: int, h: int, w: int, C: int, S: int, ys=None, xs=None) -> tuple:
    """(x0, fx, y0, fy) of the destination pixels ys x xs (all of them by default), int64 [len(ys), len(xs)]"""
    assert max(H, W, h, w) <= 8192 and min(H, W, h, w) >= 1
    y = np.arange(H, dtype=I64) if ys is None else np.asarray(ys, I64)
    x = np.arange(W, dtype=I64) if xs is None else np.asarray(xs, I64)
    X2, Y2 = (2 * x + 1 - W)[None, :], (2 * y + 1 - H)[:, None]
    U = C * X2 - S * Y2 + (w - 1) * 65536
    V = S * X2 + C * Y2 + (h - 1) * 65536
    assert max(np.abs(U).max(), np.abs(V).max()) < 1 << 31                  # int32 on the device
    return U >> 17, (U >> 9) & 255, V >> 17, (V >> 9) & 255


def rotate_ref(plane: np.ndarray, H: int, W: int, C: int, S: int) -> np.ndarray:
    """uint8 [h, w] or [N, h, w] -> uint8 [N?, H, W] under candidate (C, S)"""
    assert plane.dtype == np.uint8 and plane.ndim in (2, 3)
    h, w = plane.shape[-2:]
    x0, fx, y0, fy = coords_ref(H, W, h, w, C, S)
    K = weights_ref().astype(I64)
    px = plane.reshape(plane.shape[:-2] + (h * w,)).astype(I64)
    xi = [np.clip(x0 - 1 + i, 0, w - 1) for i in range(4)]
    kx = [K[fx, i] for i in range(4)]
    acc = np.zeros(plane.shape[:-2] + (H, W), I64)
    for j in range(4):
        yj = np.clip(y0 - 1 + j, 0, h - 1) * w
        row = sum(kx[i] * np.take(px, yj + xi[i], axis=-1) for i in range(4))
        assert np.abs(row).max() < (1 << 31) - (1 << 7)
        acc += K[fy, j] * ((row + (1 << 7)) >> 8)
    assert np.abs(acc).max() < (1 << 31) - (1 << 19)                        # every sum is int32 on the device
    return np.clip((acc + (1 << 19)) >> 20, 0, 255).astype(np.uint8)


def valid_ref(H: int, W: int, h: int, w: int, C: int, S: int, every_pixel: bool = False) -> np.ndarray:
    """bool [H / 8, W / 8]: the tiles whose footprint lies inside the source - tested at the four corner pixels as the rule
    says, or with ``every_pixel`` at all 64"""
    assert H % 8 == 0 and W % 8 == 0
    if every_pixel:
        ys, xs = np.arange(H), np.arange(W)
    else:
        ys = np.sort(np.concatenate([np.arange(0, H, 8), np.arange(7, H, 8)]))
        xs = np.sort(np.concatenate([np.arange(0, W, 8), np.arange(7, W, 8)]))
    x0, _, y0, _ = coords_ref(H, W, h, w, C, S, ys, xs)
    ok = (x0 - 1 >= 0) & (x0 + 2 <= w - 1) & (y0 - 1 >= 0) & (y0 + 2 <= h - 1)
    k = 8 if every_pixel else 2
    return ok.reshape(H // 8, k, W // 8, k).all(axis=(1, 3))


def footprint_ref(H: int, W: int, h: int, w: int, C: int, S: int, block: int = 32) -> int:
    """the largest side, over the block x block destination blocks, of a block's source window (x0 - 1 .. x0 + 2)"""
    x0, _, y0, _ = coords_ref(H, W, h, w, C, S)
    worst = 0
    for by in range(0, H, block):
        for bx in range(0, W, block):
            for a in (x0[by:by + block, bx:bx + block], y0[by:by + block, bx:bx + block]):
                worst = max(worst, int(a.max() - a.min()) + 4)
    return worst


# ---- the attackers ---------------------------------------------------------------------------------------------------
def expanded_shape(H: int, W: int, deg: float) -> tuple:
    c, s = abs(math.cos(math.radians(deg))), abs(math.sin(math.radians(deg)))
    return int(math.ceil(H * c + W * s)), int(math.ceil(W * c + H * s))


def _cubic(x: np.ndarray) -> np.ndarray:
    """resample_refs.cubic_ref of every element"""
    x = np.abs(x)
    return np.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1.0, np.where(x < 2.0, -0.5 * (((x - 5.0) * x + 8.0) * x - 4.0), 0.0))


def rotate_float(plane: np.ndarray, deg: float, kind: str = "bilinear", expand: bool = False) -> np.ndarray:
    """A float rotation of a uint8 plane about its centre, as an editor does it: canvas of the same size (corners cut) or
    expanded to hold the whole frame, pixels outside the source 0, bilinear or Catmull-Rom sampling in float64, round half up.
    attacked(d) = plane(R(-deg) d): the rule's theta = +deg restores it."""
    H, W = plane.shape
    h, w = expanded_shape(H, W, deg) if expand else (H, W)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    yc = (np.arange(h, dtype=np.float64) - (h - 1) / 2.0)[:, None]
    xc = (np.arange(w, dtype=np.float64) - (w - 1) / 2.0)[None, :]
    xs = c * xc + s * yc + (W - 1) / 2.0
    ys = -s * xc + c * yc + (H - 1) / 2.0
    pad = 3
    src = np.zeros((H + 2 * pad, W + 2 * pad), np.float64)
    src[pad:-pad, pad:-pad] = plane
    inside = (xs > -1.0) & (xs < W) & (ys > -1.0) & (ys < H)
    xs, ys = np.clip(xs, -1.0, W), np.clip(ys, -1.0, H)
    x0, y0 = np.floor(xs).astype(I64), np.floor(ys).astype(I64)
    tx, ty = xs - x0, ys - y0
    if kind == "bilinear":
        offs, wx, wy = (0, 1), (1.0 - tx, tx), (1.0 - ty, ty)
    elif kind == "cubic":
        offs = (-1, 0, 1, 2)
        wx, wy = [_cubic(tx - o) for o in offs], [_cubic(ty - o) for o in offs]
    else:
        raise ValueError(kind)
    out = np.zeros((h, w), np.float64)
    for j, oy in enumerate(offs):
        for i, ox in enumerate(offs):
            out += wy[j] * wx[i] * src[y0 + oy + pad, x0 + ox + pad]
    out = np.where(inside, out, 0.0)
    return np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def attacked(cover: tuple, delta: float, dither: bool, deg: float, kind: str, expand: bool) -> np.ndarray:
    a = rotate_float(np.asarray(rr.marked(cover, delta, dither)), deg, kind, expand)
    a.setflags(write=False)
    return a


# ---- the search ------------------------------------------------------------------------------------------------------
def schedule_ref(H: int, W: int, max_angle: float, around=None) -> tuple:
    """(numerators, denominator): theta = numerator / denominator"""
    R = math.hypot(H, W) / 2.0
    if around is None:
        n = int(math.floor(math.radians(max_angle) * R))
        return list(range(-n, n + 1)), R
    return [8 * around + j for j in range(-8, 9)], 8.0 * R


def pick_ref(scores, counts):
    best = None
    for a, (s, n) in enumerate(zip(scores, counts)):
        if n > 0 and (best is None or int(s) * best[2] > best[1] * int(n)):
            best = (a, int(s), int(n))
    return None if best is None else best[0]


def read_ref(plane: np.ndarray, H: int, W: int, theta: float, u, delta: float) -> tuple:
    """(metric float32 [nby, nbx], valid bool [nby, nbx], score, count) of one candidate"""
    C, S = candidate_ref(theta)
    m = pdr.metric_ref(rotate_ref(plane, H, W, C, S), u, delta)
    ok = valid_ref(H, W, *plane.shape, C, S)
    votes = np.rint(np.abs(m).astype(np.float32) * np.float32(VOTE_ONE)).astype(I64)
    return m, ok, int(votes[ok].sum()), int(ok.sum())


def decode_ref(m: np.ndarray, ok: np.ndarray, H: int, W: int, code: int = 0) -> dict:
    """the winner's metrics and mask -> what the search's tail makes of them"""
    bits, carried, tbi, order, offs, _ = rr.plan(H, W, code)
    votes = np.where(ok, np.rint(m.astype(np.float32) * np.float32(VOTE_ONE)).astype(I64), 0)
    soft, count = P.soft_of_votes(votes, tbi.reshape(m.shape), carried.size)
    got = rr.decode_k7_ref(P.quantise_soft(soft)) if code else soft < 0
    data, valid = P.payload_unframe(got)
    tile_bit = carried[tbi].reshape(m.shape)
    return dict(data=data, valid=bool(valid), confidence=P.sync_confidence(soft, count), soft=soft,
                wrong_bits=int(np.count_nonzero((soft < 0) != (carried != 0))),
                wrong_votes=int(np.count_nonzero(ok & (votes != 0) & ((votes < 0) != (tile_bit != 0)))),
                min_valid_tiles_per_bit=int(np.bincount(tbi.reshape(-1)[ok.reshape(-1)], minlength=carried.size).min()))


def search_plane_ref(plane: np.ndarray, H: int, W: int, delta: float, dither: bool, max_angle: float = MAX_ANGLE, code: int = 0) -> dict:
    """the whole rule on the restatement: a uint8 plane [h, w] searched over the two stages, the fine winner decoded"""
    u = rr.table(H, W, dither)
    stages, around = [], None
    for _ in range(2):
        nums, den = schedule_ref(H, W, max_angle, around)
        reads = [read_ref(plane, H, W, k / den, u, delta) for k in nums]
        scores, counts = [r[2] for r in reads], [r[3] for r in reads]
        win = pick_ref(scores, counts)
        stages.append(dict(nums=nums, den=den, scores=scores, counts=counts, win=win))
        around = nums[win]
    coarse, fine = stages
    m, ok = reads[win][:2]
    out = decode_ref(m, ok, H, W, code)
    mean = [s / (VOTE_ONE * n) if n else 0.0 for s, n in zip(coarse["scores"], coarse["counts"])]
    far = [v for k, v in zip(coarse["nums"], mean) if abs(k - coarse["nums"][coarse["win"]]) >= 4]
    out.update(theta=fine["nums"][fine["win"]] / fine["den"], step=1.0 / coarse["den"], coarse=coarse, fine=fine,
               score=fine["scores"][fine["win"]] / (VOTE_ONE * fine["counts"][fine["win"]]), far=max(far),
               valid_tiles=fine["counts"][fine["win"]], metric=m, mask=ok)
    out["angle"] = math.degrees(out["theta"])
    return out


@functools.lru_cache(maxsize=None)
def search_ref(cover: tuple, delta: float, dither: bool, deg: float, kind: str, expand: bool, max_angle: float = MAX_ANGLE,
               code: int = 0) -> dict:
    """search_plane_ref of attacked(...); steps_off: the found angle's distance from the true one in coarse steps"""
    H, W, _ = cover
    out = search_plane_ref(np.asarray(attacked(cover, delta, dither, deg, kind, expand)), H, W, delta, dither, max_angle, code)
    out["steps_off"] = abs(out["theta"] - math.radians(deg)) / out["step"]
    return out
