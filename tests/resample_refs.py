"""Resize resynchronisation of the blind payload: the NumPy restatement of the integer resampler as include/wmhip.h states it
("resize resynchronisation"), the attackers the tests resize a stego with, and the restatement's decode of a restored plane,
built on the oracle's sigma and tests/payload_refs.py / payload_dither_refs.py.  The keyed tile-to-bit map, the frame and the
dither table are the product's own (payload.py under hostglue.derive_key): host code the GPU tests do not question.  Nothing
here touches the device.

    one axis   scale = n_in / n_out, fs = max(scale, 1), sup = 2 fs, T = 2 ceil(sup) + 1
               c = (i + 0.5) scale, lo = max(0, int(c - sup + 0.5)), hi = min(n_in, int(c + sup + 0.5))
               Catmull-Rom (a = -0.5) at (k + 0.5 - c) / fs, normalised, rint(. 2^14), the residue to the largest tap
    a pixel    clip((sum_t w[i][t] px[min(first[i] + t, n_in - 1)] + 2^13) >> 14, 0, 255), int32, floor shift
    a plane    the horizontal pass into uint8 [h_in, W_out], then the vertical pass
"""
import functools
import importlib
import math

import numpy as np

import __graft_entry__ as ge
import mask_refs as mr
import payload_dither_refs as pdr
import payload_refs as pr
from oracle import wm_oracle as o

P = importlib.import_module(ge.PKG_NAME + ".payload")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")

F = np.float32
ONE = 1 << 14
PASSWORD, NONCE, DATA = "pw", bytes([3] * 8), b"id"
COVER = (136, 200, 2)                                                       # mask_refs.host(H, W, seed): 17 x 25 tiles
SIZES = ((122, 180), (102, 150), (68, 100), (170, 250), (272, 400), (95, 200), (136, 199), (204, 120), (137, 200))
DELTA = 32.0
MARGIN_FLOOR = 0.15                                                         # the measured worst at delta 32 is 0.191
# (1 -> 9 and 9 -> 1 lie beyond the rule's 8x - 9 -> 1 would take 37 taps - and are refused; 1 <-> 8 are the one-sample shapes)
TAP_CASES = ((1, 8), (8, 1), (8, 64), (64, 8), (100, 75), (75, 100), (200, 199), (7, 7))


# ---- the rule --------------------------------------------------------------------------------------------------------
def cubic_ref(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return a * (((x - 5.0) * x + 8.0) * x - 4.0)
    return 0.0


@functools.lru_cache(maxsize=None)
def taps_ref(n_in: int, n_out: int) -> tuple:
    """(first int32 [n_out], w int16 [n_out, T]), one output and one tap at a time"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    sup = 2.0 * fs
    T = 2 * math.ceil(sup) + 1
    first = np.zeros(n_out, np.int32)
    w = np.zeros((n_out, T), np.int16)
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo, hi = max(0, int(c - sup + 0.5)), min(n_in, int(c + sup + 0.5))
        f = np.array([cubic_ref((k + 0.5 - c) / fs) for k in range(lo, hi)], np.float64)
        f = f / f.sum()
        iw = [int(v) for v in np.rint(f * ONE)]
        big = max(range(len(iw)), key=lambda k: (iw[k], -k))               # the largest, the first of equals
        iw[big] += ONE - sum(iw)
        first[i] = lo
        w[i, :len(iw)] = iw
    first.setflags(write=False); w.setflags(write=False)
    return first, w


def pass_acc(px: np.ndarray, first: np.ndarray, w: np.ndarray) -> np.ndarray:
    """the accumulators of one pass along the LAST axis of uint8 px [..., n_in] -> int64 [..., n_out]"""
    n_in = px.shape[-1]
    idx = np.minimum(first[:, None].astype(np.int64) + np.arange(w.shape[1]), n_in - 1)      # [n_out, T]
    return (px[..., idx].astype(np.int64) * w.astype(np.int64)).sum(axis=-1)


def round_acc(acc: np.ndarray) -> np.ndarray:
    assert np.abs(acc).max(initial=0) < 1 << 23
    return np.clip((acc + (ONE >> 1)) >> 14, 0, 255).astype(np.uint8)


def resample_ref(plane: np.ndarray, H: int, W: int, return_acc: bool = False):
    """uint8 [h, w] or [N, h, w] -> uint8 [N?, H, W]; ``return_acc``: (out, horizontal accumulators, vertical accumulators)"""
    assert plane.dtype == np.uint8 and plane.ndim in (2, 3)
    h, w = plane.shape[-2:]
    acc_h = pass_acc(plane, *taps_ref(w, W))                                # [.., h, W]
    mid = round_acc(acc_h)
    acc_v = np.swapaxes(pass_acc(np.swapaxes(mid, -1, -2), *taps_ref(h, H)), -1, -2)
    out = round_acc(acc_v)
    return (out, acc_h, acc_v) if return_acc else out


# ---- planes that reach both clips ------------------------------------------------------------------------------------
def checkerboard(h: int = 24, w: int = 40) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def step_edge(h: int = 24, w: int = 40) -> np.ndarray:
    """0 | 255 along a column, and 255 over 0 along a row: both passes overshoot on both sides"""
    p = np.zeros((h, w), np.uint8)
    p[:h // 2, w // 2:] = 255
    p[h // 2:, :w // 2] = 255
    return p


CLIP_SHAPES = ((37, 67), (24, 40), (12, 20), (9, 100))                      # what the clip planes are resampled to


# ---- the attackers ---------------------------------------------------------------------------------------------------
def bilinear_ref(plane: np.ndarray, H: int, W: int) -> np.ndarray:
    """a float bilinear resize without antialiasing (half-pixel centres, edges clamped, round half up)"""
    h, w = plane.shape

    def axis(n_in, n_out):
        x = np.clip((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0, n_in - 1.0)
        x0 = np.floor(x).astype(np.int64)
        return x0, np.minimum(x0 + 1, n_in - 1), x - x0
    y0, y1, fy = axis(h, H)
    x0, x1, fx = axis(w, W)
    p = plane.astype(np.float64)
    top = p[y0][:, x0] * (1 - fx) + p[y0][:, x1] * fx
    bot = p[y1][:, x0] * (1 - fx) + p[y1][:, x1] * fx
    return np.clip(np.floor(top * (1 - fy)[:, None] + bot * fy[:, None] + 0.5), 0, 255).astype(np.uint8)


ATTACKERS = {
    "rule": resample_ref,
    "bilinear": bilinear_ref,
    "area": lambda plane, H, W: hg.resize_area(plane, W, H),
}


def attack_bgr(bgr: np.ndarray, name: str, h: int, w: int) -> np.ndarray:
    """every channel of a BGR image through one attacker"""
    return np.stack([ATTACKERS[name](np.ascontiguousarray(bgr[..., c]), h, w) for c in range(3)], axis=-1)


# ---- the payload under test ----------------------------------------------------------------------------------------------
def key() -> bytes:
    return hg.derive_key(PASSWORD, NONCE)


@functools.lru_cache(maxsize=None)
def plan(H: int, W: int, code: int = 0) -> tuple:
    """(frame bits, carried bits, tile_bit_index, order, offs, tile_bit) of DATA on an H x W frame"""
    bits = P.payload_frame(DATA)
    carried = P.encode_k7(bits) if code else bits
    tbi, order, offs = P.payload_map(H // 8, W // 8, key(), carried.size)
    return bits, carried, tbi, order, offs, P.tile_bits(carried, tbi)


def table(H: int, W: int, dither: bool, frame_index: int = 0):
    """the dither words of a frame, or zeros: u = 0 is the dither-free rule bit for bit"""
    n = (H // 8) * (W // 8)
    return P.dither_table(H // 8, W // 8, key(), frame_index) if dither else np.zeros(n, np.uint16)


@functools.lru_cache(maxsize=None)
def marked(cover: tuple, delta: float, dither: bool) -> np.ndarray:
    """the restatement's stego plane of mask_refs.host(*cover)"""
    H, W, seed = cover
    st = pdr.embed_ref(mr.host(H, W, seed), plan(H, W)[5], table(H, W, dither), delta)["stego"]
    st.setflags(write=False)
    return st


def decode_ref(restored: np.ndarray, delta: float, dither: bool, code: int = 0, frame_index: int = 0) -> dict:
    """the restatement's decode of a restored plane [H, W] (or planes [N, H, W] of one frame index: an image)"""
    H, W = restored.shape[-2:]
    bits, carried, tbi, order, offs, _ = plan(H, W, code)
    planes = restored[None] if restored.ndim == 2 else restored
    u = table(H, W, dither, frame_index)
    m = np.stack([pdr.metric_ref(p, u, delta) for p in planes])
    soft = pr.soft_ref(m.reshape(len(planes), -1), order, offs)
    count = np.diff(offs) * len(planes)
    got = decode_k7_ref(P.quantise_soft(soft)) if code else soft < 0
    data, valid = P.payload_unframe(got)
    return dict(soft=soft, data=data, valid=bool(valid), margin=float(np.min(np.abs(soft) / count)),
                confidence=P.confidence(soft, offs, len(planes)),
                wrong_bits=int(np.count_nonzero((soft < 0) != (carried != 0))))


def decode_k7_ref(L: np.ndarray) -> np.ndarray:
    import payload_code_refs as cr
    return cr.viterbi_ref(L, len(L) // 2 - cr.TAIL)[0]


VIDEO = dict(shape=(72, 104), n_frames=4, frame_interval=2, size=(54, 78), seed=20)         # 9 x 13 = 117 tiles


def video_frames() -> np.ndarray:
    """the cover's luma frames, uint8 [n_frames, H, W]"""
    H, W = VIDEO["shape"]
    return np.stack([mr.host(H, W, VIDEO["seed"] + f) for f in range(VIDEO["n_frames"])])


@functools.lru_cache(maxsize=None)
def video_round_trip(dither: bool, delta: float = DELTA) -> dict:
    """The video case on the restatement: every frame_interval-th frame marked under its own frame index's table, all frames
    resized to VIDEO["size"] by the rule and restored by it, the marked frames' soft values added."""
    H, W = VIDEO["shape"]
    bits, carried, tbi, order, offs, tile_bit = plan(H, W)
    soft = np.zeros(carried.size, np.float64)
    marked_at = range(0, VIDEO["n_frames"], VIDEO["frame_interval"])
    for f in marked_at:
        u = table(H, W, dither, f)
        st = pdr.embed_ref(video_frames()[f], tile_bit, u, delta)["stego"]
        restored = resample_ref(resample_ref(st, *VIDEO["size"]), H, W)
        soft += pr.soft_ref(pdr.metric_ref(restored, u, delta).reshape(1, -1), order, offs)
    count = np.diff(offs) * len(marked_at)
    data, valid = P.payload_unframe(soft < 0)
    return dict(soft=soft, data=data, valid=bool(valid), margin=float(np.min(np.abs(soft) / count)),
                confidence=P.confidence(soft, offs, len(marked_at)))


@functools.lru_cache(maxsize=None)
def round_trip(cover: tuple, delta: float, dither: bool, attacker: str, size: tuple) -> dict:
    """marked -> attacked to ``size`` -> restored by the rule -> decoded, all on the restatement"""
    H, W, _ = cover
    attacked = ATTACKERS[attacker](np.asarray(marked(cover, delta, dither)), *size)
    return decode_ref(resample_ref(attacked, H, W), delta, dither)
