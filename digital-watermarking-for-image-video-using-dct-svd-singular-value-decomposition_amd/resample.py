"""The integer resampler of the blind payload's resize resynchronisation (include/wmhip.h, "resize resynchronisation";
DESIGN.md section 14): its tap tables.  Device-free, float64 on the host; what the device does with the tables is integer
work, so the device and a NumPy restatement of the rule agree to the bit.

One axis, n_in -> n_out samples:
    scale = n_in / n_out;  fs = max(scale, 1);  sup = 2 fs;  T = 2 ceil(sup) + 1            (5 when enlarging, at most 33)
    output i:  c = (i + 0.5) scale;  lo = max(0, int(c - sup + 0.5));  hi = min(n_in, int(c + sup + 0.5))
               f_k = cubic((k + 0.5 - c) / fs) for k in [lo, hi), normalised to sum 1        (Catmull-Rom, a = -0.5)
               iw_k = rint(f_k 2^14); the residue 2^14 - sum iw goes to the largest tap, the first of equals
    first[i] = lo;  w[i] = the iw_k, then zeros
    out[i] = clip((sum_t w[i][t] px[min(first[i] + t, n_in - 1)] + 2^13) >> 14, 0, 255)      (int32, a floor shift)
A plane goes through the horizontal pass into a uint8 intermediate, then through the vertical one.

Below, for the rotation resynchronisation ("rotation resynchronisation" there): the 256-phase weight table K of the integer
rotation and the (C, S) = rint((cos, sin) 2^16) of a candidate angle.
"""
from __future__ import annotations

import functools
import math

import numpy as np

MAX_SCALE = 8                                       # n_in / n_out and n_out / n_in, on either axis
WEIGHT_BITS = 14
WEIGHT_ONE = 1 << WEIGHT_BITS
MAX_TAPS = 2 * 2 * MAX_SCALE + 1                    # 33
_A = -0.5


def cubic(x):
    """the Catmull-Rom kernel (a = -0.5) of float64 x"""
    x = np.abs(np.asarray(x, np.float64))
    near = ((_A + 2.0) * x - (_A + 3.0)) * x * x + 1.0
    far = _A * (((x - 5.0) * x + 8.0) * x - 4.0)
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def check_scale(n_in: int, n_out: int, what: str = "axis") -> None:
    """both sizes positive and within MAX_SCALE of each other, or a ValueError"""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"{what}: sizes must be positive, got {n_in} -> {n_out}")
    if n_in > MAX_SCALE * n_out or n_out > MAX_SCALE * n_in:
        raise ValueError(f"{what}: {n_in} -> {n_out} is a resize beyond {MAX_SCALE}x")


@functools.lru_cache(maxsize=16)
def _taps(n_in: int, n_out: int) -> tuple:
    scale = n_in / n_out
    fs = max(scale, 1.0)
    sup = 2.0 * fs
    T = 2 * math.ceil(sup) + 1
    first = np.zeros(n_out, np.int32)
    w = np.zeros((n_out, T), np.int16)
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = max(0, int(c - sup + 0.5))
        hi = min(n_in, int(c + sup + 0.5))
        f = cubic((np.arange(lo, hi) + 0.5 - c) / fs)
        f = f / f.sum()
        iw = np.rint(f * WEIGHT_ONE).astype(np.int64)
        iw[int(np.argmax(iw))] += WEIGHT_ONE - int(iw.sum())
        first[i] = lo
        w[i, :hi - lo] = iw
    first.setflags(write=False); w.setflags(write=False)
    return first, w


def resample_taps(n_in: int, n_out: int) -> tuple:
    """(first int32 [n_out], w int16 [n_out, T]) of one axis, by the rule above; read-only, memoised"""
    check_scale(n_in, n_out)
    return _taps(int(n_in), int(n_out))


# ---- rotation resynchronisation (include/wmhip.h, "rotation resynchronisation"): the weights and the candidates ---------------
ROTATE_PHASES = 256
ROTATE_MAX_SIDE = 8192
ANGLE_ONE = 1 << 16


@functools.lru_cache(maxsize=1)
def rotate_weights() -> np.ndarray:
    """K int16 [256, 4]: row f is Catmull-Rom at offsets -1, 0, 1, 2 for phase f / 256, rint(. 2^14), the residue to 2^14 added
    to the largest tap, the first of equals; K[0] = (0, 2^14, 0, 0).  Read-only, memoised."""
    t = np.arange(ROTATE_PHASES, dtype=np.float64)[:, None] / ROTATE_PHASES
    iw = np.rint(cubic(t + 1.0 - np.arange(4)) * WEIGHT_ONE).astype(np.int64)
    big = np.argmax(iw, axis=1)                                            # (argmax: the first of equals)
    iw[np.arange(ROTATE_PHASES), big] += WEIGHT_ONE - iw.sum(axis=1)
    K = iw.astype(np.int16)
    K.setflags(write=False)
    return K


def angle_candidate(theta: float) -> tuple:
    """(C, S) of an angle in radians: rint(cos 2^16), rint(sin 2^16), float64 on the host"""
    return int(np.rint(math.cos(float(theta)) * ANGLE_ONE)), int(np.rint(math.sin(float(theta)) * ANGLE_ONE))


def angle_candidates_cs(thetas) -> np.ndarray:
    """int32 [n, 2]: angle_candidate of every theta"""
    return np.array([angle_candidate(t) for t in np.asarray(thetas, np.float64).reshape(-1)], np.int32).reshape(-1, 2)


def check_rotate(h: int, w: int, H: int, W: int, noun: str = "stego") -> None:
    """an h x w ``noun`` and an H x W frame whose every side the rotation's 32-bit coordinates hold, or a ValueError"""
    if min(int(h), int(w), int(H), int(W)) < 1 or max(int(h), int(w), int(H), int(W)) > ROTATE_MAX_SIDE:
        raise ValueError(f"{noun} is {w}x{h} for a {W}x{H} frame: a rotation takes sides in 1..{ROTATE_MAX_SIDE}")


def check_resize(h: int, w: int, H: int, W: int, noun: str = "stego") -> None:
    """an h x w ``noun`` that the rule can bring back to H x W, or a ValueError"""
    try:
        check_scale(h, H, "rows"); check_scale(w, W, "columns")
    except ValueError as e:
        raise ValueError(f"{noun} is {w}x{h} and the meta was written for {W}x{H}: {e}") from None
