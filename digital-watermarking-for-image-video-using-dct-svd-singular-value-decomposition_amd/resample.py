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


def check_resize(h: int, w: int, H: int, W: int, noun: str = "stego") -> None:
    """an h x w ``noun`` that the rule can bring back to H x W, or a ValueError"""
    try:
        check_scale(h, H, "rows"); check_scale(w, W, "columns")
    except ValueError as e:
        raise ValueError(f"{noun} is {w}x{h} and the meta was written for {W}x{H}: {e}") from None
