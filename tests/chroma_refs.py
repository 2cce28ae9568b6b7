"""NumPy statement of the colour video frame codec for subsampled chroma (video.py, csrc/wm_pixel.hip k_frame_codec).

A stored frame is Y [H, W], Cb [ch, cw], Cr [ch, cw] packed, ch x cw = ceil(H / sy) x ceil(W / sx), sub = (sx, sy):
(1, 1) for 4:4:4, (2, 1) for 4:2:2, (2, 2) for 4:2:0.
  decode: chroma replicated to full resolution, then the oracle's YCrCb -> BGR per pixel -> planar B, G, R
  encode: the oracle's BGR -> YCrCb per pixel, Y as is, Cb / Cr the mean over the pixels of each sx x sy block that lie
          inside the plane, rounded half up in integers: (2 sum + cnt) // (2 cnt)
"""
import numpy as np

from oracle import wm_oracle as o

SUBS = ((1, 1), (2, 1), (2, 2))


def chroma_shape(H: int, W: int, sub):
    sx, sy = sub
    return -(-H // sy), -(-W // sx)


def frame_bytes(H: int, W: int, sub) -> int:
    ch, cw = chroma_shape(H, W, sub)
    return H * W + 2 * ch * cw


def replicate(c: np.ndarray, H: int, W: int, sub) -> np.ndarray:
    """chroma [..., ch, cw] -> [..., H, W]: out[r, c] = in[r // sy, c // sx]"""
    sx, sy = sub
    return np.repeat(np.repeat(c, sy, axis=-2), sx, axis=-1)[..., :H, :W]


def box_down(p: np.ndarray, sub) -> np.ndarray:
    """plane [..., H, W] uint8 -> [..., ch, cw] uint8: mean over the pixels of each block that exist, half up"""
    sx, sy = sub
    H, W = p.shape[-2:]
    ch, cw = chroma_shape(H, W, sub)
    pad = [(0, 0)] * (p.ndim - 2) + [(0, ch * sy - H), (0, cw * sx - W)]
    total = np.pad(p.astype(np.int64), pad).reshape(p.shape[:-2] + (ch, sy, cw, sx)).sum(axis=(-3, -1))
    cnt = np.pad(np.ones((H, W), np.int64), pad[-2:]).reshape(ch, sy, cw, sx).sum(axis=(1, 3))
    return ((2 * total + cnt) // (2 * cnt)).astype(np.uint8)


def split_frames(frames: np.ndarray, H: int, W: int, sub):
    """frames uint8 [n, fsz] -> (Y [n, H, W], Cb [n, ch, cw], Cr [n, ch, cw])"""
    ch, cw = chroma_shape(H, W, sub)
    n = frames.shape[0]
    assert frames.shape == (n, frame_bytes(H, W, sub))
    y = frames[:, :H * W].reshape(n, H, W)
    cb = frames[:, H * W:H * W + ch * cw].reshape(n, ch, cw)
    cr = frames[:, H * W + ch * cw:].reshape(n, ch, cw)
    return y, cb, cr


def decode_frames(frames: np.ndarray, H: int, W: int, sub) -> np.ndarray:
    """stored frames uint8 [n, fsz] -> B, G, R planes uint8 [n, 3, H, W]"""
    y, cb, cr = split_frames(frames, H, W, sub)
    ycc = np.stack([y, replicate(cr, H, W, sub), replicate(cb, H, W, sub)], axis=-1)       # OpenCV order: Y, Cr, Cb
    return np.ascontiguousarray(np.moveaxis(o.ycrcb_to_bgr(ycc), -1, 1))


def encode_frames(planes: np.ndarray, sub) -> np.ndarray:
    """B, G, R planes uint8 [n, 3, H, W] -> stored frames uint8 [n, fsz]"""
    n = planes.shape[0]
    ycc = o.bgr_to_ycrcb(np.moveaxis(planes, 1, -1))
    y, cr, cb = ycc[..., 0], ycc[..., 1], ycc[..., 2]
    return np.concatenate([y.reshape(n, -1), box_down(cb, sub).reshape(n, -1), box_down(cr, sub).reshape(n, -1)], axis=1)
