"""Video frame loop.

The reference's video modules exist only as CPython-3.12 bytecode
(``watermark/__pycache__/video_dct_svd.cpython-312.pyc``; names recovered from
its string table: ``embed_watermark_video(host_video_path, watermark_path,
output_video_path, metadata_path, alpha, frame_interval)``,
``extract_watermark_video``, ``detect_watermark_video``).  What they show is the
*shape* of the loop: the watermark is decomposed ONCE, every
``frame_interval``-th frame's luma is embedded with it, per-frame host singular
values go to the metadata, extraction averages over the marked frames.  That
shape is built here on the tile-mode kernels, batched: one K3 launch per
watermark, one K1 launch per batch of frames with the watermark sigma shared
(``sigma_w_plane_stride = 0``).

Container: YUV4MPEG2 (``.y4m``) - uncompressed planar YUV, readable and
writable with NumPy alone (there is no OpenCV / ffmpeg in this image; the
reference uses ``cv2.VideoCapture`` / ``VideoWriter('mp4v')``).  The luma plane
IS the "Y channel" the hot path works on, so no colour conversion is involved.
Arrays of frames (``[N, H, W]`` uint8 luma) are accepted directly as well.
"""
from __future__ import annotations

import collections
import os
from typing import Iterator, Optional, Tuple

import numpy as np

from . import hostapi
from . import hostglue as hg
from . import meta as M
from . import payload as P
from . import payload_flow as F
from . import resample as R
from . import sharding

TILE = M.TILE


# ---------------------------------------------------------------------------
# YUV4MPEG2
# ---------------------------------------------------------------------------
_CHROMA_DIV = {"420": (2, 2), "420jpeg": (2, 2), "420mpeg2": (2, 2), "420paldv": (2, 2),
               "422": (2, 1), "444": (1, 1), "mono": (0, 0)}


class Y4M:
    """Minimal 8-bit YUV4MPEG2 reader: header fields + per-frame (Y, U, V) planes."""

    def __init__(self, path: str):
        self.path = path
        self._f = open(path, "rb")
        head = self._f.readline()
        if not head.startswith(b"YUV4MPEG2"):
            raise ValueError(f"Không mở được video: {path}")
        self.fields = head.decode("ascii", "replace").split()[1:]
        self.W = self.H = 0
        self.chroma = "420"
        for tok in self.fields:
            if tok[0] == "W": self.W = int(tok[1:])
            elif tok[0] == "H": self.H = int(tok[1:])
            elif tok[0] == "C": self.chroma = tok[1:]
        if self.chroma not in _CHROMA_DIV:
            raise ValueError(f"unsupported Y4M chroma format C{self.chroma} (8-bit 420/422/444/mono only)")
        dx, dy = _CHROMA_DIV[self.chroma]
        self.cw, self.ch = ((self.W + dx - 1) // dx, (self.H + dy - 1) // dy) if dx else (0, 0)
        self.header_line = head

    def __iter__(self) -> Iterator[Tuple[bytes, np.ndarray, np.ndarray]]:
        ysz, csz = self.W * self.H, self.cw * self.ch
        while True:
            line = self._f.readline()
            if not line:
                return
            if not line.startswith(b"FRAME"):
                raise ValueError("corrupt Y4M stream (FRAME marker expected)")
            buf = self._f.read(ysz + 2 * csz)
            if len(buf) < ysz + 2 * csz:
                raise ValueError("truncated Y4M frame")
            y = np.frombuffer(buf, np.uint8, ysz).reshape(self.H, self.W)
            yield line, y, np.frombuffer(buf, np.uint8, 2 * csz, ysz)

    def close(self):
        self._f.close()


def write_y4m(path: str, frames_y: np.ndarray, chroma: Optional[np.ndarray] = None, fps: str = "25:1",
              chroma_tag: Optional[str] = None):
    """Write luma frames [N, H, W] (+ optional packed chroma bytes per frame)."""
    n, H, W = frames_y.shape
    tag = chroma_tag or ("mono" if chroma is None else "420")
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F{fps} Ip A1:1 C{tag}\n".encode("ascii"))
        for i in range(n):
            f.write(b"FRAME\n")
            f.write(np.ascontiguousarray(frames_y[i]).tobytes())
            if chroma is not None:
                f.write(np.ascontiguousarray(chroma[i]).tobytes())


# ---------------------------------------------------------------------------
# array level: batches of luma frames
# ---------------------------------------------------------------------------
def prepare_watermark(ctx: hostapi.Context, wm_bgr: np.ndarray, H: int, W: int, key: bytes,
                      tile: Optional[int] = TILE):
    """resize -> gray -> keyed pixel shuffle -> SVD of its DCT, once per video.
    tile=8: per-tile factors; tile=None: the reference's full-plane factors."""
    wm = hg.resize_area(wm_bgr, W, H)
    idx = hg.permutation_index(H, W, key)
    wy_s = ctx.permute_planes(hg.bgr_to_gray(wm), idx)                 # single:66-72, index pass on the device
    Uw, Sw, Vwt = ctx.svd_tiles(wy_s) if tile else ctx.ref_svd(wy_s, apply_dct=True)
    return Uw, Sw, Vwt, idx


def _embed_frames_into(ctx: hostapi.Context, frames_y: np.ndarray, Sw: np.ndarray, alpha: float, K: int, batch: int,
                       tile: Optional[int], stego: np.ndarray, mask=None) -> np.ndarray:
    """embed_frames with the stego frames written into ``stego`` ([N, H, W], may be strided); returns Sc."""
    M.check_strength("uniform" if mask is None else "masked", mask, tile)
    n, H, W = frames_y.shape
    sc = np.empty((n, H // TILE, W // TILE, 8) if tile else (n, min(H, W)), np.float32)
    for b0 in range(0, n, batch):
        if tile:
            s, c, _ = ctx.embed_tiles(frames_y[b0:b0 + batch], Sw, alpha, K, mask=mask)
        else:
            s, c, _ = ctx.ref_embed_planes(frames_y[b0:b0 + batch], Sw, alpha, K)
        stego[b0:b0 + batch] = s; sc[b0:b0 + batch] = c
    return sc


def embed_frames(ctx: hostapi.Context, frames_y: np.ndarray, Sw: np.ndarray, alpha: float, K: int = 8,
                 batch: int = 32, tile: Optional[int] = TILE, mask=None):
    """frames_y uint8 [N, H, W] -> (stego [N, H, W], Sc); one set of launches per batch.
    tile=8: Sc [N, nby, nbx, 8] (K1); tile=None: Sc [N, min(H, W)] (batched full-plane SVDs).
    ``mask=(lo, hi, cut)``: texture-masked strength (tile mode), every frame with the gain of its own tiles."""
    stego = np.empty_like(frames_y)
    return stego, _embed_frames_into(ctx, frames_y, Sw, alpha, K, batch, tile, stego, mask)


def extract_frames_mean(ctx: hostapi.Context, frames_y: np.ndarray, Sc: np.ndarray, Uw, Vwt, alpha: float,
                        K: int = 8, batch: int = 32, tile: Optional[int] = TILE, mask=None) -> np.ndarray:
    """Mean over frames of the scrambled-watermark estimates (float32 [H, W]).  With ``mask`` every frame's estimate
    follows the masked rule with that frame's own gains; the multi-frame estimate stays the PLAIN mean of the per-frame
    estimates (a tile that some frames do not carry contributes zeros there: no weighting by carried counts)."""
    M.check_strength("uniform" if mask is None else "masked", mask, tile)
    n, H, W = frames_y.shape
    acc = np.zeros((H, W), np.float64)
    for b0 in range(0, n, batch):
        if tile:      # the batch's estimates are added on the device: one plane per batch crosses PCIe
            acc += ctx.extract_tiles(frames_y[b0:b0 + batch], Sc[b0:b0 + batch], Uw, Vwt, alpha, K, sum_planes=True, mask=mask)
        else:
            w = ctx.ref_extract_planes(frames_y[b0:b0 + batch], Sc[b0:b0 + batch], Uw, Vwt, alpha, K)
            acc += w.sum(axis=0, dtype=np.float64)
    return (acc / max(n, 1)).astype(np.float32)


def detect_frames(ctx: hostapi.Context, frames_y: np.ndarray, Sc: np.ndarray, Sw: np.ndarray, alpha: float,
                  batch: int = 32, tile: Optional[int] = TILE, mask=None) -> np.ndarray:
    """Per-frame NC scores; ``mask``: over the values the masked rule takes (tile mode)."""
    M.check_strength("uniform" if mask is None else "masked", mask, tile)
    scores = np.empty(frames_y.shape[0], np.float64)
    for b0 in range(0, frames_y.shape[0], batch):
        if tile:
            scores[b0:b0 + batch] = ctx.detect_tiles(frames_y[b0:b0 + batch], Sc[b0:b0 + batch], Sw, alpha, mask=mask)
        else:
            scores[b0:b0 + batch] = ctx.ref_detect_planes(frames_y[b0:b0 + batch], Sc[b0:b0 + batch], Sw, alpha)
    return scores


def embed_frames_sharded(ctx: hostapi.Context, frames_y: np.ndarray, Sw: np.ndarray, alpha: float, K: int = 8,
                         rank: int = 0, world_size: int = 1, batch: int = 32, tile: Optional[int] = TILE, mask=None):
    """This rank's share [r*N//W, (r+1)*N//W) of a batch of frames (no collective:
    the watermark sigma was broadcast beforehand, sharding.broadcast_watermark)."""
    lo, hi = sharding.frame_range(rank, world_size, frames_y.shape[0])
    stego, sc = embed_frames(ctx, frames_y[lo:hi], Sw, alpha, K, batch, tile, mask)
    return (lo, hi), stego, sc


# ---------------------------------------------------------------------------
# colour frames.  The reference's ``color_video_dct_svd`` module is bytecode-only too (``embed_watermark_video_color`` /
# ``extract_watermark_video_color``); its source is not in the tree, so the SHAPE is the colour image embed of single:121-166
# put into the luma loop: the colour watermark's B, G, R planes are decomposed ONCE, every marked frame's B, G, R planes
# are embedded with them, per-frame host singular values per channel go to the metadata, extraction averages over the marked
# frames per channel.  Container: 8-bit 4:4:4 ``.y4m`` (planes Y, Cb, Cr); the frames pass through OpenCV's fixed-point
# YCrCb <-> BGR conversion on the device (``wm_color_u8``) on the way in and out, so - like any YUV container - the stored
# stego differs from the embedded BGR planes by that conversion's rounding (a grey level or two per channel).  No audio remux.
#
# 4:2:0 (``C420``, ``C420jpeg``, ``C420mpeg2``, ``C420paldv``) and 4:2:2 (``C422``) containers, ``subsampling="box"``: the
# chroma planes are ceil(H / sy) x ceil(W / sx).  On the way in every pixel takes the chroma sample of its block (replication),
# then the same YCrCb -> BGR conversion; on the way out BGR -> YCrCb, Y stored as is, Cb and Cr each the mean over the pixels
# of their sx x sy block that lie inside the plane, rounded half up in integers ((2 sum + cnt) // (2 cnt), cnt 1, 2 or 4).
# Averaging replicated chroma gives it back exactly, so a frame the embed did not change keeps its chroma bytes.  The
# siting the tag names (jpeg: centred, mpeg2: co-sited left, paldv) travels in the copied header line and is otherwise
# ignored: one filter for all of them.  Both directions run on the device for all marked frames of a flush in one call
# (``wm_yuv_frames_to_bgr_planes_u8`` / ``wm_bgr_planes_to_yuv_frames_u8``), planar on both sides.
# ---------------------------------------------------------------------------
def _frame_to_bgr_planes(ctx: hostapi.Context, y: np.ndarray, chroma: np.ndarray, H: int, W: int) -> np.ndarray:
    cb = chroma[:H * W].reshape(H, W); cr = chroma[H * W:].reshape(H, W)
    bgr = ctx.color("ycrcb2bgr", np.ascontiguousarray(np.stack([y, cr, cb], axis=-1)))       # OpenCV order: Y, Cr, Cb
    return np.ascontiguousarray(np.moveaxis(bgr, -1, 0))                                       # [3, H, W]: B, G, R


def _bgr_planes_to_frame(ctx: hostapi.Context, planes: np.ndarray):
    ycc = ctx.color("bgr2ycrcb", np.ascontiguousarray(np.moveaxis(planes, 0, -1)))
    return np.ascontiguousarray(ycc[..., 0]), np.ascontiguousarray(ycc[..., 2]), np.ascontiguousarray(ycc[..., 1])   # Y, Cb, Cr


def prepare_watermark_color(ctx: hostapi.Context, wm_bgr: np.ndarray, H: int, W: int, key: bytes, tile: Optional[int] = TILE):
    """resize -> B, G, R planes -> ONE keyed pixel shuffle for all three (single:124-126) -> their three decompositions in one
    batched call.  Returns (Uw [3, ...], Sw [3, ...], Vwt [3, ...], idx)."""
    wm = hg.resize_area(wm_bgr, W, H)
    idx = hg.permutation_index(H, W, key)
    planes = ctx.permute_planes(np.ascontiguousarray(np.moveaxis(wm, -1, 0)), idx)
    if tile:
        Uw, Sw, Vwt = ctx.svd_tiles(planes)
    else:
        Uw, Sw, Vwt = ctx.ref_svd_planes(planes.astype(np.float32), apply_dct=True)
    return Uw, Sw, Vwt, idx


def embed_frames_color(ctx: hostapi.Context, planes: np.ndarray, Sw: np.ndarray, alpha: float, K: int = 8, batch: int = 8,
                       tile: Optional[int] = TILE, mask=None):
    """planes uint8 [n, 3, H, W] (B, G, R of n frames), Sw [3, ...] -> (stego [n, 3, H, W], [Sb, Sg, Sr]): channel c of every
    frame gets the watermark's channel c (single:139-152); one set of launches per channel and batch.  (Any number of
    channels: the luma loop passes [n, 1, H, W].)  ``mask``: as in embed_frames, one gain per channel plane."""
    st = np.empty_like(planes)
    sc = [_embed_frames_into(ctx, np.ascontiguousarray(planes[:, ch]), Sw[ch], alpha, K, batch, tile, st[:, ch], mask)
          for ch in range(planes.shape[1])]
    return st, sc


# ---------------------------------------------------------------------------
# file level (names of the reference's bytecode-only video modules).  One loop, one reader, one extract and one detect,
# over [n, C, H, W] planes; what differs between luma (C = 1), 4:4:4 colour and subsampled colour (C = 3) is the frame codec:
#   planes(ctx, [(y, chroma), ...], H, W) -> [n, C, H, W]      frame_bytes(ctx, stego [n, C, H, W], [chroma, ...]) -> per frame,
#   the byte strings that follow its FRAME line.  Both take all marked frames of a flush.
# ---------------------------------------------------------------------------
_Codec = collections.namedtuple("_Codec", "mode writer chroma prepare planes frame_bytes members")
# luma: the luma plane IS the plane the hot path works on ([1, H, W]); write-back replaces y and keeps the chroma bytes
_Luma = _Codec(
    mode="video_gray", writer="embed_watermark_video", chroma=None,
    prepare=lambda ctx, wm_bgr, H, W, key, tile: [x[None] for x in prepare_watermark(ctx, wm_bgr, H, W, key, tile)[:3]],
    planes=lambda ctx, frames, H, W: np.stack([y[None] for y, _ in frames]),
    frame_bytes=lambda ctx, st, chromas: [(p[0].tobytes(), c.tobytes()) for p, c in zip(st, chromas)],
    members=lambda S, Uw, Vwt, Sw: M.gray_members(S[0], Uw[0], Vwt[0], Sw[0]))
# 4:4:4 colour: the B, G, R planes of a frame ([3, H, W]); write-back converts the three stego planes to Y, Cb, Cr
_Bgr444 = _Codec(
    mode="video_color", writer="embed_watermark_video_color", chroma="444",
    prepare=lambda ctx, wm_bgr, H, W, key, tile: prepare_watermark_color(ctx, wm_bgr, H, W, key, tile)[:3],
    planes=lambda ctx, frames, H, W: np.stack([_frame_to_bgr_planes(ctx, y, chroma, H, W) for y, chroma in frames]),
    frame_bytes=lambda ctx, st, chromas: [[p.tobytes() for p in _bgr_planes_to_frame(ctx, planes)] for planes in st],
    members=M.channel_members)                                             # the colour image meta's key names (single:157-166)


def _bgr_subsampled(tag: str) -> _Codec:
    """Colour on a 4:2:0 / 4:2:2 container (tag as in the header, e.g. "420jpeg"): the B, G, R planes of all marked frames of
    a flush come from, and go back to, the stored frames through the device's frame codec, one call each way."""
    sub = _CHROMA_DIV[tag]

    def planes(ctx, frames, H, W):
        packed = np.empty((len(frames), ctx.frame_bytes(H, W, sub)), np.uint8)
        for f, (y, chroma) in zip(packed, frames):
            f[:H * W] = y.ravel(); f[H * W:] = chroma
        return ctx.yuv_frames_to_bgr_planes(packed, H, W, sub)

    return _Bgr444._replace(
        chroma=tag, planes=planes,
        frame_bytes=lambda ctx, st, chromas: [(f.tobytes(),) for f in ctx.bgr_planes_to_yuv_frames(st, sub)],
        members=lambda *arrays: dict(M.channel_members(*arrays), **M.chroma_members(tag)))


SUBSAMPLING = ("refuse", "box")


def _check_subsampling(subsampling) -> None:
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {SUBSAMPLING}, got {subsampling!r}")


def _container_codec(codec, vid: Y4M, accept, refusal: str) -> _Codec:
    """The codec that reads and writes this container, for a caller that takes the chroma formats ``accept`` (siting
    suffix stripped: "444", "420", "422").  The luma codec takes every container."""
    if not codec.chroma:
        return codec
    if M.chroma_format(vid.chroma) not in accept:
        raise ValueError(refusal)
    return codec if vid.chroma == codec.chroma else _bgr_subsampled(vid.chroma)


def _is_marked(i: int, frame_interval: int) -> bool:
    return i % max(1, int(frame_interval)) == 0


def _embed_frame_loop(vid: Y4M, out, frame_interval: int, batch: int, embed_marked) -> int:
    """The one embed loop: every frame of ``vid`` goes to the open file ``out`` behind its FRAME line, the unmarked ones
    byte for byte.  Frames are held until ``batch`` marked ones are pending; ``embed_marked([(y, chroma), ...])`` then
    returns, per marked frame and in order, the byte strings that follow its FRAME line.  Returns the frame count."""
    pend, n_frames = [], 0          # (frame_line, y, chroma, marked)

    def flush():
        marked = [p[1:3] for p in pend if p[3]]
        stored = iter(embed_marked(marked) if marked else ())
        for line, y, chroma, is_marked in pend:
            out.write(line)
            if is_marked:
                out.writelines(next(stored))
            else:
                out.write(y.tobytes()); out.write(chroma.tobytes())
        pend.clear()

    for line, y, chroma in vid:
        pend.append((line, y.copy(), chroma.copy(), _is_marked(n_frames, frame_interval)))
        n_frames += 1
        if len(pend) >= batch * max(1, frame_interval):
            flush()
    flush()
    return n_frames


def _marked_batches(vid: Y4M, frame_interval: int, batch: int, limit: Optional[int] = None):
    """The marked frames of ``vid`` in order, ``batch`` at a time: lists of (y, chroma); with ``limit`` the first that
    many marked frames only."""
    pend, seen = [], 0
    for i, (_, y, chroma) in enumerate(vid):
        if _is_marked(i, frame_interval) and (limit is None or seen < limit):
            pend.append((y, chroma)); seen += 1
            if len(pend) >= batch:
                yield pend
                pend = []
    if pend:
        yield pend


def _embed_video(codec, host_video_path, watermark_path, output_video_path, metadata_path, alpha, frame_interval,
                 password, nonce, kfrac, k_floor, batch, device, tile, subsampling="refuse", strength="uniform",
                 mask=M.MASK_DEFAULT):
    M.check_tile(tile)
    mask = M.check_strength(strength, mask, tile)                          # None: uniform
    M.require_password(password, "embed")
    _check_subsampling(subsampling)
    ctx = hostapi.Context(device)
    vid = Y4M(host_video_path)
    try:
        codec = _container_codec(codec, vid, ("444", "420", "422") if subsampling == "box" else ("444",),
                                 "embed_watermark_video_color needs an 8-bit 4:4:4 .y4m (C444): per-channel embedding "
                                 "needs full-resolution chroma")
        H, W = vid.H, vid.W
        if nonce is None:
            nonce = os.urandom(8)
        key = hg.derive_key(password, nonce)
        Uw, Sw, Vwt = codec.prepare(ctx, hg.read_image_bgr(watermark_path), H, W, key, tile)
        K = M.k_of(tile or min(H, W), kfrac, k_floor)                     # single:137, L = 8 per tile or min(H, W) per plane
        sc_all = [[] for _ in Sw]
        psnrs = []

        def embed_marked(marked):
            planes = codec.planes(ctx, marked, H, W)                                         # [n, C, H, W]
            st, sc = embed_frames_color(ctx, planes, Sw, alpha, K, batch, tile, mask)
            for ch, c in enumerate(sc):
                sc_all[ch].append(c)
            psnrs.extend(hg.psnr(planes[i], st[i]) for i in range(len(marked)))
            return codec.frame_bytes(ctx, st, [chroma for _, chroma in marked])

        with open(output_video_path, "wb") as out:
            out.write(vid.header_line)
            n_frames = _embed_frame_loop(vid, out, frame_interval, batch, embed_marked)
        empty = np.zeros((0, H // TILE, W // TILE, 8) if tile else (0, min(H, W)), np.float32)
        S = [np.concatenate(c) if c else empty for c in sc_all]
        members = {"mode": codec.mode, **M.common_members(H, W, alpha, kfrac, nonce),
                   **M.video_members(frame_interval, n_frames, tile, k_floor), **M.mask_members(mask),
                   **codec.members(S, Uw, Vwt, Sw)}
        digest = hg.hmac_digest(key, M.hmac_parts(members))                # the coverage of single:152-156,182
        # uncompressed .npz: the per-frame singular values are float noise to zlib (ratio ~1.1) and compressing them was
        # 80 % of this function's time (1.7 s for 64 frames of 1080p); np.load reads either form
        np.savez(metadata_path, **M.sealed(members, tile, digest))
        return output_video_path, metadata_path, float(np.mean(psnrs)) if psnrs else 99.0
    finally:
        vid.close(); ctx.close()


def _load_video_meta(codec, metadata_path: str):
    data = np.load(metadata_path, allow_pickle=False)
    M.refuse_payload(data, codec.writer.replace("embed", "extract / detect"))
    if str(data["mode"]) != codec.mode:
        raise ValueError("metadata was not written by " + codec.writer)
    return data


def _marked_planes(codec, ctx: hostapi.Context, stego_video_path: str, data, n: int, C: int, batch: int) -> np.ndarray:
    """The first n marked frames' planes, uint8 [n, C, H, W], decoded ``batch`` frames at a time.  The container must be what
    the meta was written for: a colour meta's ``chroma`` member, 4:4:4 when it has none."""
    vid = Y4M(stego_video_path)
    try:
        want = M.chroma_of(data)
        codec = _container_codec(codec, vid, (want,), "a colour-watermarked video is 4:4:4" if want == "444" else
                                 f"the metadata was written for a C{want} video, this one is C{vid.chroma}")
        out = [codec.planes(ctx, frames, vid.H, vid.W) for frames in _marked_batches(vid, int(data["frame_interval"]), batch, n)]
    finally:
        vid.close()
    if sum(len(p) for p in out) < n:
        raise ValueError("video has fewer marked frames than the metadata")
    return np.concatenate(out) if out else np.zeros((0, C) + tuple(map(int, data["shape"])), np.uint8)


def _extract_video(codec, stego_video_path, metadata_path, output_image_path, password, normalize, batch, device, enhance):
    M.check_enhance(enhance)
    M.require_password(password, "extract")
    data = _load_video_meta(codec, metadata_path)
    H, W = map(int, data["shape"])
    key = hg.derive_key(password, M.nonce_of(data))
    if not M.authentic(data, key):
        raise ValueError(M.WRONG_PASSWORD)
    ctx = hostapi.Context(device)
    try:
        factors = M.per_plane(data, "Sc", "Uw", "Vwt")
        planes = _marked_planes(codec, ctx, stego_video_path, data, factors[0][0].shape[0], len(factors), batch)
        tile = M.tile_of(data)
        K = M.k_of(tile or min(H, W), M.kfrac_of(data), M.k_floor_of(data))
        idx = hg.permutation_index(H, W, key)
        chans = []
        for ch, (Sc, Uw, Vwt) in enumerate(factors):
            w_s = extract_frames_mean(ctx, np.ascontiguousarray(planes[:, ch]), Sc, Uw, Vwt, float(data["alpha"]), K, batch, tile,
                                      M.mask_of(data))
            chans.append(ctx.unpermute_normalize_u8(w_s, idx, normalize))                    # single:74-80, 221-222, 265-271 on the device
        img = hg.apply_enhance(ctx, chans[0] if len(chans) == 1 else np.stack(chans, axis=-1), enhance)   # single:223-227, 275-277
    finally:
        ctx.close()
    output_image_path = M.out_name(output_image_path, "_wm.png")
    if not hg.write_png(output_image_path, img, 1):
        raise IOError("Ghi watermark thất bại.")
    return output_image_path


def _detect_video(codec, stego_video_path, metadata_path, thresh, batch, device):
    data = _load_video_meta(codec, metadata_path)
    ctx = hostapi.Context(device)
    try:
        sigmas = M.per_plane(data, "Sc", "Sw")
        planes = _marked_planes(codec, ctx, stego_video_path, data, sigmas[0][0].shape[0], len(sigmas), batch)
        tile = M.tile_of(data)
        per_ch = [detect_frames(ctx, np.ascontiguousarray(planes[:, ch]), Sc, Sw, float(data["alpha"]), batch, tile, M.mask_of(data))
                  for ch, (Sc, Sw) in enumerate(sigmas)]
    finally:
        ctx.close()
    scores = per_ch[0] if len(per_ch) == 1 else (per_ch[0] + per_ch[1] + per_ch[2]) / 3.0      # single:317
    mean = float(scores.mean()) if scores.size else 0.0
    return bool(mean >= thresh), mean, scores


def embed_watermark_video(host_video_path: str, watermark_path: str, output_video_path: str,
                          metadata_path: str, alpha: float = 0.1, frame_interval: int = 1, *,
                          password: str = "", nonce: Optional[bytes] = None, kfrac: float = hg.K_FRAC_DEFAULT,
                          k_floor: int = 8, batch: int = 32, device: int = 0, tile: Optional[int] = TILE,
                          strength: str = "uniform", mask=M.MASK_DEFAULT):
    """Embed the watermark into the luma of every ``frame_interval``-th frame of a
    .y4m video.  Returns (output_video_path, metadata_path, mean PSNR of marked frames).
    tile=8: 8x8-block formulation (fast path); tile=None: one SVD per frame like the reference's
    image embed (batched over the frames of a chunk; use a smaller ``batch``, e.g. 8).
    ``strength="masked"`` with ``mask=(lo, hi, cut)``: texture-masked strength as in dct_svd_core_secure.embed (tile mode);
    the meta carries the rule and extract / detect read it back."""
    return _embed_video(_Luma, host_video_path, watermark_path, output_video_path, metadata_path, alpha, frame_interval,
                        password, nonce, kfrac, k_floor, batch, device, tile, strength=strength, mask=mask)


def extract_watermark_video(stego_video_path: str, metadata_path: str, output_image_path: str,
                            password: str, normalize: bool = True, *, batch: int = 32, device: int = 0,
                            enhance=False) -> str:
    """Averaged multi-frame extraction -> watermark image (PNG).  ``enhance`` as in dct_svd_core_secure.extract.  A meta
    written with ``strength="masked"`` is extracted by its rule, frame by frame; the frames' estimates are then averaged
    plainly (extract_frames_mean)."""
    return _extract_video(_Luma, stego_video_path, metadata_path, output_image_path, password, normalize, batch, device, enhance)


def detect_watermark_video(stego_video_path: str, metadata_path: str, thresh: float = 0.6, *,
                           batch: int = 32, device: int = 0):
    """(bool, mean score, per-frame scores) over the marked frames; a masked meta is scored by its rule."""
    return _detect_video(_Luma, stego_video_path, metadata_path, thresh, batch, device)


def embed_watermark_video_color(host_video_path: str, watermark_path: str, output_video_path: str,
                                metadata_path: str, alpha: float = 0.1, frame_interval: int = 1, *,
                                password: str = "", nonce: Optional[bytes] = None, kfrac: float = hg.K_FRAC_DEFAULT,
                                k_floor: int = 8, batch: int = 8, device: int = 0, tile: Optional[int] = TILE,
                                subsampling: str = "refuse", strength: str = "uniform", mask=M.MASK_DEFAULT):
    """Embed a colour watermark into the B, G, R planes of every ``frame_interval``-th frame of a .y4m video.
    Returns (output_video_path, metadata_path, mean PSNR of the marked frames' BGR planes).
    ``subsampling``: what to do with a container whose chroma is subsampled.  "refuse" (default): only 4:4:4 (C444) is
    taken.  "box": 4:2:0 (C420, C420jpeg, C420mpeg2, C420paldv) and 4:2:2 (C422) are taken too - chroma is replicated to
    full resolution on the way in and box-averaged (half up) on the way out; the siting a C420* tag names is carried
    through in the header and otherwise ignored, one filter serves all of them.  The meta then names the chroma format
    and extract / detect read the same kind of container with nothing but the meta and the password.
    ``strength`` / ``mask``: as in embed_watermark_video, one gain per channel plane."""
    return _embed_video(_Bgr444, host_video_path, watermark_path, output_video_path, metadata_path, alpha, frame_interval,
                        password, nonce, kfrac, k_floor, batch, device, tile, subsampling, strength, mask)


def extract_watermark_video_color(stego_video_path: str, metadata_path: str, output_image_path: str, password: str,
                                  normalize: bool = True, *, batch: int = 8, device: int = 0, enhance=False) -> str:
    """Averaged multi-frame extraction per channel -> colour watermark image (PNG).  ``enhance`` as in
    dct_svd_core_secure.extract; a masked meta as in extract_watermark_video."""
    return _extract_video(_Bgr444, stego_video_path, metadata_path, output_image_path, password, normalize, batch, device, enhance)


def detect_watermark_video_color(stego_video_path: str, metadata_path: str, thresh: float = 0.6, *,
                                 batch: int = 8, device: int = 0):
    """(bool, mean score, per-frame scores): a frame's score is the mean of its three channels' NC (single:317); a masked
    meta is scored by its rule."""
    return _detect_video(_Bgr444, stego_video_path, metadata_path, thresh, batch, device)


# ---------------------------------------------------------------------------
# blind payload in the luma of a .y4m (payload.py, include/wmhip.h): every marked frame carries the same bits under the
# same tile-to-bit map, and the decoder adds the frames' soft votes.  The meta holds the rule, not the frames.
# ---------------------------------------------------------------------------
def payload_soft_frames(ctx: hostapi.Context, frames_y: np.ndarray, order, offs, n_bits: int, delta: float,
                        batch: int = 32, dither=None) -> np.ndarray:
    """soft [n_bits] float64 over all frames of uint8 [N, H, W]: one device call per batch, the batches' vectors added on
    the host in batch order.  ``dither``: uint16 [N, n_tiles], a row of keyed dither words per frame (None: dither-free)."""
    soft = np.zeros(int(n_bits), np.float64)
    for b0 in range(0, frames_y.shape[0], max(1, int(batch))):
        soft += ctx.payload_soft(frames_y[b0:b0 + batch], order, offs, n_bits, delta,
                                 dither=None if dither is None else dither[b0:b0 + batch])
    return soft


def _payload_frame_dithers(H: int, W: int, key: bytes, first_marked: int, n: int, frame_interval: int) -> np.ndarray:
    """uint16 [n, n_tiles]: the dither tables of n consecutive marked frames, the first of them the ``first_marked``-th
    marked frame of the file - frame index first_marked * frame_interval"""
    fi = max(1, int(frame_interval))
    return P.dither_tables(H // TILE, W // TILE, key, [(first_marked + i) * fi for i in range(n)])


def embed_payload_video(host_video_path: str, payload, output_video_path: str, metadata_path: str, *, password: str = "",
                        payload_type: str = "text", frame_interval: int = 1, delta: float = P.DELTA_DEFAULT,
                        nonce: Optional[bytes] = None, batch: int = 32, device: int = 0, verify: bool = True,
                        dither: bool = False, code=None):
    """Embed a text / JSON / bytes payload (``payload`` as in dct_svd_core_secure.embed_payload) into the luma of every
    ``frame_interval``-th frame of an 8-bit .y4m; chroma and unmarked frames are copied byte for byte.
    Returns (output_video_path, metadata_path, mean PSNR of the marked frames' luma).
    ``verify``: the soft votes of the marked stego frames are added up as they are written, and a payload that does not
    decode from them raises ValueError after the last frame; neither the output file nor the meta remains.
    ``dither``: keyed dither (dct_svd_core_secure.embed_payload_arrays); every marked frame gets a table of its own, keyed
    by the frame's index in the file, and a batch is one call with a table row per frame.
    ``code="k7"``: the channel code of dct_svd_core_secure.embed_payload_arrays; the frames' summed soft values go through
    ONE decode."""
    M.require_password(password, "embed")
    delta = hostapi.check_delta(delta)
    code = P.check_code(code)
    data = P.payload_bytes(payload, payload_type)
    batch = max(1, int(batch))
    vid = Y4M(host_video_path)
    ctx = None
    try:
        H, W = vid.H, vid.W
        if nonce is None:
            nonce = os.urandom(8)
        key = hg.derive_key(password, nonce)
        bits, carried, _, order, offs, tile_bit = F.embed_plan(data, code, H, W, key)
        ctx = hostapi.Context(device)
        psnrs = []
        soft = np.zeros(carried.size, np.float64)

        def embed_marked(marked):
            ys = np.stack([y for y, _ in marked])
            # the marked frames arrive in file order: the m-th of them is frame m * frame_interval
            dz = _payload_frame_dithers(H, W, key, len(psnrs), len(marked), frame_interval) if dither else None
            st, _, _ = ctx.embed_tiles_payload(ys, tile_bit, delta, dither=dz)
            psnrs.extend(hg.psnr(ys[i], st[i]) for i in range(len(marked)))
            if verify:
                np.add(soft, payload_soft_frames(ctx, st, order, offs, carried.size, delta, batch, dither=dz), out=soft)
            return [(s.tobytes(), chroma.tobytes()) for s, (_, chroma) in zip(st, marked)]

        with open(output_video_path, "wb") as out:
            out.write(vid.header_line)
            n_frames = _embed_frame_loop(vid, out, frame_interval, batch, embed_marked)
        if verify and psnrs:
            try:
                P.check_decodes(soft, bits, data, F.read(ctx, soft, code) if code else None)
            except ValueError:
                os.remove(output_video_path)
                raise
        members = M.payload_members(payload_type, H, W, delta, bits.size, nonce, frame_interval, n_frames,
                                    dither=P.DITHER_TABLE if dither else 0, code=code)
        M.save_payload_meta(metadata_path, M.sealed(members, TILE, hg.hmac_digest(key, M.hmac_parts(members))))
        return output_video_path, metadata_path, float(np.mean(psnrs)) if psnrs else 99.0
    finally:
        vid.close()
        if ctx is not None:
            ctx.close()


VIDEO_SEARCHES = (None, P.SEARCH_CLIP)                                     # the search for a cut, cropped clip
SEARCH_RESIZE = "resize"                                                   # no search: the meta's shape says what to restore


def _count_frames(vid: Y4M) -> int:
    """the whole frames of an open Y4M's file, by its FRAME lines alone: no frame is read"""
    size = os.path.getsize(vid.path)
    step = vid.W * vid.H + 2 * vid.cw * vid.ch
    n = 0
    with open(vid.path, "rb") as f:
        f.readline()
        while f.readline().startswith(b"FRAME") and f.tell() + step <= size:
            f.seek(step, os.SEEK_CUR)
            n += 1
    return n


def _extract_payload_clip(vid: Y4M, rule: F.Rule, batch: int, device: int, anchors: int, return_soft: bool):
    """search="clip" (include/wmhip.h, "clip resynchronisation"): the file is a run of consecutive frames of a video marked
    with dither=True, every frame cropped to the same rectangle.  Every refusal comes before the first device call; the
    frames are read once."""
    if not rule.dither:
        raise ValueError("search='clip' reads a payload embedded with dither=True; this one has none")
    anchors = int(anchors)
    if anchors < 1:
        raise ValueError(f"anchors must be at least 1, got {anchors}")
    h, w, n_f = vid.H, vid.W, rule.n_frames
    F.check_crop_shape(h, w, rule.H, rule.W, "clip")
    n_c = _count_frames(vid)
    if n_c > n_f:
        raise ValueError(f"clip has {n_c} frames, the marked video had {n_f}: not a cut of it")
    if n_c < 1:
        raise ValueError("clip has no frame")
    fi = max(1, rule.frame_interval)
    nby, nbx = rule.grid
    A = min(n_c, anchors * fi)
    table_of = P.clip_table_of(n_f, fi, n_c, A)
    n_tables = (n_f + fi - 1) // fi
    tables = P.dither_tables(nby, nbx, rule.key, [k * fi for k in range(n_tables)]).reshape(n_tables, nby, nbx)
    tbi = rule.map()[0].reshape(nby, nbx)
    frames = iter(vid)
    held = [y for _, (_, y, _) in zip(range(A), frames)]                   # the anchors, kept for the decode
    ctx = hostapi.Context(device)
    try:
        _, win = ctx.payload_locate_clip(np.stack(held), tables, table_of, rule.delta, pick=True)
        if win is None:                                                    # (n_c < fi and no candidate with a marked frame among the anchors)
            out = (b"", False, 0.0, None, None)
            return out + (np.zeros(rule.carried, np.float64),) if return_soft else out
        t0, (py, px), (ty, tx) = win
        ny, nx = (h - py) // TILE, (w - px) // TILE
        votes = np.zeros((ny, nx), np.int64)
        n_marked = 0

        def decode(pend):
            ys = np.stack([y[py:py + TILE * ny, px:px + TILE * nx] for _, y in pend])
            dz = np.stack([tables[(t0 + i) // fi, ty:ty + ny, tx:tx + nx].reshape(-1) for i, _ in pend])
            m = ctx.payload_metric(ys, rule.delta, dither=dz)
            np.add(votes, np.rint(m * np.float32(P.VOTE_ONE)).astype(np.int64).sum(axis=0), out=votes)

        pend = []
        for i, y in enumerate(_chain_frames(held, frames)):
            if (t0 + i) % fi == 0:
                pend.append((i, y)); n_marked += 1
                if len(pend) >= batch:
                    decode(pend); pend = []
        if pend:
            decode(pend)
        out = F.search_tail(ctx, votes, py, px, ty, tx, tbi, rule.carried, rule.code, n_marked, return_soft)
    finally:
        ctx.close()
    return out[:4] + (int(t0),) + out[4:]


def _chain_frames(held, frames):
    """the anchors already read, then the luma of the frames still in the file"""
    yield from held
    for _, y, _ in frames:
        yield y


def _extract_payload_frames(vid: Y4M, rule: F.Rule, batch: int, device: int, anchors: int, return_soft: bool):
    """search="frames" (include/wmhip.h, "frame resynchronisation"): the file holds frames of a video marked with dither=True
    in any order - dropped, repeated, reordered, unmarked or foreign ones among them - every frame cropped to the same
    rectangle.  Every refusal comes before the first device call; the frames are read once, and beside the anchors only one
    batch of them, its sigma_1, the int64 vote grid and frame_map live on the host."""
    if not rule.dither:
        raise ValueError("search='frames' reads a payload embedded with dither=True; this one has none")
    anchors = int(anchors)
    if anchors < 1:
        raise ValueError(f"anchors must be at least 1, got {anchors}")
    h, w = vid.H, vid.W
    F.check_crop_shape(h, w, rule.H, rule.W, "clip")
    n_c = _count_frames(vid)
    if n_c < 1:
        raise ValueError("clip has no frame")
    fi = max(1, rule.frame_interval)
    nby, nbx = rule.grid
    K = (rule.n_frames + fi - 1) // fi
    tables = P.dither_tables(nby, nbx, rule.key, [k * fi for k in range(K)]).reshape(K, nby, nbx)
    tbi = rule.map()[0].reshape(nby, nbx)
    frame_map = np.full(n_c, -1, np.int32)
    empty = (b"", False, 0.0, None, frame_map)
    if return_soft:
        empty += (np.zeros(rule.carried, np.float64),)
    if K < 1:
        return empty
    frames = iter(vid)
    held = [y for _, (_, y, _) in zip(range(min(n_c, anchors * fi)), frames)]
    ctx = hostapi.Context(device)
    try:
        # step 1: the first anchor whose own table, phase and place stand out fixes the geometry of every frame
        geometry = None
        counts = P.phase_counts(h, w)
        every_table = np.arange(K, dtype=np.int32)[:, None]
        for y in held:
            best, win = ctx.payload_locate_clip(y[None], tables, every_table, rule.delta, pick=True)
            if win is not None and P.anchor_accepted(best, counts, (win[0], 8 * win[1][0] + win[1][1])):
                geometry = win[1:]
                break
        if geometry is None:
            return empty
        (py, px), (ty, tx) = geometry
        ny, nx = (h - py) // TILE, (w - px) // TILE
        votes = np.zeros((ny, nx), np.int64)
        n_accepted = 0

        def match(f0, pend):
            # steps 2 - 4 on one batch: sigma pass and scores on the device, assignment and votes on the host
            ys = np.stack([y[py:py + TILE * ny, px:px + TILE * nx] for y in pend])
            scores, s1 = ctx.payload_match_frames(ys, tables, ty, tx, rule.delta)
            named = P.pick_frames(scores, ny * nx)
            for j, k in enumerate(named):
                if k >= 0:
                    frame_map[f0 + j] = k * fi
                    np.add(votes, P.keyed_votes(s1[j], tables[k, ty:ty + ny, tx:tx + nx], rule.delta), out=votes)
            return int(np.count_nonzero(named >= 0))

        pend, f0 = [], 0
        for y in _chain_frames(held, frames):
            pend.append(y)
            if len(pend) >= batch:
                n_accepted += match(f0, pend)
                f0 += len(pend); pend = []
        if pend:
            n_accepted += match(f0, pend)
        if n_accepted == 0:
            return empty
        out = F.search_tail(ctx, votes, py, px, ty, tx, tbi, rule.carried, rule.code, n_accepted, return_soft)
    finally:
        ctx.close()
    return out[:4] + (frame_map,) + out[4:]


def extract_payload_video(stego_video_path: str, metadata_path: str, *, password: str = "", batch: int = 32,
                          device: int = 0, return_soft: bool = False, search=None, anchors: int = P.CLIP_ANCHORS):
    """-> (data, valid, confidence) from the marked frames' luma; with ``return_soft`` the summed soft vector follows.
    ``search="clip"``: the file may be any run of consecutive frames of the marked video, every frame cropped to the same
    axis-aligned rectangle (a payload embedded with dither=True).  The first frame, the tile grid and the crop's place are
    searched for on the device over the first ``anchors`` marked frames' worth of the clip, and the result is (data, valid,
    confidence, origin, first_frame): origin = (y0, x0) of the crop in the marked frames, first_frame the clip's first frame
    in the marked file - meaningful where valid is True ("Clip resynchronisation").
    ``search="resize"``: the file may be the marked video with every frame resized to another size, the frames' number and
    order unchanged.  Each batch of marked luma frames is resampled back to the meta's size on the device in one call and
    decoded as unresized frames; the result is the plain one followed by scale = (h / H, w / W), ahead of the soft vector
    where that is asked for ("Resize resynchronisation").
    ``search="frames"``: the file may hold frames of the marked video in any order - frames dropped or repeated (a frame-rate
    conversion), scenes spliced, a reversed or reordered reel - with frames that were never marked mixed in (the unmarked
    ones of ``frame_interval`` > 1, a title card), every frame cropped to the same axis-aligned rectangle; it may have more
    frames than the marked video had (a payload embedded with dither=True).  The tile grid and the crop's place come from
    the first of the first ``anchors`` marked frames' worth of the file that names a table of its own; then every frame is
    scored against every marked frame's table on the device and votes under the one it names.  The result is (data, valid,
    confidence, origin, frame_map): frame_map int32 [frames of the file], the marked file's frame index every frame was
    matched to, -1 for a frame that took no part.  Where no anchor or no frame names a table the result is (b"", False, 0.0,
    None, frame_map of -1), not an exception ("Frame resynchronisation")."""
    if search not in VIDEO_SEARCHES + (SEARCH_RESIZE, P.SEARCH_FRAMES):
        raise ValueError(f"search must be None, 'clip', 'resize' or 'frames', got {search!r}")
    M.require_password(password, "extract")
    rule = F.checked_rule(M.load_payload_meta(metadata_path), password, video=True)
    H, W, fi = rule.H, rule.W, rule.frame_interval
    batch = max(1, int(batch))
    vid = Y4M(stego_video_path)
    ctx = None
    try:
        if search == P.SEARCH_CLIP:
            return _extract_payload_clip(vid, rule, batch, device, anchors, return_soft)
        if search == P.SEARCH_FRAMES:
            return _extract_payload_frames(vid, rule, batch, device, anchors, return_soft)
        _, order, offs = rule.map()
        resized = search == SEARCH_RESIZE and (vid.H, vid.W) != (H, W)
        if search == SEARCH_RESIZE:
            R.check_resize(vid.H, vid.W, H, W, "video")
        elif (vid.H, vid.W) != (H, W):
            raise ValueError(f"video is {vid.W}x{vid.H} but the meta was written for {W}x{H}")
        ctx = hostapi.Context(device)
        soft = np.zeros(rule.carried, np.float64)
        n_marked = 0
        for frames in _marked_batches(vid, fi, batch):
            dz = _payload_frame_dithers(H, W, rule.key, n_marked, len(frames), fi) if rule.dither else None
            ys = np.stack([y for y, _ in frames])
            if resized:
                soft += ctx.payload_soft_resized(ys, H, W, order, offs, rule.carried, rule.delta, dither=dz)
            else:
                soft += ctx.payload_soft(ys, order, offs, rule.carried, rule.delta, dither=dz)
            n_marked += len(frames)
        read = F.read(ctx, soft, rule.code)                                # (one decode of the summed values)
    finally:
        vid.close()
        if ctx is not None:
            ctx.close()
    payload, valid = P.payload_unframe(read)
    out = (payload, bool(valid), P.confidence(soft, offs, n_marked))
    if search == SEARCH_RESIZE:
        out += ((vid.H / H, vid.W / W),)
    return out + (soft,) if return_soft else out
