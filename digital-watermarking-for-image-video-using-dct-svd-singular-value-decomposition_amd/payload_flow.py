"""The steps of the blind payload's flow that the image entry points (dct_svd_core_secure.py) and the video ones (video.py)
share: what an authentic meta says (the rule), what an embed carries (the plan), how soft values become bits (the read), how a
search ends (the tail), which crop a search takes.  payload.py stays device-free; here its arithmetic meets meta, key and device."""
from __future__ import annotations

import collections

from . import hostapi
from . import hostglue as hg
from . import meta as M
from . import payload as P

TILE = M.TILE


class Rule(collections.namedtuple("Rule", "H W delta frame_bits carried code dither key frame_interval n_frames")):
    """What an authentic payload meta says.  frame_bits: the frame's bits (``payload_bits``); carried: the bits the tiles
    carry - the coded bits under a channel code, else the frame's; frame_interval, n_frames: None for an image's meta."""

    @property
    def grid(self) -> tuple:
        return self.H // TILE, self.W // TILE

    def map(self) -> tuple:
        """(tile_bit_index, order, offs) of the carried bits (payload.payload_map)"""
        return P.payload_map(*self.grid, self.key, self.carried)


def checked_rule(meta, password: str, video: bool = False) -> Rule:
    """The rule of a payload meta (packed or in member form) under ``password``.  Refusals in this order: not a payload
    meta; ``video``: not a video's; wrong password or a changed member; members that describe no frame of this size."""
    meta = M.unpack_payload(meta)
    M.require_payload(meta)
    if video and "n_frames" not in meta:
        raise ValueError("metadata was not written by embed_payload_video")
    key = hg.derive_key(password, M.nonce_of(meta))
    if not M.authentic(meta, key):
        raise ValueError(M.WRONG_PASSWORD)
    H, W = map(int, meta["shape"])
    n_bits = int(meta["payload_bits"])
    code = M.payload_code_of(meta)
    carried = P.coded_bits(n_bits) if code else n_bits
    if n_bits < 8 * P.OVERHEAD_BYTES or n_bits % 8 or carried > P.capacity_bits(H, W) or M.tile_of(meta) != TILE:
        raise ValueError("payload meta does not describe a frame of this image size")
    P.check_type(str(meta["payload_type"]))
    fi, n_frames = (int(meta["frame_interval"]), int(meta["n_frames"])) if "n_frames" in meta else (None, None)
    return Rule(H, W, hostapi.check_delta(float(meta["delta"])), n_bits, carried, code, M.payload_dither_of(meta), key, fi, n_frames)


def embed_plan(data: bytes, code: int, H: int, W: int, key: bytes) -> tuple:
    """(bits, carried, tile_bit_index, order, offs, tile_bit): the frame, what the tiles carry (the frame, through the channel
    code if any), their keyed map and every tile's bit.  A payload beyond the capacity is refused here, before any device call."""
    bits = P.payload_frame(data)
    carried = P.encode_k7(bits) if code else bits
    P.check_capacity(carried.size, P.capacity_bits(H, W))
    tbi, order, offs = P.payload_map(H // TILE, W // TILE, key, carried.size)
    return bits, carried, tbi, order, offs, P.tile_bits(carried, tbi)


def read(ctx, soft, code: int):
    """The frame's bits out of the soft values of the bits the tiles carry: their signs, or with the channel code the
    Viterbi decode of their quantised values on the device (include/wmhip.h, "channel code")"""
    return ctx.payload_decode(P.quantise_soft(soft))[0] if code else soft < 0


def check_crop_shape(h: int, w: int, H: int, W: int, noun: str) -> None:
    """an h x w ``noun`` ("stego", "clip") that can be a crop of the H x W marked frame, or a ValueError"""
    if h > H or w > W:
        raise ValueError(f"{noun} is {w}x{h}, larger than the {W}x{H} the meta was written for: not a crop of it")
    if h < TILE or w < TILE:
        raise ValueError(f"{noun} is {w}x{h}: a crop without a whole 8x8 tile carries nothing")


def search_tail(ctx, votes, py: int, px: int, ty: int, tx: int, tbi, carried: int, code: int, multiplicity: int = 1,
                return_soft: bool = False) -> tuple:
    """How every search ends.  votes: the winner's int votes [ny, nx], found at grid phase (py, px) and placement (ty, tx) of
    the embed's [nby, nbx] map ``tbi``; multiplicity: the frames added into every vote (a clip's marked frames).
    -> (data, valid, confidence, origin), origin = (y0, x0) of the crop in the marked frame; ``return_soft`` appends soft."""
    ny, nx = votes.shape
    soft, count = P.soft_of_votes(votes, tbi[ty:ty + ny, tx:tx + nx], carried)
    data, valid = P.payload_unframe(read(ctx, soft, code))
    out = (data, bool(valid), P.sync_confidence(soft, count * max(int(multiplicity), 1)), (TILE * ty - py, TILE * tx - px))
    return out + (soft,) if return_soft else out
