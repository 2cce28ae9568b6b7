"""The ``.npz`` meta of the drop-in and of the video functions: the one statement of its layout.

Member names, their order in the file, what the HMAC covers and in which order (single:152-156, 182), how the nonce,
the digest, ``kfrac``, ``k_floor`` and the tile size are read back, and the small argument rules the public functions
share.  The reference's ``extract`` / ``detect`` read the full-frame image metas written through here, so a slip in this
file is a file they cannot authenticate.  NumPy and hashlib only (through hostglue; hostapi for the one statement of the
masked rule's parameter check, which loads nothing): nothing here touches the device.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

from . import hostapi
from . import hostglue as hg

TILE = 8
CHANNELS = "bgr"                                   # plane order of a colour meta (single:122)


# ---- key names ----------------------------------------------------------------
def s_key(n: str) -> str:
    return "S" + n                                 # host singular values of channel n, single:157-166


def uw_key(n: str) -> str:
    return "UW" + n


def vwt_key(n: str) -> str:
    return "VW" + n + "t"


def sw_key(n: str) -> str:
    return "SW" + n


_GRAY = ("Sc", "Uw", "Vwt", "Sw")
# ``mask``: float32 (lo, hi, cut) of a tile-mode meta written with texture-masked strength, directly after k_floor; a meta
# written without masking has no such member
_IMAGE_COMMON = ("payload_type", "shape", "alpha", "kfrac", "nonce", "tile", "k_floor", "mask")
_VIDEO_COMMON = ("payload_type", "shape", "alpha", "kfrac", "frame_interval", "n_frames", "tile", "k_floor", "mask", "nonce")
# a colour video meta written from a subsampled container names it ("420" / "422") directly after n_frames
_VIDEO_COLOR_COMMON = tuple(x for k in _VIDEO_COMMON for x in ((k, "chroma") if k == "n_frames" else (k,)))
_BY_CHANNEL = tuple(f(n) for n in CHANNELS for f in (s_key, uw_key, vwt_key, sw_key))
_BY_CHANNEL_THEN_S = tuple(f(n) for n in CHANNELS for f in (uw_key, vwt_key, sw_key)) + tuple(s_key(n) for n in CHANNELS)

# mode -> member order in the file; a member a writer does not set is skipped
_ORDER = {
    "gray": ("mode",) + _GRAY + _IMAGE_COMMON + ("digest",),                                # single:183-189 (+ tile, k_floor)
    "color": ("mode",) + _IMAGE_COMMON + _BY_CHANNEL + ("digest",),                         # single:157-166 (+ tile, k_floor)
    "video_gray": ("mode", "payload_type") + _GRAY + _VIDEO_COMMON[1:] + ("digest",),
    "video_color": ("mode",) + _VIDEO_COLOR_COMMON + ("digest",) + _BY_CHANNEL,
}
# A blind payload (payload.py, include/wmhip.h): the rule's step, the bit count and the key's nonce - no Sc, Uw or Vwt, so the
# file's size depends neither on the image size nor on the frame count.  A video writes frame_interval and n_frames too
# (and chroma, should a colour container ever be named); payload_type is "text", "json" or "bytes".  ``dither`` (uint8,
# directly after delta): 1 for a payload embedded with keyed dither under payload.dither_table; a meta written without
# dither has no such member, so the files written before it existed load, hash and weigh as they did.  ``code`` (uint8,
# directly after dither): 1 for a payload protected by the rate-1/2 K = 7 convolutional code of payload.encode_k7; present
# only when the code is on, by the same reasoning.  payload_bits stays the frame's bit count whatever the code.
PAYLOAD_MODE = "payload"
_PAYLOAD = ("payload_type", "shape", "delta", "dither", "code", "payload_bits", "nonce", "tile", "frame_interval", "n_frames", "chroma")
_ORDER[PAYLOAD_MODE] = ("mode",) + _PAYLOAD + ("digest",)
_ORDER_FULL_FRAME = dict(_ORDER, color=("mode",) + _IMAGE_COMMON + _BY_CHANNEL_THEN_S + ("digest",))


def is_color(meta) -> bool:
    return str(meta["mode"]) not in ("gray", "video_gray")                 # single:196,293: whatever is not gray


def hmac_parts(meta) -> list:
    """The arrays the HMAC covers, in its order: Sc, Uw, Vwt (single:182) or Sb Sg Sr, UWb UWg UWr, VWbt VWgt VWrt
    (single:152-156)."""
    if is_payload(meta):
        return payload_hmac_parts(meta)
    if is_color(meta):
        return [meta[f(n)] for f in (s_key, uw_key, vwt_key) for n in CHANNELS]
    return [meta["Sc"], meta["Uw"], meta["Vwt"]]


def is_payload(meta) -> bool:
    return str(meta["mode"]) == PAYLOAD_MODE


# what a payload meta's members are stored as - and hashed as, whatever a reader's np.load made of them
_PAYLOAD_DTYPES = dict(shape=np.int64, delta=np.float32, dither=np.uint8, code=np.uint8, payload_bits=np.int32, nonce=np.uint8, tile=np.int32,
                       frame_interval=np.int32, n_frames=np.int32)


def payload_hmac_parts(meta) -> list:
    """A payload meta has no factors to protect; its HMAC covers every member but the digest, in file order: the strings as
    UTF-8 bytes, the numbers in their stored dtypes.  A changed delta, bit count or nonce is a wrong password."""
    parts = []
    for k in _ORDER[PAYLOAD_MODE]:
        if k == "digest" or k not in meta:
            continue
        if k in _PAYLOAD_DTYPES:
            parts.append(np.asarray(meta[k]).astype(_PAYLOAD_DTYPES[k]).reshape(-1))
        else:
            parts.append(np.frombuffer((k + "=" + str(meta[k])).encode("utf-8"), dtype=np.uint8))
    return parts


def payload_members(payload_type: str, H: int, W: int, delta: float, n_bits: int, nonce: bytes, frame_interval=None,
                    n_frames=None, dither: int = 0, code: int = 0) -> dict:
    out = dict(mode=PAYLOAD_MODE, payload_type=str(payload_type), shape=np.array((H, W), dtype=np.int64),
               delta=np.float32(delta))
    if dither:
        out.update(dither=np.uint8(dither))
    if code:
        out.update(code=np.uint8(code))
    out.update(payload_bits=np.int32(n_bits), nonce=np.frombuffer(nonce, dtype=np.uint8), tile=np.int32(TILE))
    if n_frames is not None:
        out.update(frame_interval=np.int32(frame_interval), n_frames=np.int32(n_frames))
    return out


# The file.  Every member of a .npz costs a zip local header, a central-directory entry and a .npy header: about 200 bytes
# for a 4-byte integer, 2 KB for the members above.  A payload meta is therefore written as ONE member, ``payload``: a 0-d
# structured array whose fields are the members, in their order and dtypes (strings at fixed widths) - a plain .npz that
# np.load reads without pickle, about 0.5 KB, the same size to the byte whatever the values (the member is stored, not
# deflated).  pack_payload / unpack_payload go between the two forms; everything else sees the members.
PAYLOAD_MEMBER = "payload"
_PAYLOAD_STR = dict(mode="<U7", payload_type="<U5", chroma="<U8")


def is_packed_payload(meta) -> bool:
    return PAYLOAD_MEMBER in meta and "mode" not in meta


def pack_payload(meta: dict) -> dict:
    """The sealed members of a payload meta -> {"payload": 0-d structured array}, what goes to the file."""
    fields, values = [], []
    for k in _ORDER[PAYLOAD_MODE]:
        if k not in meta:
            continue
        if k in _PAYLOAD_STR:
            if len(str(meta[k])) > int(_PAYLOAD_STR[k][2:]):
                raise ValueError(f"{k} {str(meta[k])!r} is too long for a payload meta")
            fields.append((k, _PAYLOAD_STR[k])); values.append(str(meta[k]))
        else:
            a = np.asarray(meta[k]).astype(_PAYLOAD_DTYPES.get(k, np.uint8))
            fields.append((k, a.dtype.str) if a.ndim == 0 else (k, a.dtype.str, a.shape)); values.append(a)
    rec = np.zeros((), dtype=np.dtype(fields))
    for (k, *_), v in zip(fields, values):
        rec[k] = v
    return {PAYLOAD_MEMBER: rec}


def unpack_payload(meta) -> dict:
    """The members of a payload meta, in their order, from its file form (a dict or an np.load handle); a meta that is
    already in member form comes back as it is."""
    if not is_packed_payload(meta):
        return meta
    rec = np.asarray(meta[PAYLOAD_MEMBER])
    if rec.dtype.names is None or rec.ndim != 0 or "mode" not in rec.dtype.names:
        raise ValueError("not a payload meta")
    out = {k: (str(rec[k]) if k in _PAYLOAD_STR else np.array(rec[k])) for k in rec.dtype.names}
    for k in out:
        if k not in _PAYLOAD_STR and out[k].ndim == 0:
            out[k] = out[k][()]                                            # numpy scalars, as payload_members writes them
    return out


def save_payload_meta(path: str, meta: dict) -> str:
    return hg.save_npz(path, pack_payload(meta), compressed=False)


def load_payload_meta(path: str) -> dict:
    return unpack_payload(hg.load_npz(path))


def payload_dither_of(meta) -> int:
    """0 for a payload meta without the ``dither`` member (the dither-free rule), else its value; only 1 is known"""
    d = int(meta["dither"]) if "dither" in meta else 0
    if d not in (0, 1):
        raise ValueError(f"payload meta names dither table {d}, which this version does not know")
    return d


def payload_code_of(meta) -> int:
    """0 for a payload meta without the ``code`` member (repetition alone), else its value; only 1 (payload.CODE_K7) is known"""
    c = int(meta["code"]) if "code" in meta else 0
    if c not in (0, 1):
        raise ValueError(f"payload meta names code {c}, which this version does not know")
    return c


def refuse_payload(meta, what: str) -> None:
    """extract / detect read a watermark image's factors; a payload meta has none."""
    if is_packed_payload(meta) or ("mode" in meta and is_payload(meta)):
        raise ValueError(f"{what}: this meta carries a blind payload (mode='payload'), not a watermark image - "
                         "use extract_payload / extract_payload_video")


def require_payload(meta) -> None:
    if "mode" not in meta or not is_payload(meta):
        raise ValueError("this meta was not written by embed_payload / embed_payload_video")


# ---- writers ------------------------------------------------------------------
def common_members(H: int, W: int, alpha: float, kfrac: float, nonce: bytes) -> dict:
    return dict(payload_type="image", shape=np.array((H, W)), alpha=float(alpha), kfrac=float(kfrac),
                nonce=np.frombuffer(nonce, dtype=np.uint8))


def image_members(tile: Optional[int], k_floor: int) -> dict:
    """Tile mode names its tile and floor; a full-frame image meta is exactly the reference's (keys of single:157-166,
    183-189), with no extra unless k_floor differs from the literal 8 of single:174."""
    if tile:
        return dict(tile=np.int32(TILE), k_floor=np.int32(k_floor))
    return dict(k_floor=np.int32(k_floor)) if k_floor != 8 else {}


def video_members(frame_interval: int, n_frames: int, tile: Optional[int], k_floor: int) -> dict:
    return dict(frame_interval=np.int32(frame_interval), n_frames=np.int32(n_frames), tile=np.int32(tile or 0),
                k_floor=np.int32(k_floor))


def mask_members(mask) -> dict:
    """The texture-masked rule's parameters (``check_strength``'s result); nothing for uniform strength.  Like ``alpha``
    they are not covered by the HMAC."""
    return {} if mask is None else dict(mask=np.asarray(mask, dtype=np.float32))


def gray_members(Sc, Uw, Vwt, Sw) -> dict:
    return dict(Sc=Sc, Uw=Uw, Vwt=Vwt, Sw=Sw)                              # single:183-189


def channel_members(S, UW, VWt, SW) -> dict:
    """Each argument holds the three channels' arrays along its first axis (a stacked [3, ...] array or a list)."""
    out = {}
    for ch, n in enumerate(CHANNELS):                                      # single:157-166
        out[s_key(n)] = S[ch]; out[uw_key(n)] = UW[ch]; out[vwt_key(n)] = VWt[ch]; out[sw_key(n)] = SW[ch]
    return out


# 8-bit Y4M chroma tags -> chroma format (the tag without its siting suffix)
_CHROMA_FORMAT = {"420": "420", "420jpeg": "420", "420mpeg2": "420", "420paldv": "420", "422": "422", "444": "444"}


def chroma_format(container_tag: str) -> str:
    """A Y4M chroma tag with its siting suffix stripped: "420jpeg" -> "420".  Any other tag ("mono", "420p10",
    "444alpha") is no 8-bit three-plane format and stands for itself."""
    return _CHROMA_FORMAT.get(container_tag, container_tag)


def chroma_members(container_tag: str) -> dict:
    """The chroma format of the subsampled container a colour video was written to; a 4:4:4 meta has no such member and
    stays what it was."""
    fmt = chroma_format(container_tag)
    return {} if fmt == "444" else dict(chroma=fmt)


def sealed(members: dict, tile: Optional[int], digest: bytes) -> dict:
    """The meta as it goes to the file: the members (``mode`` among them) in their writer's order, with the digest."""
    have = dict(members, digest=np.frombuffer(digest, dtype=np.uint8))
    order = (_ORDER if tile else _ORDER_FULL_FRAME)[have["mode"]]
    assert set(have) <= set(order), sorted(set(have) - set(order))
    return {k: have[k] for k in order if k in have}


# ---- readers ------------------------------------------------------------------
def _bytes_of(x) -> bytes:
    return bytes(bytearray(np.asarray(x).astype(np.uint8).tolist()))


def nonce_of(meta) -> bytes:
    return _bytes_of(meta["nonce"])


def digest_of(meta) -> bytes:
    return _bytes_of(meta["digest"])


def kfrac_of(meta) -> float:
    return float(meta["kfrac"]) if "kfrac" in meta else hg.K_FRAC_DEFAULT  # single:211


def k_floor_of(meta) -> int:
    return int(meta["k_floor"]) if "k_floor" in meta else 8


def tile_of(meta) -> Optional[int]:
    """Tile size a meta was written with: the explicit ``tile`` key (0: full-frame), else inferred from the
    singular-value array (per-tile [nby, nbx, 8] against full-frame [L])."""
    if "tile" in meta:
        t = int(meta["tile"])
        if t == 0:
            return None
        if t != TILE:
            raise ValueError("tile must be 8 or None")
        return TILE
    s = meta["Sc"] if "Sc" in meta else meta[s_key(CHANNELS[0])]
    return TILE if np.asarray(s).ndim == 3 else None


def mask_of(meta):
    """None, or the (lo, hi, cut) a tile-mode meta was written with (texture-masked strength)."""
    if "mask" not in meta:
        return None
    return check_mask(np.asarray(meta["mask"], dtype=np.float32).reshape(-1).tolist())


def chroma_of(meta) -> str:
    """Chroma format of the container a colour video meta was written for: its ``chroma`` member, else 4:4:4."""
    return str(meta["chroma"]) if "chroma" in meta else "444"


def by_channel(meta, key_rule) -> list:
    """[meta of b, of g, of r] for one of s_key / uw_key / vwt_key / sw_key."""
    return [meta[key_rule(n)] for n in CHANNELS]


def stacked(meta, key_rule) -> np.ndarray:
    """The [3, ...] array of one of a colour meta's S / UW / VWt / SW."""
    return np.stack(by_channel(meta, key_rule))


_RULE_OF = dict(Sc=s_key, Uw=uw_key, Vwt=vwt_key, Sw=sw_key)              # a gray member's name -> its per-channel rule


def per_plane(meta, *names) -> list:
    """The named members (among Sc, Uw, Vwt, Sw - the gray names) plane by plane: one tuple for a gray meta, three for a
    colour one.  Only the named members are read (an ``np.load`` handle inflates a member on every access)."""
    if is_color(meta):
        return list(zip(*(by_channel(meta, _RULE_OF[k]) for k in names)))
    return [tuple(meta[k] for k in names)]


def batched(meta, *names) -> tuple:
    """The named members as one array each for all planes: a gray meta's own, a colour meta's stacked to [3, ...]."""
    if is_color(meta):
        return tuple(stacked(meta, _RULE_OF[k]) for k in names)
    return tuple(meta[k] for k in names)


def authentic(meta, key: bytes) -> bool:
    """single:206-209, 244-247"""
    return hg.digests_equal(hg.hmac_digest(key, hmac_parts(meta)), digest_of(meta))


# ---- small rules --------------------------------------------------------------
def k_of(L: int, kfrac: float, k_floor: int) -> int:
    return min(L, max(int(k_floor), int(kfrac * L)))                       # single:174 (capped at L)


NO_PASSWORD = {"embed": "Vui lòng nhập mật khẩu để nhúng.",               # single:115-116
               "extract": "Vui lòng nhập mật khẩu để giải trích."}        # single:193-194
WRONG_PASSWORD = "Sai mật khẩu hoặc meta không khớp."                      # single:208-209,246-247


def check_password_type(password, what: str) -> None:
    """The authoritative signatures (single:112-114,192) take the password as a string.  The legacy module of the
    same name had ``extract(stego, meta, out, normalize=True)`` and ``embed(..., payload_type, text_data)`` without one
    (core:85-92,203): a positional ``True`` from such a call site would otherwise be hashed as a password."""
    if password is not None and not isinstance(password, str):
        raise TypeError(f"password must be a str, got {type(password).__name__}: {what}(...) follows "
                        "app_dct_svd_single.py's signature (password before normalize / kfrac), not the legacy "
                        "dct_svd_core_secure.py one - pass password= and normalize= by keyword")


def require_password(password, what: str) -> None:
    if not password:
        raise ValueError(NO_PASSWORD[what])


def check_tile(tile) -> None:
    if tile is not None and int(tile) != TILE:
        raise ValueError("tile must be 8 or None")


STRENGTHS = ("uniform", "masked")
MASK_DEFAULT = (8.0, 64.0, 0.25)       # a texture RMS of 1 and of 8 gray levels per pixel; at most 4x noise gain on carried tiles


def check_mask(mask) -> tuple:
    """(lo, hi, cut) as floats holding the float32 values the meta stores, checked by the binding's own rule
    (hostapi.check_mask: 0 <= lo < hi, both finite, 0 < cut <= 1)."""
    try:
        mask = [float(np.float32(x)) for x in mask]
    except (TypeError, ValueError):
        raise ValueError("mask must be (lo, hi, cut)") from None
    return hostapi.check_mask(mask)


def check_strength(strength, mask, tile):
    """The rule an embed call asks for: None for ``strength="uniform"``, the checked (lo, hi, cut) for "masked".  Masking
    is a per-tile gain: full-frame mode (tile=None) has no tiles to mask."""
    if strength not in STRENGTHS:
        raise ValueError(f"strength must be one of {STRENGTHS}, got {strength!r}")
    if strength == "uniform":
        return None
    if not tile:
        raise ValueError('strength="masked" needs tile=8: full-frame mode has no tiles')
    return check_mask(mask)


def mask_gain(Sc, lo: float, hi: float) -> np.ndarray:
    """The rule's per-tile gain g from cover singular values Sc [..., 8], float32 [...]: a caller's look at the map
    without a device.  r = sqrt(s_2^2 + .. + s_8^2), g = clamp((r - lo) / (hi - lo), 0, 1), all in float32."""
    Sc = np.asarray(Sc, dtype=np.float32)
    r = np.sqrt(np.sum(Sc[..., 1:] * Sc[..., 1:], axis=-1, dtype=np.float32))
    return np.clip((r - np.float32(lo)) / (np.float32(hi) - np.float32(lo)), 0, 1).astype(np.float32)


check_enhance = hg.check_enhance


def out_name(path: str, suffix: str) -> str:
    """single:148-149,178-179 (``_stego.png``), 225-226,278-279 (``_wm.png``)"""
    return path if path.lower().endswith(".png") else os.path.splitext(path)[0] + suffix
