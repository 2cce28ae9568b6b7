"""Blind text / JSON / bytes payload: the host side of the sigma_1 quantisation rule (include/wmhip.h, DESIGN.md
section 14).  Framing of the bytes into bits, the keyed tile-to-bit map and its CSR inverse, the keyed dither table, what a
caller's payload argument means.  NumPy, hashlib, json and zlib only: nothing here touches the device.

Frame: ``len(data)`` as 4 little-endian bytes, ``data``, ``zlib.crc32(data)`` as 4 little-endian bytes, most significant
bit of every byte first - the header and bit order of the reference's bit image (core:56-60), with a checksum the
reference does not have.  n_bits = 8 * (len(data) + 8).
"""
from __future__ import annotations

import hashlib
import json
import math
import os
import zlib

import numpy as np

from . import hostglue as hg

TYPES = ("text", "json", "bytes")
DELTA_DEFAULT = 16.0
OVERHEAD_BYTES = 8                                  # length header + CRC


def payload_frame(data: bytes) -> np.ndarray:
    """bytes -> the bits that are embedded, uint8 [8 * (len(data) + 8)]"""
    data = bytes(data)
    framed = len(data).to_bytes(4, "little") + data + (zlib.crc32(data) & 0xFFFFFFFF).to_bytes(4, "little")
    return np.unpackbits(np.frombuffer(framed, dtype=np.uint8))


def payload_unframe(bits) -> tuple:
    """decoded bits -> (data, crc_ok).  crc_ok: the length header is the one a frame of this many bits has AND the checksum
    matches; a header that does not fit (a stego without this payload, too many bit errors) gives the bytes that are
    there and False, never an exception."""
    bits = (np.asarray(bits).reshape(-1) != 0).astype(np.uint8)
    n_bytes = bits.size // 8
    if n_bytes < OVERHEAD_BYTES:
        return b"", False
    raw = np.packbits(bits[:n_bytes * 8]).tobytes()
    L = int.from_bytes(raw[:4], "little")
    room = n_bytes - OVERHEAD_BYTES
    if L != room or bits.size != n_bytes * 8:
        return raw[4:4 + min(L, room)], False
    data = raw[4:4 + L]
    return data, int.from_bytes(raw[4 + L:8 + L], "little") == (zlib.crc32(data) & 0xFFFFFFFF)


def capacity_bits(H: int, W: int) -> int:
    return (H // 8) * (W // 8)


def check_capacity(n_bits: int, n_tiles: int) -> None:
    if n_bits > n_tiles:
        # the reference's wording (core:63), with the tile count where it has the pixel count
        raise ValueError(f"Payload quá dài ({n_bits} bits) > dung lượng ({n_tiles} tiles, 1 bit mỗi tile 8x8). "
                         "Dùng ảnh host lớn hơn hoặc rút gọn dữ liệu.")


def payload_map(nby: int, nbx: int, key: bytes, n_bits: int) -> tuple:
    """The keyed tile-to-bit map of an nby x nbx tile grid and its CSR inverse:
      tile_bit_index  int32 [n_tiles]: tile t carries bit perm[t] % n_bits, perm = hostglue.permutation_index(nby, nbx, key)
      order           int32 [n_tiles]: the tiles grouped by bit, ascending tile index within a bit (a stable argsort)
      offs            int32 [n_bits + 1]: bit j owns order[offs[j] : offs[j + 1]]
    perm is a permutation of the tiles, so the bits' tile counts differ by at most 1."""
    n_tiles = int(nby) * int(nbx)
    n_bits = int(n_bits)
    if n_bits < 1:
        raise ValueError("n_bits must be at least 1")
    check_capacity(n_bits, n_tiles)
    tbi = (np.asarray(hg.permutation_index(nby, nbx, key)) % n_bits).astype(np.int32)
    order = np.argsort(tbi, kind="stable").astype(np.int32)
    offs = np.concatenate([[0], np.cumsum(np.bincount(tbi, minlength=n_bits))]).astype(np.int32)
    return tbi, order, offs


def tile_bits(bits: np.ndarray, tile_bit_index: np.ndarray) -> np.ndarray:
    """the bit every tile carries, uint8 [n_tiles]"""
    return np.asarray(bits, np.uint8)[tile_bit_index]


DITHER_TABLE = 1                                    # the meta's ``dither`` member: the table below


def dither_table(nby: int, nbx: int, key: bytes, frame_index: int = 0) -> np.ndarray:
    """The keyed dither words of an nby x nbx tile grid, uint16 [n_tiles]: tile t's lattice is shifted by
    float(u[t]) * delta * 2^-15 (include/wmhip.h).  NumPy's PCG64 seeded as hostglue.rng_from_key seeds it, from
    sha256(key + b"payload-dither" + frame_index as 8 little-endian bytes): a video's frames get a table each.  Host work
    like the tile-to-bit map; part of the meta format (``dither`` = 1)."""
    frame_index = int(frame_index)
    if frame_index < 0:
        raise ValueError("frame_index must not be negative")
    seed = hashlib.sha256(bytes(key) + b"payload-dither" + frame_index.to_bytes(8, "little")).digest()
    return hg.rng_from_key(seed).integers(0, 65536, int(nby) * int(nbx), dtype=np.uint16)


def dither_tables(nby: int, nbx: int, key: bytes, frame_indices) -> np.ndarray:
    """uint16 [N, n_tiles]: dither_table of every frame index, one row per plane of a batch"""
    return np.stack([dither_table(nby, nbx, key, i) for i in frame_indices]) if len(frame_indices) else \
        np.zeros((0, int(nby) * int(nbx)), np.uint16)


def confidence(soft: np.ndarray, offs: np.ndarray, n_planes: int) -> float:
    """mean over the bits of |soft[j]| / count[j], count[j] = the number of tiles summed into bit j: 1 when every tile sits
    on its lattice point, 0 when the votes cancel"""
    count = np.diff(np.asarray(offs, np.int64)) * max(int(n_planes), 1)
    return float(np.mean(np.abs(soft) / np.maximum(count, 1))) if len(soft) else 0.0


# ---- crop resynchronisation (include/wmhip.h): the exact comparisons and the tie rules -------------
VOTE_ONE = 32768                                    # the vote of m = 1
SYNC_MAX_BITS = 16384                               # the offset scan's histogram: 64 KiB of LDS


def phase_counts(h: int, w: int) -> np.ndarray:
    """int64 [8, 8]: count[py, px] = ((h - py) // 8) * ((w - px) // 8), the windows of grid phase (py, px) in an h x w crop"""
    ny = np.maximum(int(h) - np.arange(8), 0) // 8
    nx = np.maximum(int(w) - np.arange(8), 0) // 8
    return (ny[:, None] * nx[None, :]).astype(np.int64)


def pick_phase(sums, counts):
    """The phase (py, px) with the largest sums / counts, compared exactly (cross-multiplied Python integers); ties go to
    the smallest p = 8 py + px; phases with count 0 do not take part.  None when every count is 0."""
    s = np.asarray(sums).reshape(-1)
    n = np.asarray(counts).reshape(-1)
    if s.size != 64 or n.size != 64:
        raise ValueError("sums and counts must hold the 64 phases")
    best = None
    for p in range(64):
        sp, cp = int(s[p]), int(n[p])
        if cp > 0 and (best is None or sp * best[2] > best[1] * cp):
            best = (p, sp, cp)
    return None if best is None else (best[0] // 8, best[0] % 8)


def pick_offset(scores):
    """The placement (ty, tx) with the largest score, ties to the smallest (ty, tx) (row-major); None without a placement."""
    sc = np.asarray(scores)
    if sc.ndim != 2:
        raise ValueError("scores must be [placements down, placements across]")
    if sc.size == 0:
        return None
    ty, tx = np.unravel_index(int(np.argmax(sc)), sc.shape)        # (argmax: the first of equals in row-major order)
    return int(ty), int(tx)


def soft_of_votes(votes, tile_bit_window, n_bits: int) -> tuple:
    """(soft float64 [n_bits], count int64 [n_bits]) of the winner's votes [ny, nx] under the window tile_bit_index[ty : ty +
    ny, tx : tx + nx] of the original grid's map: soft[j] = (the integer sum of the votes of bit j's tiles) / 32768, count[j]
    the number of those tiles.  Entries outside 0 .. n_bits - 1 are skipped, as on the device."""
    v = np.asarray(votes).reshape(-1).astype(np.int64)
    t = np.asarray(tile_bit_window).reshape(-1).astype(np.int64)
    n_bits = int(n_bits)
    if v.size != t.size:
        raise ValueError(f"{v.size} votes for a window of {t.size} tiles")
    ok = (t >= 0) & (t < n_bits)
    count = np.bincount(t[ok], minlength=n_bits).astype(np.int64)
    # (float64 weights hold these integers exactly: |vote| <= 2^15 and far fewer than 2^38 tiles)
    hist = np.bincount(t[ok], weights=v[ok].astype(np.float64), minlength=n_bits)
    return hist / float(VOTE_ONE), count


def sync_confidence(soft: np.ndarray, count: np.ndarray) -> float:
    """``confidence`` over the bits that still have a tile in the crop: the mean of |soft[j]| / count[j]"""
    have = np.asarray(count) > 0
    return float(np.mean(np.abs(np.asarray(soft)[have]) / np.asarray(count)[have])) if have.any() else 0.0


# ---- keyed crop resynchronisation (include/wmhip.h): a dithered payload's crop ---------------------
def keyed_score_pitch(h: int, w: int, nby: int, nbx: int) -> int:
    """int64 scores per phase of wm_payload_keyed_scores: the placements of the phase with the fewest windows, (7, 7)"""
    return (int(nby) - max(int(h) - 7, 0) // 8 + 1) * (int(nbx) - max(int(w) - 7, 0) // 8 + 1)


def pick_keyed(scores, counts):
    """The winner ((py, px), (ty, tx)) of the keyed scores: ``scores`` holds the 64 phases' int64 [n_ty_p, n_tx_p] grids,
    ``counts`` their window counts (phase_counts).  The largest score / count wins, compared exactly: within a phase the
    counts are equal, so the first maximum in row-major order; across phases cross-multiplied Python integers; ties go to
    the smallest (p, ty, tx).  Phases with count 0 or without a placement do not take part.  None when none does."""
    n = np.asarray(counts).reshape(-1)
    if len(scores) != 64 or n.size != 64:
        raise ValueError("scores and counts must hold the 64 phases")
    best = None
    for p in range(64):
        sc, cp = np.asarray(scores[p]), int(n[p])
        if sc.ndim != 2:
            raise ValueError("a phase's scores must be [placements down, placements across]")
        if cp <= 0 or sc.size == 0:
            continue
        i = int(np.argmax(sc))                                             # (the first of equals in row-major order)
        sp = int(sc.reshape(-1)[i])
        if best is None or sp * best[2] > best[1] * cp:
            best = (p, sp, cp, divmod(i, sc.shape[1]))
    return None if best is None else ((best[0] // 8, best[0] % 8), (int(best[3][0]), int(best[3][1])))


def keyed_votes(s1, u, delta: float) -> np.ndarray:
    """int32 votes of sigma_1 values under dither words u (same shape): the rule's metric and vote stated in NumPy, every
    step rounded to float32 - d = float(u) * (delta * 2^-15), x = (s1 - d) * (1 / (2 delta)), f = x - floor(x),
    m = 2 |2 f - 1| - 1, vote = rint(m * 32768).  Where 1 / (2 delta) is no power of two the device contracts x - floor(x)
    into one fused multiply-add and its vote may differ from this one by a unit."""
    F = np.float32
    s1 = np.asarray(s1, F)
    d = (np.asarray(u).astype(F) * (F(delta) * F(2.0 ** -15))).astype(F)
    if d.shape != s1.shape:
        raise ValueError(f"{d.shape} dither words for sigma_1 of shape {s1.shape}")
    x = ((s1 - d).astype(F) * (F(1.0) / (F(2.0) * F(delta)))).astype(F)
    f = (x - np.floor(x)).astype(F)
    m = (F(2.0) * np.abs(F(2.0) * f - F(1.0)) - F(1.0)).astype(F)
    return np.rint(m * F(VOTE_ONE)).astype(np.int32)


# ---- rotation resynchronisation (include/wmhip.h): a stego rotated about its centre ----------------
ANGLE_FINE = 8                                      # fine steps in a coarse one
MAX_ANGLE_DEFAULT, MAX_ANGLE_LIMIT = 10.0, 45.0     # degrees


def check_max_angle(max_angle) -> float:
    """the search's reach in degrees, in (0, 45], or a ValueError"""
    try:
        a = float(max_angle)
    except (TypeError, ValueError):
        raise ValueError("max_angle must be a number of degrees") from None
    if not (0.0 < a <= MAX_ANGLE_LIMIT):                                   # (NaN fails both comparisons)
        raise ValueError(f"max_angle must lie in (0, {MAX_ANGLE_LIMIT:g}] degrees, got {max_angle}")
    return a


def angle_candidates(H: int, W: int, max_angle: float, around=None) -> tuple:
    """The search's schedule on an H x W frame, R = hypot(H, W) / 2: an angle error of 1 / R rad moves a corner tile by a pixel.
    -> (numerators int64 [n], denominator): theta = numerator / denominator rad.  Coarse (``around`` None): k / R for
    |k| <= floor(radians(max_angle) R).  Fine: (8 k* + j) / (8 R) for |j| <= 8 around the coarse winner's k* = ``around``."""
    Rr = math.hypot(int(H), int(W)) / 2.0
    if around is None:
        n = int(math.floor(math.radians(check_max_angle(max_angle)) * Rr))
        return np.arange(-n, n + 1, dtype=np.int64), Rr
    return ANGLE_FINE * int(around) + np.arange(-ANGLE_FINE, ANGLE_FINE + 1, dtype=np.int64), ANGLE_FINE * Rr


def pick_angle(scores, counts):
    """The candidate with the largest scores / counts, compared exactly (cross-multiplied Python integers); ties go to the
    smallest index; a candidate with count 0 takes no part.  None when every count is 0."""
    s = np.asarray(scores).reshape(-1)
    n = np.asarray(counts).reshape(-1)
    if s.size != n.size:
        raise ValueError(f"{s.size} scores for {n.size} counts")
    best = None
    for a in range(s.size):
        sa, ca = int(s[a]), int(n[a])
        if ca > 0 and (best is None or sa * best[2] > best[1] * ca):
            best = (a, sa, ca)
    return None if best is None else best[0]


def votes_of_metric(m, valid=None) -> np.ndarray:
    """int32 votes rint(m 2^15) of float32 metrics, 0 where ``valid`` (same shape) is false: a tile that does not vote"""
    v = np.rint(np.asarray(m, np.float32) * np.float32(VOTE_ONE)).astype(np.int32)
    return v if valid is None else np.where(np.asarray(valid) != 0, v, 0).astype(np.int32)


# ---- clip resynchronisation (include/wmhip.h): a dithered video's clip, cut in time and cropped ------
SEARCH_CLIP = "clip"                               # extract_payload_video's ``search`` value
CLIP_ANCHORS = 4                                    # marked anchor frames a candidate's score adds up, by default


def clip_table_of(F: int, fi: int, n_c: int, A: int) -> np.ndarray:
    """int32 [F - n_c + 1, A]: candidate g = t0 (the clip's first frame is file frame t0) pairs anchor a, clip frame a, with
    the table of marked frame (t0 + a) // fi where (t0 + a) % fi == 0 and with none (-1) otherwise.  With n_c < fi some
    candidates have no marked anchor at all."""
    F, fi, n_c, A = int(F), max(1, int(fi)), int(n_c), int(A)
    if n_c < 1 or n_c > F or A < 1 or A > n_c:
        raise ValueError(f"a clip of {n_c} frames with {A} anchors is no clip of a {F}-frame video")
    t = np.arange(F - n_c + 1, dtype=np.int64)[:, None] + np.arange(A, dtype=np.int64)[None, :]
    return np.where(t % fi == 0, t // fi, -1).astype(np.int32)


def pick_clip(best, counts, marked):
    """The winner (g, p, index) of wm_payload_keyed_best's ``best`` int64 [n_cand, 64, 2] = (score, index): the largest
    score / (counts[p] * marked[g]) - counts the phases' window counts (phase_counts), marked[g] the candidate's marked
    anchors - compared by cross-multiplied Python integers; ties go to the smallest (g, p, index).  Entries of -1, phases
    without a window and candidates without a marked anchor do not take part.  None when none does."""
    b = np.asarray(best)
    n = np.asarray(counts).reshape(-1)
    m = np.asarray(marked).reshape(-1)
    if b.ndim != 3 or b.shape[1:] != (64, 2) or n.size != 64 or m.size != b.shape[0]:
        raise ValueError("best must be [n_cand, 64, 2], counts hold the 64 phases and marked the candidates")
    win = None
    for g in range(b.shape[0]):
        for p in range(64):
            s, i, d = int(b[g, p, 0]), int(b[g, p, 1]), int(n[p]) * int(m[g])
            if s < 0 or i < 0 or d <= 0:
                continue
            if win is None or s * win[1] > win[0] * d:
                win = (s, d, g, p, i)
    return None if win is None else win[2:]


# ---- frame resynchronisation (include/wmhip.h): a dithered video's frames dropped, repeated, reordered ---
SEARCH_FRAMES = "frames"                           # extract_payload_video's ``search`` value
FRAME_GAP_DEN = 10                                  # a frame names its table when it leads the runner-up by 1 / 10 of full scale


def leads_by_the_bar(s_w: int, n_w: int, s_e: int, n_e: int) -> bool:
    """s_w / n_w - s_e / n_e >= 32768 / FRAME_GAP_DEN, in exact integers: the bar of the frame search between two scores
    over n_w and n_e windows"""
    s_w, n_w, s_e, n_e = int(s_w), int(n_w), int(s_e), int(n_e)
    return FRAME_GAP_DEN * (s_w * n_e - s_e * n_w) >= VOTE_ONE * n_w * n_e


def anchor_accepted(best, counts, win) -> bool:
    """Step 1 of the frame search: does the winner ``win`` = (g, p, index) of one anchor's ``best`` int64 [K, 64, 2]
    (pick_clip with marked = 1) lead every other (candidate, phase) entry by the bar?  Entries of -1 and phases without a
    window do not take part."""
    b = np.asarray(best)
    n = np.asarray(counts).reshape(-1)
    g, p = int(win[0]), int(win[1])
    s_w, n_w = int(b[g, p, 0]), int(n[p])
    for e in range(b.shape[0]):
        for q in range(64):
            if (e, q) == (g, p) or int(b[e, q, 0]) < 0 or int(n[q]) <= 0:
                continue
            if not leads_by_the_bar(s_w, n_w, int(b[e, q, 0]), int(n[q])):
                return False
    return True


def pick_frames(scores, n_win: int) -> np.ndarray:
    """Step 3 of the frame search: int32 [n_frames], for every row of ``scores`` int64 [n_frames, K] the index k* of its
    FIRST maximum where the row names a table, else -1.  second = max(the largest score among the other tables, 16384 n_win)
    - the floor is the score of a uniform phase, so one table follows the same rule - and the row names k* when
    FRAME_GAP_DEN * (score[k*] - second) >= 32768 * n_win, in Python integers."""
    s = np.asarray(scores)
    n_win = int(n_win)
    if s.ndim != 2 or s.shape[1] < 1 or n_win < 1:
        raise ValueError("scores must be [n_frames, n_tables >= 1] and n_win at least 1")
    out = np.full(s.shape[0], -1, np.int32)
    for f in range(s.shape[0]):
        row = [int(x) for x in s[f]]
        k = row.index(max(row))                                            # (the first of equals)
        second = max(row[:k] + row[k + 1:] + [(VOTE_ONE // 2) * n_win])
        if FRAME_GAP_DEN * (row[k] - second) >= VOTE_ONE * n_win:
            out[f] = k
    return out


# ---- channel code (include/wmhip.h, "channel code"): rate 1/2, K = 7, generators 171 / 133 octal --------
CODES = (None, "k7")                                # what a caller's ``code`` argument may be
CODE_K7 = 1                                         # the meta's ``code`` member: this code
K7_TAIL = 6                                         # zero bits behind the frame
K7_MAX_STEPS = 1 << 18                              # n_info + 6 of one decode
K7_LLR_MAX = 1024                                   # |L| of a quantised soft value
_K7_G = (0o171, 0o133)
_K7_PARITY = np.array([bin(r).count("1") & 1 for r in range(128)], np.uint8)


def check_code(code) -> int:
    """the meta's ``code`` member of a caller's ``code`` argument: 0 for None, 1 for "k7" """
    if code not in CODES:
        raise ValueError(f"code must be None or 'k7', got {code!r}")
    return CODE_K7 if code else 0


def coded_bits(n_info: int) -> int:
    """n_coded of a frame of n_info bits: two coded bits for every info bit and every tail bit"""
    return 2 * (int(n_info) + K7_TAIL)


def encode_k7(bits) -> np.ndarray:
    """info bits u (the frame) -> coded bits uint8 [2 (len(u) + 6)]: the register starts at 0 and steps as r = ((r << 1) | u_t)
    & 127 through u and 6 zero tail bits; coded[2 t] = parity(r & 0o171), coded[2 t + 1] = parity(r & 0o133).  Host work,
    like the map and the dither table."""
    u = np.concatenate([(np.asarray(bits).reshape(-1) != 0).astype(np.int64), np.zeros(K7_TAIL, np.int64)])
    # r_t holds u_t .. u_{t-6}: seven shifted copies of u, without a Python loop over the steps
    r = np.zeros(u.size, np.int64)
    for k in range(7):
        r[k:] |= u[:u.size - k] << k
    out = np.empty(2 * u.size, np.uint8)
    out[0::2] = _K7_PARITY[r & _K7_G[0]]
    out[1::2] = _K7_PARITY[r & _K7_G[1]]
    return out


def quantise_soft(soft) -> np.ndarray:
    """float64 soft values (positive: the bit reads 0; 0: no tile voted, an erasure) -> the decoder's int32 L in -1024 .. 1024:
    L[j] = clip(rint(soft[j] * (1024 / peak)), -1024, 1024) with peak = max |soft|, 1 where that is 0 - all in float64,
    halves to even.  Past this line the decode is integer arithmetic."""
    s = np.asarray(soft, np.float64)
    peak = float(np.max(np.abs(s))) if s.size else 0.0
    if not peak > 0.0:
        peak = 1.0
    return np.clip(np.rint(s * (float(K7_LLR_MAX) / peak)), -K7_LLR_MAX, K7_LLR_MAX).astype(np.int32)


def check_decodes(soft: np.ndarray, bits: np.ndarray, data: bytes, decoded=None) -> None:
    """The embed's own check: ``soft`` is what the decoder reads from the finished stego (every marked frame added).  Tiles
    pinned by clipping - text on a white page, saturated regions - vote for the WRONG bit at full weight, and with few tiles
    per bit they win; such a payload must not be reported as embedded.  ``decoded``: with a channel code, the info bits its
    decoder made of ``soft`` (``bits`` is the frame either way); the count is then of info bits."""
    got_bits = np.asarray(soft) < 0 if decoded is None else np.asarray(decoded) != 0
    got, valid = payload_unframe(got_bits)
    if valid and got == bytes(data):
        return
    wrong = int(np.count_nonzero(got_bits != (np.asarray(bits) != 0)))
    if decoded is None:
        raise ValueError(f"payload does not decode from its own stego: {wrong} of {len(bits)} bits wrong (tiles pinned by "
                         "clipping vote against their bit). Use a shorter payload (more tiles per bit), a larger delta, a "
                         "larger cover or code='k7'.")
    raise ValueError(f"payload does not decode from its own stego: {wrong} of {len(bits)} info bits wrong after the channel "
                     "code's decode (tiles pinned by clipping vote against their bit). Use a shorter payload (more tiles per "
                     "coded bit), a larger delta or a larger cover.")


def check_type(payload_type: str) -> None:
    if payload_type not in TYPES:
        raise ValueError(f"payload_type must be one of {TYPES}, got {payload_type!r}")


def payload_bytes(payload, payload_type: str, allow_file: bool = True) -> bytes:
    """What a caller's ``payload`` stands for: bytes as they are; a str that names an existing file is read (text and
    json: as UTF-8 text with undecodable bytes dropped, core:105; bytes: raw), any other str is the text itself.  json is
    canonicalised through json.loads / json.dumps(ensure_ascii=False, separators=(',', ':')) (core:109-110).
    ``allow_file=False`` (the array level): a str is always the text itself."""
    check_type(payload_type)
    if isinstance(payload, (bytes, bytearray, memoryview)):
        raw = bytes(payload)
        if payload_type == "bytes":
            return raw
        text = raw.decode("utf-8", errors="ignore")
    elif isinstance(payload, (str, os.PathLike)):
        if allow_file and os.path.isfile(payload):
            if payload_type == "bytes":
                with open(payload, "rb") as f:
                    return f.read()
            with open(payload, "r", encoding="utf-8", errors="ignore") as f:
                text = f.read()
        elif isinstance(payload, str):
            text = payload
        else:
            raise ValueError(f"payload file not found: {os.fspath(payload)}")
    else:
        raise TypeError(f"payload must be str, bytes or a path, got {type(payload).__name__}")
    if payload_type == "json":
        try:
            text = json.dumps(json.loads(text), ensure_ascii=False, separators=(",", ":"))
        except Exception as e:
            raise ValueError(f"JSON không hợp lệ: {e}") from None
    return text.encode("utf-8")


def out_name(path: str, payload_type: str) -> str:
    """core:235-240: ``_data.json`` / ``_text.txt`` unless the path already ends in .json / .txt (bytes: ``_data.bin``)"""
    ext, suffix = {"json": (".json", "_data.json"), "text": (".txt", "_text.txt"), "bytes": (".bin", "_data.bin")}[payload_type]
    return path if path.lower().endswith(ext) else os.path.splitext(path)[0] + suffix


def write_payload(path: str, data: bytes, payload_type: str) -> str:
    """The decoded payload to a file named by out_name: text as UTF-8 with undecodable bytes dropped; json re-indented when
    it parses, else as text (core:229-242); bytes raw."""
    path = out_name(path, payload_type)
    if payload_type == "bytes":
        with open(path, "wb") as f:
            f.write(data)
        return path
    text = data.decode("utf-8", errors="ignore")
    if payload_type == "json":
        try:
            text = json.dumps(json.loads(text), ensure_ascii=False, indent=2)
        except Exception:
            pass
    with open(path, "w", encoding="utf-8", errors="ignore") as f:
        f.write(text)
    return path
