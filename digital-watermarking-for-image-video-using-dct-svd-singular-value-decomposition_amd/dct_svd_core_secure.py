"""Drop-in for the reference's ``embed / extract / detect`` surface
(app_dct_svd_single.py:112-318 - the authoritative "SECURE CORE"; imported by
app_dct_svd_pyside6.py:8 as ``from dct_svd_core_secure import embed, extract,
detect``), with the numeric hot path on MI355X HIP kernels.

Same positional/keyword arguments, return values, side effects (``_stego.png``
/ ``_wm.png`` renaming, ``.npz`` meta with the same keys) and exception types
as the reference.  Keyword-only extras, all with reference-preserving
defaults where the reference has a behaviour:

  tile     8 (default): the north_star's block formulation - the reference's
           per-matrix arithmetic applied to every 8x8 tile.
           Its meta carries ``tile=8`` and is not readable by the reference's
           own full-frame extract.  ``tile=None``: the reference's own
           full-frame semantics (one DCT + one dense SVD per plane) on the
           GPU; stego + meta written this way are what the reference's
           extract/detect expect (same keys, dtypes, shapes, HMAC coverage):
           tests/test_gpu_reference_files.py puts them through the reference
           program itself.  Neither mode has a CPU fallback.
  k_floor  the literal 8 of ``K = max(8, int(kfrac*L))`` (single:174); at
           tile=8 the formula is 8 for every kfrac, so a mid-band sweep sets
           k_floor < 8.
  strength "uniform" (default): every tile adds alpha * sigma_w.  "masked" (tile
           mode only): a per-tile gain from the cover's own singular values
           scales all but the leading component ("Texture-masked
           strength"), so flat tiles stay clean; ``mask=(lo, hi, cut)`` are the
           rule's parameters.  The meta then carries ``mask`` and extract /
           detect take the rule from it.  Colour: one gain per channel plane.
  nonce    inject the 8-byte nonce (reference: ``os.urandom(8)``, single:119).
  device   HIP device index.

``embed_watermark`` / ``extract_watermark`` are aliases (the names
BASELINE.json's north_star uses).
"""
from __future__ import annotations

import collections
import os
import threading
from typing import Optional

import numpy as np

from . import hostapi
from . import hostglue as hg
from . import meta as M
from . import payload as P
from . import payload_flow as F
from . import resample as R

K_FRAC_DEFAULT = hg.K_FRAC_DEFAULT
TILE = 8

_tls = threading.local()


def _ctx(device: int = 0, companion: bool = False) -> hostapi.Context:
    """One cached context per (calling thread, device): a context owns its stream and grow-only
    scratch buffers, so two threads inside embed()/extract() at once must not share one (the
    reference's functions are re-entrant).  Released when the thread ends.
    companion: this thread's second context, handed to the worker that decomposes the watermark while the
    first one decomposes the host planes (full-frame embed)."""
    cache = getattr(_tls, "contexts", None)
    if cache is None:
        cache = _tls.contexts = {}
    key = (device, bool(companion))
    c = cache.get(key)
    if c is None:
        c = cache[key] = hostapi.Context(device)
    return c


# ---------------------------------------------------------------------------
# array level (decoded images in, arrays out) - what the file level wraps
# ---------------------------------------------------------------------------
class _Later:
    """A host-only computation (the HMAC over the meta's factors: 28 ms per 66 MB at 4K, the largest single item of a
    tile-mode call) on a worker thread while this thread drives the device; hashlib and ctypes both release the GIL."""

    def __init__(self, fn):
        self._out = self._exc = None

        def run():
            try:
                self._out = fn()
            except BaseException as e:            # re-raised in result()
                self._exc = e
        self._t = threading.Thread(target=run, daemon=True)
        self._t.start()

    def result(self):
        self._t.join()
        if self._exc is not None:
            raise self._exc
        return self._out


def _interleave(planes: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.moveaxis(planes, 0, -1))


# The two modes.  Gray is the one-plane case of colour: its planes are 2-D ([H, W] where colour has [3, H, W]), and every
# Context method below takes either.
_Mode = collections.namedtuple("_Mode", "name want_yw planes_in wm_planes planes_out ssim_operand members wm_out score")
_Gray = _Mode(
    name="gray", want_yw=True,                                             # the float Yw is SSIM's second operand
    planes_in=lambda ctx, img: ctx.color("bgr2y", img),                    # single:169,204,296  (_to_Y)
    wm_planes=lambda ctx, wm: ctx.color("bgr2gray", wm),                   # single:170
    planes_out=lambda ctx, cover, stego_y: ctx.color("replace_y", cover, stego_y),   # single:26-30 (_from_Y)
    ssim_operand=lambda ctx, stego, Yw: Yw,                                # single:190
    members=M.gray_members,                                                # single:183-189
    wm_out=lambda plane: plane,
    score=lambda nc: float(nc[0]))                                         # single:297-302
_Color = _Mode(
    name="color", want_yw=False,
    planes_in=lambda ctx, img: np.ascontiguousarray(np.moveaxis(img, -1, 0)),        # b, g, r planes  single:122,232,303
    wm_planes=lambda ctx, wm: np.ascontiguousarray(np.moveaxis(wm, -1, 0)),          # single:123
    planes_out=lambda ctx, cover, planes: _interleave(planes),
    ssim_operand=lambda ctx, stego, Yw: ctx.color("bgr2gray", stego),      # single:167
    members=M.channel_members,                                             # single:157-166
    wm_out=_interleave,
    score=lambda nc: float((nc[0] + nc[1] + nc[2]) / 3.0))                 # single:317


def _mode_of(meta):
    return _Color if M.is_color(meta) else _Gray                           # single:196,293


def _embed_tiles(ctx, mode, hosts, wm, idx, alpha, K, mask=None):
    """tile=8: -> (stego planes, Sc, Yw or None, (U, S, Vt) of the watermark), every array with the planes' own rank."""
    wms = ctx.permute_planes(mode.wm_planes(ctx, wm), idx)                 # single:123-126,170-171 (index pass on the device)
    U, S, Vt = ctx.svd_tiles(wms)                                          # single:131-134,173
    stego, Sc, Yw = ctx.embed_tiles(hosts, S, alpha, K, want_yw=mode.want_yw, mask=mask)   # single:127-147,172-177
    return stego, Sc, Yw, (U, S, Vt)


def _embed_fullframe(ctx, mode, hosts, wm, idx, alpha, K, mask=None):
    """tile=None.  single:123-134 / 170-173: the scrambled watermark planes, their DCTs and SVDs (colour: as ONE batch) on the
    companion context and a worker thread, under the host planes' own decomposition (the two do not depend on each other
    until single:139's S + alpha * Sw)."""
    one = hosts.ndim == 2
    ctx_w = _ctx(ctx.device, companion=True)

    def watermark_side():
        w_s = ctx_w.permute_planes(mode.wm_planes(ctx_w, wm), idx)         # one shared permutation, single:124-126
        U, S, Vt = (ctx_w.ref_svd if one else ctx_w.ref_svd_planes)(w_s, apply_dct=True)
        return S, (U, S, Vt)
    st, Sc, Yw, factors = ctx.ref_embed_planes_when(hosts[None] if one else hosts, watermark_side, not one, alpha, K,
                                                    want_yw=mode.want_yw)  # single:127-147,172-177, one batched call
    return (st[0], Sc[0], Yw[0], factors) if one else (st, Sc, Yw, factors)


def embed_arrays(cover: np.ndarray, wm: np.ndarray, password: str, nonce: bytes,
                 alpha: float = 0.1, color: bool = False, kfrac: float = K_FRAC_DEFAULT,
                 tile: Optional[int] = TILE, k_floor: int = 8, device: int = 0, *, strength: str = "uniform",
                 mask=M.MASK_DEFAULT) -> dict:
    """cover, wm: BGR uint8.  Returns dict(stego BGR uint8, meta dict, psnr, ssim)."""
    M.check_password_type(password, "embed")
    M.require_password(password, "embed")                                  # single:115-116
    M.check_tile(tile)
    mask = M.check_strength(strength, mask, tile)                          # None: uniform
    ctx = _ctx(device)
    H, W = cover.shape[:2]
    wm = hg.resize_area_cached(wm, W, H)                                   # single:118
    key = hg.derive_key(password, nonce)                                   # single:119
    idx = hg.permutation_index(H, W, key)
    mode = _Color if color else _Gray
    K = M.k_of(TILE if tile else min(H, W), kfrac, k_floor)                # single:174
    hosts = mode.planes_in(ctx, cover)
    stego_p, Sc, Yw, (U, S, Vt) = (_embed_tiles if tile else _embed_fullframe)(ctx, mode, hosts, wm, idx, alpha, K, mask)
    members = {"mode": mode.name, **M.common_members(H, W, alpha, kfrac, nonce), **M.image_members(tile, k_floor),
               **M.mask_members(mask), **mode.members(Sc, U, Vt, S)}
    # single:152-156,182 (39 MB for a 1080p colour cover: 16 ms), under the colour conversion / interleave and the metrics
    dg = _Later(lambda: hg.hmac_digest(key, M.hmac_parts(members)))
    stego = mode.planes_out(ctx, cover, stego_p)
    ps = ctx.psnr(cover, stego)
    ss = ctx.ssim(ctx.color("bgr2gray", cover), mode.ssim_operand(ctx, stego, Yw))   # single:167,190
    return dict(stego=stego, meta=M.sealed(members, tile, dg.result()), psnr=ps, ssim=ss)


def _same_size(stego: np.ndarray, meta) -> bool:
    H, W = map(int, meta["shape"])
    return tuple(stego.shape[:2]) == (H, W)


def _check_stego_shape(stego: np.ndarray, meta):
    """Tile mode: a meta belongs to one stego size (per-tile factors; the mismatch is named before any
    device call).  Full-frame mode follows the reference, which goes on with the shortest of the
    lengths involved (single:210, 299) - see _sigma_hat's callers."""
    if not _same_size(stego, meta):
        H, W = map(int, meta["shape"])
        raise ValueError(f"stego is {stego.shape[1]}x{stego.shape[0]} but the meta was written for {W}x{H}")


def _sigma_hat(S_cw, Sc, alpha, L):
    return (S_cw[:L] - Sc[:L]) / np.float32(max(alpha, 1e-8))              # single:212,250-252,300,314


def _estimate_plane(ctx, S_cw, Sc, Uw, Vwt, alpha, kfrac, k_floor, H, W):
    """single:210-218 / 248-264 from a stego plane's singular values S_cw, whatever its size (a resized or cropped
    stego): the reference does not look at the size - L = the shortest of the four lengths, the [:L,:L] corner of the
    meta's factors, the META's H x W for the zero plane and the permutation."""
    Sc = np.asarray(Sc, dtype=np.float32)
    L = min(len(Sc), len(S_cw), Uw.shape[0], Vwt.shape[0])                 # single:210,248
    K = M.k_of(L, kfrac, k_floor)                                          # single:211,249
    sw_hat = _sigma_hat(S_cw, Sc, alpha, L).astype(np.float32)             # single:212,250-252
    sw_hat[K:] = 0                                                         # single:213
    return ctx.ref_reconstruct(Uw, sw_hat, Vwt, H, W)                      # single:214-218,257-264


def _nc(a, b) -> float:
    """single:284-289"""
    a = np.asarray(a, dtype=np.float32).reshape(-1); b = np.asarray(b, dtype=np.float32).reshape(-1)
    if a.size == 0 or b.size == 0:
        return 0.0                                                         # single:286
    a = a - a.mean(); b = b - b.mean()
    return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-8))


def _nc_truncated(S_cw, Sc, Sw, alpha) -> float:
    """single:297-301,311-316 from a stego plane's singular values: the three vectors cut to the shortest (single:299)."""
    Sc = np.asarray(Sc, dtype=np.float32).reshape(-1); Sw = np.asarray(Sw, dtype=np.float32).reshape(-1)
    L = min(len(Sc), len(S_cw), len(Sw))
    return _nc(Sw[:L], _sigma_hat(S_cw, Sc, alpha, L))


def _stego_sigmas(ctx, planes):
    """[S_cw of every plane]: colour's three in ONE batched call (a single full-frame SVD is latency-bound on a fraction
    of the chip: 3 planes cost 1.4 x one, not 3 x), single:205,232-236,304-310"""
    return [ctx.ref_sigma(planes)] if planes.ndim == 2 else ctx.ref_sigma_planes(planes)


def extract_arrays(stego: np.ndarray, meta, password: str, normalize: bool = True,
                   device: int = 0, *, enhance=False) -> np.ndarray:
    """Watermark estimate (uint8 [H,W] gray / [H,W,3] colour).  ``enhance``: False (default) returns it before the
    reference's denoise/enhance step (single:223-227,275-277); True applies the unsharp half on the host; "reference"
    runs the reference's whole chain (NL-means, CLAHE, unsharp) on the device."""
    M.check_enhance(enhance)
    M.check_password_type(password, "extract")
    M.require_password(password, "extract")                                # single:193-194
    M.refuse_payload(meta, "extract")
    mode = _mode_of(meta); alpha = float(meta["alpha"])                    # single:196
    H, W = map(int, meta["shape"])
    nonce = M.nonce_of(meta); digest = M.digest_of(meta)
    key = hg.derive_key(password, nonce)                                   # single:200
    kfrac = M.kfrac_of(meta); k_floor = M.k_floor_of(meta)                 # single:211
    parts = M.hmac_parts(meta)
    # single:206-209,244-247: the HMAC check runs on a worker thread UNDER the device work (it is 28 ms per 66 MB of factors,
    # more than everything else of a tile-mode extract); nothing is returned before it has passed, and a mismatch takes
    # precedence over whatever else went wrong meanwhile, as in the reference, where it comes first.  The overlap is only
    # taken for a key whose permutation is already cached (the extract that follows an embed, the frames of a clip): for any
    # other key the check is joined BEFORE the expensive key-dependent steps - the PCG64 shuffle of H*W indices, the route
    # build, the factor upload - so that a wrong password or a tampered meta costs one HMAC, evicts nothing from the
    # permutation / device-index caches and never reaches the native code (which would otherwise see unauthenticated
    # factors guarded by its shape checks alone).
    check = _Later(lambda: hg.digests_equal(hg.hmac_digest(key, parts), digest))
    if not hg.permutation_is_cached(H, W, key) and not check.result():
        raise ValueError(M.WRONG_PASSWORD)                                 # single:208-209,246-247
    try:
        out = _extract_checked(stego, meta, mode, alpha, kfrac, k_floor, H, W, key, normalize, device)
    except BaseException:
        if not check.result():
            raise ValueError(M.WRONG_PASSWORD) from None
        raise
    if not check.result():
        raise ValueError(M.WRONG_PASSWORD)                                 # single:208-209,246-247
    if enhance is False:
        return out
    return hg.apply_enhance(_ctx(device) if isinstance(enhance, str) else None, out, enhance)   # single:223-227,275-277


def _extract_checked(stego, meta, mode, alpha, kfrac, k_floor, H, W, key, normalize, device):
    tile = M.tile_of(meta)
    if tile is not None:
        _check_stego_shape(stego, meta)
    ctx = _ctx(device)
    idx = hg.permutation_index(H, W, key)                                  # single:219,265
    planes = mode.planes_in(ctx, stego)                                    # single:204,232
    if tile is not None:
        Sc, U, Vt = M.batched(meta, "Sc", "Uw", "Vwt")
        # single:205-222 / 233-274 in one device-resident chain: sigma -> rank-8 product -> unscramble -> normalise -> uint8
        return mode.wm_out(ctx.extract_tiles_unscrambled_u8(planes, Sc, U, Vt, alpha, M.k_of(TILE, kfrac, k_floor), idx, normalize,
                                                            mask=M.mask_of(meta)))
    if planes.ndim == 2 and _same_size(stego, meta):
        # gray, the meta's own size: sigma_hat and the product inside the library
        (Sc, Uw, Vwt), = M.per_plane(meta, "Sc", "Uw", "Vwt")
        L = min(len(Sc), min(H, W), Uw.shape[0], Vwt.shape[0])             # single:210
        return ctx.unpermute_normalize_u8(ctx.ref_extract(planes, Sc, Uw, Vwt, alpha, M.k_of(L, kfrac, k_floor)), idx, normalize)
    # colour (single:248-264 per channel with its own factors), and a stego of another size: the reference's truncation rules
    outs = [ctx.unpermute_normalize_u8(_estimate_plane(ctx, S_cw, Sc, U, Vt, alpha, kfrac, k_floor, H, W), idx, normalize)
            for S_cw, (Sc, U, Vt) in zip(_stego_sigmas(ctx, planes), M.per_plane(meta, "Sc", "Uw", "Vwt"))]
    return outs[0] if planes.ndim == 2 else np.stack(outs, axis=-1)


def detect_arrays(stego: np.ndarray, meta, thresh: float = 0.6, device: int = 0):
    M.refuse_payload(meta, "detect")
    mode = _mode_of(meta); alpha = float(meta["alpha"])                    # single:293
    tile = M.tile_of(meta)
    if tile is not None:
        _check_stego_shape(stego, meta)
    ctx = _ctx(device)
    planes = mode.planes_in(ctx, stego)                                    # single:296,303
    if tile is not None:
        Sc, Sw = M.batched(meta, "Sc", "Sw")
        nc = ctx.detect_tiles(planes, Sc, Sw, alpha, mask=M.mask_of(meta)) # single:297-301,304-316
    elif planes.ndim == 2 and _same_size(stego, meta):
        nc = [ctx.ref_detect(planes, meta["Sc"], meta["Sw"], alpha)]       # single:297-301, NC inside the library
    else:
        # colour, and a stego of another size: the NC of each plane on the host, the vectors cut to the shortest (single:299,311-313)
        nc = [_nc_truncated(S_cw, Sc, Sw, alpha)
              for S_cw, (Sc, Sw) in zip(_stego_sigmas(ctx, planes), M.per_plane(meta, "Sc", "Sw"))]
    score = mode.score(nc)
    return bool(score >= thresh), score                                    # single:302,318


# ---------------------------------------------------------------------------
# file level: the reference's public functions
# ---------------------------------------------------------------------------
def embed(cover_path: str, wm_source: str, out_path: str, meta_path: str,
          alpha: float = 0.1, color: bool = False, password: Optional[str] = None,
          kfrac: float = K_FRAC_DEFAULT, *, tile: Optional[int] = TILE, k_floor: int = 8,
          nonce: Optional[bytes] = None, device: int = 0, compress_meta: bool = True, strength: str = "uniform",
          mask=M.MASK_DEFAULT):
    """single:112-190.  Returns (out_path, meta_path, psnr, ssim).  ``compress_meta=False`` writes the .npz
    uncompressed (np.load - and the reference's extract / detect - read either form; tests/test_gpu_reference_files.py runs
    the reference program on both): the tile-mode factors are
    float noise to zlib, and compressing the 70 MB of a 4K cover costs ten times the rest of the call."""
    M.check_password_type(password, "embed")
    M.require_password(password, "embed")
    M.check_strength(strength, mask, tile)                                 # refused before anything is read
    cover = hg.read_image_bgr(cover_path)                                  # single:117
    wm = hg.read_image_bgr(wm_source)                                      # single:118
    if nonce is None:
        nonce = os.urandom(8)                                              # single:119
    r = embed_arrays(cover, wm, password, nonce, alpha, color, kfrac, tile, k_floor, device, strength=strength, mask=mask)
    out_path = M.out_name(out_path, "_stego.png")                          # single:148-149,178-179
    if not hg.write_png(out_path, r["stego"], 0):                          # single:150,180
        raise IOError("Ghi stego thất bại.")
    hg.save_npz(meta_path, r["meta"], compressed=compress_meta)            # single:157-166,183-189 (np.savez_compressed; members deflated concurrently)
    return out_path, meta_path, r["psnr"], r["ssim"]


def extract(stego_path: str, meta_path: str, out_path: str, password: str,
            normalize: bool = True, *, enhance=False, device: int = 0) -> str:
    """single:192-282.  ``enhance="reference"`` writes what the reference writes: the estimate after its
    post-processing chain (NL-means, CLAHE, unsharp; single:223-227,275-277), on the device.  ``enhance=True`` applies
    the unsharp half only, on the host; the default writes the extracted plane as is."""
    M.check_enhance(enhance)
    M.check_password_type(password, "extract")
    M.require_password(password, "extract")
    img = _Later(lambda: hg.read_image_bgr(stego_path))                    # single:201, decoded while the meta is read
    data = hg.load_npz(meta_path)                                          # single:195 (all members, inflated concurrently); its errors come first, as in the reference
    st = img.result()
    wm = extract_arrays(st, data, password, normalize, device, enhance=enhance)   # single:223-227,275-277 per enhance
    out_path = M.out_name(out_path, "_wm.png")                             # single:225-226,278-279
    if not hg.write_png(out_path, wm, 1):
        raise IOError("Ghi watermark thất bại.")                           # single:229,281
    return out_path


def detect(stego_path: str, meta_path: str, thresh: float = 0.6, *, device: int = 0):
    """single:291-318.  Returns (bool, score)."""
    data = np.load(meta_path, allow_pickle=False)                          # single:292
    M.refuse_payload(data, "detect")
    st = hg.read_image_bgr(stego_path)                                     # single:294
    return detect_arrays(st, data, thresh, device)


# ---------------------------------------------------------------------------
# blind text / JSON / bytes payload (tile mode): one bit per 8x8 tile in the parity of its leading singular value
# (include/wmhip.h).  The payload goes into Y of BGR2YCrCb and comes back through _from_Y - the gray
# pipeline the reference's text branch uses (core:116-123) - and is read back with the password and a meta of a few
# hundred bytes: nothing of the cover.
# ---------------------------------------------------------------------------
def embed_payload_arrays(cover_bgr: np.ndarray, data, password: str, nonce: bytes, *, payload_type: str = "text",
                         delta: float = P.DELTA_DEFAULT, device: int = 0, verify: bool = True, dither: bool = False,
                         code=None) -> dict:
    """cover BGR uint8, data bytes (or a str: the text / JSON itself).  Returns dict(stego BGR uint8, meta dict, psnr, ssim).
    ``dither``: every tile's lattice is shifted by a keyed offset (payload.dither_table), so that the stego shows neither
    the payload's presence nor delta to a reader without the password; the meta says so and the extract follows it.
    ``verify``: the stego is decoded by the extract's own path before it is returned, and a payload that does not come back
    valid and equal to ``data`` is a ValueError (tiles pinned by clipping vote for the wrong bit: DESIGN.md section 14).
    ``code="k7"``: the frame goes through the rate-1/2 convolutional code of payload.encode_k7 before it is spread over the
    tiles (twice the bits plus 12, so half the tiles per bit), and every decode goes through the Viterbi decoder on the
    device: wrong votes and the bits a crop erased are corrected.  The meta says so and the extract follows it."""
    M.check_password_type(password, "embed")
    M.require_password(password, "embed")
    delta = hostapi.check_delta(delta)
    code = P.check_code(code)
    data = P.payload_bytes(data, payload_type, allow_file=False)
    if cover_bgr.dtype != np.uint8 or cover_bgr.ndim != 3 or cover_bgr.shape[2] != 3:
        raise ValueError("cover must be uint8 [H, W, 3]")
    H, W = cover_bgr.shape[:2]
    key = hg.derive_key(password, nonce)
    bits, carried, _, order, offs, tile_bit = F.embed_plan(data, code, H, W, key)
    ctx = _ctx(device)
    Y = _Gray.planes_in(ctx, cover_bgr)                                    # core:117 (_to_Y)
    dz = P.dither_table(H // TILE, W // TILE, key) if dither else None     # the image's keyed dither words (frame index 0)
    stego_y, _, Yw = ctx.embed_tiles_payload(Y, tile_bit, delta, want_yw=True, dither=dz)
    members = M.payload_members(payload_type, H, W, delta, bits.size, nonce, dither=P.DITHER_TABLE if dither else 0, code=code)
    digest = hg.hmac_digest(key, M.hmac_parts(members))
    stego = _Gray.planes_out(ctx, cover_bgr, stego_y)                      # core:123 (_from_Y)
    if verify:                                                             # one metric and reduce pass on the final BGR stego
        soft = ctx.payload_soft(_Gray.planes_in(ctx, stego), order, offs, carried.size, delta, dither=dz)
        P.check_decodes(soft, bits, data, F.read(ctx, soft, code) if code else None)
    ps = ctx.psnr(cover_bgr, stego)
    ss = ctx.ssim(ctx.color("bgr2gray", cover_bgr), Yw)
    return dict(stego=stego, meta=M.sealed(members, TILE, digest), psnr=ps, ssim=ss)


SEARCHES = (None, "crop", "crop-keyed")                                   # the searches for a crop
SEARCH_RESIZE = "resize"                                                   # no search: the meta's shape says what to restore


SEARCH_ROTATE = "rotate"                                                   # the one number the meta does not hold: the angle


def _check_search(search, max_angle=None):
    if search not in SEARCHES + (SEARCH_RESIZE, SEARCH_ROTATE):
        raise ValueError(f"search must be None, 'crop', 'crop-keyed', 'resize' or 'rotate', got {search!r}")
    if max_angle is not None and search != SEARCH_ROTATE:
        raise ValueError("max_angle goes with search='rotate' only")
    if search == SEARCH_ROTATE:
        P.check_max_angle(P.MAX_ANGLE_DEFAULT if max_angle is None else max_angle)


def _extract_payload_rotated(stego_bgr: np.ndarray, rule: F.Rule, max_angle: float, device: int):
    """search="rotate" (include/wmhip.h, "rotation resynchronisation"): the stego is the whole marked image rotated about its
    centre by at most ``max_angle`` degrees, on a canvas of the marked size (corners cut) or an expanded one.  The angle is
    searched for on the device - every candidate rotates the luma back, the plain metric reads it - and the winner is
    decoded as the meta says, the tiles whose footprint leaves the stego not voting.  Every refusal comes before the first
    device call."""
    if stego_bgr.dtype != np.uint8 or stego_bgr.ndim != 3 or stego_bgr.shape[2] != 3:
        raise ValueError("stego must be uint8 [h, w, 3]")
    R.check_rotate(*stego_bgr.shape[:2], rule.H, rule.W, "stego")
    tbi = rule.map()[0].reshape(rule.grid)
    dz = P.dither_table(*rule.grid, rule.key) if rule.dither else None
    ctx = _ctx(device)
    found = ctx.payload_locate_angle(_Gray.planes_in(ctx, stego_bgr), rule.H, rule.W, max_angle, rule.delta, dither=dz)
    if found is None:                                                      # no candidate has a whole tile inside the stego
        return b"", False, 0.0, None
    theta, m, tile_ok, _ = found
    data, valid, conf, _ = F.search_tail(ctx, P.votes_of_metric(m, tile_ok), 0, 0, 0, 0, tbi, rule.carried, rule.code)
    return data, valid, conf, float(np.degrees(theta))


def _extract_payload_resized(stego_bgr: np.ndarray, rule: F.Rule, device: int):
    """search="resize" (include/wmhip.h, "resize resynchronisation"): the stego is the whole marked image, resized to any
    shape within resample.MAX_SCALE of the meta's on either axis.  Its luma - one plane, taken at the stego's own size - is
    resampled back to the marked shape on the device and decoded as the meta says.  Every refusal comes before the first
    device call."""
    if stego_bgr.dtype != np.uint8 or stego_bgr.ndim != 3 or stego_bgr.shape[2] != 3:
        raise ValueError("stego must be uint8 [h, w, 3]")
    h, w = stego_bgr.shape[:2]
    R.check_resize(h, w, rule.H, rule.W, "stego")
    _, order, offs = rule.map()
    ctx = _ctx(device)
    dz = P.dither_table(*rule.grid, rule.key) if rule.dither else None
    Y = _Gray.planes_in(ctx, stego_bgr)
    if (h, w) == (rule.H, rule.W):                                         # nothing to restore: the plain extract
        soft = ctx.payload_soft(Y, order, offs, rule.carried, rule.delta, dither=dz)
    else:
        soft = ctx.payload_soft_resized(Y, rule.H, rule.W, order, offs, rule.carried, rule.delta, dither=dz)
    data, valid = P.payload_unframe(F.read(ctx, soft, rule.code))
    return data, bool(valid), P.confidence(soft, offs, 1), (h / rule.H, w / rule.W)


def _extract_payload_cropped(stego_bgr: np.ndarray, rule: F.Rule, keyed: bool, device: int):
    """search="crop" and, ``keyed``, search="crop-keyed" (include/wmhip.h, "crop resynchronisation" and "keyed crop
    resynchronisation"): the stego is any axis-aligned crop of the marked image - one marked with dither=True for the keyed
    search, with dither=False for the other.  Every refusal comes before the first device call."""
    if keyed and not rule.dither:
        raise ValueError("search='crop-keyed' reads a payload embedded with dither=True; this one has none: use search='crop'")
    if not keyed and rule.dither:
        raise ValueError("resynchronising a dithered payload is not supported: keyed dither removes the grid's keyless "
                         "signal (search='crop' needs a payload embedded with dither=False); use search='crop-keyed'")
    if not keyed and rule.carried > P.SYNC_MAX_BITS:
        raise ValueError(f"search='crop' takes payloads of at most {P.SYNC_MAX_BITS} bits, this one has {rule.carried}")
    if stego_bgr.dtype != np.uint8 or stego_bgr.ndim != 3 or stego_bgr.shape[2] != 3:
        raise ValueError("stego must be uint8 [h, w, 3]")
    F.check_crop_shape(*stego_bgr.shape[:2], rule.H, rule.W, "stego")
    tbi = rule.map()[0].reshape(rule.grid)
    table = P.dither_table(*rule.grid, rule.key).reshape(rule.grid) if keyed else None
    ctx = _ctx(device)
    Y = _Gray.planes_in(ctx, stego_bgr)
    if keyed:
        (py, px), (ty, tx), s1 = ctx.payload_locate_keyed(Y, table, rule.delta)
        votes = P.keyed_votes(s1, table[ty:ty + s1.shape[0], tx:tx + s1.shape[1]], rule.delta)
    else:
        (py, px), place, votes = ctx.payload_locate(Y, tbi, rule.carried, rule.delta)
        if place is None:                                                  # (cannot happen for h <= H, w <= W; the rule names it)
            return b"", False, 0.0, None
        ty, tx = place
    return F.search_tail(ctx, votes, py, px, ty, tx, tbi, rule.carried, rule.code)


def extract_payload_arrays(stego_bgr: np.ndarray, meta, password: str, device: int = 0, *, search=None, max_angle=None):
    """-> (data bytes, valid, confidence).  valid: the decoded frame's length header and CRC hold.  confidence: the mean
    over the bits of |soft| / (tiles voting), 1 for an untouched stego and near 0 for an image that carries nothing.
    ``search="crop"``: the stego may be any axis-aligned crop of the marked image (h <= H, w <= W, origin anywhere); the
    embed's tile grid and the crop's place in it are searched for on the device, and the result is (data, valid,
    confidence, origin) with origin = (y0, x0) of the crop in the marked image - meaningful where valid is True.
    ``search="crop"`` takes payloads embedded with dither=False, ``search="crop-keyed"`` those embedded with dither=True
    (one keyed search over grid phase and place); each refuses the other's meta ("Crop
    resynchronisation" and "Keyed crop resynchronisation").
    ``search="resize"``: the stego may be the whole marked image resized to another shape, the aspect included, up to
    resample.MAX_SCALE either way on either axis; it is resampled back to the meta's shape on the device and decoded as an
    unresized one, dither and channel code as the meta says.  The result is (data, valid, confidence, scale) with scale =
    (h / H, w / W); a stego of the meta's own shape gives the plain extract's values ("Resize resynchronisation").
    ``search="rotate"``: the stego may be the whole marked image rotated about its centre by up to ``max_angle`` degrees
    (10 by default, at most 45), on a canvas of the marked size or an expanded one; the angle is searched for on the device
    and the winner decoded, dither and channel code as the meta says.  The result is (data, valid, confidence, angle), angle
    the winning candidate's theta in degrees in the rule's sense - the rotation that was undone ("Rotation
    resynchronisation").  ``max_angle`` goes with this search only."""
    _check_search(search, max_angle)
    M.check_password_type(password, "extract")
    M.require_password(password, "extract")
    rule = F.checked_rule(meta, password)
    if search == SEARCH_RESIZE:
        return _extract_payload_resized(stego_bgr, rule, device)
    if search == SEARCH_ROTATE:
        return _extract_payload_rotated(stego_bgr, rule, P.MAX_ANGLE_DEFAULT if max_angle is None else float(max_angle), device)
    if search is not None:
        return _extract_payload_cropped(stego_bgr, rule, search == "crop-keyed", device)
    _check_stego_shape(stego_bgr, dict(shape=(rule.H, rule.W)))
    _, order, offs = rule.map()
    ctx = _ctx(device)
    dz = P.dither_table(*rule.grid, rule.key) if rule.dither else None
    soft = ctx.payload_soft(_Gray.planes_in(ctx, stego_bgr), order, offs, rule.carried, rule.delta, dither=dz)
    data, valid = P.payload_unframe(F.read(ctx, soft, rule.code))
    return data, bool(valid), P.confidence(soft, offs, 1)


def embed_payload(cover_path: str, payload, out_path: str, meta_path: str, *, password: Optional[str] = None,
                  payload_type: str = "text", delta: float = P.DELTA_DEFAULT, nonce: Optional[bytes] = None, device: int = 0,
                  verify: bool = True, dither: bool = False, code=None):
    """``payload``: a str or bytes, or the path of a .txt / .json file (read when it exists, like the reference's
    text_data / wm_source, core:102-106).  Returns (out_path, meta_path, psnr, ssim); the stego is written as PNG.
    ``verify`` as in embed_payload_arrays: a payload that does not decode from its own stego raises, and neither the
    stego nor the meta is written.  ``dither`` and ``code`` as there."""
    M.check_password_type(password, "embed")
    M.require_password(password, "embed")
    hostapi.check_delta(delta)
    P.check_code(code)
    data = P.payload_bytes(payload, payload_type)                          # refused before anything else is read
    cover = hg.read_image_bgr(cover_path)
    if nonce is None:
        nonce = os.urandom(8)
    # (a json payload is canonical by now; canonicalising it again inside leaves it as it is)
    r = embed_payload_arrays(cover, data, password, nonce, payload_type=payload_type, delta=delta, device=device, verify=verify,
                             dither=dither, code=code)
    out_path = M.out_name(out_path, "_stego.png")
    if not hg.write_png(out_path, r["stego"], 0):
        raise IOError("Ghi stego thất bại.")
    M.save_payload_meta(meta_path, r["meta"])                              # one packed member: 0.7 KB, the same size whatever the values
    return out_path, meta_path, r["psnr"], r["ssim"]


def extract_payload(stego_path: str, meta_path: str, out_path: Optional[str] = None, *, password: Optional[str] = None,
                    device: int = 0, search=None, max_angle=None):
    """-> (data, valid, confidence, path written or None).  With ``out_path`` the payload is written as ``_text.txt`` /
    ``_data.json`` by the reference's renaming (core:229-242).  ``search="crop"`` / ``"crop-keyed"`` as in extract_payload_arrays: the stego
    file may be a crop of the marked image, and the result is (data, valid, confidence, path, origin).  ``search="resize"``:
    the file may be the marked image resized as a whole, and the result is (data, valid, confidence, path, scale).
    ``search="rotate"``, with ``max_angle`` degrees (10 by default): the file may be the marked image rotated about its centre,
    and the result is (data, valid, confidence, path, angle)."""
    _check_search(search, max_angle)
    M.check_password_type(password, "extract")
    M.require_password(password, "extract")
    meta = M.load_payload_meta(meta_path)
    data, valid, conf, *origin = extract_payload_arrays(hg.read_image_bgr(stego_path), meta, password, device, search=search,
                                                           max_angle=max_angle)
    written = P.write_payload(out_path, data, str(meta["payload_type"])) if out_path else None
    return (data, valid, conf, written, *origin)


embed_watermark = embed
extract_watermark = extract
