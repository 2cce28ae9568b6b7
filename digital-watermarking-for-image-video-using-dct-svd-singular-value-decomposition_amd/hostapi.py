"""ctypes binding of libwmhip.so (include/wmhip.h) - the thin Python side of
the C ABI.  No CPU fallback: if the HIP library is missing or there is no GPU,
calls raise (``WmLibraryError`` / ``WmError``) instead of computing anything
on the host.

The error mapping mirrors what the reference's callers see
(app_dct_svd_single.py:115-116,208-209, numpy LinAlgError):
  WM_ERR_BADARG -> ValueError, WM_ERR_NOCONV -> numpy.linalg.LinAlgError,
  WM_ERR_NOMEM  -> MemoryError, WM_ERR_HIP -> WmError (RuntimeError).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
from typing import Optional

import numpy as np

from . import payload as P
from . import resample as R

WM_OK, WM_ERR_BADARG, WM_ERR_HIP, WM_ERR_NOCONV, WM_ERR_NOMEM = 0, 1, 2, 3, 4
TILE = 8
ABI_VERSION = 1

_HERE = os.path.dirname(os.path.abspath(__file__))
# WMHIP_LIB selects another build of the same HIP library (A/B timing of kernel variants)
LIB_PATH = os.environ.get("WMHIP_LIB") or os.path.join(_HERE, "csrc", "libwmhip.so")


class WmLibraryError(ImportError):
    """libwmhip.so is not built / not loadable."""


class WmError(RuntimeError):
    """A HIP runtime call inside libwmhip.so failed."""


_lib = None

_sz = C.c_size_t
_vp = C.c_void_p
_i = C.c_int
_f = C.c_float

# name -> argtypes  (every symbol include/wmhip.h declares); "wm_x*" is wm_x and wm_x_dev, which take the same
_DECLARED = {
    "wm_abi_version": [],
    "wm_last_error": [],
    "wm_device_count": [C.POINTER(_i)],
    "wm_create": [_i, _vp, C.POINTER(_vp)],
    "wm_destroy": [_vp],
    "wm_sync": [_vp],
    "wm_check_status": [_vp],
    "wm_malloc": [_vp, _sz, C.POINTER(_vp)],
    "wm_free": [_vp, _vp],
    "wm_memcpy_h2d": [_vp, _vp, _vp, _sz],
    "wm_memcpy_d2h": [_vp, _vp, _vp, _sz],
    "wm_memset": [_vp, _vp, _i, _sz],
    "wm_copy_mapped_dev": [_vp, _vp, _vp, _sz, _i],
    "wm_event_record": [_vp, _i],
    "wm_event_elapsed_ms": [_vp, _i, _i, C.POINTER(_f)],
    "wm_embed_tiles_u8*": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i],
    "wm_sigma_tiles_u8*": [_vp, _vp, _vp, _i, _i, _i, _i, _sz],
    "wm_svd_tiles_f32*": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz],
    "wm_extract_tiles_u8*": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i],
    "wm_extract_tiles_px_u8_dev": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i],
    "wm_tile_factors_to_pixel_dev": [_vp, _vp, _vp, _vp, _vp, _sz],
    "wm_extract_tiles_sum_u8": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i],
    "wm_reconstruct_tiles*": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i],
    "wm_detect_tiles_u8*": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f],
    # texture-masked strength: the unmasked argument lists with (lo, hi) or (lo, hi, cut) appended
    "wm_mask_sigma_w_tiles_u8*": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _f],
    "wm_embed_tiles_masked_u8*": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i, _f, _f],
    "wm_extract_tiles_masked_u8*": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i, _f, _f, _f],
    "wm_extract_tiles_px_masked_u8_dev": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i, _f, _f, _f],
    "wm_extract_tiles_sum_masked_u8": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i, _f, _f, _f],
    "wm_extract_unscrambled_masked_u8_dev": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i, _i, _i, _f, _f, _f],
    "wm_detect_tiles_masked_u8*": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _f, _f, _f],
    # blind payload (one bit per tile in the parity of sigma_1): the plane arguments, then delta
    "wm_payload_sigma_w_tiles_u8*": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _f],
    "wm_embed_tiles_payload_u8*": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _f],
    "wm_payload_metric_tiles_u8*": [_vp, _vp, _vp, _i, _i, _i, _i, _sz, _f],
    "wm_payload_soft_tiles_u8*": [_vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _sz, _f],
    # the same with keyed dither: tile_dither after the tile bits / the stego, dither_plane_stride before delta
    "wm_payload_sigma_w_tiles_dither_u8*": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f],
    "wm_embed_tiles_payload_dither_u8*": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f],
    "wm_payload_metric_tiles_dither_u8*": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f],
    "wm_payload_soft_tiles_dither_u8*": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _sz, _sz, _f],
    # crop resynchronisation: (stego, votes, sums, the plane arguments, delta); (votes, tile_bit_index, scores, ny, nx, nby, nbx, n_bits)
    "wm_payload_phase_scan_u8*": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _f],
    "wm_payload_offset_scores*": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i],
    # keyed crop resynchronisation: (stego, s1, the plane arguments); (s1, tile_dither, scores, h, w, nby, nbx, delta)
    "wm_payload_sigma1_scan_u8*": [_vp, _vp, _vp, _i, _i, _i, _i, _sz],
    "wm_payload_keyed_scores*": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f],
    # clip resynchronisation: (s1, n_anchor, tables, n_tables, table_of, n_cand, best, h, w, nby, nbx, delta)
    "wm_payload_keyed_best*": [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _f],
    # frame resynchronisation: (s1, s1_window_stride, s1_frame_stride, n_frames, tables, n_tables, scores, ny, nx, nby, nbx, ty, tx, delta)
    "wm_payload_frame_scores*": [_vp, _vp, _sz, _sz, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _f],
    # channel code: (llr, n_info, n_codewords, llr_stride, info_bits, final_metric, decisions)
    "wm_payload_decode_k7*": [_vp, _vp, _i, _i, _sz, _vp, _vp, _vp],
    # resize resynchronisation: (src, dst, n_planes, h_in, w_in, src strides, h_out, w_out, dst strides, first_x, w_x, T_x, first_y, w_y, T_y)
    "wm_resample_planes_u8*": [_vp, _vp, _vp, _i, _i, _i, _i, _sz, _i, _i, _i, _sz, _vp, _vp, _i, _vp, _vp, _i],
    # rotation resynchronisation: (src, dst, n_planes, h, w, src strides, H, W, dst strides, cand, n_angles, K);
    # (metric, cand, n_angles, scores, counts, valid, h, w, H, W)
    "wm_rotate_planes_u8*": [_vp, _vp, _vp, _i, _i, _i, _i, _sz, _i, _i, _i, _sz, _vp, _i, _vp],
    "wm_payload_angle_scores*": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i],
    "wm_ref_embed_u8": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i],
    "wm_ref_sigma_u8": [_vp, _vp, _vp, _i, _i, _i],
    "wm_ref_last_sweeps": [_vp, C.POINTER(_i)],
    "wm_ref_last_flops": [_vp, C.POINTER(C.c_double), C.POINTER(_i)],
    "wm_ref_embed_planes_u8_when": [_vp, _vp, _vp, C.POINTER(_i), _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i],
    "wm_ref_embed_planes_u8*": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i],
    "wm_ref_sigma_planes_u8*": [_vp, _vp, _vp, _i, _i, _i, _i, _sz],
    "wm_ref_extract_planes_u8*": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _f, _i],
    "wm_ref_detect_planes_u8*": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _f],
    "wm_ref_svd_f32": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i],
    "wm_ref_svd_planes_f32": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _i],
    "wm_ref_extract_u8": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i],
    "wm_ref_reconstruct_f32": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i],
    "wm_ref_detect_u8": [_vp, _vp, _vp, _vp, C.POINTER(C.c_double), _i, _i, _i, _f],
    "wm_bgr_to_ycrcb_u8_dev": [_vp, _vp, _vp, _sz],
    "wm_ycrcb_to_bgr_u8_dev": [_vp, _vp, _vp, _sz],
    "wm_bgr_to_gray_u8_dev": [_vp, _vp, _vp, _sz],
    "wm_bgr_to_y_u8_dev": [_vp, _vp, _vp, _sz],
    "wm_replace_y_u8_dev": [_vp, _vp, _vp, _vp, _sz],
    "wm_sqdiff_u8_dev": [_vp, _vp, _vp, _sz, _vp],
    "wm_ssim_dev": [_vp, _vp, _sz, _vp, _sz, _i, _i, _i, _vp],
    "wm_normalize_u8*": [_vp, _vp, _sz, _i, _vp],
    "wm_permute_u8_f32_dev": [_vp, _vp, _vp, _vp, _sz, _i],
    "wm_permute_f32_dev": [_vp, _vp, _vp, _vp, _sz, _i],
    "wm_unpermute_f32_dev": [_vp, _vp, _vp, _vp, _sz, _i],
    "wm_route_create_dev": [_vp, _vp, _sz, C.POINTER(_vp)],
    "wm_route_destroy": [_vp, _vp],
    "wm_unpermute_normalize_u8_dev": [_vp, _vp, _vp, _vp, _sz, _i, _i],
    "wm_permute_u8_f32_routed_dev": [_vp, _vp, _vp, _vp, _sz, _i],
    "wm_extract_unscrambled_u8_dev": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _sz, _sz, _f, _i, _i, _i],
    "wm_yuv_frames_to_bgr_planes_u8*": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _sz],
    "wm_bgr_planes_to_yuv_frames_u8*": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _sz],
    "wm_color_u8": [_vp, _i, _vp, _vp, _vp, _vp, _sz],
    "wm_psnr_u8": [_vp, _vp, _vp, _sz, C.POINTER(C.c_double)],
    "wm_ssim": [_vp, _vp, _vp, _i, _i, _i, C.POINTER(C.c_double)],
    "wm_nlmeans_u8_dev": [_vp, _vp, _vp, _i, _i, _i, _f, _i, _i],
    "wm_clahe_u8_dev": [_vp, _vp, _vp, _i, _i, _f, _i, _i],
    "wm_unsharp_u8_dev": [_vp, _vp, _vp, _i, _i, _i, _f],
    "wm_bgr_to_lab_u8_dev": [_vp, _vp, _vp, _sz],
    "wm_lab_to_bgr_u8_dev": [_vp, _vp, _vp, _sz],
    "wm_enhance_extract_u8*": [_vp, _vp, _vp, _i, _i, _i],
}
SIGNATURES = {n: a for d, a in _DECLARED.items() for n in ((d[:-1], d[:-1] + "_dev") if d.endswith("*") else (d,))}


def load_library(path: Optional[str] = None):
    """dlopen libwmhip.so and type every entry point.  Raises WmLibraryError -
    never falls back to a host implementation."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise WmLibraryError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    try:
        lib = C.CDLL(p)
    except OSError as e:  # missing libamdhip64 etc.
        raise WmLibraryError(f"cannot load {p}: {e}") from e
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)            # AttributeError if the ABI drifted
        fn.argtypes = argtypes
        fn.restype = C.c_char_p if name == "wm_last_error" else _i
    if lib.wm_abi_version() != ABI_VERSION:
        raise WmLibraryError(f"ABI version mismatch: library {lib.wm_abi_version()} != binding {ABI_VERSION}")
    if path is None:
        _lib = lib
    return lib


def _raise(lib, rc: int):
    msg = (lib.wm_last_error() or b"").decode("utf-8", "replace")
    if rc == WM_ERR_BADARG:
        raise ValueError(msg)
    if rc == WM_ERR_NOCONV:
        raise np.linalg.LinAlgError(msg)
    if rc == WM_ERR_NOMEM:
        raise MemoryError(msg)
    raise WmError(f"[{rc}] {msg}")


def device_count() -> int:
    lib = load_library()
    n = _i(0)
    rc = lib.wm_device_count(C.byref(n))
    if rc:
        _raise(lib, rc)
    return n.value


def _plane_layout(a: np.ndarray):
    """(n_planes, H, W, row_stride, plane_stride) in elements of a [H,W] or
    [N,H,W] array whose last axis is contiguous."""
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("planes must be [H, W] or [n_planes, H, W]")
    n, H, W = a.shape
    it = a.itemsize
    if W > 1 and a.strides[2] != it:
        raise ValueError("last axis must be contiguous")
    if any(st < 0 or st % it for st in a.strides):
        raise ValueError("negative or unaligned strides are not supported")
    rs = max(W, a.strides[1] // it) if H > 1 else W       # elements between rows
    ps = a.strides[0] // it if n > 1 else rs * H           # elements between planes
    if n > 1 and ps < rs * (H - 1) + W:
        raise ValueError("planes overlap")
    return n, H, W, rs, ps


def _p(a):
    """an array's address as the ABI takes it; None (an output the caller does not want) stays None"""
    return None if a is None else _vp(a.ctypes.data)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _digest(a) -> bytes:
    """what a device cache knows an array's contents by"""
    return hashlib.blake2b(np.ascontiguousarray(a).view(np.uint8), digest_size=16).digest()


def _dense(a: np.ndarray, dtype, ndim: int, what: str):
    """a [H, W] (ndim 2) or [N, H, W] (ndim 3) input of the given dtype, made dense -> (array, H, W, min(H, W))"""
    if a.dtype != dtype or a.ndim != ndim:
        raise ValueError(what)
    H, W = a.shape[-2:]
    return np.ascontiguousarray(a), H, W, min(H, W)


def check_mask(mask) -> tuple:
    """The texture-masked rule's (lo, hi, cut) as floats, checked on the host as the library checks them
    (include/wmhip.h): 0 <= lo < hi, both finite, 0 < cut <= 1."""
    try:
        lo, hi, cut = (float(x) for x in mask)
    except (TypeError, ValueError):
        raise ValueError("mask must be (lo, hi, cut)") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 <= lo < hi):
        raise ValueError(f"mask needs finite 0 <= lo < hi, got lo={lo}, hi={hi}")
    if not (0.0 < cut <= 1.0):                                             # (NaN fails both comparisons)
        raise ValueError(f"mask needs 0 < cut <= 1, got {cut}")
    return lo, hi, cut


def _mask_args(mask) -> tuple:
    """() for uniform strength (mask None), else the checked (lo, hi, cut) the masked entry points take after the
    unmasked arguments."""
    return () if mask is None else check_mask(mask)


PAYLOAD_DELTA_MIN, PAYLOAD_DELTA_MAX = 8.0, 512.0


def check_delta(delta) -> float:
    """The payload rule's step as a float holding a float32 value, checked on the host as the library checks it
    (include/wmhip.h): finite, 8 <= delta <= 512."""
    try:
        d = float(np.float32(delta))
    except (TypeError, ValueError):
        raise ValueError("delta must be a number") from None
    if not (np.isfinite(d) and PAYLOAD_DELTA_MIN <= d <= PAYLOAD_DELTA_MAX):
        raise ValueError(f"payload needs a finite delta in 8..512, got {delta}")
    return d


def _tile_bits(tile_bit, n_tiles: int) -> np.ndarray:
    """tile_bit as the ABI takes it: uint8 [n_tiles] of 0 / 1"""
    tb = np.ascontiguousarray(tile_bit).reshape(-1)
    if tb.size != n_tiles:
        raise ValueError(f"tile_bit has {tb.size} entries for {n_tiles} tiles")
    if tb.size and (tb.min() < 0 or tb.max() > 1):
        raise ValueError("tile_bit entries must be 0 or 1")
    return tb.astype(np.uint8)


def _dither_words(dither, n_planes: int, n_tiles: int):
    """``dither=`` of a payload call as the ABI takes it: None (the dither-free rule), else (uint16 words, plane stride) of a
    [n_tiles] table shared by the planes (stride 0) or an [N, n_tiles] one with a row per plane (stride n_tiles)."""
    if dither is None:
        return None
    d = np.ascontiguousarray(dither)
    if d.dtype != np.uint16:
        raise ValueError("dither must be uint16")
    if d.shape == (n_tiles,):
        return d, 0
    if d.shape == (n_planes, n_tiles):
        return d, n_tiles
    raise ValueError(f"dither has shape {d.shape} for {n_planes} planes of {n_tiles} tiles: [n_tiles] or [N, n_tiles]")


def check_payload_csr(order, offs, n_bits: int, n_tiles: int):
    """(order int32 [n_tiles], offs int32 [n_bits + 1]) of a tile-to-bit map, checked as the host-pointer entry point checks
    them: 1 <= n_bits <= n_tiles, offs from 0 to n_tiles without decreasing, every order entry a tile of the grid."""
    n_bits = int(n_bits)
    if n_bits < 1 or n_bits > n_tiles:
        raise ValueError(f"n_bits must be in 1..n_tiles ({n_tiles}), got {n_bits}")
    order = np.ascontiguousarray(order).reshape(-1); offs = np.ascontiguousarray(offs).reshape(-1)
    if order.size != n_tiles or offs.size != n_bits + 1:
        raise ValueError(f"order / offs have {order.size} / {offs.size} entries for {n_tiles} tiles and {n_bits} bits")
    if int(offs[0]) != 0 or int(offs[-1]) != n_tiles or np.any(np.diff(offs) < 0):
        raise ValueError("offs must run from 0 to n_tiles without decreasing")
    if int(order.min()) < 0 or int(order.max()) >= n_tiles:
        raise ValueError("order names a tile outside the grid")
    return order.astype(np.int32), offs.astype(np.int32)


def _planes_of(a: np.ndarray, dtype, what: str):
    """_plane_layout of a [H, W] / [N, H, W] input of the given dtype, which may be strided"""
    if a.dtype != dtype:
        raise ValueError(what)
    return _plane_layout(a)


class _Staging:
    """Context._staging(): the device buffers of one call, freed together."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def alloc(self, nbytes: int) -> int:
        self.bufs.append(self.ctx.malloc(nbytes))
        return self.bufs[-1]

    def up(self, *arrays, floor: int = 0):
        ds = [self.alloc(max(a.nbytes, floor)) for a in arrays]
        for d, a in zip(ds, arrays):
            self.ctx.h2d(d, a)
        return ds

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        while self.bufs:
            self.ctx.free(self.bufs.pop())


class Context:
    """One device + one HIP stream (wm_ctx).  ``stream`` may be a raw
    hipStream_t handle (e.g. ``torch.cuda.current_stream().cuda_stream``)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self.lib = load_library()
        h = _vp()
        rc = self.lib.wm_create(device, _vp(stream) if stream else None, C.byref(h))
        if rc:
            _raise(self.lib, rc)
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            for entries in self.__dict__.pop("_dev_cache", {}).values():
                for ent in entries:
                    self._drop(ent)
            for d in self.__dict__.pop("_enh_bufs", (0, 0, 0))[1:]:
                self.lib.wm_free(self._h, _vp(d))
            self.lib.wm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _call(self, name, *args):
        rc = getattr(self.lib, name)(self._h, *args)
        if rc:
            _raise(self.lib, rc)

    # ---- plumbing -------------------------------------------------------
    def sync(self):
        self._call("wm_sync")

    def check_status(self):
        self._call("wm_check_status")

    def malloc(self, nbytes: int) -> int:
        p = _vp()
        self._call("wm_malloc", nbytes, C.byref(p))
        return p.value

    def free(self, dptr: int):
        self._call("wm_free", _vp(dptr))

    def h2d(self, dptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._call("wm_memcpy_h2d", _vp(dptr), _p(arr), arr.nbytes)
        self.sync()

    def d2h(self, arr: np.ndarray, dptr: int):
        assert arr.flags.c_contiguous
        self._call("wm_memcpy_d2h", _p(arr), _vp(dptr), arr.nbytes)

    def _staging(self):
        """``with self._staging() as dev``: the device buffers of one call.  dev.alloc(nbytes) -> address;
        dev.up(a, b, .., floor=0) -> addresses of copies of the arrays, every one a wm_malloc of its own (of at least floor
        bytes), all allocated before the first is copied.  On exit all are freed, last first - also when the body, or
        an allocation after the first, raised."""
        return _Staging(self)

    def _cached(self, kind: str, tag, upload) -> dict:
        """The device-resident entry of (kind, tag); on a miss ``upload()`` -> {"d": address, ..} makes it.  Two entries
        per kind: a third sends the oldest away, after a sync (queued work may still read it).  close() drops the rest."""
        entries = self.__dict__.setdefault("_dev_cache", {}).setdefault(kind, [])     # (made here: a Context may skip __init__)
        for ent in entries:
            if ent["tag"] == tag:
                return ent
        ent = dict(upload(), tag=tag)
        entries.append(ent)
        while len(entries) > 2:
            old = entries.pop(0)
            self.sync()
            self._drop(old)
        return ent

    def _drop(self, ent: dict):
        try:
            if ent.get("route"):
                self.lib.wm_route_destroy(self._h, _vp(ent["route"]))
            self.free(ent["d"])
        except Exception:
            pass

    def copy_mapped(self, dst: int, src: int, nbytes: int, n_workgroups: int = 0):
        """async copy kernel between device memory and mapped pinned host memory (either direction) on this stream"""
        self._call("wm_copy_mapped_dev", _vp(dst), _vp(src), nbytes, n_workgroups)

    def memset(self, dptr: int, value: int, nbytes: int):
        self._call("wm_memset", _vp(dptr), value, nbytes)

    def event_record(self, slot: int):
        self._call("wm_event_record", slot)

    def event_elapsed_ms(self, a: int, b: int) -> float:
        ms = _f(0)
        self._call("wm_event_elapsed_ms", a, b, C.byref(ms))
        return ms.value

    # ---- device-pointer entry points (ints are device addresses) ---------
    def embed_tiles_u8_dev(self, host, sigma_w, stego, sigma_c, yw, n_planes, H, W, row_stride,
                           plane_stride, sigma_w_plane_stride, alpha, K):
        self._call("wm_embed_tiles_u8_dev", _vp(host), _vp(sigma_w), _vp(stego), _vp(sigma_c),
                   _vp(yw) if yw else None, n_planes, H, W, row_stride, plane_stride,
                   sigma_w_plane_stride, alpha, K)

    def embed_tiles_masked_u8_dev(self, host, sigma_w, stego, sigma_c, yw, n_planes, H, W, row_stride,
                                  plane_stride, sigma_w_plane_stride, alpha, K, lo, hi):
        """embed_tiles_u8_dev with texture-masked strength (include/wmhip.h)."""
        self._call("wm_embed_tiles_masked_u8_dev", _vp(host), _vp(sigma_w), _vp(stego), _vp(sigma_c),
                   _vp(yw) if yw else None, n_planes, H, W, row_stride, plane_stride,
                   sigma_w_plane_stride, alpha, K, lo, hi)

    def mask_sigma_w_tiles_u8_dev(self, planes, sigma_w, sigma_w_eff, gain, n_planes, H, W, row_stride, plane_stride,
                                  sigma_w_plane_stride, lo, hi):
        self._call("wm_mask_sigma_w_tiles_u8_dev", _vp(planes), _vp(sigma_w) if sigma_w else None,
                   _vp(sigma_w_eff) if sigma_w_eff else None, _vp(gain) if gain else None,
                   n_planes, H, W, row_stride, plane_stride, sigma_w_plane_stride, lo, hi)

    def sigma_tiles_u8_dev(self, planes, sigma, n_planes, H, W, row_stride, plane_stride):
        self._call("wm_sigma_tiles_u8_dev", _vp(planes), _vp(sigma), n_planes, H, W, row_stride, plane_stride)

    def svd_tiles_f32_dev(self, planes, U, S, Vt, n_planes, H, W, row_stride, plane_stride):
        self._call("wm_svd_tiles_f32_dev", _vp(planes), _vp(U), _vp(S), _vp(Vt), n_planes, H, W,
                   row_stride, plane_stride)

    def extract_tiles_u8_dev(self, stego, sigma_c, Uw, Vwt, out, n_planes, H, W, row_stride,
                             plane_stride, uv_plane_stride, alpha, K):
        self._call("wm_extract_tiles_u8_dev", _vp(stego), _vp(sigma_c), _vp(Uw), _vp(Vwt), _vp(out),
                   n_planes, H, W, row_stride, plane_stride, uv_plane_stride, alpha, K)

    def extract_tiles_px_u8_dev(self, stego, sigma_c, Ux, Vxt, out, n_planes, H, W, row_stride,
                                plane_stride, uv_plane_stride, alpha, K):
        """extract_tiles_u8_dev with pixel-domain factors (tile_factors_to_pixel_dev)."""
        self._call("wm_extract_tiles_px_u8_dev", _vp(stego), _vp(sigma_c), _vp(Ux), _vp(Vxt), _vp(out),
                   n_planes, H, W, row_stride, plane_stride, uv_plane_stride, alpha, K)

    def tile_factors_to_pixel_dev(self, Uw, Vwt, Ux, Vxt, n_tiles):
        self._call("wm_tile_factors_to_pixel_dev", _vp(Uw), _vp(Vwt), _vp(Ux), _vp(Vxt), n_tiles)

    def reconstruct_tiles_dev(self, Uw, sw_hat, Vwt, out, n_planes, H, W):
        self._call("wm_reconstruct_tiles_dev", _vp(Uw), _vp(sw_hat), _vp(Vwt), _vp(out), n_planes, H, W)

    def detect_tiles_u8_dev(self, stego, sigma_c, sigma_w, scores, n_planes, H, W, row_stride,
                            plane_stride, sigma_w_plane_stride, alpha):
        self._call("wm_detect_tiles_u8_dev", _vp(stego), _vp(sigma_c), _vp(sigma_w), _vp(scores),
                   n_planes, H, W, row_stride, plane_stride, sigma_w_plane_stride, alpha)

    # full-frame mode, device-resident planes / factors (ints are device addresses)
    def ref_embed_planes_u8_dev(self, host, sigma_w, stego, sigma_c, yw, n_planes, H, W, row_stride, plane_stride,
                                sigma_w_plane_stride, alpha, K):
        self._call("wm_ref_embed_planes_u8_dev", _vp(host), _vp(sigma_w), _vp(stego), _vp(sigma_c),
                   _vp(yw) if yw else None, n_planes, H, W, row_stride, plane_stride, sigma_w_plane_stride, alpha, K)

    def ref_sigma_planes_u8_dev(self, planes, sigma, n_planes, H, W, row_stride, plane_stride):
        self._call("wm_ref_sigma_planes_u8_dev", _vp(planes), _vp(sigma), n_planes, H, W, row_stride, plane_stride)

    def ref_extract_planes_u8_dev(self, stego, sigma_c, Uw, Vwt, out, n_planes, H, W, row_stride, plane_stride, alpha, K):
        self._call("wm_ref_extract_planes_u8_dev", _vp(stego), _vp(sigma_c), _vp(Uw), _vp(Vwt), _vp(out), n_planes,
                   H, W, row_stride, plane_stride, alpha, K)

    def ref_detect_planes_u8_dev(self, stego, sigma_c, sigma_w, scores, n_planes, H, W, row_stride, plane_stride, alpha):
        self._call("wm_ref_detect_planes_u8_dev", _vp(stego), _vp(sigma_c), _vp(sigma_w), _vp(scores), n_planes,
                   H, W, row_stride, plane_stride, alpha)

    # ---- NumPy (host-buffer) entry points --------------------------------
    def embed_tiles(self, host: np.ndarray, sigma_w: np.ndarray, alpha: float, K: int = 8,
                    want_yw: bool = False, mask=None):
        """host uint8 [H,W] or [N,H,W]; sigma_w float32 [nby,nbx,8] (shared) or
        [N,nby,nbx,8].  Returns (stego uint8, sigma_c float32 [N?,nby,nbx,8], yw or None).
        ``mask=(lo, hi, cut)``: texture-masked strength (include/wmhip.h) - every tile adds alpha * G * sigma_w with
        G = (1, g, .., g) and g from its own cover singular values (a black tile, which has no singular vectors of its
        own, along the flat one: it becomes the constant alpha * sw_1 / 8); ``cut`` plays no part in the embed."""
        m = _mask_args(mask)
        n, H, W, rs, ps = _planes_of(host, np.uint8, "host planes must be uint8")
        nby, nbx = H // TILE, W // TILE
        sw = _f32(sigma_w)
        per_plane = sw.ndim == 4
        if sw.shape[-3:] != (nby, nbx, 8) or (per_plane and sw.shape[0] != n):
            raise ValueError(f"sigma_w shape {sw.shape} does not match {n}x{nby}x{nbx}x8")
        return self._embed_tiles_with(host, want_yw, lambda hostc, *outs: self._call(
            "wm_embed_tiles_masked_u8" if m else "wm_embed_tiles_u8", _p(hostc), _p(sw), *outs, n, H, W, W, H * W,
            nby * nbx * 8 if per_plane else 0, float(alpha), int(K), *m[:2]))

    def _embed_tiles_with(self, host: np.ndarray, want_yw: bool, call):
        """What the tile-mode embeds share: ``call(dense host [n, H, W], stego, sigma_c, yw or None)`` fills the outputs
        (the last three as the ABI takes them), which come back without the leading axis for a [H, W] host."""
        n, H, W = _plane_layout(host)[:3]
        hostc = np.ascontiguousarray(host.reshape(n, H, W))    # stego is dense; host may be strided: both share one layout
        stego, sc, yw = self._embed_outputs(hostc, (n, H // TILE, W // TILE, 8), want_yw)
        call(hostc, _p(stego), _p(sc), _p(yw))
        if host.ndim == 2:
            return stego[0], sc[0], (yw[0] if want_yw else None)
        return stego, sc, yw

    def mask_gain_tiles(self, planes: np.ndarray, lo: float, hi: float) -> np.ndarray:
        """The masked rule's gain g of every tile of uint8 planes [H,W] / [N,H,W] -> float32 [N?, nby, nbx], from the
        device's own singular values (what a masked embed of these planes uses)."""
        lo, hi, _ = _mask_args((lo, hi, 1.0))
        n, H, W, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        nby, nbx = H // TILE, W // TILE
        g = np.empty((n, nby, nbx), np.float32)
        self._call("wm_mask_sigma_w_tiles_u8", _p(planes), None, None, _p(g), n, H, W, rs, ps, 0, lo, hi)
        return g[0] if planes.ndim == 2 else g

    # ---- blind payload: raw-bit level (include/wmhip.h; the framing and the keyed map are payload.py's) ----------------
    def _payload_call(self, name: str, ins, rest, dz, delta: float):
        """The payload entry point ``name(*ins, *rest, delta)`` with dz None; with dz = (table, plane stride) its ``_dither``
        twin, which takes the table after ``ins`` (the planes and, in an embed, the tile bits) and the stride in front of
        delta (include/wmhip.h).  ``ins`` and the table are host arrays or device addresses, as the entry point wants them."""
        def ptr(x):
            return _p(x) if isinstance(x, np.ndarray) else _vp(x)
        if dz is None:
            self._call(name, *map(ptr, ins), *rest, delta)
        else:
            self._call(name.replace("_u8", "_dither_u8"), *map(ptr, ins), ptr(dz[0]), *rest, dz[1], delta)

    def payload_sigma_w(self, planes: np.ndarray, tile_bit: np.ndarray, delta: float, dither=None) -> np.ndarray:
        """The rule's sigma_w rows (target - s_1, 0, .., 0) of uint8 planes [H,W] / [N,H,W] whose tile t carries
        tile_bit[t] -> float32 [N?, nby, nbx, 8].  ``dither`` (here and below): the keyed dither words, uint16 [n_tiles]
        shared by the planes or [N, n_tiles] with a row per plane; None is the dither-free rule."""
        delta = check_delta(delta)
        n, H, W, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        nby, nbx = H // TILE, W // TILE
        tb = _tile_bits(tile_bit, nby * nbx)
        dz = _dither_words(dither, n, nby * nbx)
        eff = np.empty((n, nby, nbx, 8), np.float32)
        self._payload_call("wm_payload_sigma_w_tiles_u8", (planes, tb), (_p(eff), n, H, W, rs, ps), dz, delta)
        return eff[0] if planes.ndim == 2 else eff

    def embed_tiles_payload(self, planes: np.ndarray, tile_bit: np.ndarray, delta: float, want_yw: bool = False, dither=None):
        """One bit per tile into the parity of sigma_1 on the lattice of step delta; every plane carries the same bits.
        Returns (stego uint8, the cover's sigma_c float32 [N?, nby, nbx, 8], yw or None) like embed_tiles."""
        delta = check_delta(delta)
        n, H, W, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        nby, nbx = H // TILE, W // TILE
        tb = _tile_bits(tile_bit, nby * nbx)
        dz = _dither_words(dither, n, nby * nbx)
        return self._embed_tiles_with(planes, want_yw, lambda hostc, *outs: self._payload_call(
            "wm_embed_tiles_payload_u8", (hostc, tb), (*outs, n, H, W, W, H * W), dz, delta))

    def payload_metric(self, planes: np.ndarray, delta: float, dither=None) -> np.ndarray:
        """The decoder's soft value m of every tile -> float32 [N?, nby, nbx]."""
        delta = check_delta(delta)
        n, H, W, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        dz = _dither_words(dither, n, (H // TILE) * (W // TILE))
        m = np.empty((n, H // TILE, W // TILE), np.float32)
        self._payload_call("wm_payload_metric_tiles_u8", (planes,), (_p(m), n, H, W, rs, ps), dz, delta)
        return m[0] if planes.ndim == 2 else m

    def _payload_csr_dev(self, order: np.ndarray, offs: np.ndarray):
        """Device copies of a checked (order, offs) in one buffer, cached by content."""
        def upload():
            d = self.malloc(order.nbytes + 256 + offs.nbytes)
            d_offs = d + (order.nbytes + 255) // 256 * 256
            self.h2d(d, order); self.h2d(d_offs, offs)
            return {"d": d, "d_offs": d_offs}
        ent = self._cached("payload", (order.size, offs.size, _digest(order), _digest(offs)), upload)
        return ent["d"], ent["d_offs"]

    def _cached_array(self, kind: str, arr: np.ndarray) -> int:
        """Device copy of one array, cached by shape and content under ``kind``: "dither", a dither table shared by the
        planes, always passed flat ([n_tiles]: a video decodes batch after batch of one frame size under few tables);
        "payload_tbi", a tile-to-bit map [nby, nbx] (one image size under one key decodes crop after crop); "frame_tables", the
        tables of a frame search, flat (payload_match_frames: batch after batch of one file under the same tables)."""
        def upload():
            d = self.malloc(max(arr.nbytes, arr.itemsize))
            self.h2d(d, arr)
            return {"d": d}
        return self._cached(kind, (arr.shape, _digest(arr)), upload)["d"]

    def payload_soft(self, planes: np.ndarray, order: np.ndarray, offs: np.ndarray, n_bits: int, delta: float,
                     dither=None) -> np.ndarray:
        """soft[j] = sum over the planes and over the tiles order[offs[j] : offs[j + 1]] of the decoder's m -> float64
        [n_bits]; bit j decodes to soft[j] < 0.  The planes stay on the device; only n_bits doubles come back."""
        delta = check_delta(delta)
        n, H, W, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        order, offs = check_payload_csr(order, offs, n_bits, (H // TILE) * (W // TILE))
        dz = _dither_words(dither, n, (H // TILE) * (W // TILE))
        soft = np.zeros(int(n_bits), np.float64)
        if n == 0:
            return soft
        d_order, d_offs = self._payload_csr_dev(order, offs)
        with self._staging() as dev:
            d_soft = dev.alloc(soft.nbytes)
            d_p, = dev.up(np.ascontiguousarray(planes.reshape(n, H, W)))
            if dz is not None:             # a shared table is cached; a per-plane one lives for this call only
                dz = (self._cached_array("dither", dz[0]) if dz[1] == 0 else dev.up(dz[0])[0], dz[1])
            self._payload_call("wm_payload_soft_tiles_u8_dev", (d_p,),
                               (_vp(d_order), _vp(d_offs), int(n_bits), _vp(d_soft), n, H, W, W, H * W), dz, delta)
            self.d2h(soft, d_soft)
            self.check_status()
        return soft

    # ---- channel code of the blind payload (include/wmhip.h; the encoder and the quantiser are payload.py's) ------------
    def payload_decode(self, L: np.ndarray, decisions: bool = False):
        """The Viterbi decode of quantised soft values L, int32 [n_coded] or [n, n_coded] with n_coded = 2 (n_info + 6) ->
        (info_bits uint8 [n?, n_info], final_metric int32 [n?]), with ``decisions=True`` also the decision words uint64
        [n?, n_info + 6].  A strided [n, n_coded] view with contiguous rows is read in place."""
        L = np.asarray(L)
        if L.dtype != np.int32 or L.ndim not in (1, 2):
            raise ValueError("L must be int32 [n_coded] or [n, n_coded]")
        rows = L[None] if L.ndim == 1 else L
        n, n_coded = rows.shape
        n_info = n_coded // 2 - P.K7_TAIL
        if n < 1 or n_coded % 2 or n_info < 1 or n_coded > 2 * P.K7_MAX_STEPS:
            raise ValueError(f"L holds {n} codewords of {n_coded} values: 2 (n_info + 6) each, n_info in 1..{P.K7_MAX_STEPS - P.K7_TAIL}")
        if rows.strides[1] != 4 or (n > 1 and (rows.strides[0] % 4 or rows.strides[0] < 4 * n_coded)):
            rows = np.ascontiguousarray(rows)
        stride = rows.strides[0] // 4 if n > 1 else n_coded
        info = np.zeros((n, n_info), np.uint8)
        metric = np.zeros(n, np.int32)
        words = np.zeros((n, n_info + P.K7_TAIL), np.uint64) if decisions else None
        self._call("wm_payload_decode_k7", _p(rows), n_info, n, stride, _p(info), _p(metric), _p(words))
        out = (info, metric) if L.ndim == 2 else (info[0], metric[0])
        return out if not decisions else out + ((words if L.ndim == 2 else words[0]),)

    # ---- crop resynchronisation of the blind payload (include/wmhip.h; the comparisons and tie rules are payload.py's) ----
    def payload_phase_scan(self, planes: np.ndarray, delta: float):
        """The votes of every 8x8 window of all 64 grid phases of uint8 planes [h, w] / [N, h, w] (strided views included)
        -> (votes, sums int64 [N?, 8, 8], counts int64 [8, 8]).  votes[py][px] is the int32 [N?, ny_p, nx_p] grid of phase
        (py, px), ny_p = (h - py) // 8, nx_p = (w - px) // 8; sums[.., py, px] = sum of |vote| over it, counts its size."""
        delta = check_delta(delta)
        n, h, w, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        pitch = (h // TILE) * (w // TILE)
        raw = np.zeros((n, 64, pitch), np.int32)
        sums = np.zeros((n, 8, 8), np.int64)
        self._call("wm_payload_phase_scan_u8", _p(planes), _p(raw), _p(sums), n, h, w, rs, ps, delta)
        one = planes.ndim == 2
        return self._phase_grids(raw, h, w, one), (sums[0] if one else sums), P.phase_counts(h, w)

    @staticmethod
    def _offset_args(votes, tile_bit_index, n_bits):
        v = np.ascontiguousarray(votes, np.int32)
        t = np.ascontiguousarray(tile_bit_index, np.int32)
        if v.ndim != 2 or t.ndim != 2:
            raise ValueError("votes must be [ny, nx] and tile_bit_index [nby, nbx]")
        n_bits = int(n_bits)
        if n_bits < 1 or n_bits > P.SYNC_MAX_BITS:
            raise ValueError(f"n_bits must be in 1..{P.SYNC_MAX_BITS}, got {n_bits}")
        return v, t, n_bits

    def payload_offset_scores(self, votes: np.ndarray, tile_bit_index: np.ndarray, n_bits: int) -> np.ndarray:
        """score[ty, tx] = sum over the bits of |sum of votes[r, c] with tile_bit_index[ty + r, tx + c] == j| for every
        placement of the [ny, nx] votes inside the [nby, nbx] map -> int64 [nby - ny + 1, nbx - nx + 1] (empty where the
        votes do not fit).  Map entries outside 0 .. n_bits - 1 are skipped."""
        v, t, n_bits = self._offset_args(votes, tile_bit_index, n_bits)
        (ny, nx), (nby, nbx) = v.shape, t.shape
        scores = np.zeros((max(nby - ny + 1, 0), max(nbx - nx + 1, 0)), np.int64)
        if scores.size:
            self._call("wm_payload_offset_scores", _p(v), _p(t), _p(scores), ny, nx, nby, nbx, n_bits)
        return scores

    def payload_locate(self, plane: np.ndarray, tile_bit_index: np.ndarray, n_bits: int, delta: float):
        """The chain of the rule's steps 1-3 on one uint8 plane [h, w]: phase scan, pick_phase, offset scan on the winner's
        votes, pick_offset.  The votes stay on the device; the 64 sums, the scores and the winner's votes come back.
        -> ((py, px), (ty, tx), votes int32 [ny, nx]); (ty, tx) is None where the winner's grid does not fit the map, and
        the whole result is None for a plane without a whole tile."""
        delta = check_delta(delta)
        if plane.ndim != 2:
            raise ValueError("plane must be [h, w]")
        n, h, w, rs, ps = _planes_of(plane, np.uint8, "plane must be uint8")
        _, t, n_bits = self._offset_args(np.zeros((0, 0), np.int32), tile_bit_index, n_bits)
        nby, nbx = t.shape
        pitch = (h // TILE) * (w // TILE)
        if pitch == 0:
            return None
        sums = np.zeros((8, 8), np.int64)
        d_t = self._cached_array("payload_tbi", t) if t.size else 0
        with self._staging() as dev:
            d_votes, d_sums = dev.alloc(64 * pitch * 4), dev.alloc(sums.nbytes)
            d_p, = dev.up(np.ascontiguousarray(plane))
            self._call("wm_payload_phase_scan_u8_dev", _vp(d_p), _vp(d_votes), _vp(d_sums), 1, h, w, w, h * w, delta)
            self.d2h(sums, d_sums)
            self.check_status()
            py, px = P.pick_phase(sums, P.phase_counts(h, w))
            ny, nx = (h - py) // TILE, (w - px) // TILE
            d_win = d_votes + (8 * py + px) * pitch * 4
            votes = np.empty((ny, nx), np.int32)
            self.d2h(votes, d_win)
            if ny > nby or nx > nbx:
                self.sync()
                return (py, px), None, votes
            scores = np.zeros((nby - ny + 1, nbx - nx + 1), np.int64)
            d_scores = dev.alloc(scores.nbytes)
            self._call("wm_payload_offset_scores_dev", _vp(d_win), _vp(d_t), _vp(d_scores), ny, nx, nby, nbx, n_bits)
            self.d2h(scores, d_scores)
            self.sync()
        return (py, px), P.pick_offset(scores), votes

    # ---- keyed crop resynchronisation: a dithered payload's crop (include/wmhip.h; the winner's rule is payload.pick_keyed) ----
    @staticmethod
    def _phase_grids(raw: np.ndarray, h: int, w: int, one: bool) -> list:
        """grids[py][px] = the [N?, ny_p, nx_p] grid of phase (py, px) out of a [N, 64, pitch] scan"""
        grids = []
        for py in range(8):
            ny = max(h - py, 0) // TILE
            row = []
            for px in range(8):
                nx = max(w - px, 0) // TILE
                v = raw[:, 8 * py + px, :ny * nx].reshape(raw.shape[0], ny, nx).copy()
                row.append(v[0] if one else v)
            grids.append(row)
        return grids

    def payload_sigma1_scan(self, planes: np.ndarray):
        """sigma_1 of every 8x8 window of all 64 grid phases of uint8 planes [h, w] / [N, h, w] (strided views included) ->
        s1[py][px], the float32 [N?, ny_p, nx_p] grid of phase (py, px), shaped as payload_phase_scan's votes."""
        n, h, w, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        raw = np.zeros((n, 64, (h // TILE) * (w // TILE)), np.float32)
        self._call("wm_payload_sigma1_scan_u8", _p(planes), _p(raw), n, h, w, rs, ps)
        return self._phase_grids(raw, h, w, planes.ndim == 2)

    @staticmethod
    def _keyed_args(table, h, w, delta):
        u = np.ascontiguousarray(table, np.uint16)
        h, w = int(h), int(w)
        if u.ndim != 2:
            raise ValueError("the dither table must be [nby, nbx]")
        nby, nbx = u.shape
        if h < TILE or w < TILE:
            raise ValueError(f"a keyed search needs a whole tile, got {h} x {w}")
        if h // TILE > nby or w // TILE > nbx:
            raise ValueError(f"a {h} x {w} plane has more tiles than the {nby} x {nbx} table: not a crop of that grid")
        return u, h, w, nby, nbx, check_delta(delta)

    @staticmethod
    def _packed_scans(scans, h: int, w: int, name: str) -> np.ndarray:
        """float32 [len(scans), 64, pitch] as the keyed entry points read sigma_1 scans: scans[a][py][px] is the [ny_p, nx_p]
        grid of phase (py, px) of an [h, w] plane (payload_sigma1_scan), checked against that shape; ``name`` is what a
        refusal calls scan a ("{}" stands for a)."""
        raw = np.zeros((len(scans), 64, (h // TILE) * (w // TILE)), np.float32)
        for a, scan in enumerate(scans):
            for p in range(64):
                g = np.asarray(scan[p // 8][p % 8], np.float32)
                want = (max(h - p // 8, 0) // TILE, max(w - p % 8, 0) // TILE)
                if g.shape != want:
                    raise ValueError(f"phase {divmod(p, 8)} of {name.format(a)} is {g.shape}, an {h} x {w} plane has {want}")
                raw[a, p, :g.size] = g.reshape(-1)
        return raw

    @staticmethod
    def _keyed_grids(raw: np.ndarray, h: int, w: int, nby: int, nbx: int) -> list:
        """the 64 phases' own [nby - ny_p + 1, nbx - nx_p + 1] score grids out of [64, spitch]; [0, 0] without a window"""
        out = []
        for p in range(64):
            ny, nx = max(h - p // 8, 0) // TILE, max(w - p % 8, 0) // TILE
            n_ty, n_tx = (nby - ny + 1, nbx - nx + 1) if ny * nx else (0, 0)
            out.append(raw[p, :n_ty * n_tx].reshape(n_ty, n_tx).copy())
        return out

    def payload_keyed_scores(self, s1_scan, table: np.ndarray, h: int, w: int, delta: float) -> list:
        """The keyed scores of one plane's sigma_1 scan (s1_scan[py][px] float32 [ny_p, nx_p], as payload_sigma1_scan
        returns it for an [h, w] plane) under the embed's dither table [nby, nbx] -> the list of the 64 phases' int64
        [nby - ny_p + 1, nbx - nx_p + 1] grids: score[ty, tx] = sum of |vote| of the phase's windows read on the lattices
        of the tiles (ty + r, tx + c).  A phase without a window has an empty grid."""
        u, h, w, nby, nbx, delta = self._keyed_args(table, h, w, delta)
        raw = self._packed_scans([s1_scan], h, w, "the scan")[0]
        scores = np.zeros((64, P.keyed_score_pitch(h, w, nby, nbx)), np.int64)
        self._call("wm_payload_keyed_scores", _p(raw), _p(u), _p(scores), h, w, nby, nbx, delta)
        return self._keyed_grids(scores, h, w, nby, nbx)

    def payload_locate_keyed(self, plane: np.ndarray, table: np.ndarray, delta: float):
        """The rule's steps 1-3 on one uint8 plane [h, w] of a dithered payload's crop: sigma_1 scan, keyed scores under the
        embed's dither table [nby, nbx], pick_keyed.  The scan stays on the device; the scores and the winner's sigma_1
        come back.  -> ((py, px), (ty, tx), s1 float32 [ny, nx])."""
        if plane.ndim != 2:
            raise ValueError("plane must be [h, w]")
        _planes_of(plane, np.uint8, "plane must be uint8")
        u, h, w, nby, nbx, delta = self._keyed_args(table, plane.shape[0], plane.shape[1], delta)
        pitch = (h // TILE) * (w // TILE)
        scores = np.zeros((64, P.keyed_score_pitch(h, w, nby, nbx)), np.int64)
        d_u = self._cached_array("dither", u.reshape(-1))
        with self._staging() as dev:
            d_s1, d_scores = dev.alloc(64 * pitch * 4), dev.alloc(scores.nbytes)
            d_p, = dev.up(np.ascontiguousarray(plane))
            self._call("wm_payload_sigma1_scan_u8_dev", _vp(d_p), _vp(d_s1), 1, h, w, w, h * w)
            self._call("wm_payload_keyed_scores_dev", _vp(d_s1), _vp(d_u), _vp(d_scores), h, w, nby, nbx, delta)
            self.d2h(scores, d_scores)
            self.check_status()
            (py, px), place = P.pick_keyed(self._keyed_grids(scores, h, w, nby, nbx), P.phase_counts(h, w))
            s1 = np.empty(((h - py) // TILE, (w - px) // TILE), np.float32)
            self.d2h(s1, d_s1 + (8 * py + px) * pitch * 4)
            self.sync()
        return (py, px), place, s1

    # ---- clip resynchronisation: a dithered video's clip (include/wmhip.h; the winner's rule is payload.pick_clip) ----------
    @staticmethod
    def _clip_args(tables, table_of, n_anchor, h, w, delta):
        u = np.ascontiguousarray(tables, np.uint16)
        if u.ndim != 3 or u.shape[0] < 1:
            raise ValueError("the dither tables must be [n_tables, nby, nbx] with at least one table")
        _, h, w, nby, nbx, delta = Context._keyed_args(u[0], h, w, delta)
        tof = np.ascontiguousarray(table_of, np.int32)
        if tof.ndim != 2 or tof.shape[0] < 1 or tof.shape[1] != n_anchor or n_anchor < 1:
            raise ValueError(f"table_of must be [n_cand >= 1, {n_anchor} anchors], got {tof.shape}")
        if tof.min() < -1 or tof.max() >= u.shape[0]:
            raise ValueError(f"table_of names a table outside -1 .. {u.shape[0] - 1}")
        if (h // TILE) * (w // TILE) * n_anchor >= 1 << 24:
            raise ValueError(f"{n_anchor} anchors of {(h // TILE) * (w // TILE)} tiles: their product must stay below 2^24")
        return u, tof, h, w, nby, nbx, delta

    def payload_keyed_best(self, s1_scans, tables: np.ndarray, table_of: np.ndarray, h: int, w: int, delta: float) -> np.ndarray:
        """wm_payload_keyed_best on host arrays: ``s1_scans[a]`` is anchor a's sigma_1 scan (s1[py][px] float32 [ny_p, nx_p],
        as payload_sigma1_scan returns it for an [h, w] plane), ``tables`` uint16 [n_tables, nby, nbx], ``table_of`` int32
        [n_cand, n_anchor] with -1 for an anchor the candidate skips -> best int64 [n_cand, 64, 2]: per candidate and phase
        (the largest summed score, the row-major index of its first maximum), (-1, -1) where there is none."""
        n_anchor = len(s1_scans)
        u, tof, h, w, nby, nbx, delta = self._clip_args(tables, table_of, n_anchor, h, w, delta)
        raw = self._packed_scans(s1_scans, h, w, "scan {}")
        best = np.zeros((tof.shape[0], 64, 2), np.int64)
        self._call("wm_payload_keyed_best", _p(raw), n_anchor, _p(u), u.shape[0], _p(tof), tof.shape[0], _p(best), h, w, nby, nbx, delta)
        return best

    CLIP_TABLE_BYTES = 64 << 20                      # device memory payload_locate_clip spends on the tables of one call

    def payload_locate_clip(self, planes: np.ndarray, tables: np.ndarray, table_of: np.ndarray, delta: float, *,
                            pick: bool = False, cands_per_call: Optional[int] = None):
        """The clip rule's steps 1 and 3 on the anchors, uint8 planes [n_anchor, h, w]: their sigma_1 scans stay on the
        device and only ``best`` int64 [n_cand, 64, 2] comes back (payload_keyed_best).  The candidates go in runs of
        ``cands_per_call`` (by default as many as keep a run's tables within CLIP_TABLE_BYTES), each with the tables its
        table_of rows name and no others; the result does not depend on the split.  With ``pick`` -> (best, winner), winner
        = (g, (py, px), (ty, tx)) by payload.pick_clip, None where nothing took part."""
        if planes.ndim != 3:
            raise ValueError("planes must be [n_anchor, h, w]")
        n_anchor, h, w, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        u, tof, h, w, nby, nbx, delta = self._clip_args(tables, table_of, n_anchor, h, w, delta)
        pitch = (h // TILE) * (w // TILE)
        n_cand = tof.shape[0]
        if cands_per_call is None:
            cands_per_call = max(1, self.CLIP_TABLE_BYTES // max(u[0].nbytes, 1) - n_anchor)
        step = max(1, int(cands_per_call))
        best = np.full((n_cand, 64, 2), -1, np.int64)
        with self._staging() as dev:
            d_s1 = dev.alloc(n_anchor * 64 * pitch * 4)
            d_p, = dev.up(np.ascontiguousarray(planes))
            self._call("wm_payload_sigma1_scan_u8_dev", _vp(d_p), _vp(d_s1), n_anchor, h, w, w, h * w)
            for c0 in range(0, n_cand, step):
                rows = tof[c0:c0 + step]
                ids = np.unique(rows[rows >= 0])
                if ids.size == 0:                                          # (no marked anchor in the run: every entry stays -1)
                    continue
                local = np.where(rows >= 0, np.searchsorted(ids, np.maximum(rows, 0)), -1).astype(np.int32)
                part = np.zeros((rows.shape[0], 64, 2), np.int64)
                with self._staging() as run:
                    d_best = run.alloc(part.nbytes)
                    d_u, d_of = run.up(np.ascontiguousarray(u[ids]), local)
                    self._call("wm_payload_keyed_best_dev", _vp(d_s1), n_anchor, _vp(d_u), int(ids.size), _vp(d_of), rows.shape[0],
                               _vp(d_best), h, w, nby, nbx, delta)
                    self.d2h(part, d_best)
                    self.sync()
                best[c0:c0 + step] = part
            self.check_status()
        if not pick:
            return best
        win = P.pick_clip(best, P.phase_counts(h, w), (tof >= 0).sum(axis=1))
        if win is None:
            return best, None
        g, p, i = win
        n_tx = nbx - (w - p % 8) // TILE + 1
        return best, (g, (p // 8, p % 8), (i // n_tx, i % n_tx))

    # ---- frame resynchronisation: a dithered video's frames in any order (include/wmhip.h; the assignment is payload.pick_frames) ----
    @staticmethod
    def _frame_args(tables, ny, nx, ty, tx, delta):
        u = np.ascontiguousarray(tables, np.uint16)
        if u.ndim != 3 or u.shape[0] < 1:
            raise ValueError("the dither tables must be [n_tables, nby, nbx] with at least one table")
        ny, nx, ty, tx = int(ny), int(nx), int(ty), int(tx)
        nby, nbx = u.shape[1:]
        if ny < 1 or nx < 1 or ty < 0 or tx < 0 or ty + ny > nby or tx + nx > nbx:
            raise ValueError(f"a {ny} x {nx} window grid at ({ty}, {tx}) does not lie inside the {nby} x {nbx} table")
        return u, ny, nx, ty, tx, nby, nbx, check_delta(delta)

    def payload_frame_scores(self, s1: np.ndarray, tables: np.ndarray, ny: int, nx: int, ty: int, tx: int, delta: float) -> np.ndarray:
        """wm_payload_frame_scores on host arrays: ``s1`` float32 [n_frames, ny, nx] (the frames' sigma_1 at one grid phase),
        ``tables`` uint16 [n_tables, nby, nbx] -> scores int64 [n_frames, n_tables]: frame f's windows read on the lattices
        of table k's tiles (ty + r, tx + c), |vote| added."""
        u, ny, nx, ty, tx, nby, nbx, delta = self._frame_args(tables, ny, nx, ty, tx, delta)
        s = _f32(s1)
        if s.ndim != 3 or s.shape[0] < 1 or s.shape[1:] != (ny, nx):
            raise ValueError(f"s1 must be [n_frames >= 1, {ny}, {nx}], got {s.shape}")
        scores = np.zeros((s.shape[0], u.shape[0]), np.int64)
        self._call("wm_payload_frame_scores", _p(s), 1, ny * nx, s.shape[0], _p(u), u.shape[0], _p(scores), ny, nx, nby, nbx, ty, tx, delta)
        return scores

    def payload_match_frames(self, planes_view: np.ndarray, tables: np.ndarray, ty: int, tx: int, delta: float,
                             tables_per_call: Optional[int] = None):
        """Step 2 of the frame search on uint8 views [n, 8 ny, 8 nx] of the frames at the found grid phase: the sigma pass,
        then the scores against all tables with sigma_1 resident (the sigma pass's [n][ny nx][8] output is read in place,
        window stride 8).  Tables go to the device in runs of ``tables_per_call`` (by default as many as stay within
        CLIP_TABLE_BYTES); tables that fit one run are uploaded once and stay resident from call to call (the device cache),
        longer lists go up run by run on every call; the result does not depend on the split.  -> (scores int64 [n, K], s1 float32 [n, ny, nx])."""
        if planes_view.ndim != 3 or planes_view.shape[0] < 1:
            raise ValueError("planes_view must be [n >= 1, h, w]")
        n, h, w = _planes_of(planes_view, np.uint8, "planes must be uint8")[:3]         # (the view is uploaded dense)
        if h < TILE or w < TILE or h % TILE or w % TILE:
            raise ValueError(f"the view must be whole tiles, got {h} x {w}")
        u, ny, nx, ty, tx, nby, nbx, delta = self._frame_args(tables, h // TILE, w // TILE, ty, tx, delta)
        K = u.shape[0]
        if tables_per_call is None:
            tables_per_call = max(1, self.CLIP_TABLE_BYTES // max(u[0].nbytes, 1))
        step = max(1, int(tables_per_call))
        scores = np.zeros((n, K), np.int64)
        sig = np.empty((n, ny, nx, 8), np.float32)
        # tables that fit one run stay on the device from batch to batch (a file is matched batch after batch under the same ones)
        d_all = self._cached_array("frame_tables", u.reshape(-1)) if step >= K else 0
        with self._staging() as dev:
            d_sig = dev.alloc(sig.nbytes)
            d_p, = dev.up(np.ascontiguousarray(planes_view))
            self._call("wm_sigma_tiles_u8_dev", _vp(d_p), _vp(d_sig), n, h, w, w, h * w)
            for k0 in range(0, K, step):
                part = np.zeros((n, min(step, K - k0)), np.int64)
                with self._staging() as run:
                    d_sc = run.alloc(part.nbytes)
                    d_u = d_all or run.up(np.ascontiguousarray(u[k0:k0 + step]))[0]
                    self._call("wm_payload_frame_scores_dev", _vp(d_sig), 8, ny * nx * 8, n, _vp(d_u), part.shape[1], _vp(d_sc),
                               ny, nx, nby, nbx, ty, tx, delta)
                    self.d2h(part, d_sc)
                    self.sync()
                scores[:, k0:k0 + step] = part
            self.d2h(sig, d_sig)
            self.check_status()
        return scores, np.ascontiguousarray(sig[..., 0])

    # ---- resize resynchronisation of the blind payload (include/wmhip.h; the tap tables are resample.py's) ----------------
    def resample_planes(self, planes: np.ndarray, H: int, W: int) -> np.ndarray:
        """uint8 planes [h, w] / [N, h, w] (strided views are read in place) through the rule's integer filter -> uint8
        [N?, H, W].  Host arrays in and out: for tests and tools; the extract keeps its planes on the device
        (payload_soft_resized)."""
        if planes.ndim == 3 and planes.shape[0] == 0 and planes.dtype == np.uint8:
            n, (h, w) = 0, planes.shape[1:]                                 # (an empty batch has no strides to speak of)
            rs, ps = w, h * w
        else:
            n, h, w, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        H, W = int(H), int(W)
        R.check_resize(h, w, H, W, "planes")
        (fx, wx), (fy, wy) = R.resample_taps(w, W), R.resample_taps(h, H)
        out = np.zeros((n, H, W), np.uint8)
        self._call("wm_resample_planes_u8", _p(planes), _p(out), n, h, w, rs, ps, H, W, W, H * W,
                   _p(fx), _p(wx), wx.shape[1], _p(fy), _p(wy), wy.shape[1])
        return out[0] if planes.ndim == 2 else out

    def _resample_taps_dev(self, h: int, w: int, H: int, W: int) -> tuple:
        """The device copies of the tap tables of an [h, w] -> [H, W] resize, as wm_resample_planes_u8_dev takes them behind
        its plane arguments: (first_x, w_x, T_x, first_y, w_y, T_y).  One buffer, cached by content: a video decodes batch
        after batch under one pair of tables."""
        tabs = (*R.resample_taps(w, W), *R.resample_taps(h, H))

        def upload():
            offs = np.cumsum([0] + [(t.nbytes + 255) // 256 * 256 for t in tabs])
            d = self.malloc(int(offs[-1]))
            for o, t in zip(offs, tabs):
                self.h2d(d + int(o), t)
            return {"d": d, "at": [d + int(o) for o in offs[:4]]}
        at = self._cached("resample", tuple((t.shape, _digest(t)) for t in tabs), upload)["at"]
        return _vp(at[0]), _vp(at[1]), tabs[1].shape[1], _vp(at[2]), _vp(at[3]), tabs[3].shape[1]

    def resample_planes_dev(self, src: int, dst: int, n_planes: int, h: int, w: int, src_row_stride: int, src_plane_stride: int,
                            H: int, W: int, dst_row_stride: int, dst_plane_stride: int):
        """wm_resample_planes_u8_dev on device addresses under the cached tables of the sizes; enqueued, not synchronised"""
        R.check_resize(h, w, H, W, "planes")
        self._call("wm_resample_planes_u8_dev", _vp(src), _vp(dst), n_planes, h, w, src_row_stride, src_plane_stride, H, W,
                   dst_row_stride, dst_plane_stride, *self._resample_taps_dev(h, w, H, W))

    def payload_soft_resized(self, planes: np.ndarray, H: int, W: int, order: np.ndarray, offs: np.ndarray, n_bits: int,
                             delta: float, dither=None) -> np.ndarray:
        """payload_soft of uint8 planes [h, w] / [N, h, w] that are a marked [H, W] frame resized as a whole: upload,
        the rule's resample back to [H, W] and the soft decode in one staging scope.  The restored planes never leave the
        device (rows 16-byte multiples apart, so the resampler stores whole lines); only n_bits doubles come back."""
        delta = check_delta(delta)
        n, h, w, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        H, W = int(H), int(W)
        R.check_resize(h, w, H, W, "planes")
        n_tiles = (H // TILE) * (W // TILE)
        order, offs = check_payload_csr(order, offs, n_bits, n_tiles)
        dz = _dither_words(dither, n, n_tiles)
        soft = np.zeros(int(n_bits), np.float64)
        if n == 0:
            return soft
        d_order, d_offs = self._payload_csr_dev(order, offs)
        pitch = (W + 15) // 16 * 16
        with self._staging() as dev:
            d_soft, d_out = dev.alloc(soft.nbytes), dev.alloc(n * H * pitch)
            d_p, = dev.up(np.ascontiguousarray(planes.reshape(n, h, w)))
            if dz is not None:
                dz = (self._cached_array("dither", dz[0]) if dz[1] == 0 else dev.up(dz[0])[0], dz[1])
            self.resample_planes_dev(d_p, d_out, n, h, w, w, h * w, H, W, pitch, H * pitch)
            self._payload_call("wm_payload_soft_tiles_u8_dev", (d_out,),
                               (_vp(d_order), _vp(d_offs), int(n_bits), _vp(d_soft), n, H, W, pitch, H * pitch), dz, delta)
            self.d2h(soft, d_soft)
            self.check_status()
        return soft

    # ---- rotation resynchronisation of the blind payload (include/wmhip.h; weights and candidates are resample.py's, the
    # schedule and the winner's rule payload.py's) -------------------------------------------------------------------------
    ROTATE_PLANE_BYTES = 256 << 20                   # device memory payload_locate_angle spends on one chunk's restored planes

    @staticmethod
    def _angle_cands(cands) -> np.ndarray:
        c = np.asarray(cands)
        if c.ndim != 2 or c.shape[1] != 2 or c.shape[0] < 1 or c.dtype.kind not in "iu":
            raise ValueError("candidates must be integers [n_angles >= 1, 2]: (C, S) of every angle")
        return np.ascontiguousarray(c, np.int32)

    @staticmethod
    def _rotate_sizes(h: int, w: int, H, W, tiles: bool) -> tuple:
        H, W = int(H), int(W)
        R.check_rotate(h, w, H, W, "planes")
        if tiles and (H % TILE or W % TILE):
            raise ValueError(f"the restored frame is {W}x{H}: both sides must be multiples of {TILE}")
        return H, W

    def rotate_planes(self, planes: np.ndarray, H: int, W: int, cands) -> np.ndarray:
        """uint8 planes [h, w] / [N, h, w] (strided views are read in place) rotated onto an [H, W] frame about the common
        centre under every candidate (C, S) of ``cands`` int [n_angles, 2] -> uint8 [n_angles, N?, H, W].  Host arrays in and
        out: for tests and tools; the search keeps its planes on the device (payload_locate_angle)."""
        n, h, w, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        H, W = self._rotate_sizes(h, w, H, W, False)
        c = self._angle_cands(cands)
        if n < 1:
            raise ValueError("a rotation takes at least one plane")
        out = np.zeros((c.shape[0], n, H, W), np.uint8)
        self._call("wm_rotate_planes_u8", _p(planes), _p(out), n, h, w, rs, ps, H, W, W, H * W, _p(c), c.shape[0],
                   _p(np.ascontiguousarray(R.rotate_weights())))
        return out[:, 0] if planes.ndim == 2 else out

    def payload_angle_scores(self, metric: np.ndarray, cands, h: int, w: int) -> tuple:
        """The candidates' scores over the metrics float32 [n_angles, nby, nbx] of their restored planes, which came from an
        [h, w] source -> (scores int64 [n_angles], counts int32 [n_angles], valid bool [n_angles, nby, nbx]): the sum of
        rint(|m| 2^15) over a candidate's valid tiles, their number, and which they are."""
        c = self._angle_cands(cands)
        m = np.asarray(metric)
        if m.dtype != np.float32 or m.ndim != 3 or m.shape[0] != c.shape[0]:
            raise ValueError(f"metric must be float32 [n_angles = {c.shape[0]}, nby, nbx]")
        m = np.ascontiguousarray(m)
        _, nby, nbx = m.shape
        self._rotate_sizes(int(h), int(w), TILE * nby, TILE * nbx, True)
        scores, counts = np.zeros(c.shape[0], np.int64), np.zeros(c.shape[0], np.int32)
        valid = np.zeros(m.shape, np.uint8)
        self._call("wm_payload_angle_scores", _p(m), _p(c), c.shape[0], _p(scores), _p(counts), _p(valid), int(h), int(w),
                   TILE * nby, TILE * nbx)
        return scores, counts, valid.astype(bool)

    def payload_locate_angle(self, plane: np.ndarray, H: int, W: int, max_angle: float, delta: float, dither=None):
        """The rule's search on one uint8 plane [h, w], a marked [H, W] frame rotated about its centre by at most
        ``max_angle`` degrees: the coarse and the fine stage of payload.angle_candidates, each candidate rotated back,
        read by the plain metric (``dither``: the frame's shared table, uint16 [n_tiles], or None) and scored, all resident;
        the candidates go in chunks whose restored planes stay within ROTATE_PLANE_BYTES, and the fine winner is run once more
        alone for its metrics and mask.  Only the scores, the counts and those come back.  -> (theta in radians, metric float32 [nby, nbx], valid bool [nby, nbx],
        stages), stages = [(numerators, denominator, scores, counts, winner's index)] of the two stages; None where no
        candidate has a valid tile."""
        delta = check_delta(delta)
        if plane.ndim != 2:
            raise ValueError("plane must be [h, w]")
        _, h, w, rs, ps = _planes_of(plane, np.uint8, "plane must be uint8")
        H, W = self._rotate_sizes(h, w, H, W, True)
        max_angle = P.check_max_angle(max_angle)
        nby, nbx = H // TILE, W // TILE
        n_tiles = nby * nbx
        dz = _dither_words(dither, 1, n_tiles)
        if dz is not None and dz[1] != 0:
            dz = (dz[0].reshape(-1), 0)                                    # (one plane: a [1, n_tiles] table is the shared one)
        pitch = (W + 15) // 16 * 16
        per = max(1, self.ROTATE_PLANE_BYTES // (H * pitch))
        d_K = self._cached_array("rotate_k", R.rotate_weights())
        if dz is not None:
            dz = (self._cached_array("dither", dz[0]), 0)
        stages, around = [], None
        with self._staging() as dev:
            d_p, = dev.up(np.ascontiguousarray(plane))
            for stage in range(2):
                nums, den = P.angle_candidates(H, W, max_angle, around)
                cs = R.angle_candidates_cs(nums / den)
                n = cs.shape[0]
                scores, counts = np.zeros(n, np.int64), np.zeros(n, np.int32)
                with self._staging() as run:
                    d_out, d_m, d_v = run.alloc(min(per, n) * H * pitch), run.alloc(min(per, n) * n_tiles * 4), run.alloc(n_tiles)
                    d_s, d_n = run.alloc(scores.nbytes), run.alloc(counts.nbytes)
                    d_c, = run.up(cs)

                    def chunk(a0, k, d_valid):                             # candidates a0 .. a0 + k - 1: restored, read, scored
                        self._call("wm_rotate_planes_u8_dev", _vp(d_p), _vp(d_out), 1, h, w, w, h * w, H, W, pitch, H * pitch,
                                   _vp(d_c + 8 * a0), k, _vp(d_K))
                        self._payload_call("wm_payload_metric_tiles_u8_dev", (d_out,), (_vp(d_m), k, H, W, pitch, H * pitch), dz, delta)
                        self._call("wm_payload_angle_scores_dev", _vp(d_m), _vp(d_c + 8 * a0), k, _vp(d_s + 8 * a0), _vp(d_n + 4 * a0),
                                   _vp(d_valid) if d_valid else None, h, w, H, W)
                    for a0 in range(0, n, per):
                        chunk(a0, min(per, n - a0), 0)
                    self.d2h(scores, d_s); self.d2h(counts, d_n)
                    self.check_status()
                    win = P.pick_angle(scores, counts)
                    stages.append((nums, den, scores, counts, win))
                    if win is None:
                        return None
                    if stage == 0:
                        around = int(nums[win])
                        continue
                    chunk(win, 1, d_v)                                     # the winner once more, alone: its metrics and mask
                    m, valid = np.empty((nby, nbx), np.float32), np.empty((nby, nbx), np.uint8)
                    self.d2h(m, d_m); self.d2h(valid, d_v)
                    self.sync()
        return float(nums[win] / den), m, valid.astype(bool), stages

    def sigma_tiles(self, planes: np.ndarray) -> np.ndarray:
        n, H, W, rs, ps = _planes_of(planes, np.uint8, "planes must be uint8")
        s = np.empty((n, H // TILE, W // TILE, 8), np.float32)
        self._call("wm_sigma_tiles_u8", _p(planes), _p(s), n, H, W, rs, ps)
        return s[0] if planes.ndim == 2 else s

    def svd_tiles(self, planes: np.ndarray):
        """float32 planes -> (U [..,nby,nbx,8,8], S [..,nby,nbx,8], Vt [..,nby,nbx,8,8])."""
        n, H, W, rs, ps = _planes_of(planes, np.float32, "planes must be float32")
        nby, nbx = H // TILE, W // TILE
        U = np.empty((n, nby, nbx, 8, 8), np.float32)
        S = np.empty((n, nby, nbx, 8), np.float32)
        Vt = np.empty((n, nby, nbx, 8, 8), np.float32)
        self._call("wm_svd_tiles_f32", _p(planes), _p(U), _p(S), _p(Vt), n, H, W, rs, ps)
        if planes.ndim == 2:
            return U[0], S[0], Vt[0]
        return U, S, Vt

    @staticmethod
    def _sigma_c_tiles(sigma_c, n: int, nby: int, nbx: int) -> np.ndarray:
        sc = _f32(sigma_c)
        if sc.size != n * nby * nbx * 8:
            raise ValueError(f"sigma_c has {sc.size} values, the planes need {n}x{nby}x{nbx}x8")
        return sc.reshape(n, nby, nbx, 8)

    @classmethod
    def _tile_factors(cls, sigma_c, Uw, Vwt, n: int, nby: int, nbx: int):
        """(sigma_c, Uw, Vwt, uv_plane_stride) of a tile-mode meta, dense float32, checked against n planes of nby x nbx
        tiles: the factors [nby, nbx, 8, 8] shared by the planes (stride 0) or [n, nby, nbx, 8, 8]."""
        sc = cls._sigma_c_tiles(sigma_c, n, nby, nbx)
        Uw = _f32(Uw); Vwt = _f32(Vwt)
        per_plane = Uw.ndim == 5
        if Uw.ndim not in (4, 5) or Uw.shape[-4:] != (nby, nbx, 8, 8) or Vwt.shape != Uw.shape \
                or (per_plane and Uw.shape[0] != n):
            raise ValueError(f"Uw/Vwt shape {Uw.shape}/{Vwt.shape} does not match {n} plane(s) of {nby}x{nbx} tiles")
        return sc, Uw, Vwt, nby * nbx if per_plane else 0

    def extract_tiles(self, stego: np.ndarray, sigma_c: np.ndarray, Uw: np.ndarray, Vwt: np.ndarray,
                      alpha: float, K: int = 8, sum_planes: bool = False, mask=None) -> np.ndarray:
        """Scrambled-watermark estimate per plane, float32 [n, H, W]; with ``sum_planes`` the planes
        are added on the device and only their sum [H, W] comes back (video extract averages frames).
        ``mask=(lo, hi, cut)``: the masked rule's extract (include/wmhip.h), g taken from sigma_c."""
        m = _mask_args(mask)
        n, H, W, rs, ps = _planes_of(stego, np.uint8, "stego planes must be uint8")
        sc, Uw, Vwt, uv_stride = self._tile_factors(sigma_c, Uw, Vwt, n, H // TILE, W // TILE)
        out = np.empty((H, W) if sum_planes else (n, H, W), np.float32)
        name = ("wm_extract_tiles_sum" if sum_planes else "wm_extract_tiles") + ("_masked_u8" if m else "_u8")
        self._call(name, _p(stego), _p(sc), _p(Uw), _p(Vwt), _p(out), n, H, W, rs, ps, uv_stride, float(alpha), int(K), *m)
        return out[0] if stego.ndim == 2 and not sum_planes else out

    def reconstruct_tiles(self, Uw: np.ndarray, sw_hat: np.ndarray, Vwt: np.ndarray, H: int, W: int):
        Uw = _f32(Uw); Vwt = _f32(Vwt); sh = _f32(sw_hat)
        single = Uw.ndim == 4
        n = 1 if single else Uw.shape[0]
        nby, nbx = H // TILE, W // TILE
        if Uw.shape[-4:] != (nby, nbx, 8, 8) or Vwt.shape != Uw.shape or sh.size != n * nby * nbx * 8:
            raise ValueError("Uw / Vwt / sw_hat do not match the plane size")
        out = np.empty((n, H, W), np.float32)
        self._call("wm_reconstruct_tiles", _p(Uw), _p(sh), _p(Vwt), _p(out), n, H, W)
        return out[0] if single else out

    def detect_tiles(self, stego: np.ndarray, sigma_c: np.ndarray, sigma_w: np.ndarray,
                     alpha: float, mask=None) -> np.ndarray:
        """NC score per plane, float64 [n].  ``mask=(lo, hi, cut)``: over the values the masked rule takes."""
        m = _mask_args(mask)
        n, H, W, rs, ps = _planes_of(stego, np.uint8, "stego planes must be uint8")
        nby, nbx = H // TILE, W // TILE
        sc = self._sigma_c_tiles(sigma_c, n, nby, nbx)
        sw = _f32(sigma_w)
        per_plane = sw.ndim == 4
        if sw.ndim not in (3, 4) or sw.shape[-3:] != (nby, nbx, 8) or (per_plane and sw.shape[0] != n):
            raise ValueError(f"sigma_w shape {sw.shape} does not match {n} plane(s) of {nby}x{nbx} tiles")
        scores = np.zeros(n, np.float64)
        self._call("wm_detect_tiles_masked_u8" if m else "wm_detect_tiles_u8", _p(stego), _p(sc), _p(sw), _p(scores),
                   n, H, W, rs, ps, nby * nbx * 8 if per_plane else 0, float(alpha), *m)
        return scores

    # ---- full-frame mode (tile=None): one plane per call, or [N, H, W] planes sharing every launch ------------------
    # A one-plane method and its ``_planes`` twin prepare their arguments alike (_dense, then the plane's H, W, L) and
    # differ in the entry point they call and in the leading axis of what they return.
    def _embed_outputs(self, hosts: np.ndarray, sc_shape, want_yw: bool):
        return np.empty_like(hosts), np.empty(sc_shape, np.float32), np.empty(hosts.shape, np.float32) if want_yw else None

    def ref_embed(self, host: np.ndarray, sigma_w: np.ndarray, alpha: float, K: int, want_yw: bool = False):
        host, H, W, L = _dense(host, np.uint8, 2, "host plane must be uint8 [H, W]")
        sw = _f32(sigma_w)
        if sw.shape != (L,):
            raise ValueError(f"sigma_w must have shape ({L},)")
        stego, sc, yw = self._embed_outputs(host, L, want_yw)
        self._call("wm_ref_embed_u8", _p(host), _p(sw), _p(stego), _p(sc), _p(yw), H, W, W, float(alpha), int(K))
        return stego, sc, yw

    def ref_embed_planes(self, hosts: np.ndarray, sigma_w: np.ndarray, alpha: float, K: int, want_yw: bool = False):
        """hosts uint8 [N, H, W]; sigma_w [L] (shared) or [N, L].  All planes share every launch."""
        hosts, H, W, L = _dense(hosts, np.uint8, 3, "hosts must be uint8 [N, H, W]")
        n = hosts.shape[0]
        sw = _f32(sigma_w)
        if sw.shape not in ((L,), (n, L)):
            raise ValueError(f"sigma_w must have shape ({L},) or ({n}, {L})")
        stego, sc, yw = self._embed_outputs(hosts, (n, L), want_yw)
        self._call("wm_ref_embed_planes_u8", _p(hosts), _p(sw), _p(stego), _p(sc), _p(yw), n, H, W, W, H * W,
                   L if sw.ndim == 2 else 0, float(alpha), int(K))
        return stego, sc, yw

    def ref_embed_planes_when(self, hosts: np.ndarray, produce_sigma_w, per_plane: bool, alpha: float, K: int,
                              want_yw: bool = False):
        """``ref_embed_planes`` for a sigma_w that is still being computed: ``produce_sigma_w()`` -> (sigma_w [L] or [N, L],
        anything) runs on a worker thread - the watermark's own decomposition, on ANOTHER Context - while this context
        decomposes the host planes (single:172-173 are independent statements; one full-frame SVD leaves most of the chip
        idle).  Returns (stego, sigma_c, yw, the callable's second value); the callable's exception is re-raised here."""
        import threading
        hosts, H, W, L = _dense(hosts, np.uint8, 3, "hosts must be uint8 [N, H, W]")
        n = hosts.shape[0]
        sw = np.zeros((n, L) if per_plane else (L,), np.float32)
        flag = _i(0)
        box = {}

        def run():
            try:
                s, extra = produce_sigma_w()
                s = np.asarray(s, dtype=np.float32)
                if s.shape != sw.shape:
                    raise ValueError(f"sigma_w must have shape {sw.shape}")
                sw[...] = s
                box["extra"] = extra
                flag.value = 1                                   # read with acquire order by the library
            except BaseException as e:                           # the embed call returns WM_ERR_BADARG; re-raised below
                box["exc"] = e
                flag.value = -1
        t = threading.Thread(target=run, daemon=True)
        t.start()
        stego, sc, yw = self._embed_outputs(hosts, (n, L), want_yw)
        try:
            self._call("wm_ref_embed_planes_u8_when", _p(hosts), _p(sw), C.byref(flag), _p(stego), _p(sc), _p(yw),
                       n, H, W, W, H * W, L if per_plane else 0, float(alpha), int(K))
        except Exception:
            t.join()
            if "exc" in box:
                raise box["exc"]
            raise
        t.join()
        return stego, sc, yw, box["extra"]

    def ref_last_sweeps(self) -> int:
        n = _i(0)
        self._call("wm_ref_last_sweeps", C.byref(n))
        return n.value

    def ref_last_flops(self):
        """(matrix-core flops the last full-frame SVD's Gram / rotation products issued, ran the two-level scheme?)"""
        f = C.c_double(0.0); h = _i(0)
        self._call("wm_ref_last_flops", C.byref(f), C.byref(h))
        return f.value, bool(h.value)

    def ref_sigma_planes(self, planes: np.ndarray) -> np.ndarray:
        planes, H, W, L = _dense(planes, np.uint8, 3, "planes must be uint8 [N, H, W]")
        n = planes.shape[0]
        s = np.empty((n, L), np.float32)
        self._call("wm_ref_sigma_planes_u8", _p(planes), _p(s), n, H, W, W, H * W)
        return s

    def ref_sigma(self, plane: np.ndarray) -> np.ndarray:
        plane, H, W, L = _dense(plane, np.uint8, 2, "plane must be uint8 [H, W]")
        s = np.empty(L, np.float32)
        self._call("wm_ref_sigma_u8", _p(plane), _p(s), H, W, W)
        return s

    def ref_svd(self, plane: np.ndarray, apply_dct: bool = True):
        plane, H, W, L = _dense(plane, np.float32, 2, "plane must be float32 [H, W]")
        U = np.empty((H, L), np.float32); S = np.empty(L, np.float32); Vt = np.empty((L, W), np.float32)
        self._call("wm_ref_svd_f32", _p(plane), _p(U), _p(S), _p(Vt), H, W, W, 1 if apply_dct else 0)
        return U, S, Vt

    def ref_svd_planes(self, planes: np.ndarray, apply_dct: bool = True):
        """planes float32 [n, H, W] -> U [n, H, L], S [n, L], Vt [n, L, W]: the watermark-side SVDs of a colour watermark's
        three planes (single:128-134) as one batch."""
        planes, H, W, L = _dense(planes, np.float32, 3, "planes must be float32 [n, H, W]")
        n = planes.shape[0]
        U = np.empty((n, H, L), np.float32); S = np.empty((n, L), np.float32); Vt = np.empty((n, L, W), np.float32)
        self._call("wm_ref_svd_planes_f32", _p(planes), _p(U), _p(S), _p(Vt), n, H, W, W, H * W, 1 if apply_dct else 0)
        return U, S, Vt

    @staticmethod
    def _ref_factors(sigma_c, Uw, Vwt, sc_shape, H: int, W: int):
        """sigma_c of the given shape and the factors of one H x W plane, dense float32"""
        sc = _f32(sigma_c); Uw = _f32(Uw); Vwt = _f32(Vwt)
        L = min(H, W)
        if sc.shape != sc_shape or Uw.shape != (H, L) or Vwt.shape != (L, W):
            raise ValueError("meta arrays do not match the plane size")
        return sc, Uw, Vwt

    def ref_extract(self, stego: np.ndarray, sigma_c, Uw, Vwt, alpha: float, K: int) -> np.ndarray:
        stego, H, W, L = _dense(stego, np.uint8, 2, "stego plane must be uint8 [H, W]")
        sc, Uw, Vwt = self._ref_factors(sigma_c, Uw, Vwt, (L,), H, W)
        out = np.empty((H, W), np.float32)
        self._call("wm_ref_extract_u8", _p(stego), _p(sc), _p(Uw), _p(Vwt), _p(out), H, W, W, float(alpha), int(K))
        return out

    def ref_reconstruct(self, Uw, sw_hat, Vwt, H: int, W: int) -> np.ndarray:
        """single:214-218 with the estimates given: ``Uw[:L,:L] @ diag(sw_hat) @ Vwt[:L,:L]`` (L = len(sw_hat)) in the
        top-left corner of a zero H x W plane, then idct2.  Uw [H, min(H,W)], Vwt [min(H,W), W] as the meta holds them."""
        Lm = min(H, W)
        Uw = _f32(Uw); Vwt = _f32(Vwt)
        sh = _f32(sw_hat).reshape(-1)
        if Uw.shape != (H, Lm) or Vwt.shape != (Lm, W):
            raise ValueError(f"Uw {Uw.shape} / Vwt {Vwt.shape} are not the factors of a {H}x{W} plane")
        if sh.size > Lm:
            raise ValueError(f"{sh.size} estimates for a plane with {Lm} singular values")
        out = np.empty((H, W), np.float32)
        self._call("wm_ref_reconstruct_f32", _p(Uw), _p(sh) if sh.size else _p(out), _p(Vwt), _p(out), H, W, int(sh.size))
        return out

    def ref_extract_planes(self, stegos: np.ndarray, sigma_c, Uw, Vwt, alpha: float, K: int) -> np.ndarray:
        """stegos uint8 [n, H, W] sharing one watermark decomposition; sigma_c [n, L]."""
        stegos, H, W, L = _dense(stegos, np.uint8, 3, "stego planes must be uint8 [n, H, W]")
        n = stegos.shape[0]
        sc, Uw, Vwt = self._ref_factors(sigma_c, Uw, Vwt, (n, L), H, W)
        out = np.empty((n, H, W), np.float32)
        self._call("wm_ref_extract_planes_u8", _p(stegos), _p(sc), _p(Uw), _p(Vwt), _p(out), n, H, W, W, H * W,
                   float(alpha), int(K))
        return out

    def ref_detect(self, stego: np.ndarray, sigma_c, sigma_w, alpha: float) -> float:
        stego, H, W, L = _dense(stego, np.uint8, 2, "stego plane must be uint8 [H, W]")
        sc = _f32(sigma_c); sw = _f32(sigma_w)
        # the C side reads min(H, W) floats from each buffer; the reference would truncate to the
        # shortest of Sc / S_cw / Sw (single:299,311-313) - a meta that does not belong to this
        # stego is refused here instead of being read past its end
        if sc.shape != (L,) or sw.shape != (L,):
            raise ValueError(f"sigma_c {sc.shape} / sigma_w {sw.shape} do not match the plane's {L} singular values")
        score = C.c_double(0.0)
        self._call("wm_ref_detect_u8", _p(stego), _p(sc), _p(sw), C.byref(score), H, W, W, float(alpha))
        return score.value

    def ref_detect_planes(self, stegos: np.ndarray, sigma_c, sigma_w, alpha: float) -> np.ndarray:
        """stegos uint8 [n, H, W] carrying one watermark; sigma_c [n, L], sigma_w [L] -> scores float64 [n]."""
        stegos, H, W, L = _dense(stegos, np.uint8, 3, "stego planes must be uint8 [n, H, W]")
        n = stegos.shape[0]
        sc = _f32(sigma_c); sw = _f32(sigma_w)
        if sc.shape != (n, L) or sw.shape != (L,):
            raise ValueError("meta arrays do not match the plane size")
        scores = np.empty(n, np.float64)
        self._call("wm_ref_detect_planes_u8", _p(stegos), _p(sc), _p(sw), _p(scores), n, H, W, W, H * W, float(alpha))
        return scores

    # ---- keyed scramble / unscramble on the device (single:66-80) ------------------
    # The permutation is NumPy's own PCG64 shuffle (hostglue.permutation_index, bit-exact by construction);
    # its int32 copy is uploaded once per index array and kept (two entries, like the host-side cache).
    ROUTE_MAX_N = 2048 << 15        # wm_route: at most 2048 blocks of 32768 elements (67 M pixels, an 8K x 8K plane)

    def _index_entry(self, idx: np.ndarray) -> dict:
        """Device copy (int32) of a permutation index.  Cached on the index's identity: hostglue.permutation_index
        tags its result with (H, W, sha256(key)); any other array is keyed by a digest of its contents - never by its
        address, which NumPy reuses for the next index of the same size."""
        tag = getattr(idx, "tag", None)
        trusted = tag is not None                  # hostglue's own shuffle of arange: a bijection by construction
        if tag is None:
            tag = ("digest", idx.size, _digest(idx))

        def upload():
            if idx.size > 0x7fffffff:
                raise ValueError("plane too large for an int32 index")
            if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= idx.size):
                raise ValueError("index entries must lie in [0, n)")  # the device passes gather / scatter through it unchecked
            if not trusted and idx.size:
                seen = np.zeros(idx.size, np.bool_)
                seen[np.asarray(idx)] = True
                if not seen.all():
                    raise ValueError("index is not a permutation (repeated entries): the inverse scatter would leave holes")
            i32 = np.ascontiguousarray(idx, dtype=np.int32)
            d = self.malloc(max(i32.nbytes, 4))
            self.h2d(d, i32)
            return {"d": d, "n": int(idx.size), "route": None}
        return self._cached("index", tag, upload)

    def index_dev(self, idx: np.ndarray) -> int:
        return self._index_entry(idx)["d"]

    def route_dev(self, idx: np.ndarray):
        """The wm_route of this permutation (built once per key, kept with the device index), or None when the
        plane is empty or has more elements than a route addresses."""
        ent = self._index_entry(idx)
        if ent["route"] is None and 0 < ent["n"] <= self.ROUTE_MAX_N:
            r = _vp()
            self._call("wm_route_create_dev", _vp(ent["d"]), ent["n"], C.byref(r))
            ent["route"] = r.value
        return ent["route"]

    def permute_planes(self, planes: np.ndarray, idx: np.ndarray) -> np.ndarray:
        """``flat[idx]`` of every plane (uint8 or float32 [H, W] / [n, H, W]) -> float32, like hostglue.permute."""
        single = planes.ndim == 2
        p = np.ascontiguousarray(planes[None] if single else planes)
        n_pl, H, W = p.shape
        n = H * W
        if idx.size != n:
            raise ValueError("index length does not match the plane")
        d_idx = self.index_dev(idx)
        with self._staging() as dev:
            d_dst = dev.alloc(n_pl * n * 4)
            d_src, = dev.up(p)
            route = self.route_dev(idx) if p.dtype == np.uint8 else None
            if route is not None:          # the coalesced two-pass form (csrc/wm_route.hip), same values
                self._call("wm_permute_u8_f32_routed_dev", _vp(d_src), _vp(route), _vp(d_dst), n, n_pl)
            elif p.dtype == np.uint8:
                self._call("wm_permute_u8_f32_dev", _vp(d_src), _vp(d_idx), _vp(d_dst), n, n_pl)
            elif p.dtype == np.float32:
                self._call("wm_permute_f32_dev", _vp(d_src), _vp(d_idx), _vp(d_dst), n, n_pl)
            else:
                raise ValueError("planes must be uint8 or float32")
            out = np.empty((n_pl, H, W), np.float32)
            self.d2h(out, d_dst)
        return out[0] if single else out

    def unpermute_normalize_u8(self, planes: np.ndarray, idx: np.ndarray, normalize: bool = True) -> np.ndarray:
        """hostglue.unpermute + the reference's min-max normalise / clip / uint8 (single:220-222) per plane, on the
        device: float32 [H, W] / [n, H, W] in, uint8 out."""
        single = planes.ndim == 2
        p = np.ascontiguousarray(planes[None] if single else planes, dtype=np.float32)
        n_pl, H, W = p.shape
        with self._staging() as dev:
            out = self._unpermute_normalize_dev(dev.up(p)[0], n_pl, H, W, idx, normalize)
        return out[0] if single else out

    def _unpermute_normalize_dev(self, d_src: int, n_pl: int, H: int, W: int, idx: np.ndarray, normalize: bool) -> np.ndarray:
        """d_src: float32 [n_pl][H*W] on the device -> uint8 [n_pl, H, W] on the host (single:74-80, 221-222; every plane
        is normalised on its own, single:269-274).  Routed (coalesced two-pass) form whenever the plane fits a route."""
        n = H * W
        if idx.size != n:
            raise ValueError("index length does not match the plane")
        out = np.empty((n_pl, H, W), np.uint8)
        route = self.route_dev(idx)
        with self._staging() as dev:
            if route is not None:
                d_u8 = dev.alloc(max(n_pl * n, 16))
                self._call("wm_unpermute_normalize_u8_dev", _vp(d_src), _vp(route), _vp(d_u8), n, n_pl, 1 if normalize else 0)
                self.d2h(out, d_u8)
                return out
            d_idx = self.index_dev(idx)
            n_pad = (n + 3) & ~3                  # the normalise kernel reads float4: every plane starts 16-byte aligned
            d_tmp = dev.alloc(n_pl * n_pad * 4); d_u8 = dev.alloc(n_pl * n_pad)
            for z in range(n_pl):
                self._call("wm_unpermute_f32_dev", _vp(d_src + z * n * 4), _vp(d_idx), _vp(d_tmp + z * n_pad * 4), n, 1)
                self._call("wm_normalize_u8_dev", _vp(d_tmp + z * n_pad * 4), n, 1 if normalize else 0,
                           _vp(d_u8 + z * n_pad))
                self.d2h(out[z], d_u8 + z * n_pad)
        return out

    def extract_tiles_unscrambled_u8(self, stego: np.ndarray, sigma_c: np.ndarray, Uw: np.ndarray, Vwt: np.ndarray,
                                     alpha: float, K: int, idx: np.ndarray, normalize: bool = True, mask=None) -> np.ndarray:
        """extract_tiles + unpermute + normalise without the float plane ever leaving the device
        (single:204-222 / 232-274): uint8 stego planes in, uint8 watermark planes out.  ``mask`` as in extract_tiles."""
        m = _mask_args(mask)
        if stego.dtype != np.uint8:
            raise ValueError("stego planes must be uint8")
        single = stego.ndim == 2
        st = np.ascontiguousarray(stego[None] if single else stego)
        n, H, W = st.shape
        sc, Uw, Vwt, uv_stride = self._tile_factors(sigma_c, Uw, Vwt, n, H // TILE, W // TILE)
        route = self.route_dev(idx) if idx.size == H * W else None
        with self._staging() as dev:
            d_w = dev.alloc(max(n * H * W if route is not None else n * H * W * 4, 16))
            d_st, d_sc, d_u, d_v = dev.up(st, sc, Uw, Vwt, floor=16)
            if route is not None:          # one call: extract kernel (with its min / max) -> routed unscramble -> uint8
                self._call("wm_extract_unscrambled_masked_u8_dev" if m else "wm_extract_unscrambled_u8_dev", _vp(d_st), _vp(d_sc),
                           _vp(d_u), _vp(d_v), _vp(route), _vp(d_w), n, H, W, W, H * W, uv_stride, float(alpha), int(K), 0,
                           1 if normalize else 0, *m)
                out = np.empty((n, H, W), np.uint8)
                self.d2h(out, d_w)
            else:                          # no route (an empty plane, or more pixels than one addresses): the two steps apart
                self._call("wm_extract_tiles_masked_u8_dev" if m else "wm_extract_tiles_u8_dev", _vp(d_st), _vp(d_sc), _vp(d_u),
                           _vp(d_v), _vp(d_w), n, H, W, W, H * W, uv_stride, float(alpha), int(K), *m)
                out = self._unpermute_normalize_dev(d_w, n, H, W, idx, normalize)
            # the *_dev entry points only set the sticky status bit; without this a Jacobi that hit its sweep
            # bound would hand back a watermark silently and surface in some later, unrelated call (DESIGN 5:
            # non-convergence -> WM_ERR_NOCONV -> numpy.linalg.LinAlgError, like the host-pointer wrapper)
            self.check_status()
        return out[0] if single else out

    # ---- pixel-side kernels (colour, PSNR, SSIM, normalise) ----------------------
    _COLOR_OPS = {"bgr2ycrcb": 0, "ycrcb2bgr": 1, "bgr2gray": 2, "bgr2y": 3, "replace_y": 4}

    def color(self, op: str, img: np.ndarray, plane: Optional[np.ndarray] = None) -> np.ndarray:
        """img: uint8 [H, W, 3]; returns [H, W, 3] (ops 0, 1, 4) or the [H, W] plane (ops 2, 3)."""
        code = self._COLOR_OPS[op]
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("img must be uint8 [H, W, 3]")
        img = np.ascontiguousarray(img)
        H, W = img.shape[:2]
        if code in (2, 3):
            out = np.empty((H, W), np.uint8)
            self._call("wm_color_u8", code, _p(img), None, None, _p(out), H * W)
            return out
        out = np.empty_like(img)
        pin = None
        if code == 4:
            plane = np.ascontiguousarray(plane, dtype=np.uint8)
            if plane.shape != (H, W):
                raise ValueError("plane must be [H, W]")
            pin = _p(plane)
        self._call("wm_color_u8", code, _p(img), pin, _p(out), None, H * W)
        return out

    # ---- frame codec: stored Y, Cb, Cr frames (chroma subsampled sub = (sx, sy)) <-> planar B, G, R ----------------
    @staticmethod
    def frame_bytes(H: int, W: int, sub) -> int:
        """bytes of one stored frame: Y [H, W], then Cb and Cr [ceil(H / sy), ceil(W / sx)]"""
        sx, sy = sub
        return H * W + 2 * (-(-H // sy)) * (-(-W // sx))

    def yuv_frames_to_bgr_planes_u8_dev(self, frames, planes, n_frames, H, W, sub, frame_stride):
        self._call("wm_yuv_frames_to_bgr_planes_u8_dev", _vp(frames), _vp(planes), n_frames, H, W, int(sub[0]), int(sub[1]),
                   frame_stride)

    def bgr_planes_to_yuv_frames_u8_dev(self, planes, frames, n_frames, H, W, sub, frame_stride):
        self._call("wm_bgr_planes_to_yuv_frames_u8_dev", _vp(planes), _vp(frames), n_frames, H, W, int(sub[0]), int(sub[1]),
                   frame_stride)

    @staticmethod
    def _frames_layout(frames: np.ndarray, fsz: int) -> int:
        """frame_stride in bytes of uint8 [n, fsz] frames whose rows may lie further apart than fsz"""
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != fsz:
            raise ValueError(f"frames must be uint8 [n, {fsz}]")
        n = frames.shape[0]
        if n * fsz == 0:                           # nothing is addressed (NumPy gives an empty array arbitrary strides)
            return fsz
        if fsz > 1 and frames.strides[1] != 1:
            raise ValueError("a frame's bytes must be contiguous")
        if n > 1 and frames.strides[0] < fsz:
            raise ValueError("frames overlap")
        return frames.strides[0] if n > 1 else fsz

    def yuv_frames_to_bgr_planes(self, frames: np.ndarray, H: int, W: int, sub) -> np.ndarray:
        """frames uint8 [n, H*W + 2*ch*cw] (Y, Cb, Cr planes of each frame, packed) -> B, G, R planes uint8 [n, 3, H, W]:
        chroma replicated to full resolution, OpenCV's 8-bit YCrCb2BGR per pixel.  One upload, launch and download."""
        fsz = self.frame_bytes(H, W, sub)
        stride = self._frames_layout(frames, fsz)
        planes = np.empty((frames.shape[0], 3, H, W), np.uint8)
        self._call("wm_yuv_frames_to_bgr_planes_u8", _p(frames), _p(planes), frames.shape[0], H, W, int(sub[0]), int(sub[1]),
                   stride)
        return planes

    def bgr_planes_to_yuv_frames(self, planes: np.ndarray, sub, out: Optional[np.ndarray] = None) -> np.ndarray:
        """B, G, R planes uint8 [n, 3, H, W] -> stored frames uint8 [n, H*W + 2*ch*cw]: OpenCV's 8-bit BGR2YCrCb per pixel,
        Cb and Cr averaged over each sx x sy block (half up; edge blocks over the pixels that exist).  ``out``: frames to
        write into, which may lie further apart than a frame (the bytes between them are left alone)."""
        if planes.dtype != np.uint8 or planes.ndim != 4 or planes.shape[1] != 3:
            raise ValueError("planes must be uint8 [n, 3, H, W]")
        planes = np.ascontiguousarray(planes)
        n, _, H, W = planes.shape
        fsz = self.frame_bytes(H, W, sub)
        if out is None:
            out = np.empty((n, fsz), np.uint8)
        elif out.shape[0] != n:
            raise ValueError(f"out must hold {n} frames")
        stride = self._frames_layout(out, fsz)
        self._call("wm_bgr_planes_to_yuv_frames_u8", _p(planes), _p(out), n, H, W, int(sub[0]), int(sub[1]), stride)
        return out

    def psnr(self, a: np.ndarray, b: np.ndarray) -> float:
        a = np.ascontiguousarray(a, dtype=np.uint8); b = np.ascontiguousarray(b, dtype=np.uint8)
        if a.shape != b.shape:
            raise ValueError("shape mismatch")
        v = C.c_double(0.0)
        self._call("wm_psnr_u8", _p(a), _p(b), a.size, C.byref(v))
        return v.value

    def ssim(self, img1: np.ndarray, img2: np.ndarray) -> float:
        """planes [H, W], each uint8 or float32"""
        def prep(x):
            if x.dtype == np.uint8:
                return np.ascontiguousarray(x), 0
            return np.ascontiguousarray(x, dtype=np.float32), 1
        x, k1 = prep(img1); y, k2 = prep(img2)
        if x.shape != y.shape or x.ndim != 2:
            raise ValueError("planes must be [H, W] of equal shape")
        v = C.c_double(0.0)
        self._call("wm_ssim", _p(x), _p(y), x.shape[0], x.shape[1], k1 | (k2 << 1), C.byref(v))
        return v.value

    def normalize_u8(self, x: np.ndarray, normalize: bool = True) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(x.shape, np.uint8)
        self._call("wm_normalize_u8", _p(x), x.size, 1 if normalize else 0, _p(out))
        return out

    # ---- extract post-processing (NL-means, CLAHE, unsharp, Lab; include/wmhip.h) ----------------------------------
    def _enh_pair(self, nbytes: int):
        """two grow-only device buffers of at least nbytes for the host-array wrappers below (freed by close())"""
        have, a, b = self.__dict__.get("_enh_bufs", (0, 0, 0))
        if have < nbytes:
            for d in (a, b):
                if d:
                    self.free(d)
            self.__dict__["_enh_bufs"] = (0, 0, 0)
            a, b = self.malloc(nbytes), self.malloc(nbytes)
            self.__dict__["_enh_bufs"] = (nbytes, a, b)
        return a, b

    @staticmethod
    def _u8_image(img: np.ndarray, channels) -> np.ndarray:
        img = np.ascontiguousarray(img)
        if img.dtype != np.uint8:
            raise ValueError("image must be uint8")
        ch = 1 if img.ndim == 2 else (img.shape[2] if img.ndim == 3 else 0)
        if ch not in channels:
            raise ValueError(f"image must be [H, W] or [H, W, C] with C in {channels}")
        return img

    def _enh_run(self, img: np.ndarray, fn, *args) -> np.ndarray:
        a, b = self._enh_pair(max(img.nbytes, 1))
        self.h2d(a, img)
        self._call(fn, _vp(a), _vp(b), *args)
        out = np.empty_like(img)
        self.d2h(out, b)
        self.sync()
        return out

    def nlmeans_u8(self, img: np.ndarray, h: float, template_ws: int = 7, search_ws: int = 21) -> np.ndarray:
        """cv2.fastNlMeansDenoising(img, None, h, template_ws, search_ws): uint8 [H, W] or [H, W, 2] (interleaved)."""
        img = self._u8_image(img, (1, 2))
        ch = 1 if img.ndim == 2 else 2
        return self._enh_run(img, "wm_nlmeans_u8_dev", img.shape[0], img.shape[1], ch, float(h), int(template_ws),
                             int(search_ws))

    def clahe_u8(self, img: np.ndarray, clip_limit: float = 2.0, tiles=(8, 8)) -> np.ndarray:
        """cv2.createCLAHE(clip_limit, tiles).apply(img): uint8 [H, W]; tiles = (tiles_x, tiles_y)."""
        img = self._u8_image(img, (1,))
        return self._enh_run(img, "wm_clahe_u8_dev", img.shape[0], img.shape[1], float(clip_limit), int(tiles[0]),
                             int(tiles[1]))

    def unsharp_u8(self, img: np.ndarray, amount: float) -> np.ndarray:
        """addWeighted(img, 1 + amount, GaussianBlur(img, (0, 0), 1.0), -amount, 0): uint8 [H, W] or [H, W, 3]."""
        img = self._u8_image(img, (1, 3))
        ch = 1 if img.ndim == 2 else 3
        return self._enh_run(img, "wm_unsharp_u8_dev", img.shape[0], img.shape[1], ch, float(amount))

    def lab_u8(self, img: np.ndarray, inverse: bool = False) -> np.ndarray:
        """COLOR_LBGR2Lab (inverse: COLOR_Lab2LBGR), 8-bit: uint8 [..., 3]."""
        img = np.ascontiguousarray(img)
        if img.dtype != np.uint8 or img.shape[-1] != 3:
            raise ValueError("image must be uint8 [..., 3]")
        return self._enh_run(img, "wm_lab_to_bgr_u8_dev" if inverse else "wm_bgr_to_lab_u8_dev", img.size // 3)

    def enhance_extract_u8(self, img: np.ndarray) -> np.ndarray:
        """The reference's extract post-processing: gray [H, W] single:223-227, BGR [H, W, 3] single:275-277."""
        img = self._u8_image(img, (1, 3))
        out = np.empty_like(img)
        ch = 1 if img.ndim == 2 else 3
        self._call("wm_enhance_extract_u8", _p(img), _p(out), img.shape[0], img.shape[1], ch)
        return out
