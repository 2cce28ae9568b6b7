"""A stand-in ``cv2`` for running the reference program inside the suite.  TEST INFRASTRUCTURE ONLY.

``make()`` returns a fresh module object that offers exactly the ``cv2`` names the reference's three public functions
(embed / extract / detect) and their helpers use.  Every entry delegates to the restatement of the same meaning that
the project already has - ``oracle.wm_oracle`` for the DCT, colour conversion, resize, float blur and normalise,
``tests/enhance_oracle.py`` for NL-means, CLAHE, the 8-bit blur and the saturating cast - so running the reference
over it pins the reference's *program logic* (everything that is not a ``cv2.*`` call) and its file formats.
OpenCV's own arithmetic is NOT pinned by it: the stand-in *is* the restatements.  One
consequence: ``cv2.dct`` refuses odd sizes, the stand-in does not - size limits are OpenCV's, not the program's.

PNG I/O goes through Pillow and never through the product's ``hostglue``: an independent decoder and encoder is the
point of putting the product's files through the reference.

Every entry asserts the dtype, channel count and arguments it was written for and refuses anything else.  The
reference wraps NL-means and CLAHE in ``try/except: pass``, so a refusal there would be swallowed and silently change
the output; therefore every call and every exception raised is recorded in ``module.log`` (a ``CallLog``), and the
tests assert on it: expected calls made, nothing raised.
"""
from __future__ import annotations

import functools
import types

import numpy as np
from PIL import Image

import enhance_oracle as eo
from oracle import wm_oracle as o

F32 = np.float32

# OpenCV's values; only their identity matters here
IMREAD_COLOR = 1
COLOR_BGR2GRAY = 6
COLOR_BGR2YCrCb = 36
COLOR_YCrCb2BGR = 38
INTER_AREA = 3
NORM_MINMAX = 32
IMWRITE_PNG_COMPRESSION = 16


class CallLog:
    """calls: names in call order; errors: (name, exception) for every exception a stand-in entry raised."""

    def __init__(self):
        self.calls = []
        self.errors = []

    def clear(self):
        self.calls.clear()
        self.errors.clear()

    def count(self, name: str) -> int:
        return sum(1 for c in self.calls if c == name)


def _need(cond, what: str):
    if not cond:
        raise TypeError("cv2 stand-in: " + what)


def _is_u8(a, ndims=(2, 3)):
    return isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim in ndims and (a.ndim == 2 or a.shape[2] == 3)


def make() -> types.ModuleType:
    log = CallLog()
    m = types.ModuleType("cv2")
    m.__doc__ = "stand-in for OpenCV (tests/cv2_standin.py)"
    m.log = log

    def entry(fn):
        @functools.wraps(fn)
        def wrapped(*a, **kw):
            log.calls.append(fn.__name__)
            try:
                return fn(*a, **kw)
            except BaseException as e:
                log.errors.append((fn.__name__, e))
                raise
        setattr(m, fn.__name__, wrapped)
        return wrapped

    for name in ("IMREAD_COLOR", "COLOR_BGR2GRAY", "COLOR_BGR2YCrCb", "COLOR_YCrCb2BGR", "INTER_AREA", "NORM_MINMAX",
                 "IMWRITE_PNG_COMPRESSION"):
        setattr(m, name, globals()[name])

    # ---- files ---------------------------------------------------------------------------------------------
    @entry
    def imread(path, flags=IMREAD_COLOR):
        _need(flags == IMREAD_COLOR, "imread is written for IMREAD_COLOR")
        try:
            with Image.open(path) as im:
                _need(im.mode in ("L", "RGB"), f"imread is written for 8-bit gray or RGB files, got mode {im.mode}")
                rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
        except (OSError, SyntaxError, ValueError):
            return None                                   # cv2.imread returns None for what it cannot open
        return np.ascontiguousarray(rgb[..., ::-1])

    @entry
    def imwrite(path, img, params=None):
        _need(_is_u8(img), "imwrite is written for uint8 gray or BGR")
        _need(str(path).lower().endswith(".png"), "imwrite is written for .png paths")
        level = 1                                         # OpenCV's speed-oriented default for PNG
        if params is not None:
            _need(len(params) == 2 and params[0] == IMWRITE_PNG_COMPRESSION, "imwrite takes [IMWRITE_PNG_COMPRESSION, n]")
            level = int(params[1])
        if img.ndim == 2:
            Image.fromarray(np.ascontiguousarray(img)).save(path, format="PNG", compress_level=level)
        else:
            Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(path, format="PNG", compress_level=level)
        return True

    # ---- colour and channels -------------------------------------------------------------------------------
    @entry
    def cvtColor(src, code):
        _need(_is_u8(src, (3,)), "cvtColor is written for uint8 3-channel input")
        if code == COLOR_BGR2YCrCb:
            return o.bgr_to_ycrcb(src)
        if code == COLOR_YCrCb2BGR:
            return o.ycrcb_to_bgr(src)
        if code == COLOR_BGR2GRAY:
            return o.bgr_to_gray(src)
        _need(False, f"cvtColor code {code} is not one the reference's core uses")

    @entry
    def split(src):
        _need(isinstance(src, np.ndarray) and src.ndim == 3 and src.shape[2] == 3 and src.dtype in (np.uint8, np.float32),
              "split is written for 3-channel uint8 or float32")
        return [np.ascontiguousarray(src[..., c]) for c in range(3)]

    @entry
    def merge(planes):
        _need(len(planes) == 3 and all(isinstance(p, np.ndarray) and p.ndim == 2 and p.dtype == np.uint8 for p in planes)
              and len({p.shape for p in planes}) == 1, "merge is written for three uint8 planes of one size")
        return np.ascontiguousarray(np.stack(planes, axis=-1))

    # ---- transforms ----------------------------------------------------------------------------------------
    @entry
    def dct(src):
        _need(isinstance(src, np.ndarray) and src.dtype == np.float32 and src.ndim == 2, "dct is written for float32 planes")
        return o.dct2(src)

    @entry
    def idct(src):
        _need(isinstance(src, np.ndarray) and src.dtype == np.float32 and src.ndim == 2, "idct is written for float32 planes")
        return o.idct2(src)

    @entry
    def resize(src, dsize, interpolation=None):
        _need(_is_u8(src, (3,)), "resize is written for uint8 BGR")
        _need(interpolation == INTER_AREA, "resize is written for INTER_AREA")
        W, H = dsize
        return o.resize_area(src, int(W), int(H))

    @entry
    def GaussianBlur(src, ksize, sigmaX):
        if isinstance(src, np.ndarray) and src.dtype == np.float32:
            _need(src.ndim == 2 and tuple(ksize) == (11, 11) and sigmaX == 1.5, "float32 GaussianBlur is written for (11, 11), 1.5")
            return o.gaussian_blur(src, 11, 1.5)
        _need(_is_u8(src) and tuple(ksize) == (0, 0) and sigmaX == 1.0, "uint8 GaussianBlur is written for (0, 0), 1.0")
        return eo.blur_u8(src)

    @entry
    def normalize(src, dst, alpha, beta, norm_type):
        _need(isinstance(src, np.ndarray) and src.dtype == np.float32 and src.ndim == 2 and dst is None
              and alpha == 0 and beta == 255 and norm_type == NORM_MINMAX, "normalize is written for (f32 plane, None, 0, 255, NORM_MINMAX)")
        return o.normalize_minmax(src)

    # ---- the post-processing chain -------------------------------------------------------------------------
    class _Clahe:
        def __init__(self, clip, grid):
            self.clip, self.grid = clip, grid

        def apply(self, src):
            log.calls.append("CLAHE.apply")
            try:
                _need(_is_u8(src, (2,)), "CLAHE.apply is written for uint8 planes")
                return eo.clahe(src, self.clip, self.grid[0], self.grid[1])
            except BaseException as e:
                log.errors.append(("CLAHE.apply", e))
                raise

    @entry
    def createCLAHE(clipLimit=40.0, tileGridSize=(8, 8)):
        _need(clipLimit == 2.0 and tuple(tileGridSize) == (8, 8), "createCLAHE is written for clipLimit 2.0 on 8 x 8 tiles")
        return _Clahe(float(clipLimit), tuple(tileGridSize))

    @entry
    def addWeighted(src1, alpha, src2, beta, gamma):
        _need(_is_u8(src1) and _is_u8(src2) and src1.shape == src2.shape and gamma == 0,
              "addWeighted is written for two uint8 images of one shape and gamma 0")
        t = (src1.astype(F32) * F32(alpha)).astype(F32)
        u = (src2.astype(F32) * F32(beta)).astype(F32)
        return eo.sat_u8(t + u)

    @entry
    def fastNlMeansDenoising(src, dst, h, templateWindowSize, searchWindowSize):
        _need(_is_u8(src, (2,)) and dst is None and (h, templateWindowSize, searchWindowSize) == (7, 7, 21),
              "fastNlMeansDenoising is written for (uint8 plane, None, 7, 7, 21)")
        return eo.nlmeans(src, 7.0)

    @entry
    def fastNlMeansDenoisingColored(src, dst, h, hColor, templateWindowSize, searchWindowSize):
        _need(_is_u8(src, (3,)) and dst is None and (h, hColor, templateWindowSize, searchWindowSize) == (3, 3, 7, 21),
              "fastNlMeansDenoisingColored is written for (uint8 BGR, None, 3, 3, 7, 21)")
        return eo.denoise_color(src)

    return m
