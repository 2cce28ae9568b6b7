"""Loader for the reference program as built by ``oracle/ref_build.py``.  TEST INFRASTRUCTURE ONLY.

``load()`` executes the byte-compiled reference module from ``oracle/_ref/`` and returns a handle to it.  While (and
only while) the module's top level runs, ``sys.modules`` holds a stand-in ``cv2`` (tests/cv2_standin.py) and stub
``PySide6`` modules whose attributes are empty classes; they are taken out again before ``load()`` returns, so
nothing else in the process ever sees a fake ``cv2``.  The module itself is not registered in ``sys.modules``.  The
``os`` name inside the module's namespace is replaced by a proxy whose ``urandom`` draws from a settable nonce source
(the reference takes its nonce from ``os.urandom(8)``); everything else of ``os`` passes through.

Skipping rule, used by every test that needs the program: skip ONLY when the compiled file is absent
(``needs_program``).  A file that is present but does not load - another interpreter's magic number, a source other
than the one the committed fixtures were made from - is a failure, not a skip.
"""
from __future__ import annotations

import importlib.machinery
import importlib.util
import json
import os
import sys
import types

import numpy as np
import pytest

import cv2_standin
import enhance_oracle as eo
from oracle import ref_build
from oracle import wm_oracle as o

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "golden", "reference")
SKIP_REASON = ("the compiled reference program is absent from oracle/_ref/: run oracle/ref_build.py (build() does) on a "
               "checkout that has the reference tree")


def available() -> bool:
    return os.path.isfile(ref_build.COMPILED)


needs_program = pytest.mark.skipif(not available(), reason=SKIP_REASON)


class _StubModule(types.ModuleType):
    """``from PySide6.QtWidgets import QWidget, ...``: every attribute is an empty class of that name."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (), {})
        setattr(self, name, cls)
        return cls


class _Os:
    """The ``os`` module with ``urandom`` drawn from the handle's nonce source."""

    def __init__(self, owner):
        self._owner = owner

    def urandom(self, n):
        nonce = self._owner.next_nonce
        assert nonce is not None, "set Program.next_nonce before embed()"
        assert len(nonce) == n, (len(nonce), n)
        self._owner.next_nonce = None              # one embed, one nonce: a forgotten reset must not repeat a nonce silently
        return bytes(nonce)

    def __getattr__(self, name):
        return getattr(os, name)


class Program:
    """The loaded reference module (``.mod``), its stand-in cv2's call log (``.log``) and the nonce source."""

    def __init__(self, mod, standin):
        self.mod, self.cv2, self.log = mod, standin, standin.log
        self.next_nonce = None

    def embed(self, *a, nonce: bytes, **kw):
        self.next_nonce = nonce
        return self.mod.embed(*a, **kw)

    def extract(self, *a, **kw):
        return self.mod.extract(*a, **kw)

    def detect(self, *a, **kw):
        return self.mod.detect(*a, **kw)


def build_info() -> dict:
    return ref_build.read_info()


def load(compiled: str = ref_build.COMPILED) -> Program:
    standin = cv2_standin.make()
    stubs = {"cv2": standin}
    for name in ("PySide6", "PySide6.QtWidgets", "PySide6.QtCore", "PySide6.QtGui"):
        stubs[name] = _StubModule(name)
    stubs["PySide6"].__path__ = []
    missing = object()
    saved = {k: sys.modules.get(k, missing) for k in stubs}
    loader = importlib.machinery.SourcelessFileLoader("wm_reference_single", compiled)
    spec = importlib.util.spec_from_loader("wm_reference_single", loader)
    mod = importlib.util.module_from_spec(spec)
    try:
        sys.modules.update(stubs)
        loader.exec_module(mod)                    # ImportError on another interpreter's magic number: a failure
    finally:
        for k, v in saved.items():
            if v is missing:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert mod.cv2 is standin
    prog = Program(mod, standin)
    mod.os = _Os(prog)
    return prog


# ---- the committed fixtures (tests/golden/reference/, written by the reference: make_reference_golden.py) ------------
def results() -> dict:
    with open(os.path.join(FIXTURES, "results.json"), "r", encoding="utf-8") as f:
        return json.load(f)


def case_names():
    return sorted(results()["cases"])


def case_path(case: str, name: str) -> str:
    return os.path.join(FIXTURES, case, name)


def read_png(path: str) -> np.ndarray:
    """Pillow's decode as cv2.imread(IMREAD_COLOR) would return it (BGR, 3 channels) - independent of hostglue."""
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode in ("L", "RGB"), im.mode
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[..., ::-1])


def wm_image(path: str, color: bool) -> np.ndarray:
    """A written watermark file as the array the program wrote: [H, W] in gray mode, BGR in colour mode."""
    img = read_png(path)
    return img if color else np.ascontiguousarray(img[..., 0])


def load_meta(path: str) -> dict:
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def oracle_chain(stego_bgr, meta, password, normalize=True):
    """What the reference's extract writes, restated: the oracle's estimate, then the post-processing chain."""
    return eo.enhance(np.ascontiguousarray(o.extract_arrays(stego_bgr, meta, password, normalize, None)))


# ---- the bar for ENHANCED watermark images that were not computed from identical input ------------------------------
# The un-enhanced full-frame estimate of another LAPACK, or of the device, is held to the oracle by the bars of
# tests/test_oracle.py and tests/test_gpu_dropin.py (share of pixels off by more than 2 below 5e-2).  The reference
# writes only the ENHANCED image (NL-means, CLAHE, unsharp), and that chain amplifies: a bar for it cannot be guessed and
# must not be read off the output under test.  It is the ORACLE's own sensitivity, measured on the CPU on the
# committed fixtures (tests/golden/make_reference_golden.py --sensitivity): enhance(x) against enhance(x +- 1 LSB on
# 5e-2 of the pixels, the share the full-frame extract is allowed to miss), 8 seeds per fixture case, all 8 cases.
# Worst values measured: mean absolute difference MEASURED_MEAN_ABS grey levels, share of pixels off by more than
# ENHANCED_OFF_BY grey levels MEASURED_SHARE.  The bars are twice the worst values.
ENHANCED_OFF_BY = 8
MEASURED_MEAN_ABS = 1.8281      # gray_56x40_shrink, seed 6
MEASURED_SHARE = 0.0451         # color_32x48_x2
ENHANCED_MEAN_ABS_BAR = 2 * MEASURED_MEAN_ABS
ENHANCED_SHARE_BAR = 2 * MEASURED_SHARE


def enhanced_distance(a: np.ndarray, b: np.ndarray):
    d = np.abs(a.astype(int) - b.astype(int))
    return float(d.mean()), float(np.mean(d > ENHANCED_OFF_BY))


def assert_enhanced_close(a: np.ndarray, b: np.ndarray, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8, (what, a.shape, b.shape)
    mean_abs, share = enhanced_distance(a, b)
    print(f"enhanced distance {what}: mean abs {mean_abs:.4f} (bar {ENHANCED_MEAN_ABS_BAR}), "
          f"share off by > {ENHANCED_OFF_BY}: {share:.4f} (bar {ENHANCED_SHARE_BAR})")
    assert mean_abs <= ENHANCED_MEAN_ABS_BAR and share <= ENHANCED_SHARE_BAR, (what, mean_abs, share)
