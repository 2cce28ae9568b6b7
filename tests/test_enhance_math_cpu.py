"""csrc/wm_enhance_math.h (the arithmetic the gfx950 kernels of wm_enhance.hip are made of), compiled with g++ through
tests/enhance_harness.cpp, against the NumPy specification tests/enhance_oracle.py - bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import enhance_oracle as eo

HERE = os.path.dirname(os.path.abspath(__file__))
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def eh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("enh") / "libwm_enhance_harness.so")
    r = subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-o", so,
                        os.path.join(HERE, "enhance_harness.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.eh_nlm_weights.argtypes = [C.c_float, C.c_int, np.ctypeslib.ndpointer(np.int32), C.c_int]
    lib.eh_nlmeans.argtypes = [_u8p, _u8p, C.c_int, C.c_int, C.c_int, C.c_float]
    lib.eh_clahe.argtypes = [_u8p, _u8p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _u8p]
    lib.eh_unsharp.argtypes = [_u8p, _u8p, C.c_int, C.c_int, C.c_int, C.c_float]
    lib.eh_lab_tables.argtypes = [np.ctypeslib.ndpointer(np.uint16), np.ctypeslib.ndpointer(np.int32)]
    lib.eh_bgr_to_lab.argtypes = [_u8p, _u8p, C.c_size_t]
    lib.eh_lab_to_bgr.argtypes = [_u8p, _u8p, C.c_size_t]
    return lib


def _images(rng, H, W):
    yy, xx = np.mgrid[:H, :W]
    noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
    grad = ((xx * 255) // max(W - 1, 1)).astype(np.uint8)
    blocks = np.where(((yy // 5) + (xx // 7)) % 2 == 0, 20, 235).astype(np.uint8)     # high contrast: clipping
    return {"noise": noise, "gradient": grad, "blocks": blocks, "constant": np.full((H, W), 131, np.uint8)}


@pytest.mark.parametrize("h,ch", [(7.0, 1), (3.0, 1), (3.0, 2), (10.0, 1)])
def test_weight_table(eh, h, ch):
    w = np.zeros(2048, np.int32)
    n = eh.eh_nlm_weights(h, ch, w, 2048)
    ref = eo.nlm_weights(h, ch)
    assert n == len(ref) - 1 and np.array_equal(w[:n + 1], ref)


@pytest.mark.parametrize("shape", [(7, 9), (20, 27)])
def test_nlmeans_per_pixel(eh, shape):
    rng = np.random.default_rng(11)
    for name, img in _images(rng, *shape).items():
        out = np.empty_like(img)
        assert eh.eh_nlmeans(img, out, *shape, 1, 7.0) == 259
        assert np.array_equal(out, eo.nlmeans(img, 7.0)), name
    ab = rng.integers(100, 140, shape + (2,), dtype=np.uint8)
    out = np.empty_like(ab)
    assert eh.eh_nlmeans(ab, out, *shape, 2, 3.0) == 95
    assert np.array_equal(out, eo.nlmeans(ab, 3.0))


@pytest.mark.parametrize("shape", [(8, 8), (10, 10), (64, 64), (67, 64), (64, 75), (131, 77)])
def test_clahe_luts_and_interpolation(eh, shape):
    rng = np.random.default_rng(3)
    for name, img in _images(rng, *shape).items():
        out = np.empty_like(img)
        luts = np.empty((8, 8, 256), np.uint8)
        eh.eh_clahe(img, out, *shape, 2.0, 8, 8, luts)
        assert np.array_equal(luts, eo.clahe_luts(img)), name
        assert np.array_equal(out, eo.clahe(img)), name


@pytest.mark.parametrize("ch", [1, 3])
def test_unsharp(eh, ch):
    rng = np.random.default_rng(4)
    for shape in ((5, 4), (33, 70)):
        img = rng.integers(0, 256, shape + ((ch,) if ch == 3 else ()), dtype=np.uint8)
        out = np.empty_like(img)
        eh.eh_unsharp(img, out, *shape, ch, 0.25 if ch == 1 else 0.15)
        assert np.array_equal(out, eo.unsharp(img, 0.25 if ch == 1 else 0.15))


def test_lab_both_ways(eh):
    tab = np.empty(3072, np.uint16); coeffs = np.empty(9, np.int32)
    eh.eh_lab_tables(tab, coeffs)
    rtab, rC = eo.lab_tables()
    assert np.array_equal(tab, rtab) and np.array_equal(coeffs, rC)
    rng = np.random.default_rng(6)
    bgr = np.concatenate([rng.integers(0, 256, (4096, 3), dtype=np.uint8),
                          np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)])
    lab = np.empty_like(bgr)
    eh.eh_bgr_to_lab(bgr, lab, len(bgr))
    assert np.array_equal(lab, eo.bgr_to_lab(bgr))
    every = np.stack(np.meshgrid(np.arange(0, 256, 3), np.arange(0, 256, 5), np.arange(0, 256, 7)), -1).reshape(-1, 3)
    every = np.ascontiguousarray(every.astype(np.uint8))
    back = np.empty_like(every)
    eh.eh_lab_to_bgr(every, back, len(every))
    assert np.array_equal(back, eo.lab_to_bgr(every))


@pytest.mark.parametrize("shape,tiles", [((17, 33), (1, 1)), ((64, 64), (8, 8)), ((131, 77), (3, 5))])
def test_clahe_huge_clip_clips_nothing(eh, shape, tiles):
    """clip * total / 256 past INT_MAX saturates (a plain int cast is undefined there and gave a count of 1 on x86:
    maximal equalisation); a count at or above the tile's pixel count clips nothing, so the result is clip 0's."""
    rng = np.random.default_rng(8)
    Hp, Wp = eo.clahe_padded(*shape, *tiles)
    total = (Hp // tiles[1]) * (Wp // tiles[0])
    for name, img in _images(rng, *shape).items():
        luts = np.empty(tiles[::-1] + (256,), np.uint8)
        out0 = np.empty_like(img)
        assert eh.eh_clahe(img, out0, *shape, 0.0, *tiles, luts) == 0
        for clip in (1e9, 1e30):
            if clip * total / 256 < 2 ** 31:
                continue                                           # only the shapes where the count overflows
            out = np.empty_like(img)
            assert eh.eh_clahe(img, out, *shape, clip, *tiles, luts) == 2 ** 31 - 1
            assert np.array_equal(luts, eo.clahe_luts(img, clip, *tiles)), (name, clip)
            assert np.array_equal(out, eo.clahe(img, clip, *tiles)), (name, clip)
            assert np.array_equal(out, out0), (name, clip)
        assert np.array_equal(out0, eo.clahe(img, 0.0, *tiles)), name


@pytest.mark.parametrize("ch", [1, 2])
def test_weight_table_at_the_lds_boundary(eh, ch):
    """The longest table the kernels keep (2047 non-zero entries + the 0): at the largest h that fits, the header's
    table is the oracle's; one float32 step up it is refused."""
    h = eo.nlm_boundary_h(ch)
    ref = eo.nlm_weights(h, ch)
    assert len(ref) - 1 == 2047
    w = np.zeros(2048, np.int32)
    n = eh.eh_nlm_weights(h, ch, w, 2048)
    assert n == len(ref) - 1 and np.array_equal(w[:n + 1], ref)
    up = float(np.nextafter(np.float32(h), np.float32(np.inf)))
    assert len(eo.nlm_weights(up, ch)) - 1 > 2047
    assert eh.eh_nlm_weights(up, ch, w, 2048) == -1
