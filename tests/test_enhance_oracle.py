"""Facts of the extract post-processing specification (tests/enhance_oracle.py) that do not need a device."""
import numpy as np
import pytest

import enhance_oracle as eo


def test_nlmeans_constants_and_table_prefixes():
    assert eo.nlm_fpm(21) == 19096 and eo.nlm_shift(7) == 6
    g = eo.nlm_weights(7.0, 1)
    ab = eo.nlm_weights(3.0, 2)
    assert len(g) - 1 == 259 and len(ab) - 1 == 95          # non-zero prefixes, then one 0
    for w in (g, ab):
        assert w[0] == 19096 and w[-1] == 0 and np.all(w[:-1] > 0) and np.all(np.diff(w) <= 0)
    # no overflow by construction: 441 offsets x fpm x 255 < 2^31
    assert 441 * 19096 * 255 < 2 ** 31


def test_blur_taps():
    assert eo.BLUR_TAPS.sum() == 256 and list(eo.BLUR_TAPS) == list(eo.BLUR_TAPS[::-1])


def test_constant_image():
    c = np.full((19, 23), 77, np.uint8)
    assert np.array_equal(eo.nlmeans(c, 7.0), c)
    ab = np.full((19, 23, 2), (40, 200), np.uint8)
    assert np.array_equal(eo.nlmeans(ab, 3.0), ab)
    # CLAHE: one bin holds the whole tile; clip, spread, and the LUT at 77 is the formula's value everywhere
    H, W = 64, 64
    total = (H // 8) * (W // 8)
    clip = max(int(2.0 * total / 256), 1)
    hist = np.zeros(256, np.int64); hist[77] = total
    h2 = eo.clahe_clip_hist(hist, clip)
    expect = int(np.rint(np.float32(h2[:78].sum()) * np.float32(255.0 / total)))
    out = eo.clahe(np.full((H, W), 77, np.uint8))
    assert np.all(out == expect)
    assert np.array_equal(eo.unsharp(c, 0.25), c)


@pytest.mark.parametrize("clip,hist_seed", [(7, 0), (33, 1), (1, 2)])
def test_clahe_histogram_keeps_its_total(clip, hist_seed):
    rng = np.random.default_rng(hist_seed)
    hist = np.zeros(256, np.int64)
    np.add.at(hist, rng.integers(0, 40, 1000), 1)          # a peaked histogram: lots of excess
    out = eo.clahe_clip_hist(hist, clip)
    assert out.sum() == hist.sum()
    excess = int(np.maximum(hist - clip, 0).sum())
    assert excess % 256 != 0 or hist_seed != 0              # the first case has a non-zero residual
    assert out.max() <= clip + excess // 256 + 1


def test_clahe_residual_spread():
    hist = np.zeros(256, np.int64); hist[0] = 300         # clip 10: excess 290 = 1 * 256 + 34
    out = eo.clahe_clip_hist(hist, 10)
    step = 256 // 34
    assert out.sum() == 300
    assert out[0] == 10 + 1 + 1 and out[step] == 1 + 1 and out[step * 33] == 2 and out[step * 34] == 1


def test_clahe_padding_quirk():
    # both sides are padded when either one is not a multiple of 8, the divisible one by a whole 8
    assert eo.clahe_padded(1080, 1917) == (1088, 1920)
    assert eo.clahe_padded(1079, 1920) == (1080, 1928)
    assert 1928 // 8 == 241
    assert eo.clahe_padded(1080, 1920) == (1080, 1920)


def test_nlmeans_equals_brute_force():
    rng = np.random.default_rng(5)
    for ch, h in ((1, 7.0), (2, 3.0)):
        shape = (12, 15) if ch == 1 else (12, 15, 2)
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        img[:6] = img[:6] // 16 + 100                      # some flat area, so that many weights are non-zero
        got = eo.nlmeans(img, h)
        x = img.reshape(12, 15, ch).astype(np.int64)
        lut = eo.nlm_weights(h, ch)
        n_nz = len(lut) - 1
        # np.pad's "reflect" is reflect-101, repeated for pads wider than the image
        ext = np.pad(x, ((13, 13), (13, 13), (0, 0)), mode="reflect")
        ref = np.empty_like(x)
        for y in range(12):
            for xx in range(15):
                cy, cx = y + 13, xx + 13
                centre = ext[cy - 3:cy + 4, cx - 3:cx + 4]
                est = np.zeros(ch, np.int64); ws = 0
                for dy in range(-10, 11):
                    for dx in range(-10, 11):
                        nb = ext[cy + dy - 3:cy + dy + 4, cx + dx - 3:cx + dx + 4]
                        ssd = int(((centre - nb) ** 2).sum())
                        w = int(lut[min(ssd >> 6, n_nz)])
                        ws += w
                        est += w * ext[cy + dy, cx + dx]
                ref[y, xx] = (est + ws // 2) // ws
        assert np.array_equal(got.reshape(12, 15, ch), ref), ch


def test_reflect101_wider_than_the_image():
    for n in (1, 2, 7):
        p = np.arange(-13, n + 13)
        assert np.array_equal(eo.reflect101(p, n), np.pad(np.arange(n), 13, mode="reflect" if n > 1 else "edge"))


def test_lab_round_trip_is_close():
    rng = np.random.default_rng(2)
    bgr = rng.integers(0, 256, (50, 3), dtype=np.uint8)
    back = eo.lab_to_bgr(eo.bgr_to_lab(bgr))
    assert np.abs(back.astype(int) - bgr).max() <= 8
    assert np.array_equal(eo.bgr_to_lab(np.zeros((1, 3), np.uint8))[0], [0, 128, 128])
    assert np.array_equal(eo.bgr_to_lab(np.full((1, 3), 255, np.uint8))[0], [255, 128, 128])


def test_dropin_rejects_an_unknown_enhance_mode_without_a_device(tmp_path):
    import dct_svd_core_secure as core
    with pytest.raises(ValueError, match="enhance"):
        core.extract(str(tmp_path / "none.png"), str(tmp_path / "none.npz"), str(tmp_path / "o.png"), "pw",
                     enhance="bogus")
    with pytest.raises(ValueError, match="enhance"):
        core.extract_arrays(np.zeros((16, 16, 3), np.uint8), {}, "pw", enhance="Reference")
    import importlib
    video = importlib.import_module(core._impl.__package__ + ".video")
    with pytest.raises(ValueError, match="enhance"):
        video.extract_watermark_video("none.y4m", "none.npz", "o.png", "pw", enhance=2)
    with pytest.raises(ValueError, match="enhance"):
        video.extract_watermark_video_color("none.y4m", "none.npz", "o.png", "pw", enhance="x")


def test_clahe_clip_count_saturates():
    big = 2 ** 31 - 1
    assert eo.clahe_clip_count(2.0, 64) == 1 and eo.clahe_clip_count(2.0, 8100) == 63
    assert eo.clahe_clip_count(0.0, 561) == 0 and eo.clahe_clip_count(-1.0, 561) == 0
    assert eo.clahe_clip_count(float(big - 1), 256) == big - 1          # the largest count that is not saturated
    for clip, total in ((1e9, 561), (1e9, 550), (1e30, 1), (float(big), 256), (float("inf"), 64)):
        assert eo.clahe_clip_count(clip, total) == big, (clip, total)
    # a count >= the tile's pixel count leaves the histogram alone, so a huge clip equals no clipping at all
    hist = np.zeros(256, np.int64); hist[7] = 561
    assert np.array_equal(eo.clahe_clip_hist(hist, big), hist)
    rng = np.random.default_rng(4)
    img = rng.integers(0, 64, (17, 33), dtype=np.uint8)
    for tiles in ((1, 1), (3, 5)):
        none = eo.clahe(img, 0.0, *tiles)
        assert np.array_equal(eo.clahe(img, 1e9, *tiles), none)
        assert np.array_equal(eo.clahe(img, 1e30, *tiles), none)
        assert not np.array_equal(eo.clahe(img, 0.01, *tiles), none)      # clip count 1: maximal equalisation differs
