"""GPU: the extract post-processing chain (csrc/wm_enhance.hip) against its NumPy specification tests/enhance_oracle.py,
bit for bit - NL-means, CLAHE, unsharp, Lab, the whole gray / colour chains, and the drop-in's and the video path's
enhance="reference"."""
import importlib
import os

import numpy as np
import pytest

import enhance_oracle as eo
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _contents(H, W, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    return {
        "noise": rng.integers(0, 256, (H, W), dtype=np.uint8),
        "gradient": ((xx + yy) * 255 // max(H + W - 2, 1)).astype(np.uint8),
        "constant": np.full((H, W), 93, np.uint8),
        "blocks": np.where(((yy // 9) + (xx // 13)) % 2 == 0, 15, 240).astype(np.uint8),   # clips with a residual
    }


@pytest.fixture(scope="module")
def extracted():
    """Real extracted watermarks: the drop-in's enhance=False output on the golden fixtures."""
    import dct_svd_core_secure as core
    out = {}
    for name in ("gray_64x96_t8", "color_32x48_t8"):
        g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        r = core.embed_arrays(g["cover"], g["wm"], "golden-pw", bytes(g["meta_nonce"].tolist()), float(g["alpha"]),
                              bool(g["color"]), float(g["kfrac"]), 8, int(g["k_floor"]))
        out[name] = core.extract_arrays(r["stego"], r["meta"], "golden-pw")
    return out


@pytest.mark.parametrize("shape", [(7, 9), (64, 96), (257, 383)])
def test_nlmeans_gray_bit_exact(gpu_ctx, shape):
    for name, img in _contents(*shape, seed=shape[0]).items():
        got = gpu_ctx.nlmeans_u8(img, 7.0)
        assert np.array_equal(got, eo.nlmeans(img, 7.0)), name
        got3 = gpu_ctx.nlmeans_u8(img, 3.0)
        assert np.array_equal(got3, eo.nlmeans(img, 3.0)), name


@pytest.mark.parametrize("shape", [(7, 9), (64, 96), (257, 383)])
def test_nlmeans_two_channels_bit_exact(gpu_ctx, shape):
    c = _contents(*shape, seed=shape[1])
    for a, b in (("noise", "gradient"), ("constant", "blocks"), ("gradient", "noise")):
        ab = np.ascontiguousarray(np.stack([c[a], c[b]], axis=-1))
        assert np.array_equal(gpu_ctx.nlmeans_u8(ab, 3.0), eo.nlmeans(ab, 3.0)), (a, b)


def test_nlmeans_1080p_bit_exact(gpu_ctx):
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[:1080, :1920]
    img = np.clip(128 + 60 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + rng.normal(0, 12, (1080, 1920)), 0, 255).astype(np.uint8)
    assert np.array_equal(gpu_ctx.nlmeans_u8(img, 7.0), eo.nlmeans(img, 7.0))
    ab = np.ascontiguousarray(np.stack([img, img[::-1]], axis=-1) // 2 + 64)
    assert np.array_equal(gpu_ctx.nlmeans_u8(ab, 3.0), eo.nlmeans(ab, 3.0))


def test_nlmeans_on_extracted_watermarks(gpu_ctx, extracted):
    g = extracted["gray_64x96_t8"]
    assert np.array_equal(gpu_ctx.nlmeans_u8(g, 7.0), eo.nlmeans(g, 7.0))
    lab = eo.bgr_to_lab(extracted["color_32x48_t8"])
    ab = np.ascontiguousarray(lab[..., 1:])
    assert np.array_equal(gpu_ctx.nlmeans_u8(ab, 3.0), eo.nlmeans(ab, 3.0))
    assert np.array_equal(gpu_ctx.nlmeans_u8(np.ascontiguousarray(lab[..., 0]), 3.0), eo.nlmeans(lab[..., 0], 3.0))


def test_nlmeans_rejects_unsupported_windows(gpu_ctx):
    img = np.zeros((16, 16), np.uint8)
    for t, s in ((5, 21), (7, 15), (3, 11)):
        with pytest.raises(ValueError):
            gpu_ctx.nlmeans_u8(img, 7.0, t, s)
    with pytest.raises(ValueError):
        gpu_ctx.nlmeans_u8(img, 0.0)


@pytest.mark.parametrize("shape", [(8, 8), (10, 10), (64, 64), (1079, 1917), (1080, 1917), (1080, 1920)])
def test_clahe_bit_exact(gpu_ctx, shape):
    for name, img in _contents(*shape, seed=shape[1]).items():
        assert np.array_equal(gpu_ctx.clahe_u8(img, 2.0, (8, 8)), eo.clahe(img, 2.0)), name


def test_clahe_high_contrast_clips_with_a_residual(gpu_ctx):
    img = _contents(64, 64)["blocks"]
    total = 8 * 8
    clip = eo.clahe_clip_count(2.0, total)
    hist = np.bincount(img[:8, :8].ravel(), minlength=256)
    excess = int(np.maximum(hist - clip, 0).sum())
    assert excess > 0 and excess % 256 != 0
    assert np.array_equal(gpu_ctx.clahe_u8(img), eo.clahe(img))


@pytest.mark.parametrize("shape", [(5, 4), (64, 96), (1080, 1920)])
def test_unsharp_bit_exact(gpu_ctx, shape):
    rng = np.random.default_rng(1)
    g = rng.integers(0, 256, shape, dtype=np.uint8)
    assert np.array_equal(gpu_ctx.unsharp_u8(g, 0.25), eo.unsharp(g, 0.25))
    c = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    assert np.array_equal(gpu_ctx.unsharp_u8(c, 0.15), eo.unsharp(c, 0.15))


def test_lab_both_ways(gpu_ctx):
    every = np.stack(np.meshgrid(np.arange(256), np.arange(256), np.arange(0, 256, 3)), -1).reshape(-1, 3)
    every = np.ascontiguousarray(every.astype(np.uint8))
    # forward: integer tables, bit-exact; inverse: f32 without fused operations, bit-exact as measured (spec allows 1)
    assert np.array_equal(gpu_ctx.lab_u8(every), eo.bgr_to_lab(every))
    assert np.array_equal(gpu_ctx.lab_u8(every, inverse=True), eo.lab_to_bgr(every))


@pytest.mark.parametrize("shape", [(7, 9), (64, 96), (1080, 1920)])
def test_whole_chain(gpu_ctx, shape):
    rng = np.random.default_rng(shape[0])
    g = _contents(*shape)["noise"] // 3 + _contents(*shape)["gradient"] // 2
    assert np.array_equal(gpu_ctx.enhance_extract_u8(g), eo.enhance_gray(g))
    if shape[0] < 1000:          # the colour oracle at 1080p takes minutes
        c = rng.integers(0, 256, shape + (3,), dtype=np.uint8) // 2 + 40
        assert np.array_equal(gpu_ctx.enhance_extract_u8(c), eo.enhance_color(c))


def _write_pair(tmp_path, hg, H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    cover = np.clip(np.stack([90 + 50 * np.sin(xx / 9.0), 120 + 40 * np.cos(yy / 7.0), 100 + 30 * np.sin((xx + yy) / 11.0)], -1)
                    + rng.normal(0, 8, (H, W, 3)), 0, 255).astype(np.uint8)
    wm = np.zeros((32, 48, 3), np.uint8); wm[8:24, 10:38] = (255, 200, 40); wm[12:20, 16:30] = (0, 60, 255)
    cp, wp = str(tmp_path / "cover.png"), str(tmp_path / "wm.png")
    assert hg.write_png(cp, cover) and hg.write_png(wp, wm)
    return cp, wp


@pytest.mark.parametrize("tile", [8, None], ids=["tile8", "fullframe"])
@pytest.mark.parametrize("color", [False, True], ids=["gray", "color"])
def test_dropin_extract_reference(tmp_path, gpu_ctx, tile, color):
    import dct_svd_core_secure as core
    hg = importlib.import_module(PKG_NAME + ".hostglue")
    cp, wp = _write_pair(tmp_path, hg, 64, 96, 7)
    st, meta, _, _ = core.embed(cp, wp, str(tmp_path / "st.png"), str(tmp_path / "m.npz"), 0.15, color, "pw",
                                tile=tile, nonce=bytes(8))
    from PIL import Image
    read = lambda p: np.asarray(Image.open(p))[..., ::-1] if color else np.asarray(Image.open(p))
    w0 = read(core.extract(st, meta, str(tmp_path / "w0.png"), "pw"))
    w1 = read(core.extract(st, meta, str(tmp_path / "w1.png"), "pw", enhance=True))
    w2 = read(core.extract(st, meta, str(tmp_path / "w2.png"), "pw", enhance="reference"))
    assert w0.shape == ((64, 96, 3) if color else (64, 96))
    # enhance=False / True: what the code produced before ("reference" is the only new behaviour)
    data = hg.load_npz(meta)
    arr = core.extract_arrays(hg.read_image_bgr(st), data, "pw")
    assert np.array_equal(w0, arr)
    assert np.array_equal(w1, hg.unsharp(arr, 0.15 if color else 0.25))
    # the written PNG is the oracle chain applied to the enhance=False output; colour as exact as gray (Lab measured exact)
    assert np.array_equal(w2, eo.enhance(np.ascontiguousarray(w0)))
    assert np.array_equal(core.extract_arrays(hg.read_image_bgr(st), data, "pw", enhance="reference"), w2)


@pytest.mark.parametrize("color", [False, True], ids=["gray", "color"])
def test_video_extract_reference(tmp_path, gpu_ctx, color):
    from oracle import wm_oracle as o
    v = importlib.import_module(PKG_NAME + ".video")
    hg = importlib.import_module(PKG_NAME + ".hostglue")
    rng = np.random.default_rng(3)
    n, H, W = 5, 64, 96
    frames = rng.integers(30, 220, (n, H, W, 3), dtype=np.uint8)
    ycc = [o.bgr_to_ycrcb(f) for f in frames]
    ys = np.stack([f[..., 0] for f in ycc])
    chroma = np.stack([np.concatenate([f[..., 2].ravel(), f[..., 1].ravel()]) for f in ycc])
    p = str(tmp_path / "in.y4m")
    v.write_y4m(p, ys, chroma, chroma_tag="444")
    wm = np.random.default_rng(5).integers(0, 256, (16, 24, 3), dtype=np.uint8)
    wp = str(tmp_path / "wm.png"); assert hg.write_png(wp, wm)
    emb = v.embed_watermark_video_color if color else v.embed_watermark_video
    ext = v.extract_watermark_video_color if color else v.extract_watermark_video
    outp, meta, _ = emb(p, wp, str(tmp_path / "out.y4m"), str(tmp_path / "m.npz"), alpha=0.15, frame_interval=2,
                        password="pw", nonce=bytes(8), batch=2)
    from PIL import Image
    read = lambda q: np.asarray(Image.open(q))[..., ::-1] if color else np.asarray(Image.open(q))
    w0 = read(ext(outp, meta, str(tmp_path / "w0.png"), password="pw"))
    w2 = read(ext(outp, meta, str(tmp_path / "w2.png"), password="pw", enhance="reference"))
    assert np.array_equal(w2, eo.enhance(np.ascontiguousarray(w0)))
