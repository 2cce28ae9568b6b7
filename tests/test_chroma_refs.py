"""The NumPy frame codec for subsampled chroma (tests/chroma_refs.py) against its own definition, the meta's ``chroma``
member and the ``subsampling`` keyword of embed_watermark_video_color.  No device."""
import importlib

import numpy as np
import pytest

import chroma_refs as cr
from conftest import PKG_NAME
from oracle import wm_oracle as o

SIZES = (1, 2, 3, 5, 16, 17)


@pytest.mark.parametrize("sub", cr.SUBS)
def test_box_down_of_replicated_chroma_is_the_chroma(sub):
    rng = np.random.default_rng(11)
    for H in SIZES:
        for W in SIZES:
            ch, cw = cr.chroma_shape(H, W, sub)
            c = rng.integers(0, 256, (2, ch, cw), dtype=np.uint8)
            up = cr.replicate(c, H, W, sub)
            assert up.shape == (2, H, W)
            assert np.array_equal(up[:, ::sub[1], ::sub[0]], c)
            assert np.array_equal(cr.box_down(up, sub), c), (H, W, sub)


def test_box_down_rounds_half_up():
    def one(vals, sub, shape):
        return int(cr.box_down(np.array(vals, np.uint8).reshape(shape), sub)[0, 0])
    assert one([0, 1], (2, 1), (1, 2)) == 1
    assert one([0, 0, 0, 1], (2, 2), (2, 2)) == 0
    assert one([0, 0, 1, 1], (2, 2), (2, 2)) == 1
    assert one([255] * 4, (2, 2), (2, 2)) == 255
    assert one([0, 1, 1, 1], (2, 2), (2, 2)) == 1
    assert one([254, 255], (2, 1), (1, 2)) == 255


def test_box_down_edge_blocks_average_the_pixels_that_exist():
    p = np.array([[10, 20, 31],
                  [30, 40, 60],
                  [51, 70, 90]], np.uint8)
    # 2 x 2: a full block, a right-edge column pair, a bottom-edge row pair, the single corner pixel
    assert cr.box_down(p, (2, 2)).tolist() == [[25, 46], [61, 90]]
    # 2 x 1: the last column stands alone in every row
    assert cr.box_down(p, (2, 1)).tolist() == [[15, 31], [35, 60], [61, 90]]
    assert np.array_equal(cr.box_down(p, (1, 1)), p)


def test_sub_1x1_is_the_oracles_plain_conversion():
    rng = np.random.default_rng(12)
    H, W = 5, 7
    frames = rng.integers(0, 256, (2, 3 * H * W), dtype=np.uint8)
    y, cb, crr = cr.split_frames(frames, H, W, (1, 1))
    bgr = cr.decode_frames(frames, H, W, (1, 1))
    assert np.array_equal(np.moveaxis(bgr, 1, -1), o.ycrcb_to_bgr(np.stack([y, crr, cb], axis=-1)))
    planes = rng.integers(0, 256, (2, 3, H, W), dtype=np.uint8)
    ycc = o.bgr_to_ycrcb(np.moveaxis(planes, 1, -1))
    want = np.concatenate([ycc[..., 0].reshape(2, -1), ycc[..., 2].reshape(2, -1), ycc[..., 1].reshape(2, -1)], axis=1)
    assert np.array_equal(cr.encode_frames(planes, (1, 1)), want)


@pytest.mark.parametrize("sub", cr.SUBS)
def test_frame_layout_and_chroma_round_trip(sub):
    """decode -> encode gives the stored chroma back exactly (whatever the clipping does to Y)"""
    rng = np.random.default_rng(13)
    H, W = 5, 7
    frames = rng.integers(0, 256, (3, cr.frame_bytes(H, W, sub)), dtype=np.uint8)
    planes = cr.decode_frames(frames, H, W, sub)
    assert planes.shape == (3, 3, H, W) and planes.dtype == np.uint8
    back = cr.encode_frames(planes, sub)
    assert back.shape == frames.shape
    # in gamut (no channel clipped anywhere in the block) the chroma comes back as stored
    y, cb, crr = cr.split_frames(frames, H, W, sub)
    smooth = np.concatenate([y.reshape(3, -1), np.full((3, frames.shape[1] - H * W), 128, np.uint8)], axis=1)
    assert np.array_equal(cr.encode_frames(cr.decode_frames(smooth, H, W, sub), sub), smooth)


def test_meta_places_chroma_after_n_frames_and_omits_it_when_unset():
    M = importlib.import_module(PKG_NAME + ".meta")
    z = np.zeros(3, np.float32)
    base = {"mode": "video_color", **M.common_members(64, 96, 0.1, 0.6, bytes(8)), **M.video_members(2, 5, 8, 8),
            **M.channel_members([z] * 3, [z] * 3, [z] * 3, [z] * 3)}
    plain = list(M.sealed(base, 8, bytes(32)))
    assert "chroma" not in plain
    assert M.chroma_members("444") == {} and M.chroma_members("420jpeg") == {"chroma": "420"}
    assert M.chroma_members("420mpeg2") == {"chroma": "420"} and M.chroma_members("422") == {"chroma": "422"}
    for tile in (8, None):
        keys = list(M.sealed(dict(base, **M.chroma_members("420paldv")), tile, bytes(32)))
        assert keys[keys.index("n_frames") + 1] == "chroma"
        assert [k for k in keys if k != "chroma"] == list(M.sealed(base, tile, bytes(32)))      # nothing else moved
    assert M.chroma_of({"chroma": np.array("422")}) == "422" and M.chroma_of({}) == "444"
    # the HMAC covers the factor arrays only: the member does not change it
    assert len(M.hmac_parts(dict(base, chroma="420"))) == len(M.hmac_parts(base)) == 9


def test_subsampling_keyword_is_checked_without_a_device(tmp_path):
    v = importlib.import_module(PKG_NAME + ".video")
    args = (str(tmp_path / "none.y4m"), str(tmp_path / "none.png"), str(tmp_path / "o.y4m"), str(tmp_path / "m.npz"))
    with pytest.raises(ValueError, match="subsampling"):
        v.embed_watermark_video_color(*args, password="pw", subsampling="bogus")
    with pytest.raises(TypeError):
        v.embed_watermark_video_color(*args, 0.1, 1, "box")                   # keyword-only
