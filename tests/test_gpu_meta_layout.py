"""GPU test: what the six meta writers put into the .npz - member names in file order, dtype and shape of every member,
and the keys that must be absent - against a table written out here, on the smallest shapes that still have more than one
tile per side, a non-square plane (L = min(H, W) < max), a resized logo and more than one flush of the video loop.
Structural: no numeric bar.  Then the round trip: extract with the right password succeeds, a wrong one raises the
reference's text (single:208-209, 246-247)."""
import importlib
import zipfile

import numpy as np
import pytest

from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

WRONG = "Sai mật khẩu hoặc meta không khớp."
F, I32, I64, F64, U8 = "<f4", "<i4", "<i8", "<f8", "|u1"

# ---- images: cover 24 x 40 (3 x 5 tiles, L = 24), logo 9 x 13 ----------------------------------------------------------
_COMMON = [("payload_type", "<U5", ()), ("shape", I64, (2,)), ("alpha", F64, ()), ("kfrac", F64, ()), ("nonce", U8, (8,))]
_TILE_KEYS = [("tile", I32, ()), ("k_floor", I32, ())]
_DIGEST = [("digest", U8, (32,))]
_T_S, _T_UV = (3, 5, 8), (3, 5, 8, 8)
_F_S, _F_U, _F_V = (24,), (24, 24), (24, 40)

IMAGE = {
    ("gray", 8, 8): [("mode", "<U4", ()), ("Sc", F, _T_S), ("Uw", F, _T_UV), ("Vwt", F, _T_UV), ("Sw", F, _T_S)]
                    + _COMMON + _TILE_KEYS + _DIGEST,
    ("gray", None, 8): [("mode", "<U4", ()), ("Sc", F, _F_S), ("Uw", F, _F_U), ("Vwt", F, _F_V), ("Sw", F, _F_S)]
                       + _COMMON + _DIGEST,
    ("color", 8, 8): [("mode", "<U5", ())] + _COMMON + _TILE_KEYS
                     + [("Sb", F, _T_S), ("UWb", F, _T_UV), ("VWbt", F, _T_UV), ("SWb", F, _T_S),
                        ("Sg", F, _T_S), ("UWg", F, _T_UV), ("VWgt", F, _T_UV), ("SWg", F, _T_S),
                        ("Sr", F, _T_S), ("UWr", F, _T_UV), ("VWrt", F, _T_UV), ("SWr", F, _T_S)] + _DIGEST,
    ("color", None, 8): [("mode", "<U5", ())] + _COMMON
                        + [("UWb", F, _F_U), ("VWbt", F, _F_V), ("SWb", F, _F_S),
                           ("UWg", F, _F_U), ("VWgt", F, _F_V), ("SWg", F, _F_S),
                           ("UWr", F, _F_U), ("VWrt", F, _F_V), ("SWr", F, _F_S),
                           ("Sb", F, _F_S), ("Sg", F, _F_S), ("Sr", F, _F_S)] + _DIGEST,
    ("color", None, 5): [("mode", "<U5", ())] + _COMMON + [("k_floor", I32, ())]
                        + [("UWb", F, _F_U), ("VWbt", F, _F_V), ("SWb", F, _F_S),
                           ("UWg", F, _F_U), ("VWgt", F, _F_V), ("SWg", F, _F_S),
                           ("UWr", F, _F_U), ("VWrt", F, _F_V), ("SWr", F, _F_S),
                           ("Sb", F, _F_S), ("Sg", F, _F_S), ("Sr", F, _F_S)] + _DIGEST,
}

# ---- videos: 3 frames of 16 x 24 (2 x 3 tiles, L = 16), frame_interval 2: frames 0 and 2 are marked ---------------------
_V_TAIL = [("shape", I64, (2,)), ("alpha", F64, ()), ("kfrac", F64, ()), ("frame_interval", I32, ()), ("n_frames", I32, ()),
           ("tile", I32, ()), ("k_floor", I32, ()), ("nonce", U8, (8,)), ("digest", U8, (32,))]
_VT_SC, _VT_S, _VT_UV = (2, 2, 3, 8), (2, 3, 8), (2, 3, 8, 8)
_VF_SC, _VF_S, _VF_U, _VF_V = (2, 16), (16,), (16, 16), (16, 24)

VIDEO = {
    ("video_gray", 8): [("mode", "<U10", ()), ("payload_type", "<U5", ()),
                        ("Sc", F, _VT_SC), ("Uw", F, _VT_UV), ("Vwt", F, _VT_UV), ("Sw", F, _VT_S)] + _V_TAIL,
    ("video_gray", None): [("mode", "<U10", ()), ("payload_type", "<U5", ()),
                           ("Sc", F, _VF_SC), ("Uw", F, _VF_U), ("Vwt", F, _VF_V), ("Sw", F, _VF_S)] + _V_TAIL,
    ("video_color", 8): [("mode", "<U11", ()), ("payload_type", "<U5", ())] + _V_TAIL
                        + [("Sb", F, _VT_SC), ("UWb", F, _VT_UV), ("VWbt", F, _VT_UV), ("SWb", F, _VT_S),
                           ("Sg", F, _VT_SC), ("UWg", F, _VT_UV), ("VWgt", F, _VT_UV), ("SWg", F, _VT_S),
                           ("Sr", F, _VT_SC), ("UWr", F, _VT_UV), ("VWrt", F, _VT_UV), ("SWr", F, _VT_S)],
    ("video_color", None): [("mode", "<U11", ()), ("payload_type", "<U5", ())] + _V_TAIL
                           + [("Sb", F, _VF_SC), ("UWb", F, _VF_U), ("VWbt", F, _VF_V), ("SWb", F, _VF_S),
                              ("Sg", F, _VF_SC), ("UWg", F, _VF_U), ("VWgt", F, _VF_V), ("SWg", F, _VF_S),
                              ("Sr", F, _VF_SC), ("UWr", F, _VF_U), ("VWrt", F, _VF_V), ("SWr", F, _VF_S)],
}


def members(path):
    """[(name, dtype, shape)] in the order of the archive's directory, which is the order they were written in."""
    with zipfile.ZipFile(path) as z:
        order = [n[:-4] for n in z.namelist()]
    with np.load(path, allow_pickle=False) as d:
        assert sorted(order) == sorted(d.files)
        return [(k, d[k].dtype.str, d[k].shape) for k in order], {k: d[k] for k in order}


@pytest.fixture(scope="module")
def core(gpu_ctx):
    import dct_svd_core_secure as c
    return c


@pytest.fixture(scope="module")
def hg():
    return importlib.import_module(PKG_NAME + ".hostglue")


@pytest.fixture(scope="module")
def files(tmp_path_factory, hg):
    d = tmp_path_factory.mktemp("layout")
    rng = np.random.default_rng(11)
    cover, logo = str(d / "cover.png"), str(d / "logo.png")
    assert hg.write_png(cover, rng.integers(0, 256, (24, 40, 3), dtype=np.uint8))
    assert hg.write_png(logo, rng.integers(0, 256, (9, 13, 3), dtype=np.uint8))
    return d, cover, logo


@pytest.mark.parametrize("mode,tile,k_floor", sorted(IMAGE, key=str))
def test_image_meta_layout(core, files, mode, tile, k_floor):
    d, cover, logo = files
    tag = f"{mode}_{tile}_{k_floor}"
    out, mp, ps, ss = core.embed(cover, logo, str(d / f"{tag}.png"), str(d / f"{tag}.npz"), alpha=0.1,
                                 color=(mode == "color"), password="pw", tile=tile, k_floor=k_floor, nonce=bytes(range(8)))
    got, data = members(mp)
    assert got == IMAGE[(mode, tile, k_floor)]
    assert str(data["mode"]) == mode and str(data["payload_type"]) == "image"
    assert data["shape"].tolist() == [24, 40] and data["nonce"].tolist() == list(range(8))
    if tile is None:
        assert "tile" not in data                      # exactly the reference's keys (single:157-166, 183-189) ...
        assert ("k_floor" in data) == (k_floor != 8)   # ... unless k_floor differs from the literal 8 of single:174
    else:
        assert int(data["tile"]) == 8
    if "k_floor" in data:
        assert int(data["k_floor"]) == k_floor
    wm = core.extract(out, mp, str(d / f"{tag}_wm.png"), "pw")
    assert wm.endswith("_wm.png")
    with pytest.raises(ValueError) as e:
        core.extract(out, mp, str(d / f"{tag}_bad.png"), "pw2")
    assert str(e.value) == WRONG


@pytest.mark.parametrize("mode,tile", sorted(VIDEO, key=str))
def test_video_meta_layout(gpu_ctx, files, hg, mode, tile):
    d, _, logo = files
    v = importlib.import_module(PKG_NAME + ".video")
    rng = np.random.default_rng(12)
    ys = rng.integers(0, 256, (3, 16, 24), dtype=np.uint8)
    tag = f"{mode}_{tile}"
    src = str(d / f"{tag}_in.y4m")
    if mode == "video_color":
        v.write_y4m(src, ys, rng.integers(0, 256, (3, 2 * 16 * 24), dtype=np.uint8), chroma_tag="444")
        embed, extract = v.embed_watermark_video_color, v.extract_watermark_video_color
    else:
        v.write_y4m(src, ys, rng.integers(0, 256, (3, 2 * 8 * 12), dtype=np.uint8))
        embed, extract = v.embed_watermark_video, v.extract_watermark_video
    # batch = 1: a flush per frame_interval frames, so the two marked frames come from two flushes
    out, mp, ps = embed(src, logo, str(d / f"{tag}_out.y4m"), str(d / f"{tag}.npz"), alpha=0.1, frame_interval=2,
                        password="pw", nonce=bytes(range(8)), batch=1, tile=tile)
    got, data = members(mp)
    assert got == VIDEO[(mode, tile)]
    assert str(data["mode"]) == mode and str(data["payload_type"]) == "image"
    assert int(data["tile"]) == (tile or 0)            # video metas always name the tile; 0 is full-frame
    assert int(data["frame_interval"]) == 2 and int(data["n_frames"]) == 3 and int(data["k_floor"]) == 8
    assert data["shape"].tolist() == [16, 24] and data["nonce"].tolist() == list(range(8))
    with zipfile.ZipFile(mp) as z:                     # np.savez: stored, not deflated
        assert {i.compress_type for i in z.infolist()} == {zipfile.ZIP_STORED}
    wm = extract(out, mp, str(d / f"{tag}_wm"), "pw")
    assert wm.endswith("_wm.png")
    with pytest.raises(ValueError) as e:
        extract(out, mp, str(d / f"{tag}_bad.png"), "pw2")
    assert str(e.value) == WRONG
