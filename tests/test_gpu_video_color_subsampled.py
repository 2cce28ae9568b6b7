"""Colour video on 4:2:0 / 4:2:2 .y4m containers (embed_watermark_video_color(subsampling="box")): the stored frames are the
NumPy codec (tests/chroma_refs.py) of the embedded planes bit for bit, the embedded planes are held per plane to the oracle,
and detect / extract equal the oracle chain run on the decoded stored frames."""
import importlib

import numpy as np
import pytest

import chroma_refs as cr
from conftest import PKG_NAME
from oracle import wm_oracle as o
from test_video import _bgr_of, _video444

ALPHA, KFRAC = 0.15, 0.6
CONTAINERS = (("420jpeg", 64, 96), ("422", 64, 96), ("420", 45, 70))      # the last: odd sizes, a ragged tile border


def _source_clip(tmp_path, v, tag, H, W):
    """5 frames of the 4:4:4 test's generator, stored with this container's subsampling"""
    sub = v._CHROMA_DIV[tag]
    _, _, ys, chroma = _video444(tmp_path, n=5, H=H, W=W)
    bgr = np.stack([np.moveaxis(_bgr_of(ys[i], chroma[i]), -1, 0) for i in range(5)])
    frames = cr.encode_frames(bgr, sub)
    p = str(tmp_path / f"in{tag}.y4m")
    v.write_y4m(p, frames[:, :H * W].reshape(5, H, W), frames[:, H * W:], chroma_tag=tag)
    return p, frames, sub


def _read_frames(v, path):
    vid = v.Y4M(path)
    got = [np.concatenate([y.ravel(), c]) for _, y, c in vid]
    vid.close()
    return vid, np.stack(got)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [8, None])
@pytest.mark.parametrize("tag,H,W", CONTAINERS)
def test_video_color_subsampled(tmp_path, gpu_ctx, tag, H, W, tile):
    """The extracted PNG is held to the oracle chain on the stored frames within 2 grey levels, the bar
    test_video_fullframe_mode uses for the same chain.  For tile=8 that bar had not been run before this test; measured
    on an MI355X over the three containers: at most 1 grey level, on at most 3.3e-4 of a channel's pixels (tile=None:
    1 on 1.6e-4), so the bar of 2 stands.  The figures are printed ahead of the assertions."""
    v = importlib.import_module(PKG_NAME + ".video")
    M = importlib.import_module(PKG_NAME + ".meta")
    hg = importlib.import_module(PKG_NAME + ".hostglue")
    src_path, src, sub = _source_clip(tmp_path, v, tag, H, W)
    fmt = tag[:3]
    wm = np.random.default_rng(5).integers(0, 256, (16, 24, 3), dtype=np.uint8)
    wp = str(tmp_path / "wmc.png"); assert hg.write_png(wp, wm)
    key = o.derive_key("pw", bytes(8)); idx = o.permutation(H, W, o.rng_from_key(key))
    wm_r = o.resize_area(wm, W, H)
    w_s = [o.permute(wm_r[..., c].astype(np.float32), idx) for c in range(3)]
    wm_svd = [o.watermark_decompose(w, tile) for w in w_s]

    outp, meta, ps = v.embed_watermark_video_color(src_path, wp, str(tmp_path / "out.y4m"), str(tmp_path / "m.npz"),
                                                   alpha=ALPHA, frame_interval=2, password="pw", nonce=bytes(8), batch=2,
                                                   tile=tile, subsampling="box")
    assert 15 < ps < 60
    vid, got = _read_frames(v, outp)
    assert vid.header_line == open(src_path, "rb").readline() and vid.chroma == tag and got.shape == src.shape

    # 1. the planes as embedded, per plane against the oracle (the 4:4:4 test's bars); the stored frames are their codec
    planes = cr.decode_frames(src[::2], H, W, sub)
    Uw, Sw, Vwt, _ = v.prepare_watermark_color(gpu_ctx, wm, H, W, key, tile)
    K = 8 if tile else max(8, int(KFRAC * min(H, W)))
    st, sc = v.embed_frames_color(gpu_ctx, planes, Sw, ALPHA, K, batch=2, tile=tile)
    for j in range(3):
        for c in range(3):
            ref = o.embed_plane(planes[j, c].astype(np.float32), w_s[c], ALPHA, KFRAC, tile, wm_svd=wm_svd[c] if tile else None)
            assert np.abs(st[j, c].astype(int) - ref["stego"].astype(int)).max() <= 1
            assert np.mean(st[j, c] != ref["stego"]) < 5e-3
            assert np.max(np.abs(sc[c][j] - ref["Sc"])) / np.max(ref["Sc"]) < 1e-4
    assert np.array_equal(got[::2], cr.encode_frames(st, sub))
    # 2. unmarked frames byte for byte
    assert np.array_equal(got[1::2], src[1::2])
    # 3. the meta
    data = np.load(meta, allow_pickle=False)
    assert str(data["mode"]) == "video_color" and str(data["chroma"]) == fmt and int(data["n_frames"]) == 5
    assert data.files[data.files.index("n_frames") + 1] == "chroma"
    for c, n in enumerate("bgr"):
        assert data["S" + n].shape[0] == 3 and np.array_equal(data["S" + n], sc[c])

    # 4. detect: the oracle's score on the decoded stored frames with the meta's own arrays
    stored = cr.decode_frames(got[::2], H, W, sub)
    ok, mean, scores = v.detect_watermark_video_color(outp, meta)
    assert ok and mean > 0.9 and scores.shape == (3,)
    for j in range(3):
        want = np.mean([o.detect_plane(stored[j, c].astype(np.float32), data["S" + n][j], data["SW" + n], ALPHA, tile)
                        for c, n in enumerate("bgr")])
        print(f"detect {tag} tile={tile} frame {j}: {scores[j]:.6f} oracle {want:.6f}")
        assert abs(scores[j] - want) < 1e-4
    # 5. the source clip
    ok0, mean0, _ = v.detect_watermark_video_color(src_path, meta)
    print(f"detect {tag} tile={tile}: marked {mean:.4f} unmarked {mean0:.4f}")
    assert not ok0

    # 6. extract: per-frame oracle extract from the decoded stored planes, mean, unpermute, min-max normalise
    wout = v.extract_watermark_video_color(outp, meta, str(tmp_path / "w.png"), password="pw")
    ex = hg.read_image_bgr(wout)
    assert ex.shape == (H, W, 3)
    for c, n in enumerate("bgr"):
        est = np.mean([o.extract_plane(stored[j, c].astype(np.float32), data["S" + n][j], data["UW" + n], data["VW" + n + "t"],
                                       ALPHA, KFRAC, H, W, tile) for j in range(3)], axis=0)
        want = np.clip(o.normalize_minmax(o.unpermute(est.astype(np.float32), idx)), 0, 255).astype(np.uint8)
        diff = np.abs(ex[..., c].astype(int) - want.astype(int))
        corr = np.corrcoef(ex[..., c].ravel().astype(float), wm_r[..., c].ravel().astype(float))[0, 1]
        print(f"extract {tag} tile={tile} channel {n}: max diff {diff.max()} on {np.mean(diff > 0):.2e} of pixels, corr {corr:.3f}")
        assert diff.max() <= 2
        if (H, W) == (64, 96):
            assert corr > 0.6
    # 7. wrong password
    with pytest.raises(ValueError, match="Sai mật khẩu"):
        v.extract_watermark_video_color(outp, meta, str(tmp_path / "x.png"), password="nope")

    # 8. a meta that names another chroma format (re-sealed with the same digest: the HMAC covers the factors only, so
    #    it still authenticates) is refused with both formats named
    other = "422" if fmt == "420" else "420"
    members = {k: data[k] for k in data.files if k != "digest"}
    members.update(mode=str(data["mode"]), chroma=other)
    meta2 = str(tmp_path / "m2.npz")
    np.savez(meta2, **M.sealed(members, tile, M.digest_of(data)))
    assert M.authentic(np.load(meta2, allow_pickle=False), key)
    for call in (lambda: v.detect_watermark_video_color(outp, meta2),
                 lambda: v.extract_watermark_video_color(outp, meta2, str(tmp_path / "y.png"), password="pw")):
        with pytest.raises(ValueError, match=f"C{other}.*C{tag}"):
            call()
    # 9. the default still refuses the container
    with pytest.raises(ValueError, match="4:4:4"):
        v.embed_watermark_video_color(src_path, wp, str(tmp_path / "o2.y4m"), str(tmp_path / "m3.npz"), password="pw")
