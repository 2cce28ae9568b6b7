"""Resize resynchronisation of the blind payload on the device: the resampler against the NumPy restatement bit for bit
(tests/resample_refs.py), and search="resize" end to end on images and on a .y4m.  Every shape is tiny.

No kernel caps its grid or chunks a loop; a workgroup of k_resample_h and of k_resample_h_lds covers RS_NT * RS_H_PX = 1024
output columns and one of k_resample_v RS_NT * RS_V_PX = 4096, and test_more_than_one_workgroup_across crosses both (the
staging loops of k_resample_h_lds run RS_NT = 256 bytes a trip and take several trips at every shape wider than that)."""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import mask_refs as mr
import resample_refs as rr
from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

core = importlib.import_module(ge.PKG_NAME + ".dct_svd_core_secure")
video = importlib.import_module(ge.PKG_NAME + ".video")


def _plane(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


# ---- the resampler, bit for bit --------------------------------------------------------------------------------------
# (1 x 1 <-> 9 x 9 lie beyond the rule's 8x and are refused - 9 -> 1 would take 37 taps, the ABI takes 33; 1 <-> 8 are the
# one-sample shapes the rule admits)
SHAPES = (((1, 1), (8, 8)), ((8, 8), (1, 1)), ((8, 8), (64, 64)), ((64, 64), (8, 8)), ((37, 67), (136, 200)),
          ((136, 200), (37, 67)), ((40, 56), (40, 56)), ((9, 5), (9, 1)), ((9, 5), (11, 3)), ((9, 40), (7, 17)),
          ((21, 100), (30, 67)), ((5, 33), (5, 256)), ((16, 16), (16, 128)))


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resample_equals_the_restatement(gpu_ctx, src, dst):
    p = _plane(*src, seed=src[0] * 131 + dst[1])
    got = gpu_ctx.resample_planes(p, *dst)
    assert got.dtype == np.uint8 and got.shape == dst
    assert np.array_equal(got, rr.resample_ref(p, *dst))


def test_nine_to_one_is_refused(gpu_ctx):
    for src, dst in (((1, 1), (9, 9)), ((9, 9), (1, 1)), ((8, 9), (8, 1))):
        with pytest.raises(ValueError, match="beyond 8x"):
            gpu_ctx.resample_planes(_plane(*src), *dst)


def test_same_size_is_a_byte_copy(gpu_ctx):
    p = _plane(23, 45, seed=5)
    assert np.array_equal(gpu_ctx.resample_planes(p, 23, 45), p)


def test_strided_odd_offset_batch_equals_its_contiguous_copy(gpu_ctx):
    """three planes inside a larger buffer: odd base offset, odd row stride, a plane stride that is no multiple of 16"""
    h, w, rs = 19, 37, 45
    buf = np.random.default_rng(9).integers(0, 256, 7 + 3 * (h * rs + 11), dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[7:], (3, h, w), (h * rs + 11, rs, 1))
    assert view.ctypes.data % 2 == (buf.ctypes.data + 7) % 2 and not view.flags.c_contiguous
    got = gpu_ctx.resample_planes(view, 50, 70)
    dense = np.ascontiguousarray(view)
    assert got.shape == (3, 50, 70)
    assert np.array_equal(got, gpu_ctx.resample_planes(dense, 50, 70))
    assert np.array_equal(got, rr.resample_ref(dense, 50, 70))


def test_no_plane_is_no_launch(gpu_ctx):
    out = gpu_ctx.resample_planes(np.zeros((0, 9, 9), np.uint8), 12, 12)
    assert out.shape == (0, 12, 12)
    gpu_ctx.sync()


def test_both_clips_on_the_device(gpu_ctx):
    """the planes whose accumulators leave 0 .. 255 * 2^14 on both sides in both passes (test_payload_resize asserts that)"""
    under = over = False
    for plane in (rr.checkerboard(), rr.step_edge()):
        for H, W in rr.CLIP_SHAPES:
            ref, acc_h, acc_v = rr.resample_ref(plane, H, W, return_acc=True)
            assert np.array_equal(gpu_ctx.resample_planes(plane, H, W), ref), (H, W)
            under |= bool(acc_v.min() < 0 and acc_h.min() < 0)
            over |= bool(acc_v.max() > 255 << 14 and acc_h.max() > 255 << 14)
    assert under and over


def test_more_than_one_workgroup_across(gpu_ctx):
    """4200 output columns: 5 workgroups of k_resample_h (1024 columns each) and 2 of k_resample_v (4096 each), the last
    of each partly outside the plane"""
    p = _plane(3, 600, seed=11)
    assert np.array_equal(gpu_ctx.resample_planes(p, 5, 4200), rr.resample_ref(p, 5, 4200))
    wide = _plane(2, 4200, seed=12)
    assert np.array_equal(gpu_ctx.resample_planes(wide, 3, 1030), rr.resample_ref(wide, 3, 1030))      # 19 taps: k_resample_h
    assert np.array_equal(gpu_ctx.resample_planes(wide, 3, 1100), rr.resample_ref(wide, 3, 1100))      # 17: the LDS form's most


@pytest.mark.parametrize("W,pitch,offset", ((200, 208, 0), (67, 80, 0), (64, 64, 0), (200, 208, 3), (67, 71, 0)))
def test_device_form_with_padded_and_unaligned_destinations(gpu_ctx, W, pitch, offset):
    """wm_resample_planes_u8_dev itself.  Rows 16-byte multiples apart on an aligned base take 16-byte stores, and the last
    lane of a row, whose 16 columns end outside the plane, bytes; an odd base or pitch takes bytes everywhere.  Nothing
    outside the planes' own columns is written."""
    src = np.stack([_plane(37, 61, seed=s) for s in (1, 2)])
    n, h, w = src.shape
    H = 29
    guard = np.full(offset + n * H * pitch + 16, 0xA5, np.uint8)
    d_src, d_dst = gpu_ctx.malloc(src.nbytes), gpu_ctx.malloc(guard.nbytes)
    try:
        gpu_ctx.h2d(d_src, src); gpu_ctx.h2d(d_dst, guard)
        gpu_ctx.resample_planes_dev(d_src, d_dst + offset, n, h, w, w, h * w, H, W, pitch, H * pitch)
        got = np.empty_like(guard)
        gpu_ctx.d2h(got, d_dst); gpu_ctx.sync()
    finally:
        gpu_ctx.free(d_src); gpu_ctx.free(d_dst)
    rows = got[offset:offset + n * H * pitch].reshape(n, H, pitch)
    assert np.array_equal(rows[:, :, :W], rr.resample_ref(src, H, W))
    assert np.all(rows[:, :, W:] == 0xA5) and np.all(got[:offset] == 0xA5) and np.all(got[offset + n * H * pitch:] == 0xA5)


@pytest.mark.parametrize("dst", ((29, 333), (10, 50), (5, 1100)), ids=lambda s: "x".join(map(str, s)))
def test_device_form_with_tables_off_the_staged_alignment(gpu_ctx, hostapi, dst):
    """k_resample_h_lds wants w on an 8-byte boundary (the cached and the staged tables lie on one); a w two bytes past one
    takes k_resample_h at 5 and 13 taps too (through the binding only the reductions beyond 4x do, with 19 to 33), in two
    workgroups across for the 1100 columns: the same bytes."""
    R = importlib.import_module(ge.PKG_NAME + ".resample")
    src = _plane(37, 150, seed=7)
    h, w = src.shape
    H, W = dst
    (fx, wx), (fy, wy) = R.resample_taps(w, W), R.resample_taps(h, H)
    vp = hostapi._vp
    bufs = [gpu_ctx.malloc(n) for n in (src.nbytes, H * W, fx.nbytes + 16, wx.nbytes + 16, fy.nbytes + 16, wy.nbytes + 16)]
    d_src, d_dst, d_fx, d_wx, d_fy, d_wy = bufs
    try:
        for d, a in ((d_src, src), (d_fx + 4, fx), (d_wx + 2, wx), (d_fy + 4, fy), (d_wy + 2, wy)):
            gpu_ctx.h2d(d, a)
        gpu_ctx._call("wm_resample_planes_u8_dev", vp(d_src), vp(d_dst), 1, h, w, w, h * w, H, W, W, H * W,
                      vp(d_fx + 4), vp(d_wx + 2), wx.shape[1], vp(d_fy + 4), vp(d_wy + 2), wy.shape[1])
        got = np.empty((H, W), np.uint8)
        gpu_ctx.d2h(got, d_dst); gpu_ctx.sync()
        with pytest.raises(ValueError, match="misaligned"):
            gpu_ctx._call("wm_resample_planes_u8_dev", vp(d_src), vp(d_dst), 1, h, w, w, h * w, H, W, W, H * W,
                          vp(d_fx + 4), vp(d_wx + 1), wx.shape[1], vp(d_fy + 4), vp(d_wy + 2), wy.shape[1])
    finally:
        for d in bufs:
            gpu_ctx.free(d)
    assert np.array_equal(got, rr.resample_ref(src, H, W))
    assert np.array_equal(got, gpu_ctx.resample_planes(src, H, W))


# ---- end to end --------------------------------------------------------------------------------------------------------
H, W, SEED = rr.COVER
CONFIGS = {"plain": dict(dither=False, code=None), "dither": dict(dither=True, code=None), "k7": dict(dither=False, code="k7")}
E2E_SIZES = ((102, 150), (170, 250), (204, 120))                           # smaller, larger, the aspect changed
_marked = {}


def _embedded(config: str) -> dict:
    if config not in _marked:
        cover = np.repeat(mr.host(H, W, SEED)[..., None], 3, -1)
        _marked[config] = core.embed_payload_arrays(cover, rr.DATA, rr.PASSWORD, rr.NONCE, delta=rr.DELTA, **CONFIGS[config])
    return _marked[config]


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_resized_stego_decodes(config):
    """the product's stego, every channel resized by an attacker, read back with search="resize": the data, valid, the scale,
    and the confidence of the restatement's decode of the same restored plane to 1e-4 (the keyed-sync test's bar)"""
    r = _embedded(config)
    dither, code = CONFIGS[config]["dither"], int(CONFIGS[config]["code"] is not None)
    for k, size in enumerate(E2E_SIZES):
        attacker = sorted(rr.ATTACKERS)[(k + sorted(CONFIGS).index(config)) % 3]
        attacked = rr.attack_bgr(r["stego"], attacker, *size)
        assert attacked.shape == size + (3,)
        y = np.ascontiguousarray(o.bgr_to_ycrcb(attacked)[..., 0])
        ref = rr.decode_ref(rr.resample_ref(y, H, W), rr.DELTA, dither, code)
        print(f"{config} {attacker} {size}: restatement margin {ref['margin']:.3f} confidence {ref['confidence']:.4f}")
        assert ref["valid"] and ref["data"] == rr.DATA, "the restatement does not decode this case"
        data, valid, conf, scale = core.extract_payload_arrays(attacked, r["meta"], rr.PASSWORD, search="resize")
        assert data == rr.DATA and valid is True
        assert scale == (size[0] / H, size[1] / W)
        assert abs(conf - ref["confidence"]) <= 1e-4, (conf, ref["confidence"])


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_unresized_stego_gives_the_plain_result(config):
    r = _embedded(config)
    plain = core.extract_payload_arrays(r["stego"], r["meta"], rr.PASSWORD)
    got = core.extract_payload_arrays(r["stego"], r["meta"], rr.PASSWORD, search="resize")
    assert got[:3] == plain and got[3] == (1.0, 1.0) and plain[0] == rr.DATA and plain[1] is True


def test_a_resized_stego_without_the_search_is_still_refused():
    r = _embedded("plain")
    attacked = rr.attack_bgr(r["stego"], "rule", 102, 150)
    with pytest.raises(ValueError, match="meta was written for"):
        core.extract_payload_arrays(attacked, r["meta"], rr.PASSWORD)
    for search in ("crop", "crop-keyed"):
        with pytest.raises(ValueError):
            core.extract_payload_arrays(rr.attack_bgr(r["stego"], "rule", 170, 250), r["meta"], rr.PASSWORD, search=search)


def test_files_round_trip(tmp_path):
    hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
    M = importlib.import_module(ge.PKG_NAME + ".meta")
    r = _embedded("dither")
    stego, meta = str(tmp_path / "resized.png"), str(tmp_path / "meta.npz")
    assert hg.write_png(stego, rr.attack_bgr(r["stego"], "area", 170, 250), 0)
    M.save_payload_meta(meta, r["meta"])
    data, valid, conf, written, scale = core.extract_payload(stego, meta, str(tmp_path / "out"), password=rr.PASSWORD, search="resize")
    assert data == rr.DATA and valid and scale == (170 / H, 250 / W) and open(written, "rb").read() == rr.DATA


@pytest.mark.parametrize("dither", (False, True), ids=("plain", "dither"))
def test_resized_video_decodes(tmp_path, dither):
    """4 frames of 72 x 104, every second one marked; all frames resized to 54 x 78 by the restatement and written as .y4m"""
    pre = rr.video_round_trip(dither)                                       # the precondition, on the restatement alone
    assert pre["valid"] and pre["data"] == rr.DATA and pre["margin"] >= rr.MARGIN_FLOOR
    v = rr.VIDEO
    cover, marked, meta, small = (str(tmp_path / n) for n in ("cover.y4m", "marked.y4m", "meta.npz", "small.y4m"))
    video.write_y4m(cover, rr.video_frames())
    video.embed_payload_video(cover, rr.DATA, marked, meta, password=rr.PASSWORD, frame_interval=v["frame_interval"], delta=rr.DELTA,
                              nonce=rr.NONCE, dither=dither)
    vid = video.Y4M(marked)
    frames = np.stack([y.copy() for _, y, _ in vid])
    vid.close()
    assert frames.shape == (v["n_frames"],) + v["shape"]
    video.write_y4m(small, rr.resample_ref(frames, *v["size"]))
    with pytest.raises(ValueError, match="meta was written for"):
        video.extract_payload_video(small, meta, password=rr.PASSWORD)
    data, valid, conf, scale = video.extract_payload_video(small, meta, password=rr.PASSWORD, search="resize")
    assert data == rr.DATA and valid is True and scale == (0.75, 0.75) and conf > 0.5
    same = video.extract_payload_video(marked, meta, password=rr.PASSWORD, search="resize")
    assert same[:3] == video.extract_payload_video(marked, meta, password=rr.PASSWORD) and same[3] == (1.0, 1.0)
