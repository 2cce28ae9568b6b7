"""Rotation resynchronisation of the blind payload on the device: k_rotate_planes against the NumPy restatement bit for bit
(tests/rotate_refs.py), k_payload_angle_scores against NumPy sums of the device's own metrics and the restatement's masks, and
search="rotate" end to end on float-rotated stegos of a 256 x 384 cover.  Every other shape is tiny.

A workgroup of k_rotate_planes makes a 32 x 32 block and a lane 4 adjacent pixels of it; nothing is capped and the only strided
loop, the staging one, takes 12 trips at any angle.  A workgroup of k_payload_angle_scores takes 2048 tiles, 8 trips of 256."""
import importlib
import math

import numpy as np
import pytest

import __graft_entry__ as ge
import mask_refs as mr
import resample_refs as rr
import rotate_refs as rf
from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

core = importlib.import_module(ge.PKG_NAME + ".dct_svd_core_secure")
R = importlib.import_module(ge.PKG_NAME + ".resample")


def _plane(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _cs(*degs):
    return R.angle_candidates_cs([math.radians(d) for d in degs])


def _ref(planes, H, W, cs):
    return np.stack([rf.rotate_ref(planes, H, W, int(C), int(S)) for C, S in cs])


# ---- the rotation, bit for bit -----------------------------------------------------------------------------------------
def test_zero_angle_is_a_byte_copy(gpu_ctx):
    p = _plane(8, 8, seed=1)
    assert np.array_equal(gpu_ctx.rotate_planes(p, 8, 8, _cs(0.0))[0], p)


def test_quarter_turn_is_exact(gpu_ctx):
    p = _plane(24, 24, seed=2)
    assert np.array_equal(gpu_ctx.rotate_planes(p, 24, 24, _cs(90.0))[0], np.rot90(p, 1))


@pytest.mark.parametrize("name", ("checkerboard", "step_edge"))
def test_both_clips_on_the_device(gpu_ctx, name):
    plane = getattr(rr, name)()
    cs = _cs(5.0, 33.0)
    ref = _ref(plane, 24, 40, cs)
    assert (ref == 0).any() and (ref == 255).any()
    assert np.array_equal(gpu_ctx.rotate_planes(plane, 24, 40, cs), ref)


@pytest.mark.parametrize("w", (1, 3, 17, 67))
def test_narrow_sources(gpu_ctx, w):
    p = _plane(9, w, seed=w)
    cs = _cs(0.0, 7.0, -40.0)
    assert np.array_equal(gpu_ctx.rotate_planes(p, 16, 24, cs), _ref(p, 16, 24, cs))


@pytest.mark.parametrize("W", (33, 29, 70), ids=("one past a workgroup", "one past a dword", "three workgroups"))
def test_destination_edges(gpu_ctx, W):
    """33: a second workgroup across with one column; 29: the last lane of a row holds one pixel of its four; 40 x 70: 2 x 3 blocks"""
    p = _plane(40, 60, seed=W)
    cs = _cs(11.0, -45.0)
    assert np.array_equal(gpu_ctx.rotate_planes(p, 40, W, cs), _ref(p, 40, W, cs))


def test_expanded_canvas(gpu_ctx):
    p = _plane(37, 67, seed=5)
    cs = _cs(0.0, 12.5, 45.0)
    assert np.array_equal(gpu_ctx.rotate_planes(p, 24, 40, cs), _ref(p, 24, 40, cs))


def test_strided_odd_offset_batch_equals_its_contiguous_copy(gpu_ctx):
    """two planes inside a larger buffer: odd base offset, odd row stride, an odd plane stride; 3 angles x 2 planes in one call,
    every plane checked"""
    h, w, rs = 19, 37, 45
    buf = np.random.default_rng(9).integers(0, 256, 7 + 2 * (h * rs + 11), dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[7:], (2, h, w), (h * rs + 11, rs, 1))
    assert not view.flags.c_contiguous
    cs = _cs(-3.0, 0.0, 21.0)
    got = gpu_ctx.rotate_planes(view, 24, 40, cs)
    assert got.shape == (3, 2, 24, 40)
    ref = _ref(np.ascontiguousarray(view), 24, 40, cs)
    for a in range(3):
        for p in range(2):
            assert np.array_equal(got[a, p], ref[a, p]), (a, p)


@pytest.mark.parametrize("W,pitch,offset", ((40, 48, 0), (37, 40, 0), (40, 48, 3), (37, 41, 0)))
def test_device_form_with_padded_and_unaligned_destinations(gpu_ctx, hostapi, W, pitch, offset):
    """wm_rotate_planes_u8_dev itself: rows 4-byte multiples apart on an aligned base take dword stores, and the lane whose 4
    columns end outside the plane, bytes; an odd base or pitch takes bytes everywhere.  Nothing outside the planes' own columns
    is written."""
    src = np.stack([_plane(29, 43, seed=s) for s in (1, 2)])
    n, h, w = src.shape
    H, cs, K = 24, _cs(4.0, -17.0), np.ascontiguousarray(R.rotate_weights())
    n_out = n * len(cs)
    guard = np.full(offset + n_out * H * pitch + 16, 0xA5, np.uint8)
    vp = hostapi._vp
    bufs = [gpu_ctx.malloc(b) for b in (src.nbytes, guard.nbytes, cs.nbytes, K.nbytes)]
    d_src, d_dst, d_c, d_K = bufs
    try:
        for d, a in ((d_src, src), (d_dst, guard), (d_c, cs), (d_K, K)):
            gpu_ctx.h2d(d, a)
        gpu_ctx._call("wm_rotate_planes_u8_dev", vp(d_src), vp(d_dst + offset), n, h, w, w, h * w, H, W, pitch, H * pitch, vp(d_c),
                      len(cs), vp(d_K))
        got = np.empty_like(guard)
        gpu_ctx.d2h(got, d_dst); gpu_ctx.sync()
        with pytest.raises(ValueError, match="misaligned"):
            gpu_ctx._call("wm_rotate_planes_u8_dev", vp(d_src), vp(d_dst), n, h, w, w, h * w, H, W, pitch, H * pitch, vp(d_c),
                          len(cs), vp(d_K + 2))
    finally:
        for d in bufs:
            gpu_ctx.free(d)
    rows = got[offset:offset + n_out * H * pitch].reshape(len(cs), n, H, pitch)
    assert np.array_equal(rows[..., :W], _ref(src, H, W, cs))
    assert np.all(rows[..., W:] == 0xA5) and np.all(got[:offset] == 0xA5) and np.all(got[offset + n_out * H * pitch:] == 0xA5)


def test_bad_arguments_are_refused(gpu_ctx):
    p = _plane(8, 8)
    with pytest.raises(ValueError, match="8192"):
        gpu_ctx.rotate_planes(p, 8, 8193, _cs(0.0))
    with pytest.raises(ValueError, match="candidates"):
        gpu_ctx.rotate_planes(p, 8, 8, np.zeros((0, 2), np.int32))
    with pytest.raises(ValueError, match="multiples of 8"):
        gpu_ctx.payload_locate_angle(p, 12, 8, 5.0, 32.0)
    for args in ((0, 8, 8, 8), (8, 8, 8, 12), (8, 8, 8200, 8)):             # (h, w, H, W) the library itself refuses
        with pytest.raises(ValueError):
            gpu_ctx._call("wm_payload_angle_scores", None, None, 1, None, None, None, *args)
    with pytest.raises(ValueError, match="NULL"):
        gpu_ctx._call("wm_payload_angle_scores", None, None, 1, None, None, None, 8, 8, 8, 8)
    with pytest.raises(ValueError, match="n_angles"):
        gpu_ctx._call("wm_rotate_planes_u8", None, None, 1, 8, 8, 8, 64, 8, 8, 8, 64, None, 0, None)


# ---- the scores ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((72, 104), (136, 200), (384, 512)), ids=("117 tiles", "425 tiles", "3072 tiles"))
def test_scores_counts_and_masks(gpu_ctx, shape):
    """A workgroup takes 2048 tiles in 8 trips of 256.  117 tiles: one partly filled trip, a last wave with 53 tiles; 425: a second
    trip that ends inside a wave; 3072: two workgroups, the second half filled.  The candidates' masks differ;
    read against a 10 x 10 source no tile is valid, and every score and count is 0."""
    H, W = shape
    src = mr.host(H, W, 4)
    cs = _cs(0.0, 3.0, -9.0, 40.0)
    restored = gpu_ctx.rotate_planes(src, H, W, cs)
    m = gpu_ctx.payload_metric(restored, 32.0)
    assert m.shape == (4, H // 8, W // 8) and m.dtype == np.float32
    scores, counts, valid = gpu_ctx.payload_angle_scores(m, cs, H, W)
    ref_valid = np.stack([rf.valid_ref(H, W, H, W, int(C), int(S)) for C, S in cs])
    assert np.array_equal(valid, ref_valid)
    assert counts.tolist() == ref_valid.sum(axis=(1, 2)).tolist() and len(set(counts.tolist())) > 1 and counts.min() > 0
    votes = np.rint(np.abs(m).astype(np.float64) * 32768.0).astype(np.int64)
    assert scores.tolist() == [int(votes[a][ref_valid[a]].sum()) for a in range(4)]
    scores, counts, valid = gpu_ctx.payload_angle_scores(m, cs, 10, 10)
    assert not valid.any() and not counts.any() and not scores.any()
    assert not any(rf.valid_ref(H, W, 10, 10, int(C), int(S)).any() for C, S in cs)


# ---- end to end --------------------------------------------------------------------------------------------------------
H, W, SEED = rf.COVER
CONFIGS = {"plain": dict(dither=False, code=None), "dither": dict(dither=True, code=None), "k7": dict(dither=True, code="k7")}
E2E = (("plain", "bilinear", False, 1.0), ("dither", "cubic", False, 3.0), ("dither", "bilinear", True, -7.3), ("k7", "cubic", True, 3.0))
_marked = {}


def _embedded(config: str) -> dict:
    if config not in _marked:
        cover = np.repeat(mr.host(H, W, SEED)[..., None], 3, -1)
        _marked[config] = core.embed_payload_arrays(cover, rr.DATA, rr.PASSWORD, rr.NONCE, delta=rf.DELTA, **CONFIGS[config])
    return _marked[config]


def _attack_bgr(bgr, deg, kind, expand):
    return np.stack([rf.rotate_float(np.ascontiguousarray(bgr[..., c]), deg, kind, expand) for c in range(3)], axis=-1)


@pytest.mark.parametrize("config,kind,expand,deg", E2E, ids=[f"{c}-{k}-{'expanded' if e else 'same'}-{d}" for c, k, e, d in E2E])
def test_rotated_stego_decodes(config, kind, expand, deg):
    """the product's stego, every channel rotated by a float attacker, read back with search="rotate": the data, valid, the
    angle within one fine step of the restatement's winner on the same luma, the confidence within 1e-3 of the restatement's"""
    r = _embedded(config)
    dither, code = CONFIGS[config]["dither"], int(CONFIGS[config]["code"] is not None)
    attacked = _attack_bgr(r["stego"], deg, kind, expand)
    assert attacked.shape[:2] == (rf.expanded_shape(H, W, deg) if expand else (H, W))
    y = np.ascontiguousarray(o.bgr_to_ycrcb(attacked)[..., 0])
    ref = rf.search_plane_ref(y, H, W, rf.DELTA, dither, rf.MAX_ANGLE, code)
    print(f"{config} {kind} {deg}: restatement angle {ref['angle']:.4f} score {ref['score']:.4f} far {ref['far']:.4f} confidence "
          f"{ref['confidence']:.4f} wrong bits {ref['wrong_bits']}")
    assert ref["valid"] and ref["data"] == rr.DATA, "the restatement does not decode this case"
    data, valid, conf, angle = core.extract_payload_arrays(attacked, r["meta"], rr.PASSWORD, search="rotate", max_angle=rf.MAX_ANGLE)
    print(f"device angle {angle:.4f} confidence {conf:.4f}")
    assert data == rr.DATA and valid is True
    assert abs(angle - ref["angle"]) <= math.degrees(ref["step"] / 8) * (1 + 1e-9)
    assert abs(angle - deg) <= math.degrees(ref["step"])
    assert abs(conf - ref["confidence"]) <= 1e-3, (conf, ref["confidence"])


def test_unrotated_stego_comes_back_at_the_zero_candidate():
    """theta = 0 is the identity, but the border tiles' windows leave the source and do not vote: the confidence is the
    restatement's of the same search, below the plain extract's"""
    r = _embedded("dither")
    y = np.ascontiguousarray(o.bgr_to_ycrcb(r["stego"])[..., 0])
    ref = rf.search_plane_ref(y, H, W, rf.DELTA, True, 2.0)
    assert ref["valid"] and ref["theta"] == 0.0 and ref["valid_tiles"] == (H // 8 - 2) * (W // 8 - 2)
    data, valid, conf, angle = core.extract_payload_arrays(r["stego"], r["meta"], rr.PASSWORD, search="rotate", max_angle=2.0)
    assert data == rr.DATA and valid is True and angle == 0.0
    assert abs(conf - ref["confidence"]) <= 1e-3, (conf, ref["confidence"])
    assert conf < core.extract_payload_arrays(r["stego"], r["meta"], rr.PASSWORD)[2]


def test_files_round_trip(tmp_path):
    hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
    M = importlib.import_module(ge.PKG_NAME + ".meta")
    r = _embedded("plain")
    stego, meta = str(tmp_path / "rotated.png"), str(tmp_path / "meta.npz")
    assert hg.write_png(stego, _attack_bgr(r["stego"], 3.0, "bilinear", False), 0)
    M.save_payload_meta(meta, r["meta"])
    data, valid, conf, written, angle = core.extract_payload(stego, meta, str(tmp_path / "out"), password=rr.PASSWORD, search="rotate",
                                                             max_angle=5.0)
    assert data == rr.DATA and valid and abs(angle - 3.0) < 0.25 and open(written, "rb").read() == rr.DATA


def test_chunked_candidates_give_the_same_result(gpu_ctx, monkeypatch):
    """the search with one restored plane a chunk (ROTATE_PLANE_BYTES below two planes) against the default single chunk"""
    r = _embedded("plain")
    y = np.ascontiguousarray(o.bgr_to_ycrcb(_attack_bgr(r["stego"], 1.0, "bilinear", False))[..., 0])
    whole = gpu_ctx.payload_locate_angle(y, H, W, 2.0, rf.DELTA)
    monkeypatch.setattr(type(gpu_ctx), "ROTATE_PLANE_BYTES", H * W)
    parts = gpu_ctx.payload_locate_angle(y, H, W, 2.0, rf.DELTA)
    assert whole[0] == parts[0] and np.array_equal(whole[1], parts[1]) and np.array_equal(whole[2], parts[2])
    for a, b in zip(whole[3], parts[3]):
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4]


def test_the_refusals_raise_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call before the refusal")
    r = _embedded("plain")
    monkeypatch.setattr(core, "_ctx", no_device)
    for kw in (dict(search="rotate", max_angle=0.0), dict(search="rotate", max_angle=46.0), dict(search="resize", max_angle=5.0),
               dict(search=None, max_angle=5.0)):
        with pytest.raises(ValueError, match="max_angle"):
            core.extract_payload_arrays(r["stego"], r["meta"], rr.PASSWORD, **kw)
    with pytest.raises(ValueError, match="8192"):
        core.extract_payload_arrays(np.zeros((8200, 8, 3), np.uint8), r["meta"], rr.PASSWORD, search="rotate")
    with pytest.raises(ValueError, match=r"uint8 \[h, w, 3\]"):
        core.extract_payload_arrays(r["stego"][..., 0], r["meta"], rr.PASSWORD, search="rotate")
