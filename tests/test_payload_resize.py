"""Resize resynchronisation of the blind payload, without a device: the product's tap tables against the restatement's
(tests/resample_refs.py), the filter's invariants on the restatement, the signal the GPU tests rely on, and the refusals."""
import importlib
import math

import numpy as np
import pytest

import __graft_entry__ as ge
import resample_refs as rr

R = importlib.import_module(ge.PKG_NAME + ".resample")
M = importlib.import_module(ge.PKG_NAME + ".meta")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
core = importlib.import_module(ge.PKG_NAME + ".dct_svd_core_secure")
video = importlib.import_module(ge.PKG_NAME + ".video")
hostapi = importlib.import_module(ge.PKG_NAME + ".hostapi")


# ---- the tap tables --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", rr.TAP_CASES)
def test_taps_equal_the_restatement(n_in, n_out):
    first, w = R.resample_taps(n_in, n_out)
    rf, rw = rr.taps_ref(n_in, n_out)
    assert first.dtype == np.int32 and w.dtype == np.int16
    assert np.array_equal(first, rf) and np.array_equal(w, rw)
    T = 2 * math.ceil(2.0 * max(n_in / n_out, 1.0)) + 1
    assert w.shape == (n_out, T) and first.shape == (n_out,) and T <= R.MAX_TAPS == 33
    assert np.all(w.astype(np.int64).sum(axis=1) == 1 << 14)
    assert first.min() >= 0 and np.all(first < n_in)
    used = (w != 0).cumsum(axis=1).argmax(axis=1)                           # the last tap with a weight
    assert np.all(first + used <= n_in - 1), "a weighted tap reads past the source: the clamp would move weight"
    assert int(np.abs(w.astype(np.int64)).sum(axis=1).max()) * 255 < 1 << 23


def test_same_size_is_the_identity():
    first, w = R.resample_taps(7, 7)
    assert w.shape == (7, 5)
    for i in range(7):
        assert w[i].tolist().count(1 << 14) == 1 and np.count_nonzero(w[i]) == 1
        assert first[i] + int(np.argmax(w[i])) == i
    p = np.random.default_rng(0).integers(0, 256, (7, 7), dtype=np.uint8)
    assert np.array_equal(rr.resample_ref(p, 7, 7), p)


def test_eight_to_one_takes_all_33_taps():
    assert R.resample_taps(64, 8)[1].shape[1] == 33 and R.resample_taps(8, 64)[1].shape[1] == 5
    assert R.MAX_SCALE == 8


@pytest.mark.parametrize("value", (0, 1, 127, 254, 255))
def test_a_constant_plane_stays_constant(value):
    p = np.full((40, 56), value, np.uint8)
    for H, W in ((64, 96), (5, 7), (40, 57), (320, 448)):
        out, acc_h, acc_v = rr.resample_ref(p, H, W, return_acc=True)
        assert np.all(out == value), (value, H, W)
        assert np.all(acc_h == value << 14) and np.all(acc_v == value << 14)


def test_checkerboard_and_step_reach_both_clips():
    """The kernel's clip to 0..255 on both sides: some accumulator is negative and some exceeds 255 * 2^14, in each pass,
    so neither clip can be left out unnoticed."""
    lo_h = hi_h = lo_v = hi_v = False
    for plane in (rr.checkerboard(), rr.step_edge()):
        for H, W in rr.CLIP_SHAPES:
            out, acc_h, acc_v = rr.resample_ref(plane, H, W, return_acc=True)
            lo_h |= bool(acc_h.min() < 0); hi_h |= bool(acc_h.max() > 255 << 14)
            lo_v |= bool(acc_v.min() < 0); hi_v |= bool(acc_v.max() > 255 << 14)
            assert out.shape == (H, W) and out.dtype == np.uint8
            unclipped = (acc_v + (1 << 13)) >> 14
            assert np.array_equal(out, np.clip(unclipped, 0, 255))
    assert lo_h and hi_h and lo_v and hi_v


# ---- the signal: what the GPU tests rely on, on the restatement alone ------------------------------------------------------
@pytest.mark.parametrize("dither", (False, True), ids=("plain", "dither"))
def test_round_trips_decode_at_delta_32(dither):
    """9 sizes x 3 attackers: resized by the attacker, restored by the rule, decoded.  Every case is valid and equal with a
    margin min_j |soft_j| / count_j of at least 0.15 (the device's sigma differs from the oracle's by 1e-4 relative, which
    moves a margin by far less than that)."""
    worst = 1.0
    for attacker in rr.ATTACKERS:
        for size in rr.SIZES:
            r = rr.round_trip(rr.COVER, rr.DELTA, dither, attacker, size)
            print(f"delta 32 dither {int(dither)} {attacker:8s} {size}: margin {r['margin']:.3f} confidence {r['confidence']:.3f}")
            assert r["valid"] and r["data"] == rr.DATA, (attacker, size)
            assert r["margin"] >= rr.MARGIN_FLOOR, (attacker, size, r["margin"])
            worst = min(worst, r["margin"])
    print(f"worst margin at delta 32, dither {int(dither)}: {worst:.3f}")


@pytest.mark.parametrize("delta", (16.0, 24.0))
def test_smaller_deltas_are_recorded_not_asserted(delta):
    """Figures only (DESIGN.md section 14 quotes them): how many of the 54 cases decode at delta 16 and 24."""
    n = ok = 0
    worst = 1.0
    for dither in (False, True):
        for attacker in rr.ATTACKERS:
            for size in rr.SIZES:
                r = rr.round_trip(rr.COVER, delta, dither, attacker, size)
                n += 1; ok += int(r["valid"] and r["data"] == rr.DATA)
                worst = min(worst, r["margin"])
                if not r["valid"]:
                    print(f"delta {delta:g} dither {int(dither)} {attacker} {size}: {r['wrong_bits']} wrong bits")
    print(f"delta {delta:g}: {ok} of {n} valid, worst margin {worst:.3f}")
    assert n == 54


@pytest.mark.parametrize("dither", (False, True), ids=("plain", "dither"))
def test_the_video_case_decodes_on_the_restatement(dither):
    r = rr.video_round_trip(dither)
    print(f"video dither {int(dither)}: margin {r['margin']:.3f} confidence {r['confidence']:.3f}")
    assert r["valid"] and r["data"] == rr.DATA and r["margin"] >= rr.MARGIN_FLOOR


# ---- refusals, before a context is created -----------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a refusal must come before the first device call")
    monkeypatch.setattr(core, "_ctx", refuse)
    monkeypatch.setattr(hostapi, "Context", refuse)
    monkeypatch.setattr(hostapi, "load_library", refuse)


def _meta(H, W, video_meta=False):
    members = M.payload_members("text", H, W, rr.DELTA, 80, rr.NONCE, *((2, 4) if video_meta else ()))
    return M.sealed(members, 8, hg.hmac_digest(rr.key(), M.hmac_parts(members)))


def test_tap_refusals():
    """1 -> 9 and 9 -> 1 are beyond MAX_SCALE = 8 (9 -> 1 would need 37 taps, the ABI takes 33): refused, like every
    other ratio beyond 8; 1 -> 8 and 8 -> 1 are the single-sample shapes the rule admits."""
    for bad in ((0, 4), (4, 0), (-1, 4), (65, 8), (8, 65), (1, 9), (9, 1)):
        with pytest.raises(ValueError):
            R.resample_taps(*bad)
    assert R.resample_taps(8, 1)[1].shape == (1, 33) and R.resample_taps(1, 8)[1].shape == (8, 5)


def test_resize_refusals_come_before_any_device_call(no_device, tmp_path):
    H, W = 136, 200
    meta = _meta(H, W)
    assert core.SEARCH_RESIZE == "resize" == video.SEARCH_RESIZE
    for shape in ((16, 200, 3), (136, 24, 3), (1089, 200, 3), (136, 1601, 3), (0, 0, 3)):
        with pytest.raises(ValueError, match="resize beyond 8x|must be positive"):
            core.extract_payload_arrays(np.zeros(shape, np.uint8), meta, rr.PASSWORD, search="resize")
    for bad in (np.zeros((100, 150), np.uint8), np.zeros((100, 150, 4), np.uint8), np.zeros((100, 150, 3), np.float32)):
        with pytest.raises(ValueError, match="uint8"):
            core.extract_payload_arrays(bad, meta, rr.PASSWORD, search="resize")
    for search in ("Resize", "resized", "scale", 3):
        with pytest.raises(ValueError, match="search"):
            core.extract_payload_arrays(np.zeros((100, 150, 3), np.uint8), meta, rr.PASSWORD, search=search)
        with pytest.raises(ValueError, match="search"):
            core.extract_payload(str(tmp_path / "no.png"), str(tmp_path / "no.npz"), password=rr.PASSWORD, search=search)
        with pytest.raises(ValueError, match="search"):
            video.extract_payload_video(str(tmp_path / "no.y4m"), str(tmp_path / "no.npz"), password=rr.PASSWORD, search=search)
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        core.extract_payload_arrays(np.zeros((100, 150, 3), np.uint8), meta, "not the password", search="resize")
    with pytest.raises(ValueError, match="meta was written for"):         # without the search a resized stego is still refused
        core.extract_payload_arrays(np.zeros((100, 150, 3), np.uint8), meta, rr.PASSWORD)


def test_video_resize_refusals_come_before_any_device_call(no_device, tmp_path):
    H, W = 72, 104
    path = str(tmp_path / "meta.npz")
    M.save_payload_meta(path, _meta(H, W, video_meta=True))
    clip = str(tmp_path / "tiny.y4m")
    video.write_y4m(clip, np.zeros((4, 8, 104), np.uint8))                 # 72 rows down to 8: 9x
    with pytest.raises(ValueError, match="resize beyond 8x"):
        video.extract_payload_video(clip, path, password=rr.PASSWORD, search="resize")
    with pytest.raises(ValueError, match="meta was written for"):
        video.extract_payload_video(clip, path, password=rr.PASSWORD)


def test_resized_soft_is_one_staging_scope_under_cached_tables():
    """On test_capi's stand-in library: upload, resample and soft decode in one scope, only the soft vector comes back, and
    a second batch of the same sizes allocates nothing but its own staging (the tap tables and the map are cached)."""
    from test_capi import _fake_ctx
    ctx = _fake_ctx(hostapi)
    lib = ctx.lib
    u8 = np.zeros((2, 12, 20), np.uint8)
    order, offs = np.arange(6), np.array([0, 2, 4, 6])
    soft = ctx.payload_soft_resized(u8, 16, 24, order, offs, 3, 32.0)
    assert soft.shape == (3,) and soft.dtype == np.float64
    calls = list(lib.calls)
    assert calls.count("wm_resample_planes_u8_dev") == 1 and calls.count("wm_memcpy_d2h") == 1
    assert calls.index("wm_resample_planes_u8_dev") < calls.index("wm_payload_soft_tiles_u8_dev") < calls.index("wm_memcpy_d2h")
    assert calls.index("wm_memcpy_d2h") < calls.index("wm_check_status")
    first = calls.count("wm_malloc")
    assert first == 5                                                       # the map, the tables; soft, restored planes, planes
    ctx.payload_soft_resized(u8, 16, 24, order, offs, 3, 32.0, dither=np.zeros((2, 6), np.uint16))    # (a table row per plane)
    assert lib.calls.count("wm_malloc") - first == 4 and lib.calls[-1] == "wm_free"
    assert "wm_payload_soft_tiles_dither_u8_dev" in lib.calls[len(calls):]
    held = [a for a in lib.mallocs if a not in lib.freed]
    assert len(held) == 2                                                   # the map and the tables
    ctx.close()
    assert sorted(a for a in lib.freed if a in lib.mallocs) == sorted(lib.mallocs)


def test_binding_refusals_need_no_library():
    """Context.resample_planes / payload_soft_resized check dtype, layout and ratio before they cross the C ABI"""
    ctx = object.__new__(hostapi.Context)
    ctx._h = None

    def _call(name, *args):
        raise AssertionError(f"{name} reached the C ABI")
    ctx._call = _call
    with pytest.raises(ValueError, match="uint8"):
        ctx.resample_planes(np.zeros((8, 8), np.float32), 16, 16)
    with pytest.raises(ValueError):
        ctx.resample_planes(np.zeros((2, 2, 8, 8), np.uint8), 16, 16)
    with pytest.raises(ValueError, match="beyond 8x"):
        ctx.resample_planes(np.zeros((8, 8), np.uint8), 65, 8)
    with pytest.raises(ValueError, match="beyond 8x"):
        ctx.payload_soft_resized(np.zeros((8, 8), np.uint8), 72, 8, np.arange(9), np.array([0, 9]), 1, 32.0)
    with pytest.raises(ValueError, match="delta"):
        ctx.payload_soft_resized(np.zeros((8, 8), np.uint8), 16, 16, np.arange(4), np.array([0, 4]), 1, 4.0)
