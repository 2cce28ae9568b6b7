"""Rotation resynchronisation of the blind payload without a device (include/wmhip.h, "rotation resynchronisation"; DESIGN.md
section 14): the weights, the exact cases of the integer rotation, the validity test, the schedule and the winner's rule, the
public refusals, and the signal - asserted on the NumPy restatement (tests/rotate_refs.py) for float-rotated stegos of
mask_refs.host(256, 384, 2) at delta 32.

Measured on the restatement, the worst over the 24 cases below (dither off / on x bilinear / cubic x same-size / expanded canvas
x 1, 3, -7.3 degrees, max_angle 8): the winner's score / (32768 count) 0.787 (best 0.841), its lead over the best candidate four
or more coarse steps away 0.221 (those candidates score 0.536 to 0.572), the found angle 0.21 of a coarse step from the true one,
0 wrong bits in every case, 12 to 114 wrong votes among 1386 to 1532 valid tiles.

A limit, recorded and not asserted: on mask_refs.host(136, 200, 2) (425 tiles, 345 to 371 of them valid, bits with one or two valid
tiles), max_angle 10 (43 + 17 candidates), bilinear attacks of 2, -6, 9.7 and 0.3 degrees on the same-size canvas, the restatement
finds the angle within 0.46 of a coarse step and leads by 0.17 to 0.27 in all 12 cases; it decodes all 8 at delta 32 (dither off and
on) and returns 1 wrong bit in 3 of the 4 at delta 24 with dither.  Too small a frame for an uncoded payload below delta 32."""
import importlib
import math

import numpy as np
import pytest

import __graft_entry__ as ge
import resample_refs as rr
import rotate_refs as rf

P = importlib.import_module(ge.PKG_NAME + ".payload")
R = importlib.import_module(ge.PKG_NAME + ".resample")
core = importlib.import_module(ge.PKG_NAME + ".dct_svd_core_secure")


# ---- fail before the feature -------------------------------------------------------------------------------------------
def test_rotate_is_a_known_search():
    assert core.SEARCH_ROTATE == "rotate"
    core._check_search("rotate")
    core._check_search("rotate", 10.0)
    assert core.SEARCHES == (None, "crop", "crop-keyed") and core.SEARCH_RESIZE == "resize"
    with pytest.raises(ValueError, match="'rotate'"):
        core._check_search("turn")


def test_library_exports_the_new_entry_points(hostapi):
    ge.build_hip()
    lib = hostapi.load_library()
    for name in ("wm_rotate_planes_u8", "wm_rotate_planes_u8_dev", "wm_payload_angle_scores", "wm_payload_angle_scores_dev"):
        assert hasattr(lib, name), f"libwmhip.so does not export {name}"
        assert name in hostapi.SIGNATURES
    assert lib.wm_abi_version() == 1


# ---- the weights -------------------------------------------------------------------------------------------------------
def test_weights():
    K = R.rotate_weights()
    assert K.dtype == np.int16 and K.shape == (256, 4) and not K.flags.writeable
    assert np.array_equal(K, rf.weights_ref())
    assert np.all(K.astype(np.int64).sum(axis=1) == 1 << 14)
    assert K[0].tolist() == [0, 1 << 14, 0, 0]
    assert np.abs(K.astype(np.int64)).sum(axis=1).max() * 255 < 1 << 23     # a row sum fits the 24-bit multiply-adds


def test_candidates():
    assert R.angle_candidate(0.0) == (65536, 0) and R.angle_candidate(math.pi / 2) == (0, 65536)
    for t in (0.01, -0.3, 0.7):
        assert R.angle_candidate(t) == rf.candidate_ref(t)
    cs = R.angle_candidates_cs([0.0, 0.1])
    assert cs.dtype == np.int32 and cs.shape == (2, 2) and tuple(cs[1]) == rf.candidate_ref(0.1)


# ---- exact cases -------------------------------------------------------------------------------------------------------
def _plane(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def test_zero_angle_onto_the_same_size_is_the_plane():
    for h, w in ((8, 8), (23, 45), (1, 1)):
        p = _plane(h, w, seed=h)
        assert np.array_equal(rf.rotate_ref(p, h, w, *rf.candidate_ref(0.0)), p)


def test_quarter_turn_of_a_square_is_exact():
    p = _plane(24, 24, seed=3)
    q = rf.rotate_ref(p, 24, 24, *rf.candidate_ref(math.pi / 2))
    assert np.array_equal(q, np.rot90(p, 1))                                 # out[y][x] = p[x][23 - y]
    assert np.array_equal(rf.rotate_ref(p, 24, 24, *rf.candidate_ref(-math.pi / 2)), np.rot90(p, -1))


def test_both_clips_are_reached():
    hit_low = hit_high = False
    for plane in (rr.checkerboard(), rr.step_edge()):
        for deg in (5.0, 33.0):
            out = rf.rotate_ref(plane, 24, 40, *rf.candidate_ref(math.radians(deg)))
            hit_low |= bool((out == 0).any()); hit_high |= bool((out == 255).any())
    assert hit_low and hit_high


def test_a_block_footprint_fits_the_staged_segment():
    """k_rotate_planes stages 48 x 48 source bytes for a 32 x 32 destination block: enough at every angle"""
    worst = max(rf.footprint_ref(96, 128, 150, 150, *rf.candidate_ref(math.radians(d))) for d in (0, 1, 10, 30, 44, 45, -45, 90, 135))
    assert 36 <= worst <= 48, worst


# ---- validity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", (3.0, 40.0))
@pytest.mark.parametrize("expand", (False, True), ids=("same", "expanded"))
def test_four_corners_decide_a_tile(deg, expand):
    H, W = 64, 96
    h, w = rf.expanded_shape(H, W, deg) if expand else (H, W)
    C, S = rf.candidate_ref(math.radians(deg))
    corners, every = rf.valid_ref(H, W, h, w, C, S), rf.valid_ref(H, W, h, w, C, S, every_pixel=True)
    assert np.array_equal(corners, every)
    assert corners.any() and (expand or not corners.all())


# ---- schedule and winner -----------------------------------------------------------------------------------------------
def test_schedule():
    H, W = 256, 384
    Rr = math.hypot(H, W) / 2
    nums, den = P.angle_candidates(H, W, 8.0)
    n = int(math.floor(math.radians(8.0) * Rr))
    assert den == Rr and nums.tolist() == list(range(-n, n + 1)) == rf.schedule_ref(H, W, 8.0)[0]
    fine, fden = P.angle_candidates(H, W, 8.0, around=-5)
    assert fden == 8 * Rr and fine.tolist() == list(range(-48, -31)) == rf.schedule_ref(H, W, 8.0, -5)[0]
    assert len(P.angle_candidates(136, 200, 10.0)[0]) == 43                  # the issue's count on the small frame
    for bad in (0.0, -1.0, 45.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="max_angle"):
            P.check_max_angle(bad)
    assert P.check_max_angle(45) == 45.0


def test_pick_angle():
    assert P.pick_angle([10, 30, 20], [1, 3, 2]) == 0                        # ties to the smallest index
    assert P.pick_angle([10, 31, 20], [1, 3, 2]) == 1
    assert P.pick_angle([5, 0, 7], [0, 0, 1]) == 2                           # count 0 takes no part
    assert P.pick_angle([5, 6], [0, 0]) is None
    big = 1 << 40
    assert P.pick_angle([big * 3, big * 3 + 1], [3, 3]) == 1                 # exact, beyond float64's 53 bits of a product
    assert P.pick_angle([3, 2], [4, 3]) == rf.pick_ref([3, 2], [4, 3]) == 0


def test_votes_of_metric():
    m = np.array([[0.5, -1.0], [0.25, 1.0]], np.float32)
    assert P.votes_of_metric(m).tolist() == [[16384, -32768], [8192, 32768]]
    assert P.votes_of_metric(m, np.array([[1, 0], [0, 1]], bool)).tolist() == [[16384, 0], [0, 32768]]


# ---- the refusals, before any device call -------------------------------------------------------------------------------
def _meta():
    """a sealed payload meta made on the host alone"""
    M = importlib.import_module(ge.PKG_NAME + ".meta")
    hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
    H, W = 64, 96
    members = M.payload_members("text", H, W, 32.0, P.payload_frame(rr.DATA).size, rr.NONCE, dither=0, code=0)
    return M.sealed(members, 8, hg.hmac_digest(rr.key(), M.hmac_parts(members)))


def test_refusals_need_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call before the refusal")
    monkeypatch.setattr(core, "_ctx", no_device)
    meta, stego = _meta(), np.zeros((64, 96, 3), np.uint8)
    for bad in (0, -3.0, 45.01, float("nan")):
        with pytest.raises(ValueError, match="max_angle"):
            core.extract_payload_arrays(stego, meta, rr.PASSWORD, search="rotate", max_angle=bad)
    for search in (None, "crop", "crop-keyed", "resize"):
        with pytest.raises(ValueError, match="max_angle goes with"):
            core.extract_payload_arrays(stego, meta, rr.PASSWORD, search=search, max_angle=5.0)
    with pytest.raises(ValueError, match="8192"):
        core.extract_payload_arrays(np.zeros((8, 8193, 3), np.uint8), meta, rr.PASSWORD, search="rotate")
    for wrong in (np.zeros((64, 96), np.uint8), np.zeros((64, 96, 3), np.float32), np.zeros((64, 96, 4), np.uint8)):
        with pytest.raises(ValueError, match=r"uint8 \[h, w, 3\]"):
            core.extract_payload_arrays(wrong, meta, rr.PASSWORD, search="rotate")
    with pytest.raises(ValueError):
        core.extract_payload_arrays(stego, meta, "not the password", search="rotate")
    with pytest.raises(AssertionError, match="a device call"):            # and a good call does reach the device
        core.extract_payload_arrays(stego, meta, rr.PASSWORD, search="rotate", max_angle=45.0)


# ---- the signal, on the integer restatement ------------------------------------------------------------------------------
CASES = [(dither, kind, expand, deg) for dither in (False, True) for kind in rf.KINDS for expand in (False, True) for deg in rf.ANGLES]


@pytest.mark.parametrize("dither,kind,expand,deg", CASES,
                         ids=[f"{'dither' if d else 'plain'}-{k}-{'expanded' if e else 'same'}-{a}" for d, k, e, a in CASES])
def test_rotated_stego_is_found_and_decodes(dither, kind, expand, deg):
    r = rf.search_ref(rf.COVER, rf.DELTA, dither, deg, kind, expand)
    print(f"score {r['score']:.4f} far {r['far']:.4f} lead {r['score'] - r['far']:.4f} off {r['steps_off']:.3f} steps, angle "
          f"{r['angle']:.4f}, valid tiles {r['valid_tiles']}, wrong bits {r['wrong_bits']}, wrong votes {r['wrong_votes']}, "
          f"confidence {r['confidence']:.4f}")
    assert r["valid"] and r["data"] == rr.DATA
    assert r["score"] - r["far"] >= rf.MARGIN_BAR
    assert r["steps_off"] <= 1.0
