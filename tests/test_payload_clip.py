"""Clip resynchronisation of the dithered blind payload in a video, without a device: the precondition of the scenarios that
tests/test_gpu_payload_clip.py relies on (on the restatement alone, tests/payload_clip_refs.py), the limits DESIGN.md
section 14 ("Clip resynchronisation") quotes, payload.pick_clip and payload.clip_table_of against the restatements, and
every refusal of extract_payload_video(search="clip"), each raised before a context is created."""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import payload_clip_refs as cl
import payload_refs as pr
import payload_sync_refs as sr

M = importlib.import_module(ge.PKG_NAME + ".meta")
P = importlib.import_module(ge.PKG_NAME + ".payload")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
video = importlib.import_module(ge.PKG_NAME + ".video")

BAR = 4 * pr.slope_bar(cl.DELTA)


def _report(name, r):
    print(f"{name}: first frame {r['first_frame']}, origin {r['origin']}, top {r['top']:.3f}, best other of {r['candidates'] - 1} "
          f"{r['runner_up']:.3f}, gap {r['gap']:.3f}, tiles per bit >= {int(r['count'].min())}, bits without a tile "
          f"{int((r['count'] == 0).sum())}, valid {r['valid']}")


# ---- the precondition: a condition on the inputs, not a measurement ---------------------------------------------------
@pytest.mark.parametrize("name", list(cl.SCENARIOS))
def test_scenario_precondition_on_the_restatement(name):
    """For every scenario the true (first frame, phase, placement) beats every other candidate by at least 4 slope_bar(delta)
    = 0.102 in score / (32768 windows anchors); measured 0.188 - 0.207.  Every bit keeps a tile and the decode is valid and
    equal to the data - except where the clip has fewer tiles than the payload has bits: under the channel code (A-k7: 22 of
    172 coded bits without a tile, the decoder fills them in, the decode is still valid) and in the 48-tile clip, whose 80-bit
    frame cannot fit: there every bit that keeps a tile must read right and the frame check must fail."""
    sc, r = cl.scenario(name), cl.located(name)
    _report(name, r)
    assert BAR == pytest.approx(0.102)
    assert cl.is_true(r, sc), (r["first_frame"], r["origin"], r["phase"])
    assert r["gap"] >= BAR, (r["gap"], BAR)
    assert 0.76 <= r["top"] <= 0.80 and 0.55 <= r["runner_up"] <= 0.60
    n_tiles = (sc["crop"][2] // 8) * (sc["crop"][3] // 8)
    frame, carried, _ = cl.case_map(sc["case"], sc["code"])
    if sc["code"]:
        assert r["count"].min() == 0 and r["valid"] and r["data"] == sc["data"]
    elif n_tiles >= carried.size:
        assert r["count"].min() >= 1, int(r["count"].min())
        assert r["valid"] and r["data"] == sc["data"]
    else:
        assert name == "A-48x64" and n_tiles == 48 and carried.size == 80
        have = r["count"] > 0
        assert have.sum() <= n_tiles and np.array_equal(r["soft"][have] < 0, carried[have] != 0)
        assert not r["valid"]


def test_the_limits_the_design_quotes():
    """One anchor against several on crops of a few dozen tiles ("Clip resynchronisation", the limits):
    48 tiles - the true candidate wins either way, by 0.073 with one anchor (under the bar) and 0.188 with four;
    24 tiles - a wrong candidate wins with one anchor, the true one with six, by 0.097 (under the bar)."""
    one, four = cl.located("A-48x64-1anchor"), cl.located("A-48x64")
    _report("48x64, 1 anchor", one)
    assert cl.is_true(one, cl.scenario("A-48x64")) and one["gap"] < BAR <= four["gap"]
    assert one["gap"] == pytest.approx(0.073, abs=2e-3) and four["gap"] == pytest.approx(0.188, abs=2e-3)
    one, six = cl.located("A-24x32-1anchor"), cl.located("A-24x32-6anchors")
    _report("24x32, 1 anchor", one)
    _report("24x32, 6 anchors", six)
    assert not cl.is_true(one, cl.scenario("A-24x32-1anchor"))
    assert cl.is_true(six, cl.scenario("A-24x32-6anchors")) and 0 < six["gap"] < BAR


# ---- pick_clip ---------------------------------------------------------------------------------------------------------
def _best(n_cand, fill):
    b = np.full((n_cand, 64, 2), -1, np.int64)
    for (g, p), v in fill.items():
        b[g, p] = v
    return b


def test_pick_clip_ties_go_to_the_smallest_candidate():
    counts = np.full(64, 6, np.int64)
    marked = [2, 2, 2]
    b = _best(3, {(0, 9): (5, 4), (1, 3): (7, 1), (1, 9): (7, 0), (2, 0): (7, 0)})
    assert P.pick_clip(b, counts, marked) == (1, 3, 1) == cl.pick_clip_ref(b, counts, marked)
    # an equal ratio with unequal denominators is a tie too: 10 / (2 * 2) == 15 / (2 * 3) == 30 / (6 * 2)
    counts[:] = 0
    counts[[5, 6]] = (2, 6)
    b = _best(2, {(0, 5): (10, 3), (1, 5): (15, 0), (0, 6): (30, 2)})
    assert P.pick_clip(b, counts, [2, 3]) == (0, 5, 3) == cl.pick_clip_ref(b, counts, [2, 3])
    b[0, 5] = (9, 3)
    assert P.pick_clip(b, counts, [2, 3]) == (0, 6, 2) == cl.pick_clip_ref(b, counts, [2, 3])
    # beyond float64: 3 (k + 1) / 3 > (7 k + 6) / 7 by 1 / 7 only
    k = 2 ** 58
    counts[[1, 2]] = (7, 3)
    x, y = 7 * k + 6, 3 * (k + 1)
    assert x / 7 == y / 3
    b = _best(1, {(0, 1): (x, 0), (0, 2): (y, 0)})
    assert P.pick_clip(b, counts, [1]) == (0, 2, 0) == cl.pick_clip_ref(b, counts, [1])


def test_pick_clip_skips_minus_one_entries_and_unmarked_candidates():
    counts = np.full(64, 4, np.int64)
    counts[10] = 0
    b = _best(3, {(0, 10): (2 ** 40, 0), (1, 20): (1, 7), (2, 20): (9, 0)})
    assert P.pick_clip(b, counts, [1, 1, 0]) == (1, 20, 7)                   # count 0 and m_g 0 do not take part, whatever they score
    assert P.pick_clip(b, counts, [1, 1, 1]) == (2, 20, 0)
    assert P.pick_clip(_best(2, {}), counts, [1, 1]) is None
    assert P.pick_clip(_best(2, {(1, 0): (0, 0)}), counts, [1, 1]) == (1, 0, 0)     # an all-zero score is a candidate
    b = _best(1, {(0, 3): (5, -1)})
    assert P.pick_clip(b, counts, [1]) is None
    for bad in (np.zeros((2, 63, 2), np.int64), np.zeros((2, 64), np.int64)):
        with pytest.raises(ValueError):
            P.pick_clip(bad, counts, [1, 1])
    with pytest.raises(ValueError):
        P.pick_clip(_best(2, {}), counts, [1])
    with pytest.raises(ValueError):
        P.pick_clip(_best(2, {}), counts[:63], [1, 1])


def test_pick_clip_on_a_scenario_is_the_restatements_winner():
    sc, r = cl.scenario("A-fi2"), cl.located("A-fi2")
    h, w = sc["crop"][2:]
    tof = cl.table_of_ref(sc["F"], sc["fi"], sc["n_c"], min(sc["n_c"], sc["anchors"] * sc["fi"]))
    g, p, i = P.pick_clip(r["best"], P.phase_counts(h, w), (tof >= 0).sum(axis=1))
    n_tx = 24 - (w - p % 8) // 8 + 1
    assert (g, divmod(p, 8), divmod(i, n_tx)) == (r["first_frame"], r["phase"], r["place"])


# ---- clip_table_of -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fi", [1, 2, 3])
def test_clip_table_of_follows_the_literal_loops(fi):
    for F in (1, 2, 5, 7, 12):
        for n_c in range(1, F + 1):
            for A in {1, min(n_c, fi), min(n_c, 4 * fi), n_c}:
                got = P.clip_table_of(F, fi, n_c, A)
                assert got.dtype == np.int32 and np.array_equal(got, cl.table_of_ref(F, fi, n_c, A)), (F, fi, n_c, A)
                assert got.max() < -(-F // fi) and got.min() >= -1


def test_clip_table_of_candidates_without_an_anchor():
    """n_c < fi: a clip that may hold no marked frame at all - those candidates have a row of -1"""
    got = P.clip_table_of(7, 3, 2, 2)
    assert got.tolist() == [[0, -1], [-1, -1], [-1, 1], [1, -1], [-1, -1], [-1, 2]]
    assert P.clip_table_of(6, 1, 6, 4).tolist() == [[0, 1, 2, 3]]
    assert P.clip_table_of(7, 2, 4, 4).tolist() == [[0, -1, 1, -1], [-1, 1, -1, 2], [1, -1, 2, -1], [-1, 2, -1, 3]]
    for bad in ((6, 1, 7, 4), (6, 1, 0, 1), (6, 1, 3, 0), (6, 1, 3, 4)):
        with pytest.raises(ValueError):
            P.clip_table_of(*bad)


def test_the_search_value():
    assert P.SEARCH_CLIP == "clip" and video.VIDEO_SEARCHES == (None, "clip") and P.CLIP_ANCHORS == 4


# ---- refusals, before a context is created -----------------------------------------------------------------------------
def _meta_file(path, H, W, n_frames=6, dither=P.DITHER_TABLE, fi=1, video_meta=True):
    members = M.payload_members("text", H, W, 16.0, 80, sr.NONCE, *((fi, n_frames) if video_meta else ()), dither=dither)
    M.save_payload_meta(str(path), M.sealed(members, 8, hg.hmac_digest(sr.key(), M.hmac_parts(members))))
    return str(path)


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a refusal must come before the first device call")
    monkeypatch.setattr(video.hostapi, "Context", refuse)
    monkeypatch.setattr(video.hostapi, "load_library", refuse)


def test_clip_search_refusals_come_before_any_device_call(no_device, tmp_path):
    H, W = 128, 192
    meta = _meta_file(tmp_path / "meta.npz", H, W)

    def clip(n, h, w):
        path = str(tmp_path / f"clip_{n}_{h}_{w}.y4m")
        video.write_y4m(path, np.zeros((n, h, w), np.uint8))
        return path

    def extract(path, meta=meta, **kw):
        return video.extract_payload_video(path, meta, password=sr.PASSWORD, **{"search": "clip", **kw})

    for search in ("Clip", "crop", "crop-keyed", 1):
        with pytest.raises(ValueError, match="search"):
            extract(clip(2, 64, 64), search=search)
    with pytest.raises(ValueError, match="dither=True"):
        extract(clip(2, 64, 64), _meta_file(tmp_path / "plain.npz", H, W, dither=0))
    with pytest.raises(ValueError, match="embed_payload_video"):
        extract(clip(2, 64, 64), _meta_file(tmp_path / "image.npz", H, W, video_meta=False))
    for h, w in ((129, 192), (128, 193), (136, 200)):
        with pytest.raises(ValueError, match="larger than"):
            extract(clip(2, h, w))
    with pytest.raises(ValueError, match="7 frames"):
        extract(clip(7, 64, 64))
    for h, w in ((7, 64), (64, 7)):
        with pytest.raises(ValueError, match="whole 8x8 tile"):
            extract(clip(2, h, w))
    for anchors in (0, -1):
        with pytest.raises(ValueError, match="anchors"):
            extract(clip(2, 64, 64), anchors=anchors)
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        video.extract_payload_video(clip(2, 64, 64), meta, password="not the password", search="clip")


class _NoCallContext:
    """hostapi.Context without a device: any attempt to cross the C ABI fails the test."""

    def __new__(cls, hostapi):
        ctx = object.__new__(hostapi.Context)
        ctx._h = None

        def _call(name, *args):
            raise AssertionError(f"{name} reached the C ABI with unvalidated arguments")
        ctx._call = _call
        return ctx


def test_context_methods_validate_before_the_c_abi(hostapi):
    ctx = _NoCallContext(hostapi)
    h, w = 40, 56
    scan = [[np.zeros(sr.phase_shape(h, w, py, px), np.float32) for px in range(8)] for py in range(8)]
    planes = np.zeros((2, h, w), np.uint8)
    U = np.zeros((3, 5, 7), np.uint16)
    ok = np.array([[0, 1], [-1, 2]], np.int32)
    bad_calls = [
        (U, np.array([[0, 3]], np.int32)), (U, np.array([[0, -2]], np.int32)),      # a table that is not there; below -1
        (U, np.array([[0, 1, 2]], np.int32)), (U, ok[:, :1]), (U, ok[0]), (U, ok[:0]),     # not [n_cand >= 1, n_anchor]
        (U[0], ok), (U[:0], ok), (np.zeros((3, 4, 7), np.uint16), ok), (np.zeros((3, 5, 6), np.uint16), ok),
    ]
    for tables, tof in bad_calls:
        with pytest.raises(ValueError):
            ctx.payload_keyed_best([scan, scan], tables, tof, h, w, 16.0)
        with pytest.raises(ValueError):
            ctx.payload_locate_clip(planes, tables, tof, 16.0)
    for delta in (7.9, float("nan"), 1000.0):
        with pytest.raises(ValueError, match="delta"):
            ctx.payload_keyed_best([scan, scan], U, ok, h, w, delta)
        with pytest.raises(ValueError, match="delta"):
            ctx.payload_locate_clip(planes, U, ok, delta)
    with pytest.raises(ValueError, match="phase"):                          # a scan of another plane size
        ctx.payload_keyed_best([scan, scan], U, ok, h, 48, 16.0)
    with pytest.raises(ValueError):
        ctx.payload_locate_clip(planes[0], U, ok[:, :1], 16.0)
    with pytest.raises(ValueError):
        ctx.payload_locate_clip(planes.astype(np.float32), U, ok, 16.0)
    with pytest.raises(ValueError, match="whole tile"):
        ctx.payload_locate_clip(planes[:, :7], U, ok, 16.0)
