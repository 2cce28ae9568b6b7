"""Frame resynchronisation of the dithered blind payload in a video, without a device: the scenarios on the restatement
(tests/payload_frames_refs.py) with the precondition tests/test_gpu_payload_frames.py leans on, the limits DESIGN.md section 14
("Frame resynchronisation") quotes, payload.pick_frames and payload.anchor_accepted against the literal loops, every refusal of
extract_payload_video(search="frames"), each raised before a context is created, and the searches that existed unchanged."""
import importlib
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as ge
import payload_clip_refs as cl
import payload_dither_refs as pdr
import payload_frames_refs as fr
import payload_refs as pr
import payload_sync_refs as sr

M = importlib.import_module(ge.PKG_NAME + ".meta")
P = importlib.import_module(ge.PKG_NAME + ".payload")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
video = importlib.import_module(ge.PKG_NAME + ".video")
flow = importlib.import_module(ge.PKG_NAME + ".payload_flow")

ONE = P.VOTE_ONE


def _report(name, r, sc):
    marked = [g for g, f in zip(r["gaps"], sc["frame_map"]) if f >= 0]
    other = [g for g, f in zip(r["gaps"], sc["frame_map"]) if f < 0]
    print(f"{name}: origin {r['origin']}, {r['n_win']} windows, anchors' leads {[round(x, 3) for x in r['anchor_leads']]}, "
          f"frame_map {r['frame_map']}, marked gaps {min(marked):.3f} - {max(marked):.3f}, other gaps "
          f"{[round(x, 3) for x in other]}, valid {r['valid']}, confidence {r['confidence']:.4f}")


# ---- the scenarios and their precondition: a condition on the inputs, not a measurement -----------------------------------
def test_the_bars():
    assert fr.MARKED_GAP == pytest.approx(0.151, abs=1e-3) and fr.OTHER_GAP == pytest.approx(0.049, abs=1e-3)
    assert fr.GAP == Fraction(1, P.FRAME_GAP_DEN)


@pytest.mark.parametrize("name", list(fr.SCENARIOS))
def test_scenario_on_the_restatement(name):
    """Every marked frame maps to its file index and every other frame to -1, the payload is valid and equals the data, and the
    precondition holds: marked frames' gaps (and the accepted anchor's lead) >= 0.1 + 2 slope_bar = 0.151, other frames' gaps (and
    the refused anchors' leads) <= 0.1 - 2 slope_bar = 0.049."""
    sc, r = fr.scenario(name), fr.matched(name)
    _report(name, r, sc)
    assert r["found"] and r["origin"] == sc["crop"][:2]
    assert r["frame_map"] == sc["frame_map"]
    assert r["valid"] and r["data"] == sc["data"]
    for g, want in zip(r["gaps"], sc["frame_map"]):
        assert g >= fr.MARKED_GAP if want >= 0 else g <= fr.OTHER_GAP, (g, want)
    assert r["anchor_leads"][-1] >= fr.MARKED_GAP and all(x <= fr.OTHER_GAP for x in r["anchor_leads"][:-1])
    assert fr.meets_precondition(r, sc)
    assert r["n_accepted"] == sum(f >= 0 for f in sc["frame_map"])


def test_the_foreign_scenario_moves_on_to_its_second_anchor():
    r = fr.matched("A-fi2-foreign")
    assert len(r["anchor_leads"]) == 2 and r["frame_map"] == [-1, 4, -1, 6, -1, 8]


def test_the_limits_the_design_quotes():
    """Crops of a few dozen tiles ("Frame resynchronisation", the limits): at 48 windows the frames still
    name their tables, with gaps too close to the bar to be a GPU case; at 12 windows they do not."""
    sc, r = fr.scenario("A-48x64"), fr.matched("A-48x64")
    _report("A-48x64", r, sc)
    assert r["found"] and r["origin"] == sc["crop"][:2] and r["n_win"] == 48
    assert r["frame_map"] == sc["frame_map"] == [5, 2, 0, 3]               # every frame names its table
    assert 0.19 <= r["gaps"].min() and r["gaps"].max() <= 0.24             # 0.193 - 0.233
    assert len(r["anchor_leads"]) == 3 and max(r["anchor_leads"][:2]) < 0.1 <= r["anchor_leads"][2] < fr.MARKED_GAP     # 0.097, 0.063, 0.103
    assert not r["valid"]                                                  # (48 tiles cannot carry the 80-bit frame, as in the clip search)
    assert not fr.meets_precondition(r, sc)
    sc, r = fr.scenario("A-24x32"), fr.matched("A-24x32")
    print(f"A-24x32: no anchor accepted, leads {[round(x, 3) for x in r['anchor_leads']]}")
    assert not r["found"] and len(r["anchor_leads"]) == 4 and max(r["anchor_leads"]) < 0.05      # 0.002 - 0.029
    assert r["frame_map"] == [-1] * 4 and (r["data"], r["valid"], r["origin"]) == (b"", False, None)
    assert not fr.meets_precondition(r, sc)


# ---- pick_frames ---------------------------------------------------------------------------------------------------------
def _named(scores, n_win):
    got = P.pick_frames(scores, n_win)
    assert got.dtype == np.int32 and got.tolist() == fr.pick_frames_ref(scores, n_win)
    return got.tolist()


def test_pick_frames_follows_the_literal_loops_on_random_matrices():
    rng = np.random.default_rng(5)
    seen = set()
    for n_win in (1, 3, 48, 300, 32400):
        for K in (1, 2, 5, 24):
            s = rng.integers(0, ONE * n_win + 1, (40, K)).astype(np.int64)
            s[::3, rng.integers(0, K)] = ONE * n_win                       # rows with a table at full scale
            if K > 1:
                s[1::6, 1] = s[1::6, 0]                                    # ties of the first two
            seen.update(_named(s, n_win))
    assert -1 in seen and len(seen) > 3


def test_pick_frames_ties_go_to_the_first_maximum():
    n = 10
    assert _named([[ONE * n, ONE * n, 0]], n) == [-1]                      # a tie at the top: the gap is 0
    assert _named([[ONE * n, 0, ONE * n]], n) == [-1]
    assert _named([[0, ONE * n, 0], [ONE * n, 0, 0], [0, 0, ONE * n]], n) == [1, 0, 2]


def test_pick_frames_one_table_and_the_half_scale_floor():
    n = 100
    bar = ONE * n // P.FRAME_GAP_DEN                                       # 327 680: the gap that is exactly on the bar
    assert ONE * n % P.FRAME_GAP_DEN == 0
    floor = ONE // 2 * n
    # K = 1: only the floor stands against the score
    assert _named([[floor + bar]], n) == [0]
    assert _named([[floor + bar - 1]], n) == [-1]
    assert _named([[0]], n) == [-1] and _named([[ONE * n]], n) == [0]
    # K > 1 with every other table under the floor: the floor is the runner-up
    assert _named([[floor + bar, floor - 5, 0]], n) == [0]
    assert _named([[floor + bar - 1, floor - 5, 0]], n) == [-1]
    # a runner-up above the floor takes its place
    assert _named([[floor + bar + 7, floor + 7]], n) == [0]
    assert _named([[floor + bar + 6, floor + 7]], n) == [-1]


def test_pick_frames_a_gap_on_the_bar_is_accepted_and_one_below_is_refused():
    for n in (1, 7, 308, 32400):
        top = ONE * n
        need = -(-ONE * n // P.FRAME_GAP_DEN)                              # the smallest integer gap with 10 gap >= 32768 n
        assert _named([[top - need, top]], n) == [1]
        assert _named([[top - need + 1, top]], n) == [-1]
    with pytest.raises(ValueError):
        P.pick_frames(np.zeros((2, 0), np.int64), 4)
    with pytest.raises(ValueError):
        P.pick_frames(np.zeros(3, np.int64), 4)
    with pytest.raises(ValueError):
        P.pick_frames(np.zeros((2, 3), np.int64), 0)
    assert P.pick_frames(np.zeros((0, 3), np.int64), 4).shape == (0,)


def test_pick_frames_beyond_float64():
    n = 2 ** 40                                                             # scores near 2^55: a float64 comparison would round
    top = ONE * n
    need = -(-top // P.FRAME_GAP_DEN)
    assert _named([[top, top - need]], n) == [0] and _named([[top, top - need + 1]], n) == [-1]


def test_anchor_accepted_follows_the_exact_lead():
    counts = np.zeros(64, np.int64)
    counts[[3, 4]] = (10, 7)
    b = np.full((2, 64, 2), -1, np.int64)
    b[0, 3] = (ONE * 10 * 8 // 10, 0)                                      # 0.8 of full scale over 10 windows
    b[1, 4] = (ONE * 7 * 7 // 10, 2)                                       # 0.7 over 7: exactly on the bar
    assert ONE * 7 * 7 % 10 and fr.anchor_lead_ref(b, counts, (0, 3)) > fr.GAP      # (floor division: a hair above the bar)
    assert P.anchor_accepted(b, counts, (0, 3))
    b[1, 4, 0] += 1
    assert fr.anchor_lead_ref(b, counts, (0, 3)) < fr.GAP and not P.anchor_accepted(b, counts, (0, 3))
    b[1, 4] = (-1, -1)                                                     # nothing else takes part
    assert P.anchor_accepted(b, counts, (0, 3))
    b[1, 5] = (2 ** 40, 0)                                                 # a phase without a window does not take part
    assert P.anchor_accepted(b, counts, (0, 3))
    assert P.leads_by_the_bar(ONE * 8, 10, ONE * 7, 10) and not P.leads_by_the_bar(ONE * 8 - 1, 10, ONE * 7, 10)


def test_anchor_accepted_on_the_scenarios_anchors():
    sc = fr.scenario("A-fi2-foreign")
    clip = fr.edit(fr.video("A-fi2-foreign"), sc)
    K = -(-sc["F"] // sc["fi"])
    tables = [cl.frame_table("A", k * sc["fi"]) for k in range(K)]
    counts = P.phase_counts(*clip.shape[1:])
    got = []
    for a in range(2):
        best = cl.best_ref([fr.kr.s1_ref(clip[a])], tables, np.arange(K)[:, None], fr.DELTA)
        win = P.pick_clip(best, counts, [1] * K)
        assert win == cl.pick_clip_ref(best, counts.reshape(-1), [1] * K)
        got.append(P.anchor_accepted(best, counts, win))
    assert got == [False, True]


def test_the_kernels_chunks_and_caps_are_where_the_source_sets_them():
    """the second-trip shapes of tests/test_gpu_payload_frames.py cross what the kernel's source says they cross"""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(P.__file__)), "csrc", "wm_payload.hip")
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    with open(path, encoding="utf-8") as f:
        text = squeeze(f.read())
    for statement in fr.SOURCE:
        assert squeeze(statement) in text, f"`{statement}` is no longer in wm_payload.hip: restate it and move TRIPS with it"
    t = fr.TRIPS
    assert t["lane-0-twice"][2] * t["lane-0-twice"][3] == fr.WAVE + 1
    assert t["second-chunk-of-one-window"][2] * t["second-chunk-of-one-window"][3] == fr.FRAME_CHUNK + 1
    assert t["a-lane-in-three-chunks"][2] * t["a-lane-in-three-chunks"][3] == 2 * fr.FRAME_CHUNK + fr.WAVE + 1
    assert t["a-lane-in-three-chunks"][0] == fr.FRAME_FB + 1 and t["a-lane-in-three-chunks"][1] == fr.FRAME_TB + 1
    assert -(-t["table-blocks-past-the-grid"][1] // fr.FRAME_TB) == fr.FRAME_GRID_CAP + 1
    assert -(-t["frame-blocks-past-the-grid"][0] // fr.FRAME_FB) == fr.FRAME_GRID_CAP + 1
    assert fr.FRAME_CHUNK // fr.WAVE * P.VOTE_ONE < 2 ** 31 // fr.WAVE      # a lane's int32, and the wave's sum of 64 of them
    for n_f, n_t, ny, nx, nby, nbx, ty, tx in t.values():
        assert ty + ny <= nby and tx + nx <= nbx


def test_the_constants():
    assert P.SEARCH_FRAMES == "frames" and P.FRAME_GAP_DEN == 10
    assert video.VIDEO_SEARCHES == (None, "clip") and video.SEARCH_RESIZE == "resize" and P.CLIP_ANCHORS == 4


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


def test_frame_search_refusals_come_before_any_device_call(no_device, tmp_path):
    H, W = 128, 192
    meta = _meta_file(tmp_path / "meta.npz", H, W)

    def clip(n, h, w):
        path = str(tmp_path / f"clip_{n}_{h}_{w}.y4m")
        video.write_y4m(path, np.zeros((n, h, w), np.uint8))
        return path

    def extract(path, meta=meta, **kw):
        return video.extract_payload_video(path, meta, password=sr.PASSWORD, **{"search": "frames", **kw})

    for search in ("Frames", "frame", "crop", 1):
        with pytest.raises(ValueError, match="^search must be"):
            extract(clip(2, 64, 64), search=search)
    with pytest.raises(ValueError, match="search='frames' reads a payload embedded with dither=True"):
        extract(clip(2, 64, 64), _meta_file(tmp_path / "plain.npz", H, W, dither=0))
    with pytest.raises(ValueError, match="not written by embed_payload_video"):
        extract(clip(2, 64, 64), _meta_file(tmp_path / "image.npz", H, W, video_meta=False))
    for h, w in ((129, 192), (128, 193), (136, 200)):
        with pytest.raises(ValueError, match="larger than"):
            extract(clip(2, h, w))
    for h, w in ((7, 64), (64, 7)):
        with pytest.raises(ValueError, match="whole 8x8 tile"):
            extract(clip(2, h, w))
    empty = str(tmp_path / "empty.y4m")
    video.write_y4m(empty, np.zeros((0, 64, 64), np.uint8))
    with pytest.raises(ValueError, match="clip has no frame"):
        extract(empty)
    for anchors in (0, -1):
        with pytest.raises(ValueError, match="anchors must be at least 1"):
            extract(clip(2, 64, 64), anchors=anchors)
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        video.extract_payload_video(clip(2, 64, 64), meta, password="not the password", search="frames")


def test_more_frames_than_the_marked_video_is_no_refusal(monkeypatch, tmp_path):
    """repeats may make the file longer than the marked video: the search goes on to the device (here: to the stand-in)"""
    class Reached(Exception):
        pass

    def context(*a, **k):
        raise Reached
    monkeypatch.setattr(video.hostapi, "Context", context)
    meta = _meta_file(tmp_path / "meta.npz", 128, 192, n_frames=3)
    path = str(tmp_path / "long.y4m")
    video.write_y4m(path, np.zeros((7, 64, 64), np.uint8))
    with pytest.raises(Reached):
        video.extract_payload_video(path, meta, password=sr.PASSWORD, search="frames")
    with pytest.raises(ValueError, match="7 frames"):                       # the clip search still refuses it
        video.extract_payload_video(path, meta, password=sr.PASSWORD, search="clip")


# ---- the host flow on a stand-in context: steps 1 - 4 of video._extract_payload_frames against the restatement ---------------
class _RefContext:
    """hostapi.Context's two calls of the frame search, answered by the restatement: what video.py does around them - the
    anchors in file order, the batches, the assignment, the votes and the tail - runs as it does on the device"""

    def __init__(self, device=0):
        self.locates = []

    def close(self):
        pass

    def payload_locate_clip(self, planes, tables, table_of, delta, *, pick=False, cands_per_call=None):
        assert pick
        self.locates.append((planes.shape[0], np.asarray(table_of).copy()))
        h, w = planes.shape[1:]
        best = cl.best_ref([fr.kr.s1_ref(y) for y in planes], list(tables), table_of, delta)
        win = P.pick_clip(best, P.phase_counts(h, w), (np.asarray(table_of) >= 0).sum(axis=1))
        if win is None:
            return best, None
        g, p, i = win
        n_tx = tables.shape[2] - (w - p % 8) // 8 + 1
        return best, (g, (p // 8, p % 8), (i // n_tx, i % n_tx))

    @staticmethod
    def _s1(y):
        return fr.o.stego_sigma(np.ascontiguousarray(y).astype(np.float32), 8)[..., 0].astype(np.float32)

    def payload_metric(self, planes, delta, dither=None):
        """float32 [n, ny, nx]: the dithered metric of every tile (the clip search's decode)"""
        return np.stack([pdr.metric(self._s1(y), np.asarray(u).reshape(y.shape[0] // 8, y.shape[1] // 8), delta)
                         for y, u in zip(planes, dither)]).astype(np.float32)

    def payload_soft(self, planes, order, offs, n_bits, delta, dither=None):
        """float64 [n_bits]: the metrics of a bit's tiles added over the planes (the default extract)"""
        m = self.payload_metric(planes, delta, dither).reshape(len(planes), -1).astype(np.float64).sum(axis=0)
        return np.array([m[order[offs[j]:offs[j + 1]]].sum() for j in range(n_bits)])

    def payload_match_frames(self, view, tables, ty, tx, delta, tables_per_call=None):
        n, h, w = view.shape
        ny, nx = h // 8, w // 8
        s1 = np.stack([self._s1(v) for v in view])
        return fr.frame_scores_ref(s1, list(tables), ny, nx, ty, tx, delta), s1

    def payload_decode(self, L):
        frame = (L.size // 2) - P.K7_TAIL
        return fr.cr.viterbi_ref(L, frame)[0], None


@pytest.mark.parametrize("name", ["A-shuffle", "A-fi2-foreign", "A-k7"])
@pytest.mark.parametrize("batch", [2, 32])
def test_the_host_flow_on_the_restatements_device_calls(monkeypatch, tmp_path, name, batch):
    sc, r = fr.scenario(name), fr.matched(name)
    monkeypatch.setattr(video.hostapi, "Context", _RefContext)
    meta = str(tmp_path / "meta.npz")
    H, W = sc["shape"]
    frame, carried, _ = cl.case_map(sc["case"], sc["code"])
    members = M.payload_members("bytes", H, W, fr.DELTA, frame.size, sr.NONCE, sc["fi"], sc["F"], dither=P.DITHER_TABLE,
                                code=P.check_code(sc["code"]))
    M.save_payload_meta(meta, M.sealed(members, 8, hg.hmac_digest(sr.key(), M.hmac_parts(members))))
    path = str(tmp_path / "file.y4m")
    video.write_y4m(path, fr.edit(fr.video(name), sc))
    data, valid, conf, origin, fmap, soft = video.extract_payload_video(path, meta, password=sr.PASSWORD, search="frames", batch=batch,
                                                                        return_soft=True)
    assert (data, valid, origin) == (sc["data"], True, sc["crop"][:2])
    assert fmap.dtype == np.int32 and fmap.tolist() == sc["frame_map"]
    assert np.array_equal(soft, r["soft"]) and conf == pytest.approx(r["confidence"], abs=1e-12)
    assert len(video.extract_payload_video(path, meta, password=sr.PASSWORD, search="frames")) == 5


def test_a_file_of_frames_that_carry_nothing_gives_the_empty_result(monkeypatch, tmp_path):
    monkeypatch.setattr(video.hostapi, "Context", _RefContext)
    meta = _meta_file(tmp_path / "meta.npz", 128, 192, n_frames=3)
    path = str(tmp_path / "bare.y4m")
    video.write_y4m(path, np.stack([fr.foreign_frame("A", i) for i in range(2)])[:, 8:72, 16:112])
    out = video.extract_payload_video(path, meta, password=sr.PASSWORD, search="frames", return_soft=True)
    assert out[:4] == (b"", False, 0.0, None) and out[4].tolist() == [-1, -1] and out[4].dtype == np.int32
    assert out[5].shape == (80,) and not out[5].any()
    assert len(video.extract_payload_video(path, meta, password=sr.PASSWORD, search="frames")) == 5


def _scenario_meta(path, case, F, fi, code):
    H, W = sr.CASES[case]["shape"]
    frame = cl.case_map(case, code)[0]
    members = M.payload_members("bytes", H, W, fr.DELTA, frame.size, sr.NONCE, fi, F, dither=P.DITHER_TABLE, code=P.check_code(code))
    M.save_payload_meta(str(path), M.sealed(members, 8, hg.hmac_digest(sr.key(), M.hmac_parts(members))))
    return str(path)


def test_the_default_extract_and_the_clip_search_are_unchanged(monkeypatch, tmp_path):
    """The searches that existed, on files they could read before, with the device calls answered by the restatement: the plain
    extract of the unedited video returns its three values, search="clip" of a cut, cropped clip its five - the restatement's
    (tests/payload_clip_refs.py) - and neither goes through the new calls."""
    made = []

    class Ctx(_RefContext):
        def __init__(self, device=0):
            super().__init__(device)
            made.append(self)

        def payload_match_frames(self, *a, **k):
            raise AssertionError("only search='frames' matches frames")
    monkeypatch.setattr(video.hostapi, "Context", Ctx)
    sc = cl.scenario("A-crop")
    meta = _scenario_meta(tmp_path / "meta.npz", sc["case"], sc["F"], sc["fi"], sc["code"])
    whole, clip = str(tmp_path / "whole.y4m"), str(tmp_path / "clip.y4m")
    video.write_y4m(whole, cl.video("A-crop"))
    video.write_y4m(clip, cl.cut(cl.video("A-crop"), sc))
    plain = video.extract_payload_video(whole, meta, password=sr.PASSWORD)
    assert len(plain) == 3 and plain[:2] == (sc["data"], True) and 0.7 < plain[2] <= 1.0 and not made[-1].locates
    with_soft = video.extract_payload_video(whole, meta, password=sr.PASSWORD, search=None, return_soft=True)
    assert len(with_soft) == 4 and with_soft[:3] == plain and with_soft[3].shape == (80,)
    r = cl.located("A-crop")
    got = video.extract_payload_video(clip, meta, password=sr.PASSWORD, search="clip", return_soft=True)
    assert len(got) == 6 and got[:2] == (sc["data"], True) and got[3] == sc["crop"][:2] == r["origin"] and got[4] == sc["t0"]
    assert got[2] == pytest.approx(r["confidence"], abs=1e-6) and np.allclose(got[5], r["soft"], atol=1e-9)
    (n_anchor, tof), = made[-1].locates                                     # one search over the clip's three anchors and all first frames
    assert n_anchor == 3 and np.array_equal(tof, P.clip_table_of(sc["F"], sc["fi"], sc["n_c"], 3))
    with pytest.raises(ValueError, match="the meta was written for"):       # and a cropped file without a search is still refused
        video.extract_payload_video(clip, meta, password=sr.PASSWORD)
