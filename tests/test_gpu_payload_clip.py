"""Clip resynchronisation of the dithered blind payload on the device: wm_payload_keyed_best against the existing keyed
scores of the same device scan (bit for bit, both lane mappings), against the restatement run on the device's own sigma_1
(tests/payload_clip_refs.py; integer arithmetic: bit for bit where 1 / (2 delta) is a power of two), its (-1, -1) entries, ties,
the independence of Context.payload_locate_clip from its split, the entry points' refusals, and
extract_payload_video(search="clip") end to end on the scenarios whose precondition tests/test_payload_clip.py establishes."""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import payload_clip_refs as cl
import payload_keyed_sync_refs as kr
import payload_sync_refs as sr
import test_loop_trips as lt

pytestmark = pytest.mark.gpu

P = importlib.import_module(ge.PKG_NAME + ".payload")
video = importlib.import_module(ge.PKG_NAME + ".video")

F = np.float32
WIDE = (3, 5, 118, 180)                                                    # nx = 22, 3 placements across: a lane per window
SMALL = (40, 64, 48, 64)                                                   # nx = 8, 17 placements across: a lane per placement
NBY, NBX = 16, 24
TIES = [(24, 40, 5, 7), (16, 16, 3, 70), (24, 72, 5, 10)]                  # (h, w, nby, nbx)
# the second trips of the shared loop bodies (tests/test_loop_trips.py): a lane per placement with a group of 8 windows and a tail,
# a lane per window with nx = 65
TRIPS = list(lt.CLIP_TRIP_SHAPES.values())
TRIP_IDS = list(lt.CLIP_TRIP_SHAPES)
TIES += TRIPS


def _lanes_over_windows(w, nbx):
    """the entry point's choice (csrc/wm_payload.hip), restated only to see that the shapes below take both kernels"""
    nx, n_tx = w // 8, nbx - w // 8 + 1
    return nx * ((n_tx + 63) // 64) >= 2 * n_tx * ((nx + 63) // 64)


def test_the_shapes_take_both_lane_mappings():
    assert _lanes_over_windows(WIDE[3], NBX) and not _lanes_over_windows(SMALL[3], NBX)
    assert not _lanes_over_windows(8, NBX) and not _lanes_over_windows(9, NBX)      # the no-window planes
    assert [_lanes_over_windows(w, nbx) for _, w, _, nbx in TIES] == [False, False, True, False, True]
    assert [_lanes_over_windows(w, nbx) for _, w, _, nbx in TRIPS] == [False, True]
    assert not _lanes_over_windows(lt.CLIP_CHUNK_SHAPE[1], lt.CLIP_CHUNK_SHAPE[3])


def _tables(n):
    return np.stack([cl.frame_table("A", f) for f in range(n)])


@pytest.fixture(scope="module")
def scans(gpu_ctx):
    """crop -> the device's sigma_1 scans of frames 2 and 3 of the A video's crop (strided views)"""
    vid = cl.video("A-crop")
    return {crop: [gpu_ctx.payload_sigma1_scan(sr.crop_of(vid[f], crop)) for f in (2, 3)] for crop in (WIDE, SMALL)}


def _best_of_grids(grids):
    """(max, first row-major argmax) per phase of 64 score grids; (-1, -1) for an empty one"""
    out = np.full((64, 2), -1, np.int64)
    for p, g in enumerate(grids):
        if g.size:
            i = int(np.argmax(g))
            out[p] = (g.reshape(-1)[i], i)
    return out


# ---- against the existing keyed scores --------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", [WIDE, SMALL], ids=["lane-per-window", "lane-per-placement"])
@pytest.mark.parametrize("delta", [16.0, 24.0])
def test_one_anchor_one_candidate_is_the_argmax_of_the_keyed_scores(gpu_ctx, scans, crop, delta):
    _, _, h, w = crop
    U = _tables(3)
    grids = gpu_ctx.payload_keyed_scores(scans[crop][0], U[2], h, w, delta)
    best = gpu_ctx.payload_keyed_best(scans[crop][:1], U, np.array([[2]], np.int32), h, w, delta)
    assert best.dtype == np.int64 and best.shape == (1, 64, 2)
    assert np.array_equal(best[0], _best_of_grids(grids))
    if delta == 16.0:                                                      # the true candidate: frame 2's own table
        p = 8 * ((-crop[0]) % 8) + (-crop[1]) % 8
        n_tx = NBX - (w - p % 8) // 8 + 1
        assert P.pick_clip(best, P.phase_counts(h, w), [1]) == (0, p, (crop[0] + p // 8) // 8 * n_tx + (crop[1] + p % 8) // 8)


@pytest.mark.parametrize("crop", [WIDE, SMALL], ids=["lane-per-window", "lane-per-placement"])
def test_two_anchors_add_their_score_grids(gpu_ctx, scans, crop):
    _, _, h, w = crop
    U = _tables(4)
    g = {(a, t): gpu_ctx.payload_keyed_scores(scans[crop][a], U[t], h, w, 16.0) for a, t in ((0, 2), (1, 3), (0, 1), (1, 0))}
    tof = np.array([[2, 3], [1, 0], [2, -1], [-1, 3], [-1, -1], [1, 3]], np.int32)
    best = gpu_ctx.payload_keyed_best(scans[crop], U, tof, h, w, 16.0)

    def both(x, y):
        return _best_of_grids([a + b for a, b in zip(g[x], g[y])])
    assert np.array_equal(best[0], both((0, 2), (1, 3)))
    assert np.array_equal(best[1], both((0, 1), (1, 0)))
    assert np.array_equal(best[2], _best_of_grids(g[0, 2]))                # one entry -1: the single grid
    assert np.array_equal(best[3], _best_of_grids(g[1, 3]))
    assert np.all(best[4] == -1)                                           # a candidate without a marked anchor
    assert np.array_equal(best[5], both((0, 1), (1, 3)))
    again = gpu_ctx.payload_keyed_best(scans[crop], U, tof, h, w, 16.0)
    assert np.array_equal(best, again)


@pytest.mark.parametrize("shape", [(8, 8), (15, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_phase_without_a_window_gives_minus_one(gpu_ctx, shape):
    h, w = shape
    plane = cl.video("A-crop")[2][5:5 + h, 3:3 + w]
    scan = gpu_ctx.payload_sigma1_scan(plane)
    U = _tables(3)
    best = gpu_ctx.payload_keyed_best([scan, scan], U, np.array([[0, 1], [-1, 2]], np.int32), h, w, 16.0)
    want = cl.best_ref([scan, scan], list(U), [[0, 1], [-1, 2]], 16.0)
    assert np.array_equal(best, want)
    empty = [p for p in range(64) if scan[p // 8][p % 8].size == 0]
    assert len(empty) == (63 if shape == (8, 8) else 64 - 16) and np.all(best[:, empty] == -1) and np.all(best[:, 0] >= 0)


# ---- ties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,nby,nbx", TIES, ids=["placements-3-across", "placements-two-waves", "windows-2-across"] + TRIP_IDS)
def test_equal_scores_give_index_zero(gpu_ctx, h, w, nby, nbx):
    """a constant table: every placement of a phase reads the same lattices and scores alike - the first index must win,
    whichever wave or lane arrives first"""
    rng = np.random.default_rng(h * w)
    scan = [[rng.uniform(0.0, 2040.0, sr.phase_shape(h, w, py, px)).astype(F) for px in range(8)] for py in range(8)]
    U = np.stack([np.full((nby, nbx), 12345, np.uint16), np.zeros((nby, nbx), np.uint16)])
    best = gpu_ctx.payload_keyed_best([scan, scan], U, np.array([[0, 1], [1, -1]], np.int32), h, w, 16.0)
    grids = [gpu_ctx.payload_keyed_scores(scan, U[t], h, w, 16.0) for t in (0, 1)]
    for p in range(64):
        if scan[p // 8][p % 8].size == 0:
            assert np.all(best[:, p] == -1)
            continue
        assert grids[0][p].size > 1 and np.all(grids[0][p] == grids[0][p].flat[0])
        assert tuple(best[0, p]) == (grids[0][p].flat[0] + grids[1][p].flat[0], 0), p
        assert tuple(best[1, p]) == (grids[1][p].flat[0], 0), p


# ---- against the restatement ------------------------------------------------------------------------------------------
TOF = np.array([[2, 3], [3, 2], [0, -1], [1, 2], [-1, -1]], np.int32)


@pytest.mark.parametrize("delta", [8.0, 16.0, 512.0])
def test_best_of_the_device_scans_is_bit_equal_to_the_restatement(gpu_ctx, scans, delta):
    """1 / (2 delta) is a power of two: nothing for a compiler to contract, every vote equal, every sum equal"""
    U = _tables(4)
    for crop in (WIDE, SMALL):
        got = gpu_ctx.payload_keyed_best(scans[crop], U, TOF, crop[2], crop[3], delta)
        assert np.array_equal(got, cl.best_ref(scans[crop], list(U), TOF, delta)), crop


def test_best_at_delta_24_agrees_within_one_unit_per_window_and_anchor(gpu_ctx, scans):
    """1 / 48 is no power of two: a vote may differ by a unit (tests/test_gpu_payload_keyed_sync.py), a candidate's score by
    at most its windows times its marked anchors; the index is not compared"""
    U = _tables(4)
    for crop in (WIDE, SMALL):
        got = gpu_ctx.payload_keyed_best(scans[crop], U, TOF, crop[2], crop[3], 24.0)
        want = cl.best_ref(scans[crop], list(U), TOF, 24.0)
        bound = np.asarray(kr.counts_ref(crop[2], crop[3]))[None, :] * (TOF >= 0).sum(axis=1)[:, None]
        worst = np.abs(got[..., 0] - want[..., 0])
        print(f"{crop}: worst |score_dev - score_ref| {int(worst.max())}, bound there {int(bound.reshape(-1)[worst.argmax()])}")
        assert np.all(worst <= bound)
        assert np.array_equal(got[..., 1] < 0, want[..., 1] < 0)


# ---- second trips: the loops inside a placement, and the candidates past one launch -----------------------------------
def _synthetic_scan(h, w, seed):
    rng = np.random.default_rng(seed)
    return [[rng.uniform(0.0, 2040.0, sr.phase_shape(h, w, py, px)).astype(F) for px in range(8)] for py in range(8)]


@pytest.mark.parametrize("h,w,nby,nbx", TRIPS, ids=TRIP_IDS)
def test_second_trips_of_the_window_loops_are_bit_equal_to_the_restatement(gpu_ctx, h, w, nby, nbx):
    """two anchors' synthetic scans, the rows of TOF, random, all-0 and all-65535 tables at delta 16 (a power of two: bit for bit,
    as test_best_of_the_device_scans_is_bit_equal_to_the_restatement has it)"""
    rng = np.random.default_rng(h * w + nbx)
    scans = [_synthetic_scan(h, w, h * 100 + w + a) for a in range(2)]
    U = np.stack([rng.integers(0, 65536, (nby, nbx), dtype=np.uint16), rng.integers(0, 65536, (nby, nbx), dtype=np.uint16),
                  np.zeros((nby, nbx), np.uint16), np.full((nby, nbx), 65535, np.uint16)])
    got = gpu_ctx.payload_keyed_best(scans, U, TOF, h, w, 16.0)
    assert np.array_equal(got, cl.best_ref(scans, list(U), TOF, 16.0))
    gpu_ctx.check_status()


@pytest.fixture(scope="module")
def chunked():
    """(scan, tables, table_of [2047, 1], best_ref of all of them): made once; a candidate's row does not depend on the others, so
    the first n rows are the reference of a call with n candidates"""
    h, w, nby, nbx = lt.CLIP_CHUNK_SHAPE
    rng = np.random.default_rng(lt.CLIP_CHUNK)
    scan = _synthetic_scan(h, w, 7)
    U = rng.integers(0, 65536, (lt.CLIP_CHUNK_TABLES, nby, nbx), dtype=np.uint16)
    tof = rng.integers(-1, lt.CLIP_CHUNK_TABLES, (max(lt.CLIP_CHUNK_CANDS), 1)).astype(np.int32)
    tof[lt.CLIP_CHUNK - 1:lt.CLIP_CHUNK + 2, 0] = (0, 1, 2)                  # candidates 1022, 1023, 1024: three different tables
    want = cl.best_ref([scan], list(U), tof, 16.0)
    assert len({want[c].tobytes() for c in range(lt.CLIP_CHUNK - 1, lt.CLIP_CHUNK + 2)}) == 3   # a shift by one row shows
    assert set(tof.reshape(-1).tolist()) == set(range(-1, lt.CLIP_CHUNK_TABLES))
    want.setflags(write=False); tof.setflags(write=False)
    return scan, U, tof, want


@pytest.mark.parametrize("n_cand", lt.CLIP_CHUNK_CANDS)
def test_candidates_past_one_launch(gpu_ctx, chunked, n_cand):
    """wm_payload_keyed_best_dev hands its candidates to the kernel 1023 at a launch: one launch, two (the second of one and of
    two candidates) and three, bit-equal to the restatement"""
    scan, U, tof, want = chunked
    h, w, _, _ = lt.CLIP_CHUNK_SHAPE
    got = gpu_ctx.payload_keyed_best([scan], U, np.ascontiguousarray(tof[:n_cand]), h, w, 16.0)
    bad = np.flatnonzero((got != want[:n_cand]).any(axis=(1, 2)))
    print(f"{n_cand} candidates: {bad.size} rows differ (first {bad[:3].tolist()}, last {bad[-3:].tolist()})")
    assert got.shape == (n_cand, 64, 2) and bad.size == 0
    gpu_ctx.check_status()


def test_locate_clip_past_one_launch_does_not_depend_on_its_split(gpu_ctx, chunked):
    """Context.payload_locate_clip with its default split passes all 1025 candidates to one call of the library, whose own loop
    splits them; runs of 100 never reach that loop"""
    _, U, tof, _ = chunked
    h, w, _, _ = lt.CLIP_CHUNK_SHAPE
    plane = np.random.default_rng(3).integers(0, 256, (1, h, w), dtype=np.uint8)
    rows = np.ascontiguousarray(tof[:lt.CLIP_LOCATE_CANDS])
    one = gpu_ctx.payload_locate_clip(plane, U, rows, 16.0)
    part = gpu_ctx.payload_locate_clip(plane, U, rows, 16.0, cands_per_call=100)
    assert one.shape == (lt.CLIP_LOCATE_CANDS, 64, 2) and np.array_equal(one, part)
    marked = rows[:, 0] >= 0
    assert np.all(one[marked, 0, 0] >= 0) and np.all(one[~marked] == -1)
    assert np.array_equal(one, gpu_ctx.payload_keyed_best([gpu_ctx.payload_sigma1_scan(plane[0])], U, rows, h, w, 16.0))


# ---- the resident chain -----------------------------------------------------------------------------------------------
def test_locate_clip_does_not_depend_on_its_split(gpu_ctx):
    sc = cl.scenario("A-fi2")
    clip = cl.cut(cl.video("A-fi2"), sc)
    tof = P.clip_table_of(sc["F"], sc["fi"], sc["n_c"], 4)
    U = np.stack([cl.frame_table("A", k * 2) for k in range(4)])
    one = gpu_ctx.payload_locate_clip(clip, U, tof, 16.0)
    assert one.shape == (4, 64, 2) and np.all(one[:, 0, 0] >= 0)
    for per_call in (1, 2, 3):
        part, win = gpu_ctx.payload_locate_clip(clip, U, tof, 16.0, pick=True, cands_per_call=per_call)
        assert np.array_equal(part, one), per_call
    r = cl.located("A-fi2")
    assert win == (r["first_frame"], r["phase"], r["place"])
    scans = [gpu_ctx.payload_sigma1_scan(clip[a]) for a in range(4)]
    assert np.array_equal(one, gpu_ctx.payload_keyed_best(scans, U, tof, clip.shape[1], clip.shape[2], 16.0))
    # a run whose candidates have no marked anchor: (-1, -1) without a call
    tof3 = P.clip_table_of(7, 3, 2, 2)
    U3 = np.stack([cl.frame_table("A", k * 3) for k in range(3)])
    b3 = gpu_ctx.payload_locate_clip(clip[:2], U3, tof3, 16.0, cands_per_call=1)
    assert np.array_equal(b3, gpu_ctx.payload_locate_clip(clip[:2], U3, tof3, 16.0))
    assert np.all(b3[[1, 4]] == -1) and np.all(b3[[0, 2, 3, 5], 0, 0] >= 0)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_the_library_refuses_bad_arguments(gpu_ctx, hostapi):
    h, w, nby, nbx = 40, 56, 5, 7
    s1 = np.zeros((2, 64, 35), F)
    U = np.zeros(3 * nby * nbx + 1, np.uint16)
    tof = np.array([[0, 1], [-1, 2]], np.int32)
    best = np.zeros((2, 64, 2), np.int64)
    p = hostapi._p
    good = dict(s1=p(s1), A=2, U=p(U), T=3, tof=p(tof), C=2, best=p(best), h=h, w=w, nby=nby, nbx=nbx, delta=16.0)
    both = [dict(nby=4), dict(nbx=6), dict(h=7), dict(w=7), dict(delta=7.5), dict(delta=513.0), dict(delta=float("nan")),
            dict(A=0), dict(T=0), dict(C=0), dict(A=-1), dict(U=None), dict(U=hostapi._vp(U.ctypes.data + 1)), dict(s1=None),
            dict(tof=None), dict(best=None),
            dict(h=4096, w=4096, nby=512, nbx=512, A=64)]                   # 2^18 tiles x 64 anchors = 2^24
    dev_only = [dict(s1=hostapi._vp(s1.ctypes.data + 2)), dict(tof=hostapi._vp(tof.ctypes.data + 2)),
                dict(best=hostapi._vp(best.ctypes.data + 4))]
    for name, cases in (("wm_payload_keyed_best", both), ("wm_payload_keyed_best_dev", both + dev_only)):
        for change in cases:
            a = dict(good, **change)
            with pytest.raises(ValueError):
                gpu_ctx._call(name, a["s1"], a["A"], a["U"], a["T"], a["tof"], a["C"], a["best"], a["h"], a["w"], a["nby"], a["nbx"],
                              a["delta"])
    for entry in (3, -2, 2 ** 31 - 1):                                     # the host form reads table_of
        bad = tof.copy()
        bad[1, 0] = entry
        with pytest.raises(ValueError, match="table_of"):
            gpu_ctx._call("wm_payload_keyed_best", p(s1), 2, p(U), 3, p(bad), 2, p(best), h, w, nby, nbx, 16.0)
    assert not best.any()
    gpu_ctx.sync()
    gpu_ctx.check_status()
    gpu_ctx._call("wm_payload_keyed_best", p(s1), 2, p(U), 3, p(tof), 2, p(best), h, w, nby, nbx, 16.0)     # and the good call runs
    assert np.all(best[0, :, 0] >= 0) and np.all(best[..., 1] <= 0)


# ---- end to end -------------------------------------------------------------------------------------------------------
def _read_luma(path):
    vid = video.Y4M(path)
    try:
        return np.stack([y.copy() for _, y, _ in vid])
    finally:
        vid.close()


@pytest.fixture(scope="module")
def embedded(tmp_path_factory):
    """(case, F, fi, code) -> (the product's marked video as uint8 [F, H, W], its file, its meta file)"""
    root = tmp_path_factory.mktemp("clip")
    made = {}

    def get(name):
        sc = cl.scenario(name)
        k = (sc["case"], sc["F"], sc["fi"], sc["code"])
        if k not in made:
            tag = "_".join(map(str, k))
            host, out, meta = (str(root / f"{tag}_{x}") for x in ("host.y4m", "marked.y4m", "meta.npz"))
            video.write_y4m(host, cl.hosts(name))
            video.embed_payload_video(host, sc["data"], out, meta, password=sr.PASSWORD, payload_type="bytes", frame_interval=sc["fi"],
                                      nonce=sr.NONCE, dither=True, code=sc["code"])
            made[k] = (_read_luma(out), out, meta)
        return made[k]
    return get


@pytest.mark.parametrize("name", list(cl.SCENARIOS))
def test_a_cut_cropped_clip_decodes_and_names_its_place(embedded, tmp_path, name):
    """The data, valid, origin and first_frame of every scenario, and the confidence against the restatement run on the same
    clip file.  A-48x64 keeps 48 tiles for an 80-bit frame: it is found like the others, every bit that keeps a tile reads
    right, and the frame check fails as it must."""
    sc = cl.scenario(name)
    frames, _, meta = embedded(name)
    clip = cl.cut(frames, sc)
    path = str(tmp_path / "clip.y4m")
    video.write_y4m(path, clip)
    ref = cl.locate_clip_ref(clip, sc["case"], sc["F"], sc["fi"], sc["code"], sc["anchors"])
    assert cl.is_true(ref, sc)
    got, valid, conf, origin, first, soft = video.extract_payload_video(path, meta, password=sr.PASSWORD, search="clip", batch=2,
                                                                        anchors=sc["anchors"], return_soft=True)
    print(f"{name}: first frame {first}, origin {origin}, valid {valid}, confidence {conf:.5f}, the restatement's "
          f"{ref['confidence']:.5f} (gap {ref['gap']:.3f})")
    assert origin == sc["crop"][:2] and first == sc["t0"]
    assert abs(conf - ref["confidence"]) <= 1e-4
    if name == "A-48x64":
        _, carried, _ = cl.case_map(sc["case"], sc["code"])
        have = ref["count"] > 0
        assert np.array_equal(soft[have] < 0, carried[have] != 0) and not soft[~have].any()
        assert valid is False and valid == ref["valid"]
    else:
        assert got == sc["data"] and valid is True
    assert video.extract_payload_video(path, meta, password=sr.PASSWORD, search="clip", anchors=sc["anchors"])[:2] == (got, valid)


def test_the_default_extract_is_unchanged(embedded):
    """search=None on the uncut file: the same three values as before, and the clip search agrees with them"""
    _, out, meta = embedded("A-crop")
    plain = video.extract_payload_video(out, meta, password=sr.PASSWORD)
    assert len(plain) == 3 and plain[0] == b"id" and plain[1] is True and 0.7 < plain[2] <= 1.0
    with_soft = video.extract_payload_video(out, meta, password=sr.PASSWORD, return_soft=True, search=None)
    assert len(with_soft) == 4 and with_soft[:3] == plain and with_soft[3].shape == (80,)
    got, valid, conf, origin, first = video.extract_payload_video(out, meta, password=sr.PASSWORD, search="clip")
    assert (got, valid, origin, first) == (b"id", True, (0, 0), 0)
    assert conf == pytest.approx(plain[2], abs=1e-4)                       # (votes are m rounded to 2^-15)


def test_a_cropped_file_without_the_search_is_still_refused(embedded, tmp_path, monkeypatch):
    frames, _, meta = embedded("A-crop")
    path = str(tmp_path / "clip.y4m")
    video.write_y4m(path, cl.cut(frames, cl.scenario("A-crop")))
    with pytest.raises(ValueError, match="the meta was written for"):
        video.extract_payload_video(path, meta, password=sr.PASSWORD)

    def refuse(*a, **k):
        raise AssertionError("a refusal must come before a context is created")
    monkeypatch.setattr(video.hostapi, "Context", refuse)
    with pytest.raises(ValueError, match="anchors"):
        video.extract_payload_video(path, meta, password=sr.PASSWORD, search="clip", anchors=0)
    big = str(tmp_path / "big.y4m")
    video.write_y4m(big, np.zeros((7, 64, 64), np.uint8))
    with pytest.raises(ValueError, match="7 frames"):
        video.extract_payload_video(big, meta, password=sr.PASSWORD, search="clip")
