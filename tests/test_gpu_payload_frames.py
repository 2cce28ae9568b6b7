"""Frame resynchronisation of the dithered blind payload on the device: wm_payload_frame_scores against the restatement
(tests/payload_frames_refs.py; integer arithmetic: bit for bit where 1 / (2 delta) is a power of two) and against the existing
keyed scores of the same device scan (bit for bit at every delta: the same keyed_abs_vote), its edges, strides and second
trips, the independence of Context.payload_match_frames from its split, the entry points' refusals, and
extract_payload_video(search="frames") end to end on the scenarios whose precondition tests/test_payload_frames.py establishes."""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import payload_clip_refs as cl
import payload_frames_refs as fr
import payload_sync_refs as sr

pytestmark = pytest.mark.gpu

P = importlib.import_module(ge.PKG_NAME + ".payload")
video = importlib.import_module(ge.PKG_NAME + ".video")

F = np.float32
SMALL = (40, 64, 48, 64)                                                    # a crop of case A: 6 x 8 windows at phase (0, 0)


def _synthetic(n_frames, n_tables, ny, nx, nby, nbx, seed):
    """seeded sigma_1 values in [0, 2040] and seeded tables: the frames themselves are not the point"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 2040.0, (n_frames, ny, nx)).astype(F), rng.integers(0, 65536, (n_tables, nby, nbx), dtype=np.uint16))


def _raw(ctx, hostapi, s1, wstride, fstride, n_frames, tables, ny, nx, ty, tx, delta, scores=None, name="wm_payload_frame_scores"):
    """the host-pointer entry point on a flat float32 array with strides of the caller's choosing"""
    n_tables, nby, nbx = tables.shape
    if scores is None:
        scores = np.full((n_frames, n_tables), -7, np.int64)               # (the entry point zeroes before it adds)
    ctx._call(name, hostapi._p(s1), wstride, fstride, n_frames, hostapi._p(tables), n_tables, hostapi._p(scores), ny, nx, nby, nbx,
              ty, tx, delta)
    return scores


# ---- against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [8.0, 16.0, 512.0])
def test_scores_are_bit_equal_to_the_restatement(gpu_ctx, delta):
    """1 / (2 delta) is a power of two: nothing for a compiler to contract, every vote equal, every sum equal"""
    s1, U = _synthetic(9, 17, 7, 11, 9, 14, 1)
    got = gpu_ctx.payload_frame_scores(s1, U, 7, 11, 1, 2, delta)
    assert got.dtype == np.int64 and got.shape == (9, 17)
    assert np.array_equal(got, fr.frame_scores_ref(s1, U, 7, 11, 1, 2, delta))
    assert np.array_equal(got, gpu_ctx.payload_frame_scores(s1, U, 7, 11, 1, 2, delta))
    gpu_ctx.check_status()


def test_scores_at_delta_24_agree_within_one_unit_per_window(gpu_ctx):
    """1 / 48 is no power of two: the device contracts x - floor(x) and a vote may differ by a unit"""
    s1, U = _synthetic(9, 17, 7, 11, 9, 14, 2)
    got = gpu_ctx.payload_frame_scores(s1, U, 7, 11, 1, 2, 24.0)
    worst = np.abs(got - fr.frame_scores_ref(s1, U, 7, 11, 1, 2, 24.0))
    print(f"worst |score_dev - score_ref| {int(worst.max())} over {7 * 11} windows")
    assert np.all(worst <= 7 * 11)


# ---- against the existing device path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [16.0, 24.0])
def test_scores_are_the_keyed_scores_of_the_same_scan(gpu_ctx, delta):
    """score[f][k] is payload_keyed_scores(scan of frame f, tables[k]) at the phase and the place: the same keyed_abs_vote on
    the same device, bit for bit whatever delta"""
    vid = cl.video("A-crop")
    _, _, h, w = SMALL
    U = np.stack([cl.frame_table("A", f) for f in range(3)])
    scans = [gpu_ctx.payload_sigma1_scan(sr.crop_of(vid[f], SMALL)) for f in (2, 3)]
    for (py, px), (ty, tx) in (((0, 0), (5, 8)), ((3, 5), (0, 0)), ((7, 7), (11, 17)), ((0, 7), (2, 17))):
        ny, nx = sr.phase_shape(h, w, py, px)
        s1 = np.stack([scan[py][px] for scan in scans])
        got = gpu_ctx.payload_frame_scores(s1, U, ny, nx, ty, tx, delta)
        for f, scan in enumerate(scans):
            for k in range(3):
                grid = gpu_ctx.payload_keyed_scores(scan, U[k], h, w, delta)[8 * py + px]
                assert grid.shape == (16 - ny + 1, 24 - nx + 1)
                assert got[f, k] == grid[ty, tx], ((py, px), (ty, tx), f, k)
    # frame 2's own table scores highest at the true phase and place
    assert int(np.argmax(gpu_ctx.payload_frame_scores(scans[0][0][0][None], U, 6, 8, 5, 8, 16.0)[0])) == 2


# ---- edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", [1, fr.FRAME_FB - 1, fr.FRAME_FB + 1])
@pytest.mark.parametrize("n_tables", [1, fr.FRAME_TB + 1, 2 * fr.FRAME_TB + 1])
def test_frames_and_tables_beside_their_blocks(gpu_ctx, n_frames, n_tables):
    s1, U = _synthetic(n_frames, n_tables, 5, 9, 7, 12, n_frames * 100 + n_tables)
    assert np.array_equal(gpu_ctx.payload_frame_scores(s1, U, 5, 9, 2, 3, 16.0), fr.frame_scores_ref(s1, U, 5, 9, 2, 3, 16.0))


@pytest.mark.parametrize("ny,nx", [(1, 1), (7, 9), (5, 13), (63, 1), (1, 65)], ids=lambda v: str(v))
def test_window_counts_beside_the_wave(gpu_ctx, ny, nx):
    """1, 63 and 65 windows, one column and one row, each at the first and at the last place of a table that is wider than the
    window grid (a kernel that strides the table by nx fails the second)"""
    nby, nbx = ny + 3, nx + 4
    s1, U = _synthetic(3, 3, ny, nx, nby, nbx, ny * 1000 + nx)
    assert ny * nx in (1, 63, 65)
    for ty, tx in ((0, 0), (nby - ny, nbx - nx)):
        got = gpu_ctx.payload_frame_scores(s1, U, ny, nx, ty, tx, 16.0)
        assert np.array_equal(got, fr.frame_scores_ref(s1, U, ny, nx, ty, tx, 16.0)), (ty, tx)
    assert not np.array_equal(gpu_ctx.payload_frame_scores(s1, U, ny, nx, 0, 0, 16.0), got)      # (the place matters)
    gpu_ctx.check_status()


@pytest.mark.parametrize("wstride,fstride", [(1, 35), (8, 280), (1, 100), (8, 1000), (3, 105)])
def test_window_and_frame_strides(gpu_ctx, hostapi, wstride, fstride):
    """window stride 1 (a dense grid) and 8 (the sigma pass's output read in place), the frame stride the grid's own size and
    larger; the floats between the windows and behind a frame's grid are never read into a score"""
    n, ny, nx = 3, 5, 7
    s1, U = _synthetic(n, 4, ny, nx, 6, 9, wstride * 10 + fstride)
    flat = np.full((n - 1) * fstride + (ny * nx - 1) * wstride + 1, np.nan, F)
    for f in range(n):
        flat[f * fstride:f * fstride + ny * nx * wstride:wstride] = s1[f].reshape(-1)
    want = fr.frame_scores_ref(s1, U, ny, nx, 1, 2, 16.0)
    assert np.array_equal(_raw(gpu_ctx, hostapi, flat, wstride, fstride, n, U, ny, nx, 1, 2, 16.0), want)


def test_a_table_of_zeros_and_sigma_on_lattice_points_is_full_scale(gpu_ctx):
    ny, nx = 6, 11
    k = np.random.default_rng(4).integers(0, 60, (3, ny, nx))
    for delta in (8.0, 16.0, 24.0):
        s1 = (k * (2.0 * delta)).astype(F)                                 # (2 delta k is exact in float32)
        got = gpu_ctx.payload_frame_scores(s1, np.zeros((2, ny, nx), np.uint16), ny, nx, 0, 0, delta)
        assert np.all(got == P.VOTE_ONE * ny * nx), delta


# ---- second trips -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fr.TRIPS))
def test_second_trips_are_bit_equal_to_the_restatement(gpu_ctx, name):
    """one past the lane loop, the chunk, the blocks and each capped grid dimension (payload_frames_refs.TRIPS, held against
    the source by tests/test_payload_frames.py), at delta 16: bit for bit"""
    n_frames, n_tables, ny, nx, nby, nbx, ty, tx = fr.TRIPS[name]
    s1, U = _synthetic(n_frames, n_tables, ny, nx, nby, nbx, len(name))
    got = gpu_ctx.payload_frame_scores(s1, U, ny, nx, ty, tx, 16.0)
    want = fr.frame_scores_ref(s1, U, ny, nx, ty, tx, 16.0)
    bad = np.argwhere(got != want)
    print(f"{name}: {len(bad)} of {got.size} scores differ (first {bad[:3].tolist()}, last {bad[-3:].tolist()})")
    assert len(bad) == 0
    gpu_ctx.check_status()


# ---- the resident chain -----------------------------------------------------------------------------------------------
def test_match_frames_does_not_depend_on_its_split(gpu_ctx):
    sc = fr.scenario("A-shuffle")
    clip = fr.edit(fr.video("A-shuffle"), sc)
    y0, x0, h, w = sc["crop"]
    py, px = (-y0) % 8, (-x0) % 8
    ny, nx = sr.phase_shape(h, w, py, px)
    ty, tx = (y0 + py) // 8, (x0 + px) // 8
    view = clip[:, py:py + 8 * ny, px:px + 8 * nx]                          # (a strided view)
    U = np.stack([cl.frame_table("A", k) for k in range(sc["F"])])
    scores, s1 = gpu_ctx.payload_match_frames(view, U, ty, tx, 16.0)
    assert scores.dtype == np.int64 and scores.shape == (5, 8) and s1.dtype == F and s1.shape == (5, ny, nx)
    assert np.array_equal(s1, gpu_ctx.sigma_tiles(np.ascontiguousarray(view))[..., 0])
    assert np.array_equal(scores, gpu_ctx.payload_frame_scores(s1, U, ny, nx, ty, tx, 16.0))
    assert np.array_equal(scores, fr.frame_scores_ref(s1, U, ny, nx, ty, tx, 16.0))
    for per_call in (1, 2, 3, 8):
        part, s1_again = gpu_ctx.payload_match_frames(view, U, ty, tx, 16.0, tables_per_call=per_call)
        assert np.array_equal(part, scores) and np.array_equal(s1_again, s1), per_call
    assert (P.pick_frames(scores, ny * nx) * sc["fi"]).tolist() == sc["frame_map"]


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_the_library_refuses_bad_arguments(gpu_ctx, hostapi):
    ny, nx, nby, nbx = 5, 7, 6, 9
    s1 = np.zeros((2, ny, nx), F)
    U = np.zeros(3 * nby * nbx + 1, np.uint16)
    scores = np.full((2, 3), -7, np.int64)
    p, vp = hostapi._p, hostapi._vp
    good = dict(s1=p(s1), ws=1, fs=ny * nx, F=2, U=p(U), T=3, sc=p(scores), ny=ny, nx=nx, nby=nby, nbx=nbx, ty=1, tx=2, delta=16.0)
    bad = [dict(s1=None), dict(U=None), dict(sc=None), dict(U=vp(U.ctypes.data + 1)), dict(s1=vp(s1.ctypes.data + 2)),
           dict(sc=vp(scores.ctypes.data + 4)), dict(F=0), dict(F=-1), dict(T=0), dict(ny=0), dict(nx=0), dict(nx=-3),
           dict(ty=-1), dict(tx=-1), dict(ty=2), dict(tx=3), dict(nby=5), dict(nbx=8), dict(ws=0),
           dict(delta=7.5), dict(delta=513.0), dict(delta=float("nan"))]
    for name in ("wm_payload_frame_scores", "wm_payload_frame_scores_dev"):
        for change in bad:
            a = dict(good, **change)
            with pytest.raises(ValueError):
                gpu_ctx._call(name, a["s1"], a["ws"], a["fs"], a["F"], a["U"], a["T"], a["sc"], a["ny"], a["nx"], a["nby"], a["nbx"],
                              a["ty"], a["tx"], a["delta"])
    assert np.all(scores == -7)                                            # every refusal left the scores untouched
    gpu_ctx.sync()
    gpu_ctx.check_status()
    a = good                                                                # and the good call runs: zeros on the zero lattice
    gpu_ctx._call("wm_payload_frame_scores", a["s1"], a["ws"], a["fs"], a["F"], a["U"], a["T"], a["sc"], a["ny"], a["nx"], a["nby"],
                  a["nbx"], a["ty"], a["tx"], a["delta"])
    assert np.all(scores == P.VOTE_ONE * ny * nx)


def test_context_methods_validate_before_the_c_abi(gpu_ctx):
    s1, U = _synthetic(2, 3, 5, 7, 6, 9, 0)
    for args in ((s1, U, 5, 7, 2, 2), (s1, U, 5, 7, 1, 3), (s1, U, 5, 7, -1, 0), (s1, U, 5, 6, 0, 0), (s1[0], U, 5, 7, 0, 0),
                 (s1, U[0], 5, 7, 0, 0), (s1[:0], U, 5, 7, 0, 0), (s1, U[:0], 5, 7, 0, 0)):
        with pytest.raises(ValueError):
            gpu_ctx.payload_frame_scores(*args, 16.0)
    with pytest.raises(ValueError, match="delta"):
        gpu_ctx.payload_frame_scores(s1, U, 5, 7, 0, 0, 7.0)
    planes = np.zeros((2, 40, 56), np.uint8)
    for view, ty, tx in ((planes, 2, 0), (planes, 0, 3), (planes[:, :39], 0, 0), (planes[0], 0, 0), (planes.astype(F), 0, 0)):
        with pytest.raises(ValueError):
            gpu_ctx.payload_match_frames(view, U, ty, tx, 16.0)


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
    root = tmp_path_factory.mktemp("frames")
    made = {}

    def get(name):
        sc = fr.scenario(name)
        k = (sc["case"], sc["F"], sc["fi"], sc["code"])
        if k not in made:
            tag = "_".join(map(str, k))
            host, out, meta = (str(root / f"{tag}_{x}") for x in ("host.y4m", "marked.y4m", "meta.npz"))
            video.write_y4m(host, fr.hosts(name))
            video.embed_payload_video(host, sc["data"], out, meta, password=sr.PASSWORD, payload_type="bytes", frame_interval=sc["fi"],
                                      nonce=sr.NONCE, dither=True, code=sc["code"])
            made[k] = (_read_luma(out), out, meta)
        return made[k]
    return get


@pytest.mark.parametrize("name", list(fr.SCENARIOS))
def test_an_edited_file_decodes_and_names_its_frames(embedded, tmp_path, name):
    """The data, valid, origin and frame_map of every scenario through files, and the confidence against the restatement run on
    the same file (whose precondition the restatement's own video establishes in tests/test_payload_frames.py)"""
    sc = fr.scenario(name)
    frames, _, meta = embedded(name)
    clip = fr.edit(frames, sc)
    path = str(tmp_path / "file.y4m")
    video.write_y4m(path, clip)
    ref = fr.match_frames_ref(clip, sc["case"], sc["F"], sc["fi"], sc["code"], sc["anchors"])
    assert fr.meets_precondition(ref, sc)
    got, valid, conf, origin, fmap, soft = video.extract_payload_video(path, meta, password=sr.PASSWORD, search="frames", batch=2,
                                                                       anchors=sc["anchors"], return_soft=True)
    print(f"{name}: origin {origin}, frame_map {fmap.tolist()}, valid {valid}, confidence {conf:.5f}, the restatement's "
          f"{ref['confidence']:.5f} (gaps {ref['gaps'].min():.3f} - {ref['gaps'].max():.3f})")
    assert got == sc["data"] and valid is True and origin == sc["crop"][:2]
    assert fmap.dtype == np.int32 and fmap.tolist() == sc["frame_map"]
    assert abs(conf - ref["confidence"]) <= 1e-4
    assert soft.shape == ref["soft"].shape
    again = video.extract_payload_video(path, meta, password=sr.PASSWORD, search="frames", anchors=sc["anchors"])
    assert len(again) == 5 and again[:4] == (got, valid, conf, origin) and again[4].tolist() == sc["frame_map"]


def test_the_default_extract_and_the_clip_search_are_unchanged(embedded):
    """search=None and search="clip" on the unedited file: the values they had, and the frame search agrees with them"""
    _, out, meta = embedded("A-shuffle")
    plain = video.extract_payload_video(out, meta, password=sr.PASSWORD)
    assert len(plain) == 3 and plain[0] == b"id" and plain[1] is True and 0.7 < plain[2] <= 1.0
    with_soft = video.extract_payload_video(out, meta, password=sr.PASSWORD, return_soft=True, search=None)
    assert len(with_soft) == 4 and with_soft[:3] == plain and with_soft[3].shape == (80,)
    got, valid, conf, origin, first = video.extract_payload_video(out, meta, password=sr.PASSWORD, search="clip")
    assert (got, valid, origin, first) == (b"id", True, (0, 0), 0) and conf == pytest.approx(plain[2], abs=1e-4)
    got, valid, conf2, origin, fmap = video.extract_payload_video(out, meta, password=sr.PASSWORD, search="frames")
    assert (got, valid, origin) == (b"id", True, (0, 0)) and fmap.tolist() == list(range(8))
    assert conf2 == pytest.approx(plain[2], abs=1e-4)


def test_a_file_that_carries_nothing_gives_the_empty_result(embedded, tmp_path):
    _, _, meta = embedded("A-shuffle")
    path = str(tmp_path / "bare.y4m")
    video.write_y4m(path, np.stack([fr.foreign_frame("A", i) for i in range(2)])[:, 8:72, 16:112])
    out = video.extract_payload_video(path, meta, password=sr.PASSWORD, search="frames", return_soft=True)
    assert out[:4] == (b"", False, 0.0, None) and out[4].tolist() == [-1, -1] and not out[5].any()
