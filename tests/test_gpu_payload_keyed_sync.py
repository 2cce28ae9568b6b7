"""Keyed crop resynchronisation of the dithered blind payload on the device: the sigma_1 scan against the sigma pass (bit
for bit) and the oracle (under the sigma bar), the keyed scan's scores against the restatement run on the device's own
sigma_1 (tests/payload_keyed_sync_refs.py; integer arithmetic: bit for bit where 1 / (2 delta) is a power of two), and
extract_payload[_arrays](search="crop-keyed") end to end on the cases whose precondition tests/test_payload_keyed_sync.py
establishes."""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import payload_keyed_sync_refs as kr
import payload_refs as pr
import test_loop_trips as lt

pytestmark = pytest.mark.gpu

P = importlib.import_module(ge.PKG_NAME + ".payload")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
core = importlib.import_module(ge.PKG_NAME + ".dct_svd_core_secure")

A_CROPS = kr.CASES["A"]["crops"]
CASE_A = A_CROPS[0]                                                        # (3, 5, 118, 180)
F = np.float32


def _phases():
    return [(py, px) for py in range(8) for px in range(8)]


@pytest.fixture(scope="module")
def scan_a(gpu_ctx):
    """the device's sigma_1 scan of the Case A crop of the dithered stego, passed as a strided view"""
    view = kr.crop_of(kr.marked("A", 1), CASE_A)
    assert not view.flags.c_contiguous
    return gpu_ctx.payload_sigma1_scan(view)


# ---- sigma_1 scan -----------------------------------------------------------------------------------------------------
def _check_scan_against_sigma_pass(gpu_ctx, plane, grids):
    h, w = plane.shape
    for py, px in _phases():
        ny, nx = kr.phase_shape(h, w, py, px)
        g = grids[py][px]
        assert g.dtype == F and g.shape == (ny, nx), (py, px)
        if ny * nx:
            want = gpu_ctx.sigma_tiles(plane[py:py + 8 * ny, px:px + 8 * nx])[..., 0]
            assert np.array_equal(g, want), (py, px)


def test_scan_equals_the_sigma_pass_bit_for_bit(gpu_ctx, scan_a):
    """every phase's grid is sigma_tiles of that phase's window block: the same code on the same bytes"""
    _check_scan_against_sigma_pass(gpu_ctx, kr.crop_of(kr.marked("A", 1), CASE_A), scan_a)


def test_scan_of_a_strided_batch(gpu_ctx, scan_a):
    y0, x0, h, w = CASE_A
    both = np.stack([kr.marked("A", 1), kr.marked("A", 2)])[:, y0:y0 + h, x0:x0 + w]
    assert not both.flags.c_contiguous
    grids = gpu_ctx.payload_sigma1_scan(both)
    for py, px in _phases():
        assert grids[py][px].shape == (2,) + scan_a[py][px].shape
        assert np.array_equal(grids[py][px][0], scan_a[py][px]), (py, px)
    _check_scan_against_sigma_pass(gpu_ctx, both[1], [[g[1] for g in row] for row in grids])


def test_scan_follows_the_oracle(scan_a):
    ref = kr.located("A", 1, CASE_A)["s1"]
    worst = 0.0
    for py, px in _phases():
        rel = np.abs(scan_a[py][px].astype(np.float64) - ref[py][px]) / np.maximum(ref[py][px], 1e-30)
        worst = max(worst, float(rel.max()))
    print(f"worst |s1_dev - s1_ref| / s1_ref {worst:.2e} (bar {pr.SIGMA_RTOL:.0e})")
    assert worst <= pr.SIGMA_RTOL


@pytest.mark.parametrize("shape", [(8, 8), (15, 9), (14, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_scan_of_planes_with_empty_and_one_window_phases(gpu_ctx, shape):
    h, w = shape
    plane = kr.marked("A", 1)[5:5 + h, 3:3 + w]
    grids = gpu_ctx.payload_sigma1_scan(plane)
    sizes = [grids[py][px].size for py, px in _phases()]
    assert 0 in sizes and grids[0][0].size >= 1                           # phases without a window ...
    assert (1 in sizes) == (shape != (14, 64))                             # ... one-window phases; 14 x 64: one row of 7 or 8
    _check_scan_against_sigma_pass(gpu_ctx, plane, grids)
    ref = kr.s1_ref(plane)
    for py, px in _phases():
        if ref[py][px].size:
            assert np.all(np.abs(grids[py][px] - ref[py][px]) <= pr.SIGMA_RTOL * ref[py][px]), (py, px)
    # no whole tile: nothing to do, no error
    none = gpu_ctx.payload_sigma1_scan(plane[:7])
    assert all(none[py][px].size == 0 for py, px in _phases())


# ---- keyed scores -----------------------------------------------------------------------------------------------------
def _scores_against_restatement(gpu_ctx, scan, U, h, w, delta, exact=True):
    got = gpu_ctx.payload_keyed_scores(scan, U, h, w, delta)
    want = kr.keyed_scores_ref(scan, U, delta)
    assert len(got) == 64
    worst = 0
    for p in range(64):
        assert got[p].dtype == np.int64 and got[p].shape == want[p].shape, (p, got[p].shape, want[p].shape)
        if got[p].size:
            worst = max(worst, int(np.abs(got[p] - want[p]).max()) if exact else
                        int(np.ceil((np.abs(got[p] - want[p]) / scan[p // 8][p % 8].size).max())))
    return got, worst


def _lanes_over_windows(w, nbx):
    """the entry point's choice (csrc/wm_payload.hip): a lane per window of a row where that fills at least twice as many of a
    wave's 64 lanes as a lane per placement - restated here only to see that the shapes below take both kernels"""
    nx, n_tx = w // 8, nbx - w // 8 + 1
    return nx * ((n_tx + 63) // 64) >= 2 * n_tx * ((nx + 63) // 64)


NARROW = (3, 5, 118, 44)                                                   # 5 windows and 20 placements across: a lane per placement


@pytest.fixture(scope="module")
def scan_narrow(gpu_ctx):
    return gpu_ctx.payload_sigma1_scan(kr.crop_of(kr.marked("A", 1), NARROW))


def test_the_shapes_take_both_lane_mappings():
    assert _lanes_over_windows(CASE_A[3], 24) and not _lanes_over_windows(NARROW[3], 24)
    took = {name: _lanes_over_windows(w, nbx) for name, (h, w, (nby, nbx)) in EDGES.items()}
    assert took == {"full-width": True, "8-rows": False, "65-across": False, "129-across": False, "uncropped": True,
                    "threshold-windows": True, "threshold-lanes": False,
                    "group-and-tail-at-px0": False, "group-and-tail": False, "tail-of-4-and-3": False, "two-groups": False,
                    "two-groups-and-tail": False,
                    "one-full-trip": True, "lane-0-twice": True, "lane-0-twice-every-phase": True, "three-trips": True}


@pytest.mark.parametrize("delta", [8.0, 16.0, 512.0])
def test_scores_of_the_device_scan_are_bit_equal(gpu_ctx, scan_a, scan_narrow, delta):
    """1 / (2 delta) is a power of two: nothing for a compiler to contract, every vote equal, every sum equal - with the
    lanes over the windows (the Case A crop) and over the placements (the narrow one)"""
    _, _, h, w = CASE_A
    got, worst = _scores_against_restatement(gpu_ctx, scan_a, kr.case_table("A"), h, w, delta)
    assert worst == 0
    if delta == kr.DELTA:
        r = kr.located("A", 1, CASE_A)
        assert P.pick_keyed(got, P.phase_counts(h, w)) == (r["phase"], r["place"])     # (the precondition's gap is 4 sigma bars)
    _, worst = _scores_against_restatement(gpu_ctx, scan_narrow, kr.case_table("A"), NARROW[2], NARROW[3], delta)
    assert worst == 0


def test_scores_at_delta_24_agree_within_one_unit_per_window(gpu_ctx, scan_a, scan_narrow):
    """1 / 48 is no power of two: the device contracts x - floor(x) into a fused multiply-add, m moves by at most 4 * 2^-19
    (wm_tile_math.h) = 1 / 4 of a vote's unit, so a vote by at most 1 and a placement's score by at most its window count."""
    _, _, h, w = CASE_A
    _, worst = _scores_against_restatement(gpu_ctx, scan_a, kr.case_table("A"), h, w, 24.0, exact=False)
    _, worst2 = _scores_against_restatement(gpu_ctx, scan_narrow, kr.case_table("A"), NARROW[2], NARROW[3], 24.0, exact=False)
    print(f"worst |score_dev - score_ref| / windows {worst}, narrow crop {worst2}")
    assert worst <= 1 and worst2 <= 1


def test_two_calls_give_the_same_bits(gpu_ctx, scan_a, scan_narrow):
    for scan, (_, _, h, w) in ((scan_a, CASE_A), (scan_narrow, NARROW)):
        for delta in (16.0, 24.0):
            a = gpu_ctx.payload_keyed_scores(scan, kr.case_table("A"), h, w, delta)
            b = gpu_ctx.payload_keyed_scores(scan, kr.case_table("A"), h, w, delta)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _synthetic_scan(h, w, seed):
    rng = np.random.default_rng(seed)
    return [[rng.uniform(0.0, 2040.0, kr.phase_shape(h, w, py, px)).astype(F) for px in range(8)] for py in range(8)]


EDGES = {
    "full-width": (40, 64, (6, 8)),            # a crop as wide as the image: one placement across at px = 0
    "8-rows": (8, 40, (5, 7)),                 # one window row, and only the phases py = 0
    "65-across": (16, 16, (3, 66)),            # 65 placements across at px = 0, 66 at the others: a second, nearly empty wave
    "129-across": (16, 16, (2, 130)),          # 129 and 130: a third
    "uncropped": (24, 40, (3, 5)),             # 1 x 1 placements at phase 0
    "threshold-windows": (16, 64, (3, 11)),    # 8 windows and 4 placements across: the lanes just go over the windows ...
    "threshold-lanes": (16, 56, (3, 11)),      # ... 7 and 5: just not
}
# the second trips (tests/test_loop_trips.py holds them against STEP = 8 and the wave's 64 lanes): keyed_placement_sum's groups of
# 8 windows with a tail behind them, keyed_windows_share's c += 64; three window rows, so that sp += nx and up += nbx count
EDGES.update(lt.KEYED_PLACEMENT)
EDGES.update(lt.KEYED_WINDOWS)


@pytest.mark.parametrize("name", list(EDGES))
def test_scores_of_edge_shapes_are_bit_equal(gpu_ctx, name):
    h, w, (nby, nbx) = EDGES[name]
    scan = _synthetic_scan(h, w, h * 100 + w)
    rng = np.random.default_rng(nbx)
    for U in (rng.integers(0, 65536, (nby, nbx), dtype=np.uint16), np.zeros((nby, nbx), np.uint16),
              np.full((nby, nbx), 65535, np.uint16)):
        got, worst = _scores_against_restatement(gpu_ctx, scan, U, h, w, 16.0)
        assert worst == 0, name
        assert got[0].shape == (nby - h // 8 + 1, nbx - w // 8 + 1)
    if name == "uncropped":
        assert got[0].shape == (1, 1)
    if name == "8-rows":
        assert all(got[p].size == 0 for p in range(8, 64))
    if name.endswith("across"):
        assert got[0].shape[1] in (65, 129) and got[1].shape[1] in (66, 130)


def test_a_zero_table_reads_the_dither_free_votes(gpu_ctx, scan_a):
    """u = 0 gives d = +0: every placement of a phase has the phase's dither-free sum of |vote|"""
    _, _, h, w = CASE_A
    got = gpu_ctx.payload_keyed_scores(scan_a, np.zeros((16, 24), np.uint16), h, w, 16.0)
    for p in range(64):
        want = int(np.abs(kr.vote_of(pr.metric(scan_a[p // 8][p % 8], 16.0)).astype(np.int64)).sum())
        assert np.all(got[p] == want), p


def test_the_library_refuses_bad_arguments(gpu_ctx, hostapi):
    h, w, nby, nbx = 40, 56, 5, 7
    s1 = np.zeros((64, 35), F)
    U = np.zeros(nby * nbx + 1, np.uint16)
    scores = np.zeros((64, P.keyed_score_pitch(h, w, nby, nbx)), np.int64)
    odd = hostapi._vp(U.ctypes.data + 1)
    bad = [(h, w, 4, nbx, 16.0, hostapi._p(U)), (h, w, nby, 6, 16.0, hostapi._p(U)), (7, w, nby, nbx, 16.0, hostapi._p(U)),
           (h, 7, nby, nbx, 16.0, hostapi._p(U)), (h, w, nby, nbx, 16.0, None), (h, w, nby, nbx, 16.0, odd),
           (h, w, nby, nbx, 7.5, hostapi._p(U)), (h, w, nby, nbx, 513.0, hostapi._p(U)), (h, w, nby, nbx, float("nan"), hostapi._p(U))]
    for name in ("wm_payload_keyed_scores", "wm_payload_keyed_scores_dev"):
        for hh, ww, by, bx, delta, table in bad:
            rc = getattr(gpu_ctx.lib, name)(gpu_ctx._h, hostapi._p(s1), table, hostapi._p(scores), hh, ww, by, bx, delta)
            assert rc == hostapi.WM_ERR_BADARG, (name, hh, ww, by, bx, delta)
    assert not scores.any()
    gpu_ctx.sync()
    gpu_ctx.check_status()


# ---- end to end -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def embedded():
    """(case, seed) -> the product's dithered embed of the case host as a gray BGR stack"""
    out = {}
    for case, d in kr.CASES.items():
        H, W = d["shape"]
        for seed in d["seeds"]:
            cover = np.repeat(pr.host(H, W, seed)[..., None], 3, -1)
            out[case, seed] = core.embed_payload_arrays(cover, d["data"], kr.sr.PASSWORD, kr.sr.NONCE, dither=True)
    return out


@pytest.mark.parametrize("c", kr.all_cases(), ids=kr.case_id)
def test_cropped_dithered_stego_decodes_and_names_its_origin(embedded, c):
    case, seed, crop = c
    y0, x0, h, w = crop
    data = kr.CASES[case]["data"]
    # the precondition of this BGR path, on the CPU: what the asserts below rely on
    ref = kr.located_bgr(case, seed, crop)
    kr.check_precondition(ref, crop, data)
    r = embedded[case, seed]
    got, valid, conf, origin = core.extract_payload_arrays(r["stego"][y0:y0 + h, x0:x0 + w], r["meta"], kr.sr.PASSWORD,
                                                           search="crop-keyed")
    print(f"{kr.case_id(c)}: confidence {conf:.4f}, the restatement's {ref['confidence']:.4f}")
    assert got == data and valid is True and origin == (y0, x0)
    assert abs(conf - ref["confidence"]) <= pr.slope_bar(kr.DELTA)


def test_uncropped_stego_with_keyed_search(embedded):
    for (case, seed), r in embedded.items():
        plain = core.extract_payload_arrays(r["stego"], r["meta"], kr.sr.PASSWORD)
        got, valid, conf, origin = core.extract_payload_arrays(r["stego"], r["meta"], kr.sr.PASSWORD, search="crop-keyed")
        assert origin == (0, 0) and valid is True
        assert (got, valid) == plain[:2] and got == kr.CASES[case]["data"]
        assert conf == pytest.approx(plain[2], abs=1e-4)                   # (votes are m rounded to 2^-15)


def test_unmarked_host_is_not_valid(embedded):
    r = embedded["A", 1]
    cover = np.repeat(pr.host(128, 192, 1)[..., None], 3, -1)
    got, valid, conf, origin = core.extract_payload_arrays(cover[3:121, 5:185], r["meta"], kr.sr.PASSWORD, search="crop-keyed")
    assert valid is False and isinstance(got, bytes) and 0.0 <= conf <= 1.0 and len(origin) == 2


def test_a_crop_of_a_dozen_tiles_returns_a_result(embedded):
    """24 x 32: too few windows for the true candidate to win reliably; a result tuple, never an exception"""
    r = embedded["A", 1]
    got, valid, conf, origin = core.extract_payload_arrays(r["stego"][50:74, 60:92], r["meta"], kr.sr.PASSWORD, search="crop-keyed")
    assert isinstance(got, bytes) and isinstance(valid, bool) and 0.0 <= conf <= 1.0 and len(origin) == 2


def test_dither_free_meta_is_refused_before_any_device_call(monkeypatch):
    cover = np.repeat(pr.host(128, 192, 1)[..., None], 3, -1)
    r = core.embed_payload_arrays(cover, b"id", kr.sr.PASSWORD, kr.sr.NONCE)

    def refuse(*a, **k):
        raise AssertionError("a refusal must come before the first device call")
    monkeypatch.setattr(core, "_ctx", refuse)
    with pytest.raises(ValueError, match="search='crop'"):
        core.extract_payload_arrays(r["stego"][3:121, 5:185], r["meta"], kr.sr.PASSWORD, search="crop-keyed")


def test_file_forms_once(tmp_path):
    cover = np.repeat(pr.host(128, 192, 2)[..., None], 3, -1)
    cpath = str(tmp_path / "cover.png")
    assert hg.write_png(cpath, cover, 0)
    out, meta_path, _, _ = core.embed_payload(cpath, "id", str(tmp_path / "marked.png"), str(tmp_path / "meta.npz"),
                                              password=kr.sr.PASSWORD, nonce=kr.sr.NONCE, dither=True)
    y0, x0, h, w = CASE_A
    crop_path = str(tmp_path / "crop.png")
    assert hg.write_png(crop_path, np.ascontiguousarray(hg.read_image_bgr(out)[y0:y0 + h, x0:x0 + w]), 0)
    got, valid, conf, written, origin = core.extract_payload(crop_path, meta_path, str(tmp_path / "got"), password=kr.sr.PASSWORD,
                                                             search="crop-keyed")
    assert got == b"id" and valid is True and origin == (y0, x0)
    assert open(written, encoding="utf-8").read() == "id"
    with pytest.raises(ValueError, match="dithered payload is not supported"):
        core.extract_payload(crop_path, meta_path, password=kr.sr.PASSWORD, search="crop")
