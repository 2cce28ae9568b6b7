"""Crop resynchronisation of the blind payload on the device: the phase scan's votes against the restatement
(tests/payload_sync_refs.py) under the sigma bar, its sums and the offset scan's scores bit for bit (integer arithmetic), and
extract_payload[_arrays](search="crop") end to end on the cases whose precondition tests/test_payload_sync.py establishes."""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import payload_refs as pr
import payload_sync_refs as sr

pytestmark = pytest.mark.gpu

P = importlib.import_module(ge.PKG_NAME + ".payload")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
core = importlib.import_module(ge.PKG_NAME + ".dct_svd_core_secure")

A_CROPS = sr.CASES["A"]["crops"]


@pytest.fixture(scope="module")
def scans(gpu_ctx):
    """crop -> (votes, sums, counts) of the device on the crops of Case A seed 1, each passed as a strided view"""
    st = sr.marked("A", 1)
    return {crop: gpu_ctx.payload_phase_scan(sr.crop_of(st, crop), sr.DELTA) for crop in A_CROPS}


# ---- votes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", A_CROPS, ids=lambda c: "x".join(map(str, c)))
def test_votes_of_all_phases_follow_the_restatement(scans, crop):
    """|vote_dev - vote_ref| <= slope_bar(delta) * 32768 + 1 on every window of all 64 phases (the metric is Lipschitz in
    sigma_1: no tile is left out), and sums = sum |vote| of the device's own votes, exactly."""
    votes, sums, counts = scans[crop]
    ref = sr.located("A", 1, crop)
    bound = pr.slope_bar(sr.DELTA) * 32768 + 1
    worst = 0
    for py in range(8):
        for px in range(8):
            v, want = votes[py][px], ref["votes"][py][px]
            assert v.dtype == np.int32 and v.shape == want.shape == sr.phase_shape(crop[2], crop[3], py, px)
            worst = max(worst, int(np.abs(v.astype(np.int64) - want).max()))
            assert int(np.abs(v.astype(np.int64)).sum()) == int(sums[py, px]), (py, px)
    print(f"worst |vote_dev - vote_ref| {worst} (bound {bound:.0f})")
    assert worst <= bound
    assert sums.dtype == np.int64 and np.array_equal(counts, ref["counts"])
    assert np.abs(np.concatenate([v.reshape(-1) for row in votes for v in row])).max() <= 32768


def test_strided_view_and_contiguous_copy_agree_bit_for_bit(gpu_ctx, scans):
    st = sr.marked("A", 1)
    for crop in (A_CROPS[0], A_CROPS[3]):
        view = sr.crop_of(st, crop)
        assert not view.flags.c_contiguous
        v2, s2, c2 = gpu_ctx.payload_phase_scan(np.ascontiguousarray(view), sr.DELTA)
        v1, s1, c1 = scans[crop]
        assert np.array_equal(s1, s2) and np.array_equal(c1, c2)
        for py in range(8):
            for px in range(8):
                assert np.array_equal(v1[py][px], v2[py][px]), (crop, py, px)


def test_planes_with_empty_phases_and_a_batch(gpu_ctx):
    """h = 12: the phases py >= 5 have no window (count 0, sum 0); w = 12: px >= 5 likewise; 8 x 8: phase (0, 0) alone has
    one.  A batch of two planes gives each plane what it gets alone."""
    st = sr.marked("A", 1)
    for plane in (st[3:15, 5:45], st[8:48, 16:28], st[0:8, 0:8]):
        h, w = plane.shape
        votes, sums, counts = gpu_ctx.payload_phase_scan(plane, sr.DELTA)
        ref = sr.votes_ref(plane)
        rs, rc = sr.phase_sums(ref)
        assert np.array_equal(counts, rc) and (counts == 0).any() and counts[0, 0] > 0
        assert np.all(sums[counts == 0] == 0)
        bound = pr.slope_bar(sr.DELTA) * 32768 + 1
        for py in range(8):
            for px in range(8):
                assert votes[py][px].shape == ref[py][px].shape
                if ref[py][px].size:
                    assert np.abs(votes[py][px].astype(np.int64) - ref[py][px]).max() <= bound
                assert int(np.abs(votes[py][px].astype(np.int64)).sum()) == int(sums[py, px])
        assert P.pick_phase(sums, counts) is not None
    two = np.stack([st[3:43, 5:69], st[11:51, 2:66]])
    vb, sb, cb = gpu_ctx.payload_phase_scan(two, sr.DELTA)
    assert sb.shape == (2, 8, 8)
    for i in range(2):
        v1, s1, _ = gpu_ctx.payload_phase_scan(two[i], sr.DELTA)
        assert np.array_equal(sb[i], s1)
        assert all(np.array_equal(vb[py][px][i], v1[py][px]) for py in range(8) for px in range(8))
    # no whole tile: nothing to do, no error
    v0, s0, c0 = gpu_ctx.payload_phase_scan(st[:7, :100], sr.DELTA)
    assert not c0.any() and not s0.any() and v0[0][0].shape == (0, 12)


# ---- offset scores ----------------------------------------------------------------------------------------------------
def _scores_equal(gpu_ctx, V, T, n_bits):
    got = gpu_ctx.payload_offset_scores(V, T, n_bits)
    want = sr.offset_scores_ref(V, T, n_bits)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), (V.shape, T.shape, n_bits)
    return got


def test_offset_scores_of_the_device_votes_are_bit_equal(gpu_ctx, scans):
    bits, tbi = sr.case_map("A")
    for crop in A_CROPS:
        votes, sums, counts = scans[crop]
        py, px = P.pick_phase(sums, counts)
        assert (py, px) == sr.located("A", 1, crop)["phase"]               # (the precondition's gap is 4 sigma bars)
        got = _scores_equal(gpu_ctx, votes[py][px], tbi, bits.size)
        assert P.pick_offset(got) == sr.located("A", 1, crop)["place"]


@pytest.mark.parametrize("grid", [((14, 22), (16, 24), 80), ((16, 24), (16, 24), 80), ((1, 1), (16, 24), 80),
                                  ((9, 13), (16, 24), 64), ((10, 20), (16, 24), 384), ((3, 300), (5, 301), 64),
                                  ((15, 25), (20, 32), 16384)],
                         ids=lambda g: f"{g[0][0]}x{g[0][1]}in{g[1][0]}x{g[1][1]}b{g[2]}")
def test_offset_scores_of_random_votes_are_bit_equal(gpu_ctx, grid):
    """Seeded votes in +-32768 under a seeded map with the product's structure: the Case A grid, one placement, a 1x1
    window, n_bits = 64 and n_bits = nby nbx, more windows than a workgroup has threads in one row, the largest n_bits."""
    (ny, nx), (nby, nbx), n_bits = grid
    rng = np.random.default_rng(ny * 1000 + nx)
    V = rng.integers(-32768, 32769, (ny, nx)).astype(np.int32)
    T = pr.simple_map(nby * nbx, n_bits, seed=3)[0].reshape(nby, nbx)
    _scores_equal(gpu_ctx, V, T, n_bits)
    _scores_equal(gpu_ctx, np.full((ny, nx), 32768, np.int32), T, n_bits)   # every vote at full weight


def test_offset_scan_skips_map_entries_outside_the_bits(gpu_ctx):
    rng = np.random.default_rng(8)
    V = rng.integers(-32768, 32769, (14, 22)).astype(np.int32)
    T = pr.simple_map(16 * 24, 80, seed=3)[0].reshape(16, 24).copy()
    clean = gpu_ctx.payload_offset_scores(V, T, 80)
    T[rng.integers(0, 16, 30), rng.integers(0, 24, 30)] = -1
    T[rng.integers(0, 16, 30), rng.integers(0, 24, 30)] = 80
    T[0, 0], T[15, 23] = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    got = _scores_equal(gpu_ctx, V, T, 80)
    assert not np.array_equal(got, clean)


def test_offset_scan_refuses_more_than_16384_bits(gpu_ctx, hostapi):
    V, T = np.zeros((2, 2), np.int32), np.zeros((4, 4), np.int32)
    with pytest.raises(ValueError, match="n_bits"):
        gpu_ctx.payload_offset_scores(V, T, 16385)
    scores = np.zeros((3, 3), np.int64)
    for name in ("wm_payload_offset_scores", "wm_payload_offset_scores_dev"):     # the library's own check
        rc = getattr(gpu_ctx.lib, name)(gpu_ctx._h, hostapi._p(V), hostapi._p(T), hostapi._p(scores), 2, 2, 4, 4, 16385)
        assert rc == hostapi.WM_ERR_BADARG
        assert b"n_bits" in gpu_ctx.lib.wm_last_error()
    assert gpu_ctx.payload_offset_scores(V, T, 16384).shape == (3, 3)


# ---- end to end -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def embedded():
    """(case, seed) -> the product's embed of the case host as a gray BGR stack"""
    out = {}
    for case, d in sr.CASES.items():
        H, W = d["shape"]
        for seed in d["seeds"]:
            cover = np.repeat(pr.host(H, W, seed)[..., None], 3, -1)
            out[case, seed] = core.embed_payload_arrays(cover, d["data"], sr.PASSWORD, sr.NONCE)
    return out


@pytest.mark.parametrize("c", sr.all_cases(), ids=sr.case_id)
def test_cropped_stego_decodes_and_names_its_origin(embedded, c):
    case, seed, crop = c
    y0, x0, h, w = crop
    data = sr.CASES[case]["data"]
    # the precondition of this BGR path, on the CPU: what the asserts below rely on
    bits, tbi = sr.case_map(case)
    sr.check_precondition(sr.locate_ref(sr.crop_of(sr.marked_bgr_y(case, seed), crop), tbi, bits.size), crop, data)
    r = embedded[case, seed]
    got, valid, conf, origin = core.extract_payload_arrays(r["stego"][y0:y0 + h, x0:x0 + w], r["meta"], sr.PASSWORD, search="crop")
    print(f"{sr.case_id(c)}: confidence {conf:.3f}")
    assert got == data and valid is True and origin == (y0, x0)
    assert 0.0 < conf <= 1.0


def test_uncropped_stego_with_search(embedded):
    for (case, seed), r in embedded.items():
        plain = core.extract_payload_arrays(r["stego"], r["meta"], sr.PASSWORD)
        got, valid, conf, origin = core.extract_payload_arrays(r["stego"], r["meta"], sr.PASSWORD, search="crop")
        assert origin == (0, 0) and valid is True
        assert (got, valid) == plain[:2] and got == sr.CASES[case]["data"]
        assert np.array_equal(P.payload_frame(got), P.payload_frame(plain[0]))
        assert conf == pytest.approx(plain[2], abs=1e-4)                   # (votes are m rounded to 2^-15)


def test_cropped_stego_without_search_raises_as_before(embedded):
    r = embedded["A", 1]
    with pytest.raises(ValueError, match="but the meta was written for"):
        core.extract_payload_arrays(r["stego"][3:121, 5:185], r["meta"], sr.PASSWORD)
    with pytest.raises(ValueError, match="but the meta was written for"):
        core.extract_payload_arrays(r["stego"][3:121, 5:185], r["meta"], sr.PASSWORD, search=None)


def test_unmarked_host_is_not_valid(embedded):
    r = embedded["A", 1]
    cover = np.repeat(pr.host(128, 192, 1)[..., None], 3, -1)
    got, valid, conf, origin = core.extract_payload_arrays(cover, r["meta"], sr.PASSWORD, search="crop")
    assert valid is False and isinstance(got, bytes) and 0.0 <= conf <= 1.0
    assert origin is None or len(origin) == 2


def test_dithered_meta_is_refused_before_any_device_call(monkeypatch):
    cover = np.repeat(pr.host(128, 192, 1)[..., None], 3, -1)
    r = core.embed_payload_arrays(cover, b"id", sr.PASSWORD, sr.NONCE, dither=True)

    def refuse(*a, **k):
        raise AssertionError("a refusal must come before the first device call")
    monkeypatch.setattr(core, "_ctx", refuse)
    with pytest.raises(ValueError, match="dithered payload is not supported"):
        core.extract_payload_arrays(r["stego"][3:121, 5:185], r["meta"], sr.PASSWORD, search="crop")


def test_file_forms_once(tmp_path):
    cover = np.repeat(pr.host(128, 192, 2)[..., None], 3, -1)
    cpath = str(tmp_path / "cover.png")
    assert hg.write_png(cpath, cover, 0)
    out, meta_path, _, _ = core.embed_payload(cpath, "id", str(tmp_path / "marked.png"), str(tmp_path / "meta.npz"),
                                              password=sr.PASSWORD, nonce=sr.NONCE)
    y0, x0, h, w = A_CROPS[0]
    crop_path = str(tmp_path / "crop.png")
    assert hg.write_png(crop_path, np.ascontiguousarray(hg.read_image_bgr(out)[y0:y0 + h, x0:x0 + w]), 0)
    got, valid, conf, written, origin = core.extract_payload(crop_path, meta_path, str(tmp_path / "got"), password=sr.PASSWORD,
                                                             search="crop")
    assert got == b"id" and valid is True and origin == (y0, x0)
    assert open(written, encoding="utf-8").read() == "id"
    assert len(core.extract_payload(out, meta_path, password=sr.PASSWORD)) == 4
    with pytest.raises(ValueError, match="but the meta was written for"):
        core.extract_payload(crop_path, meta_path, password=sr.PASSWORD)
