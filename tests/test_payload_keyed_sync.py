"""Keyed crop resynchronisation of the dithered blind payload without a device: the precondition of the cases that
tests/test_gpu_payload_keyed_sync.py relies on (on the restatement alone, tests/payload_keyed_sync_refs.py), the exact
comparisons and tie rules of payload.pick_keyed, payload.keyed_votes against the restatements, payload.keyed_score_pitch,
and every refusal of search="crop-keyed", each raised before anything crosses the C ABI."""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import payload_dither_refs as pdr
import payload_keyed_sync_refs as kr
import payload_refs as pr
import payload_sync_refs as sr

M = importlib.import_module(ge.PKG_NAME + ".meta")
P = importlib.import_module(ge.PKG_NAME + ".payload")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
core = importlib.import_module(ge.PKG_NAME + ".dct_svd_core_secure")


# ---- the precondition: a condition on the inputs, not a measurement ---------------------------------------------------
def _report(name, r):
    print(f"{name}: top {r['top']:.3f}, best other of {r['candidates'] - 1} {r['runner_up']:.3f}, gap {r['gap']:.3f}, "
          f"tiles per bit >= {int(r['count'].min())}")


@pytest.mark.parametrize("c", kr.all_cases(), ids=kr.case_id)
def test_case_precondition_on_the_restatement(c):
    """For every case the true (phase, placement) beats every other candidate by at least 4 slope_bar(delta) = 0.102 in
    score / (32768 windows), every bit keeps a tile and the decode is valid and equal to the data.  The figures of DESIGN.md
    ("Keyed crop resynchronisation") are this test's: top 0.764 - 0.789, best other 0.560 - 0.584, smallest gap 0.186."""
    case, seed, crop = c
    r = kr.located(case, seed, crop)
    _report(kr.case_id(c), r)
    assert 4 * pr.slope_bar(kr.DELTA) == pytest.approx(0.102)
    kr.check_precondition(r, crop, kr.CASES[case]["data"])
    assert 0.76 <= r["top"] <= 0.80 and 0.55 <= r["runner_up"] <= 0.59


def test_case_precondition_at_delta_24():
    c = ("A", 1, kr.CASES["A"]["crops"][0])
    r = kr.located(*c, 24.0)
    _report(kr.case_id(c) + " delta 24", r)
    kr.check_precondition(r, c[2], kr.CASES["A"]["data"], 24.0)


def test_uncropped_plane_locates_the_origin_on_the_restatement():
    bits, tbi = kr.case_map("A")
    r = kr.locate_ref(kr.marked("A", 1), kr.case_table("A"), tbi, bits.size)
    assert r["phase"] == (0, 0) and r["place"] == (0, 0) and r["origin"] == (0, 0)
    assert r["scores"][0].shape == (1, 1) and r["valid"] and r["data"] == b"id"
    assert r["gap"] >= 4 * pr.slope_bar(kr.DELTA)


def test_the_keyless_read_of_a_dithered_plane_has_no_phase_signal():
    """why search="crop" cannot do this: under the dither-free metric the true phase does not stand out"""
    crop = kr.CASES["A"]["crops"][0]
    sums, counts = sr.phase_sums(sr.votes_ref(kr.crop_of(kr.marked("A", 1), crop)))
    mean = sums / (32768.0 * counts)
    print(f"keyless mean |m| per phase: {mean.min():.3f} .. {mean.max():.3f}")
    assert mean.max() - mean.min() < 4 * pr.slope_bar(kr.DELTA)


# ---- pick_keyed ---------------------------------------------------------------------------------------------------------
def _grids(fill=None):
    g = [np.zeros((0, 0), np.int64) for _ in range(64)]
    for p, a in (fill or {}).items():
        g[p] = np.asarray(a, np.int64)
    return g


def test_pick_keyed_ties_go_to_the_smallest_candidate():
    counts = np.zeros(64, np.int64)
    counts[[3, 9, 40]] = 6
    sc = {3: [[1, 5, 5], [5, 2, 0]], 9: [[5, 5, 5], [5, 5, 5]], 40: [[0, 0, 5], [0, 0, 0]]}
    assert P.pick_keyed(_grids(sc), counts) == ((0, 3), (0, 1))
    assert kr.pick_keyed_ref(_grids(sc), list(counts)) == ((0, 3), (0, 1))
    sc[3] = [[1, 4, 4], [5, 2, 0]]                                          # within a phase: the first maximum, row-major
    sc[9] = [[4, 4, 4], [4, 4, 4]]
    sc[40] = [[0, 0, 4], [0, 0, 0]]
    assert P.pick_keyed(_grids(sc), counts) == ((0, 3), (1, 0))
    # an equal ratio with unequal counts is a tie too: 10 / 4 == 15 / 6, and the earlier phase keeps it
    counts[:] = 0
    counts[[5, 6]] = (6, 4)
    assert P.pick_keyed(_grids({5: [[15]], 6: [[10]]}), counts) == ((0, 5), (0, 0))
    counts[[5, 6]] = (4, 6)
    assert P.pick_keyed(_grids({5: [[10]], 6: [[15]]}), counts) == ((0, 5), (0, 0))


def test_pick_keyed_skips_phases_without_windows_or_placements():
    counts = np.zeros(64, np.int64)
    counts[[10, 20]] = (0, 4)
    sc = {10: [[2 ** 40]], 20: [[1, 0]]}                                    # count 0 does not take part, whatever its score
    assert P.pick_keyed(_grids(sc), counts) == ((2, 4), (0, 0))
    counts[30] = 4                                                          # a count but no placement
    assert P.pick_keyed(_grids(sc), counts) == ((2, 4), (0, 0))
    assert P.pick_keyed(_grids(), np.zeros(64, np.int64)) is None
    assert P.pick_keyed(_grids({20: [[0, 0]]}), counts) == ((2, 4), (0, 0))  # all-zero scores: the first candidate
    with pytest.raises(ValueError):
        P.pick_keyed(_grids()[:63], counts)
    with pytest.raises(ValueError):
        P.pick_keyed(_grids({20: [1, 2]}), counts)


def test_pick_keyed_compares_unequal_counts_exactly():
    """Scores of 2^53 and beyond, where float64 division ties or misorders: a / n against b / m by a m against b n."""
    counts = np.zeros(64, np.int64)
    counts[[1, 2]] = (3, 3)
    a = 2 ** 53
    assert float(a) == float(a + 1)                                         # (what a float comparison would see)
    assert P.pick_keyed(_grids({1: [[a]], 2: [[a + 1]]}), counts) == ((0, 2), (0, 0))
    assert P.pick_keyed(_grids({1: [[a + 1]], 2: [[a]]}), counts) == ((0, 1), (0, 0))
    # unequal counts: 3 (k + 1) / 3 > (7 k + 6) / 7 by 1 / 7 only, invisible in float64 at k = 2^58
    k = 2 ** 58
    counts[[1, 2]] = (7, 3)
    x, y = 7 * k + 6, 3 * (k + 1)
    assert x / 7 == y / 3 and y * 7 > x * 3
    assert P.pick_keyed(_grids({1: [[x]], 2: [[y]]}), counts) == ((0, 2), (0, 0))
    assert kr.pick_keyed_ref(_grids({1: [[x]], 2: [[y]]}), list(counts)) == ((0, 2), (0, 0))
    x = 7 * k + 8                                                           # ... and by 1 / 7 the other way: float64 calls it a tie
    assert x / 7 == y / 3 and y * 7 < x * 3
    counts[[1, 2]] = (3, 7)
    assert P.pick_keyed(_grids({1: [[y]], 2: [[x]]}), counts) == ((0, 2), (0, 0))
    # the realistic range: every candidate of a case, against exact fractions
    r = kr.located("B", 1, kr.CASES["B"]["crops"][0])
    h, w = kr.CASES["B"]["crops"][0][2:]
    assert P.pick_keyed(r["scores"], P.phase_counts(h, w)) == (r["phase"], r["place"])
    assert list(P.phase_counts(h, w).reshape(-1)) == kr.counts_ref(h, w)


# ---- keyed_votes, keyed_score_pitch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", pdr.DELTAS)
def test_keyed_votes_follow_the_restatements(delta):
    rng = np.random.default_rng(int(delta * 10))
    s1 = np.concatenate([rng.uniform(0, 2040, 4000), [0.0, delta, 2 * delta, 2040.0]]).astype(np.float32)
    zero = P.keyed_votes(s1, np.zeros(s1.size, np.uint16), delta)
    assert zero.dtype == np.int32 and np.array_equal(zero, sr.vote_of(pr.metric(s1, delta)))
    for u in (rng.integers(0, 65536, s1.size, dtype=np.uint16), np.full(s1.size, 65535, np.uint16), np.resize(pdr.U_EDGES, s1.size)):
        assert np.array_equal(P.keyed_votes(s1, u, delta), kr.votes_ref(s1, u, delta))
    assert np.abs(zero).max() <= 32768
    with pytest.raises(ValueError):
        P.keyed_votes(s1, np.zeros(3, np.uint16), delta)


def test_keyed_votes_of_a_marked_plane_sit_on_the_lattice():
    """read with the right words a dithered stego's tiles vote at nearly full weight, whatever bit they carry"""
    s1 = kr.s1_ref(kr.marked("A", 1))[0][0]
    v = P.keyed_votes(s1, kr.case_table("A"), kr.DELTA)
    bits, tbi = kr.case_map("A")
    assert np.array_equal(v < 0, bits[tbi] != 0)
    assert np.abs(v).mean() / 32768 > 0.75


def test_keyed_score_pitch():
    for nby, nbx in ((2, 2), (5, 7), (16, 24)):
        for h in (8, 14, 15, 16):
            for w in (8, 14, 15, 16):
                want = max((nby - (h - py) // 8 + 1) * (nbx - (w - px) // 8 + 1)
                           for py in range(8) for px in range(8) if (h - py) // 8 > 0 and (w - px) // 8 > 0)
                fewest = (nby - max(h - 7, 0) // 8 + 1) * (nbx - max(w - 7, 0) // 8 + 1)
                assert P.keyed_score_pitch(h, w, nby, nbx) == fewest >= want, (h, w, nby, nbx)
    assert P.keyed_score_pitch(8, 8, 2, 2) == 9 and P.keyed_score_pitch(14, 14, 2, 2) == 9      # (7, 7) has no window: ny 0
    assert P.keyed_score_pitch(15, 15, 2, 2) == 4 and P.keyed_score_pitch(16, 16, 2, 2) == 4
    assert P.keyed_score_pitch(15, 8, 5, 7) == 5 * 8 and P.keyed_score_pitch(8, 16, 5, 7) == 6 * 7
    assert P.keyed_score_pitch(128, 192, 16, 24) == 2 * 2


# ---- refusals, before anything crosses the C ABI ----------------------------------------------------------------------
def _meta(H, W, n_bits=80, dither=P.DITHER_TABLE, delta=16.0):
    members = M.payload_members("text", H, W, delta, n_bits, sr.NONCE, dither=dither)
    return M.sealed(members, 8, hg.hmac_digest(kr.key(), M.hmac_parts(members)))


@pytest.fixture
def no_device(monkeypatch):
    """any context, and so any library load, fails the test"""
    def refuse(*a, **k):
        raise AssertionError("a refusal must come before the first device call")
    monkeypatch.setattr(core, "_ctx", refuse)
    monkeypatch.setattr(core.hostapi, "load_library", refuse)


def test_keyed_search_refusals_come_before_any_device_call(no_device, tmp_path):
    H, W = 128, 192
    meta = _meta(H, W)
    st = np.zeros((100, 150, 3), np.uint8)
    assert core.SEARCHES == (None, "crop", "crop-keyed")
    for search in ("crop_keyed", "Crop-Keyed", "keyed", 2):
        with pytest.raises(ValueError, match="search"):
            core.extract_payload_arrays(st, meta, sr.PASSWORD, search=search)
        with pytest.raises(ValueError, match="search"):
            core.extract_payload(str(tmp_path / "no.png"), str(tmp_path / "no.npz"), password=sr.PASSWORD, search=search)
    with pytest.raises(ValueError, match="search='crop'"):                  # a dither-free meta: the other search reads it
        core.extract_payload_arrays(st, _meta(H, W, dither=0), sr.PASSWORD, search="crop-keyed")
    for shape in ((129, 192, 3), (128, 193, 3), (136, 200, 3)):
        with pytest.raises(ValueError, match="larger than"):
            core.extract_payload_arrays(np.zeros(shape, np.uint8), meta, sr.PASSWORD, search="crop-keyed")
    for shape in ((7, 150, 3), (100, 7, 3), (0, 0, 3)):
        with pytest.raises(ValueError, match="whole 8x8 tile"):
            core.extract_payload_arrays(np.zeros(shape, np.uint8), meta, sr.PASSWORD, search="crop-keyed")
    for bad in (np.zeros((100, 150), np.uint8), np.zeros((100, 150, 4), np.uint8), np.zeros((100, 150, 3), np.float32)):
        with pytest.raises(ValueError, match="uint8"):
            core.extract_payload_arrays(bad, meta, sr.PASSWORD, search="crop-keyed")
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        core.extract_payload_arrays(st, meta, "not the password", search="crop-keyed")


def test_crop_search_still_refuses_a_dithered_meta(no_device):
    st = np.zeros((100, 150, 3), np.uint8)
    with pytest.raises(ValueError, match="dithered payload is not supported") as e:
        core.extract_payload_arrays(st, _meta(128, 192), sr.PASSWORD, search="crop")
    assert "crop-keyed" in str(e.value)


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
    st = np.zeros((40, 56), np.uint8)
    U = np.zeros((5, 7), np.uint16)
    scan = [[np.zeros(sr.phase_shape(40, 56, py, px), np.float32) for px in range(8)] for py in range(8)]
    for delta in (7.9, float("nan"), 1000.0):
        with pytest.raises(ValueError, match="delta"):
            ctx.payload_keyed_scores(scan, U, 40, 56, delta)
        with pytest.raises(ValueError, match="delta"):
            ctx.payload_locate_keyed(st, U, delta)
    with pytest.raises(ValueError):
        ctx.payload_sigma1_scan(st.astype(np.float32))
    with pytest.raises(ValueError):
        ctx.payload_locate_keyed(st.astype(np.float32), U, 16.0)
    with pytest.raises(ValueError):
        ctx.payload_locate_keyed(st[None], U, 16.0)
    for table in (U.reshape(-1), np.zeros((4, 7), np.uint16), np.zeros((5, 6), np.uint16)):     # flat; fewer tiles than the plane
        with pytest.raises(ValueError):
            ctx.payload_keyed_scores(scan, table, 40, 56, 16.0)
        with pytest.raises(ValueError):
            ctx.payload_locate_keyed(st, table, 16.0)
    with pytest.raises(ValueError, match="whole tile"):
        ctx.payload_locate_keyed(st[:7], U, 16.0)
    with pytest.raises(ValueError, match="phase"):                          # a scan of another plane size
        ctx.payload_keyed_scores(scan, U, 40, 48, 16.0)
