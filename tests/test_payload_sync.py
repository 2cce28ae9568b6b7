"""Crop resynchronisation of the blind payload without a device: the precondition of the cases that
tests/test_gpu_payload_sync.py relies on (on the restatement alone, tests/payload_sync_refs.py), payload_vote from a
stand-alone g++ program (plain and under AddressSanitizer + UBSan) against NumPy, the exact comparisons and tie rules of
payload.pick_phase / pick_offset, payload.soft_of_votes against payload_refs.soft_ref, and every refusal of
search="crop", each raised before anything crosses the C ABI."""
import importlib
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import payload_refs as pr
import payload_sync_refs as sr

M = importlib.import_module(ge.PKG_NAME + ".meta")
P = importlib.import_module(ge.PKG_NAME + ".payload")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
core = importlib.import_module(ge.PKG_NAME + ".dct_svd_core_secure")


# ---- the precondition: a condition on the inputs, not a measurement ---------------------------------------------------
@pytest.mark.parametrize("c", sr.all_cases(), ids=sr.case_id)
def test_case_precondition_on_the_restatement(c):
    """For every case the true phase beats every other by at least 4 slope_bar(delta) = 0.102 in mean |m|, the true
    placement every other by the same in score / (32768 tiles), every bit keeps a tile and the decode is valid and equal to
    the data.  A case that does not meet this is replaced, not loosened."""
    case, seed, crop = c
    r = sr.located(case, seed, crop)
    print(f"{sr.case_id(c)}: phase gap {r['phase_gap']:.3f}, offset gap {r['offset_gap']:.3f}, "
          f"tiles per bit >= {int(r['count'].min())}")
    assert 4 * pr.slope_bar(sr.DELTA) == pytest.approx(0.102)
    sr.check_precondition(r, crop, sr.CASES[case]["data"])


def test_uncropped_plane_locates_the_origin_on_the_restatement():
    bits, tbi = sr.case_map("A")
    r = sr.locate_ref(sr.marked("A", 1), tbi, bits.size)
    assert r["phase"] == (0, 0) and r["place"] == (0, 0) and r["origin"] == (0, 0)
    assert r["scores"].shape == (1, 1) and r["valid"] and r["data"] == b"id"
    assert r["phase_gap"] >= 4 * pr.slope_bar(sr.DELTA)


# ---- payload_vote -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request):
    return ge.build_payload_sync_harness(sanitize=request.param == "sanitized")


def test_vote_edges(harness):
    r = subprocess.run([harness, "edges"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_vote_against_numpy(harness, tmp_path):
    """payload_vote on a grid of m with +-1, +-0, every half-way point k + 0.5 and its float32 neighbours, and seeded
    values: equal to np.rint(m * 32768) (ties to even on both sides)."""
    k = np.arange(-32768, 32768, dtype=np.float64)
    half = ((k + 0.5) / 32768.0).astype(np.float32)
    m = np.concatenate([[1.0, -1.0, 0.0, -0.0], half, np.nextafter(half, np.float32(2)), np.nextafter(half, np.float32(-2)),
                        (k / 32768.0).astype(np.float32), np.random.default_rng(5).uniform(-1, 1, 20000).astype(np.float32),
                        pr.metric(np.arange(0, 2041, 0.25, dtype=np.float32), 16.0),
                        pr.metric(np.arange(0, 2041, 0.25, dtype=np.float32), 21.5)]).astype(np.float32)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([m.size], np.int32).tobytes() + m.tobytes())
    r = subprocess.run([harness, "run", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = np.fromfile(dst, np.int32)
    want = np.rint(m * np.float32(32768)).astype(np.int32)
    assert got.size == m.size and np.array_equal(got, want)
    assert np.array_equal(want, sr.vote_of(m))
    assert got.min() == -32768 and got.max() == 32768


# ---- the comparisons and their tie rules ------------------------------------------------------------------------------
def test_pick_phase_is_exact_and_breaks_ties_downwards():
    counts = P.phase_counts(118, 180)
    assert counts.shape == (8, 8) and counts[0, 0] == 14 * 22 and counts[7, 5] == 13 * 21
    sums = counts * 1000
    assert P.pick_phase(sums, counts) == (0, 0)                            # all equal: the smallest p
    sums[3, 5] += 1
    assert P.pick_phase(sums, counts) == (3, 5)
    sums[7, 7] += 1                                                        # the same surplus over fewer windows: a larger ratio
    assert counts[7, 7] < counts[3, 5] and P.pick_phase(sums, counts) == (7, 7)
    # a difference that float64 cannot see: 2^62 / 2^31 against (2^62 + 1) / 2^31
    big = np.zeros((8, 8), np.int64); cnt = np.zeros((8, 8), np.int64)
    cnt[1, 1] = cnt[5, 5] = 1 << 31
    big[1, 1] = 1 << 62; big[5, 5] = (1 << 62) + 1
    assert float(big[1, 1]) / float(cnt[1, 1]) == float(big[5, 5]) / float(cnt[5, 5])
    assert P.pick_phase(big, cnt) == (5, 5)
    big[5, 5] = 1 << 62
    assert P.pick_phase(big, cnt) == (1, 1)
    # cross-multiplication: 7 / 3 against 9 / 4
    s = np.zeros((8, 8), np.int64); n = np.zeros((8, 8), np.int64)
    s[0, 1], n[0, 1], s[0, 2], n[0, 2] = 9, 4, 7, 3
    assert P.pick_phase(s, n) == (0, 2)
    for c in sr.all_cases()[:3]:
        r = sr.located(*c)
        assert P.pick_phase(r["sums"], r["counts"]) == r["phase"] == sr.pick_phase_ref(r["sums"], r["counts"])


def test_pick_phase_leaves_empty_phases_out():
    counts = P.phase_counts(12, 40)                                        # py >= 5 has no window
    assert np.all(counts[5:] == 0) and np.all(counts[:5] > 0)
    sums = np.zeros((8, 8), np.int64)
    sums[6, 0] = 10 ** 9                                                   # a sum on an empty phase must not win
    assert P.pick_phase(sums, counts) == (0, 0)
    sums[4, 7] = 1
    assert P.pick_phase(sums, counts) == (4, 7)
    assert P.pick_phase(np.zeros((8, 8)), P.phase_counts(7, 100)) is None
    assert np.array_equal(P.phase_counts(7, 100), np.zeros((8, 8), np.int64))
    with pytest.raises(ValueError):
        P.pick_phase(np.zeros(63), np.zeros(63))


def test_pick_offset_ties_go_to_the_smallest_placement():
    sc = np.zeros((3, 4), np.int64)
    assert P.pick_offset(sc) == (0, 0)
    sc[1, 2] = sc[2, 0] = 5
    assert P.pick_offset(sc) == (1, 2)
    sc[1, 1] = 5
    assert P.pick_offset(sc) == (1, 1)
    sc[2, 3] = 6
    assert P.pick_offset(sc) == (2, 3)
    big = np.array([[1 << 62, (1 << 62) + 1]], np.int64)                   # beyond float64's integers
    assert P.pick_offset(big) == (0, 1)
    assert P.pick_offset(np.zeros((0, 3), np.int64)) is None and P.pick_offset(np.zeros((2, 0), np.int64)) is None
    for c in sr.all_cases()[:3]:
        r = sr.located(*c)
        assert P.pick_offset(r["scores"]) == r["place"]


def test_soft_of_votes_against_the_payload_restatement():
    """soft_of_votes on a window of the keyed map = payload_refs.soft_ref (the CSR form of the plain decode) of the votes /
    32768 over the window's own CSR inverse; counts are the window's tiles per bit; entries outside the bits are skipped."""
    bits, tbi = sr.case_map("A")
    rng = np.random.default_rng(11)
    for (ty, tx, ny, nx) in ((0, 0, 16, 24), (1, 2, 14, 22), (5, 7, 1, 1), (0, 3, 16, 19)):
        V = rng.integers(-32768, 32769, (ny, nx)).astype(np.int32)
        win = tbi[ty:ty + ny, tx:tx + nx]
        soft, count = P.soft_of_votes(V, win, bits.size)
        flat = win.reshape(-1)
        order = np.argsort(flat, kind="stable").astype(np.int32)
        offs = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=bits.size))]).astype(np.int32)
        want = pr.soft_ref((V.reshape(1, -1) / 32768.0).astype(np.float32), order, offs)
        assert soft.dtype == np.float64 and np.array_equal(soft, want)
        assert np.array_equal(count, np.diff(offs))
        s2, c2 = sr.soft_ref(V, win, bits.size)
        assert np.array_equal(soft, s2) and np.array_equal(count, c2)
    bad = tbi[:4, :4].copy()
    bad[0, 0], bad[1, 1] = -1, bits.size
    V = np.full((4, 4), 100, np.int32)
    soft, count = P.soft_of_votes(V, bad, bits.size)
    assert count.sum() == 14 and soft.sum() * 32768 == 1400
    assert P.sync_confidence(soft, count) == pytest.approx(100 / 32768)
    assert P.sync_confidence(np.zeros(4), np.zeros(4, np.int64)) == 0.0
    with pytest.raises(ValueError):
        P.soft_of_votes(V, bad[:3], bits.size)


# ---- refusals, before anything crosses the C ABI ----------------------------------------------------------------------
def _meta(H, W, n_bits=80, dither=0, delta=16.0):
    members = M.payload_members("text", H, W, delta, n_bits, sr.NONCE, dither=dither)
    return M.sealed(members, 8, hg.hmac_digest(sr.key(), M.hmac_parts(members)))


@pytest.fixture
def no_device(monkeypatch):
    """any context, and so any library load, fails the test"""
    def refuse(*a, **k):
        raise AssertionError("a refusal must come before the first device call")
    monkeypatch.setattr(core, "_ctx", refuse)
    monkeypatch.setattr(core.hostapi, "load_library", refuse)


def test_search_refusals_come_before_any_device_call(no_device, tmp_path):
    H, W = 128, 192
    meta = _meta(H, W)
    st = np.zeros((100, 150, 3), np.uint8)
    for search in ("Crop", "shift", 1, True, ""):
        with pytest.raises(ValueError, match="search"):
            core.extract_payload_arrays(st, meta, sr.PASSWORD, search=search)
        with pytest.raises(ValueError, match="search"):
            core.extract_payload(str(tmp_path / "no.png"), str(tmp_path / "no.npz"), password=sr.PASSWORD, search=search)
    with pytest.raises(ValueError, match="dithered payload is not supported"):
        core.extract_payload_arrays(st, _meta(H, W, dither=P.DITHER_TABLE), sr.PASSWORD, search="crop")
    with pytest.raises(ValueError, match="16384"):
        core.extract_payload_arrays(np.zeros((64, 64, 3), np.uint8), _meta(1032, 1032, n_bits=16392), sr.PASSWORD, search="crop")
    for shape in ((129, 192, 3), (128, 193, 3), (136, 200, 3)):
        with pytest.raises(ValueError, match="larger than"):
            core.extract_payload_arrays(np.zeros(shape, np.uint8), meta, sr.PASSWORD, search="crop")
    for shape in ((7, 150, 3), (100, 7, 3), (0, 0, 3)):
        with pytest.raises(ValueError, match="whole 8x8 tile"):
            core.extract_payload_arrays(np.zeros(shape, np.uint8), meta, sr.PASSWORD, search="crop")
    with pytest.raises(ValueError, match="uint8"):
        core.extract_payload_arrays(np.zeros((100, 150), np.uint8), meta, sr.PASSWORD, search="crop")
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        core.extract_payload_arrays(st, meta, "not the password", search="crop")
    # without the keyword a cropped stego is refused as before, also before any device call
    with pytest.raises(ValueError, match="but the meta was written for"):
        core.extract_payload_arrays(st, meta, sr.PASSWORD)


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
    T = np.zeros((5, 7), np.int32)
    V = np.zeros((4, 6), np.int32)
    for delta in (7.9, float("nan"), 1000.0):
        with pytest.raises(ValueError, match="delta"):
            ctx.payload_phase_scan(st, delta)
        with pytest.raises(ValueError, match="delta"):
            ctx.payload_locate(st, T, 16, delta)
    with pytest.raises(ValueError):
        ctx.payload_phase_scan(st.astype(np.float32), 16.0)
    for n_bits in (0, 16385, -1):
        with pytest.raises(ValueError, match="n_bits"):
            ctx.payload_offset_scores(V, T, n_bits)
        with pytest.raises(ValueError, match="n_bits"):
            ctx.payload_locate(st, T, n_bits, 16.0)
    with pytest.raises(ValueError):
        ctx.payload_offset_scores(V.reshape(-1), T, 16)
    with pytest.raises(ValueError):
        ctx.payload_locate(st[None], T, 16, 16.0)
    # votes that do not fit the map: no placement, and nothing to ask the device for
    assert ctx.payload_offset_scores(np.zeros((6, 6), np.int32), T, 16).shape == (0, 2)
    assert ctx.payload_locate(np.zeros((7, 56), np.uint8), T, 16, 16.0) is None
