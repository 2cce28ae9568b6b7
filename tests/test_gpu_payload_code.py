"""Channel code of the blind payload on the device (include/wmhip.h, "channel code"): k_payload_viterbi
bit for bit against the NumPy restatement (tests/payload_code_refs.py: info bits, final metric, every decision word), its
headroom at the largest decode, its refusals, and the product with code="k7" - the document host, the cropped stego under both
searches, files, video - on the cases whose preconditions tests/test_payload_code.py asserts on the restatement alone."""
import importlib
import os

import numpy as np
import pytest

import payload_code_refs as cr
import payload_refs as pr
import payload_sync_refs as sr
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

P = importlib.import_module(PKG_NAME + ".payload")
M = importlib.import_module(PKG_NAME + ".meta")
hg = importlib.import_module(PKG_NAME + ".hostglue")
hostapi = importlib.import_module(PKG_NAME + ".hostapi")
_vp = hostapi._vp


def _batches():
    """[(id, n_info, [names], L int32 [3, 2 n_steps])]: the shared vectors three codewords to a call - the noiseless, flipped and
    erased vector of every n_info, and per tie size the all-zero vector, the {-1, 0, 1} vector and that one scaled to +-(2^31 -
    1), which the clamp on load makes +-1024 (a different vector from +-1: restated as such)."""
    by = {}
    for name, n, _, L in cr.vectors():
        by.setdefault((name.split("-")[0] in ("zero", "unit"), n), []).append((name, L))
    out = []
    for (tie, n), vs in by.items():
        rows = [L for _, L in vs]
        names = [nm for nm, _ in vs]
        if tie:
            rows.append((rows[1].astype(np.int64) * (2 ** 31 - 1)).astype(np.int32))
            names.append(None)
        assert len(rows) == 3
        out.append((("tie" if tie else "n") + str(n), n, names, np.stack(rows)))
    return out


def _want(n, names, rows):
    return [cr.decoded(nm) if nm else cr.viterbi_ref(np.clip(row, -1024, 1024), n) for nm, row in zip(names, rows)]


def _dev_decode(ctx, wide, n_info, stride, decisions=True, metric=True):
    """wm_payload_decode_k7_dev on device copies of ``wide`` [n, stride]"""
    n = wide.shape[0]
    info = np.full((n, n_info), 7, np.uint8)
    fm = np.zeros(n, np.int32)
    D = np.zeros((n, n_info + 6), np.uint64)
    with ctx._staging() as dev:
        d_L, = dev.up(wide)
        d_info, d_fm, d_D = dev.alloc(info.nbytes), dev.alloc(fm.nbytes), dev.alloc(D.nbytes)
        ctx._call("wm_payload_decode_k7_dev", _vp(d_L), n_info, n, stride, _vp(d_info), _vp(d_fm) if metric else None,
                  _vp(d_D) if decisions else None)
        ctx.d2h(info, d_info)
        if metric:
            ctx.d2h(fm, d_fm)
        if decisions:
            ctx.d2h(D, d_D)
        ctx.sync()
    return info, fm, D


@pytest.mark.parametrize("batch", _batches(), ids=lambda b: b[0])
def test_kernel_is_the_restatement_bit_for_bit(gpu_ctx, batch):
    """Three codewords a call at a stride of 2 n_steps + 5 (odd: every second row starts off an 8-byte line), host form and
    _dev form, with and without the caller's decision words."""
    _, n, names, rows = batch
    want = _want(n, names, rows)
    stride = rows.shape[1] + 5
    wide = np.full((3, stride), 999, np.int32)
    wide[:, :rows.shape[1]] = rows
    info, fm, D = gpu_ctx.payload_decode(wide[:, :rows.shape[1]], decisions=True)       # the host form, read in place
    for k in range(3):
        assert np.array_equal(info[k], want[k][0]) and int(fm[k]) == want[k][1] and np.array_equal(D[k], want[k][2]), (names[k], "host")
    info2, fm2 = gpu_ctx.payload_decode(rows)                                # contiguous rows, the context's own words
    assert np.array_equal(info2, info) and np.array_equal(fm2, fm)
    one = gpu_ctx.payload_decode(rows[1])
    assert one[0].shape == (n,) and np.array_equal(one[0], info[1]) and int(one[1]) == int(fm[1])
    info3, fm3, D3 = _dev_decode(gpu_ctx, wide, n, stride)
    assert np.array_equal(info3, info) and np.array_equal(fm3, fm) and np.array_equal(D3, D)
    info4, _, _ = _dev_decode(gpu_ctx, wide, n, stride, decisions=False, metric=False)
    assert np.array_equal(info4, info)
    for k, nm in enumerate(names):                                          # (the precondition test_payload_code asserts)
        u = next(v[2] for v in cr.vectors() if v[0] == nm) if nm else None
        if u is not None:
            assert np.array_equal(info[k], u), nm


def test_values_at_the_int32_ends_decode_as_their_clamp(gpu_ctx):
    _, n, _, L = next(v for v in cr.vectors() if v[0] == "flip-123")
    big = np.where(L > 0, 2 ** 31 - 1, np.where(L < 0, -(2 ** 31 - 1), 0)).astype(np.int32)
    a = gpu_ctx.payload_decode(big, decisions=True)
    b = gpu_ctx.payload_decode(np.clip(big, -1024, 1024), decisions=True)
    w = cr.viterbi_ref(np.clip(big, -1024, 1024), n)
    for got in (a, b):
        assert np.array_equal(got[0], w[0]) and int(got[1]) == w[1] and np.array_equal(got[2], w[2])


def test_headroom_at_the_largest_decode(gpu_ctx):
    """n_steps = 2^18 with every value at the clamp: the metric of the all-zero path climbs by 2048 a step to 2^29 exactly, the
    others stay above -2^30 - 2^29; no restatement needed.  Then the all-ones frame's codeword at full weight."""
    n_steps = 1 << 18
    n_info = n_steps - 6
    info, fm = gpu_ctx.payload_decode(np.full(2 * n_steps, 1024, np.int32))
    assert not info.any() and int(fm) == 1 << 29
    coded = P.encode_k7(np.ones(n_info, np.uint8)).astype(np.int32)
    info, fm = gpu_ctx.payload_decode(1024 - 2048 * coded)
    assert info.all() and int(fm) == 1 << 29


def test_refusals(gpu_ctx):
    L = np.zeros(64, np.int32)
    info = np.zeros(32, np.uint8)
    p = lambda a: _vp(a.ctypes.data)
    calls = [("wm_payload_decode_k7", p(L), p(info))]
    with gpu_ctx._staging() as dev:
        d_L, = dev.up(L)
        d_info = dev.alloc(64)
        calls.append(("wm_payload_decode_k7_dev", _vp(d_L), _vp(d_info)))
        for name, a_L, a_info in calls:
            for n_info, n_cw, stride, ptrs, msg in (((1 << 18) - 5, 1, 1 << 20, (a_L, a_info), "2\\^18"),
                                                    (10, 1, 31, (a_L, a_info), "llr_stride"),
                                                    (10, 2, 31, (a_L, a_info), "llr_stride"),
                                                    (0, 1, 64, (a_L, a_info), "n_info"),
                                                    (10, 0, 64, (a_L, a_info), "n_codewords"),
                                                    (10, 1, 32, (None, a_info), "NULL"),
                                                    (10, 1, 32, (a_L, None), "NULL")):
                with pytest.raises(ValueError, match=msg):
                    gpu_ctx._call(name, ptrs[0], n_info, n_cw, stride, ptrs[1], None, None)
        gpu_ctx._call("wm_payload_decode_k7_dev", _vp(d_L), 10, 1, 32, _vp(d_info), None, None)     # and the same sizes, valid
        gpu_ctx.sync()
    gpu_ctx.check_status()


# ---- the product ----------------------------------------------------------------------------------------------------------
def _bgr(Y):
    return np.ascontiguousarray(np.stack([Y] * 3, axis=-1))


@pytest.mark.parametrize("dither", [False, True], ids=["plain", "dither"])
def test_document_host_takes_the_payloads_repetition_loses(gpu_ctx, dither):
    import dct_svd_core_secure as core
    cover = _bgr(pr.document_host(*pr.DOCUMENT, pr.DOCUMENT_SEED))
    kw = dict(payload_type="bytes", dither=dither)
    if not dither:                       # (without the code: as today - asserted on the restatement for the dither-free rule)
        with pytest.raises(ValueError, match=r"^payload does not decode from its own stego: \d+ of 136 bits wrong"):
            core.embed_payload_arrays(cover, pr.DOCUMENT_PAYLOADS[1], "pw", pr.DOCUMENT_NONCE, **kw)
    for data in cr.DOCUMENT_DATA:
        out = core.embed_payload_arrays(cover, data, "pw", pr.DOCUMENT_NONCE, code="k7", **kw)
        assert int(out["meta"]["code"]) == 1 and int(out["meta"]["payload_bits"]) == 8 * (len(data) + 8)
        got, valid, conf = core.extract_payload_arrays(out["stego"], M.pack_payload(out["meta"]), "pw")
        assert got == data and valid is True and 0.0 < conf <= 1.0
        with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
            core.extract_payload_arrays(out["stego"], dict(out["meta"], code=np.uint8(0)), "pw")
    # the page's limit with the code: 23 bytes are 508 coded bits on 512 tiles, 24 bytes are past the capacity
    with pytest.raises(ValueError, match=r"Payload quá dài \(524 bits\)"):
        core.embed_payload_arrays(cover, bytes(range(24)), "pw", pr.DOCUMENT_NONCE, code="k7", **kw)


@pytest.mark.parametrize("seed", cr.CROP_CASE["seeds"])
def test_cropped_stego_comes_back_through_the_code(gpu_ctx, seed):
    import dct_svd_core_secure as core
    H, W = cr.CROP_CASE["shape"]
    data, (y0, x0, h, w) = cr.CROP_CASE["data"], cr.CROP_CASE["crop"]
    cover = _bgr(pr.host(H, W, seed))
    crop = lambda st: np.ascontiguousarray(st[y0:y0 + h, x0:x0 + w])
    plain = core.embed_payload_arrays(cover, data, sr.PASSWORD, sr.NONCE, payload_type="bytes")
    got = core.extract_payload_arrays(crop(plain["stego"]), plain["meta"], sr.PASSWORD, search="crop")
    assert got[1] is False
    coded = core.embed_payload_arrays(cover, data, sr.PASSWORD, sr.NONCE, payload_type="bytes", code="k7")
    got, valid, conf, origin = core.extract_payload_arrays(crop(coded["stego"]), coded["meta"], sr.PASSWORD, search="crop")
    assert valid is True and origin == (y0, x0) and got == data and conf > 0.5
    # the whole stego reads back too, with the search and without it
    assert core.extract_payload_arrays(coded["stego"], coded["meta"], sr.PASSWORD)[:2] == (data, True)
    assert core.extract_payload_arrays(coded["stego"], coded["meta"], sr.PASSWORD, search="crop")[3] == (0, 0)
    # the dithered twin under the keyed search
    plain = core.embed_payload_arrays(cover, data, sr.PASSWORD, sr.NONCE, payload_type="bytes", dither=True)
    assert core.extract_payload_arrays(crop(plain["stego"]), plain["meta"], sr.PASSWORD, search="crop-keyed")[1] is False
    coded = core.embed_payload_arrays(cover, data, sr.PASSWORD, sr.NONCE, payload_type="bytes", dither=True, code="k7")
    got, valid, conf, origin = core.extract_payload_arrays(crop(coded["stego"]), coded["meta"], sr.PASSWORD, search="crop-keyed")
    assert valid is True and origin == (y0, x0) and got == data


def test_files_round_trip_and_nothing_is_left_when_refused(gpu_ctx, tmp_path):
    import dct_svd_core_secure as core
    cover = _bgr(pr.host(128, 160, 2))
    cp, sp, mp = str(tmp_path / "cover.png"), str(tmp_path / "stego.png"), str(tmp_path / "meta.npz")
    assert hg.write_png(cp, cover)
    core.embed_payload(cp, "id 7", sp, mp, password="pw", nonce=bytes([5] * 8), code="k7")
    assert os.path.getsize(mp) == 513
    data, valid, conf, written = core.extract_payload(sp, mp, str(tmp_path / "out"), password="pw")
    assert data == b"id 7" and valid is True and open(written).read() == "id 7"
    assert M.payload_code_of(M.load_payload_meta(mp)) == 1
    core.embed_payload(cp, "id 7", sp, mp, password="pw", nonce=bytes([5] * 8), code="k7", dither=True)
    assert os.path.getsize(mp) == 578
    assert core.extract_payload(sp, mp, password="pw")[:2] == (b"id 7", True)
    # 320 tiles: 19 bytes frame to 216 bits and fit without the code; 2 (216 + 6) = 444 coded bits do not
    sp2, mp2 = str(tmp_path / "s2.png"), str(tmp_path / "m2.npz")
    with pytest.raises(ValueError, match=r"Payload quá dài \(444 bits\)"):
        core.embed_payload(cp, bytes(range(65, 84)), sp2, mp2, password="pw", payload_type="bytes", code="k7")
    assert not os.path.exists(sp2) and not os.path.exists(mp2) and not os.path.exists(str(tmp_path / "s2_stego.png"))
    core.embed_payload(cp, bytes(range(65, 84)), sp2, mp2, password="pw", payload_type="bytes")
    assert os.path.getsize(mp2) == 512


@pytest.mark.parametrize("dither", [False, True], ids=["plain", "dither"])
def test_video_round_trip(gpu_ctx, tmp_path, dither):
    """A 3-frame .y4m, frame_interval = 1.  The frames are 96 x 128 (192 tiles): a 64 x 64 frame has 64 tiles and the smallest
    coded frame (no data: 64 bits) has 2 (64 + 6) = 140 coded bits, so no payload fits one with the code - asserted below."""
    v = importlib.import_module(PKG_NAME + ".video")
    assert P.capacity_bits(64, 64) == 64 < P.coded_bits(P.payload_frame(b"").size) == 140
    H, W = 96, 128
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = np.stack([np.clip(120 + 50 * np.sin(xx / 14.0 + f) * np.cos(yy / 10.0) + rng.normal(0, 6, (H, W)), 0, 255).astype(np.uint8)
                       for f in range(3)])
    src, outp, metap = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "vm.npz")
    v.write_y4m(src, frames)
    data = b"v1"                                                            # 80 bits, 172 coded, on 192 tiles
    v.embed_payload_video(src, data, outp, metap, password="pw", payload_type="bytes", nonce=bytes([3] * 8), frame_interval=1,
                          batch=2, dither=dither, code="k7")
    assert os.path.getsize(metap) == (650 if dither else 585)
    got, valid, conf, soft = v.extract_payload_video(outp, metap, password="pw", batch=3, return_soft=True)
    assert got == data and valid is True and soft.shape == (172,) and conf > 0.5
    small = str(tmp_path / "small.y4m")
    v.write_y4m(small, frames[:, :64, :64])
    with pytest.raises(ValueError, match=r"Payload quá dài \(140 bits\)"):
        v.embed_payload_video(small, b"", str(tmp_path / "o2.y4m"), str(tmp_path / "m2.npz"), password="pw", payload_type="bytes",
                              code="k7")
    assert not os.path.exists(str(tmp_path / "m2.npz"))


def test_code_off_is_the_parent(gpu_ctx, tmp_path):
    """code=None and no code argument: the same stego bytes and the same packed meta bytes; and a meta in the parent's format
    (members written out here, without the product's payload_members) extracts as it did."""
    import dct_svd_core_secure as core
    cover = _bgr(pr.host(72, 100, 1))
    for dither in (False, True):
        a = core.embed_payload_arrays(cover, "id 7", "pw", bytes([3] * 8), dither=dither)
        b = core.embed_payload_arrays(cover, "id 7", "pw", bytes([3] * 8), dither=dither, code=None)
        assert np.array_equal(a["stego"], b["stego"]) and "code" not in a["meta"] and list(a["meta"]) == list(b["meta"])
        ra, rb = M.pack_payload(a["meta"])["payload"], M.pack_payload(b["meta"])["payload"]
        assert ra.dtype == rb.dtype and ra.tobytes() == rb.tobytes()
        pa, pb = M.save_payload_meta(str(tmp_path / "a"), a["meta"]), M.save_payload_meta(str(tmp_path / "b"), b["meta"])
        assert os.path.getsize(pa) == (577 if dither else 512)
        za, zb = np.load(pa)["payload"], np.load(pb)["payload"]
        assert za.dtype == zb.dtype and za.tobytes() == zb.tobytes()
        # the parent's format, member by member
        key = hg.derive_key("pw", bytes([3] * 8))
        old = dict(mode="payload", payload_type="text", shape=np.array((72, 100), np.int64), delta=np.float32(16.0))
        if dither:
            old["dither"] = np.uint8(1)
        old.update(payload_bits=np.int32(96), nonce=np.frombuffer(bytes([3] * 8), np.uint8), tile=np.int32(8))
        old["digest"] = np.frombuffer(hg.hmac_digest(key, M.hmac_parts(old)), np.uint8)
        assert old["digest"].tobytes() == np.asarray(a["meta"]["digest"]).tobytes()
        assert core.extract_payload_arrays(a["stego"], old, "pw")[:2] == (b"id 7", True)
