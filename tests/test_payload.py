"""Blind payload without a device: the tile-math helpers the kernels call (a stand-alone g++ program, plain and under
AddressSanitizer + UBSan) against the NumPy restatement (tests/payload_refs.py), the framing, the keyed map, the meta layout
and its refusals, host-side argument validation, the value claim on the restatement alone, and - also on the restatement
alone - what tests/test_gpu_payload_edges.py may assume of its hosts (pinned tiles, letterboxed planes, a document page)."""
import importlib
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import __graft_entry__ as ge
import payload_refs as pr
from oracle import wm_oracle as o

M = importlib.import_module(ge.PKG_NAME + ".meta")
P = importlib.import_module(ge.PKG_NAME + ".payload")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")


# ---- tile math ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request):
    return ge.build_payload_harness(sanitize=request.param == "sanitized")


def _run_harness(exe, tmp_path, Sc, bits, delta):
    Sc = np.ascontiguousarray(Sc, np.float32).reshape(-1, 8)
    n = Sc.shape[0]
    bits = np.ascontiguousarray(bits, np.uint8).reshape(-1)
    assert bits.size == n
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([n], np.int32).tobytes() + np.array([delta], np.float32).tobytes() + Sc.tobytes() + bits.tobytes())
    r = subprocess.run([exe, "run", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = np.fromfile(dst, np.float32)
    assert out.size == n * 4
    return out[:n], out[n:2 * n], out[2 * n:3 * n], out[3 * n:]


def test_restatement_precondition():
    """For both bit values at delta = 16 every tile of every host (the three seeded ones and the edge host) decodes
    correctly with |m| >= 0.4, on the restatement alone (0.50 here)."""
    worst = pr.check_preconditions(pr.DELTA, 0.4)
    print(f"worst margin {worst:.3f}")


def test_tile_math_edges(harness):
    """s_1 = 0, s_1 = 2040, s_2 = s_1, delta = 8 and delta = 512, the metric's lattice points: asserted inside the program"""
    r = subprocess.run([harness, "edges"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


@pytest.mark.parametrize("delta", [16.0, 8.0, 24.0, 512.0])
def test_tile_math_against_the_restatement_on_the_hosts(harness, tmp_path, delta):
    """payload_target / payload_metric on the oracle's Sc of the hosts, bits of seed 0.  The metric is bit for bit (one
    multiply, the rest rounds the same in any form).  The target is equal except where (s_1 - b delta) / (2 delta) is within
    1e-6 of a half-integer; on the seeded hosts at delta = 16 none is within 5e-3, asserted."""
    for name, _ in pr.all_hosts():
        Sc = pr.cover_sigma(name).reshape(-1, 8)
        bits = pr.seeded_bits(Sc.shape[0], 0)
        tie = pr.tie_distance(Sc, bits, delta)
        if name != "edge" and delta == 16.0:
            assert tie.min() > 5e-3, (name, tie.min())
        target, eff, m_q, m_s = _run_harness(harness, tmp_path, Sc, bits, delta)
        far = tie > 1e-6
        want = pr.target(Sc, bits, delta)
        assert np.array_equal(target[far], want[far]), name
        assert np.array_equal(eff[far], pr.sigma_w_eff(Sc, bits, delta)[far, 0]), name
        if name != "edge":
            assert far.all()
        # wherever the rounding went, the target sits on the bit's own lattice, above s_2 + delta (or is pinned at the top)
        assert np.array_equal(m_q, np.where(bits != 0, -1.0, 1.0).astype(np.float32)), name
        assert np.all(target - 4.0 >= Sc[:, 1] + delta), name
        assert np.array_equal(m_s.view(np.uint32), pr.metric(Sc[:, 0], delta).view(np.uint32)), name


def test_metric_bit_for_bit_on_a_dense_sweep(harness, tmp_path):
    rng = np.random.default_rng(3)
    s1 = np.concatenate([rng.uniform(0, 2040, 4000), np.arange(0, 2041, 4.0), [1e-3, 2039.999]]).astype(np.float32)
    Sc = np.zeros((s1.size, 8), np.float32); Sc[:, 0] = s1
    for delta in (8.0, 16.0, 21.5, 512.0):
        _, _, _, m_s = _run_harness(harness, tmp_path, Sc, np.zeros(s1.size, np.uint8), delta)
        assert np.array_equal(m_s.view(np.uint32), pr.metric(s1, delta).view(np.uint32)), delta
        assert m_s.min() >= -1.0 and m_s.max() <= 1.0


# ---- framing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", [b"", b"x", "Thử nghiệm ✓ – ключ".encode("utf-8"), b'{"owner":"A","id":7}'],
                         ids=["empty", "one_byte", "utf8", "json"])
def test_frame_round_trip(data):
    bits = P.payload_frame(data)
    assert bits.dtype == np.uint8 and bits.size == 8 * (len(data) + 8) and set(np.unique(bits)) <= {0, 1}
    head = np.unpackbits(np.frombuffer(len(data).to_bytes(4, "little") + data, np.uint8))
    assert np.array_equal(bits[:head.size], head)                           # the reference's header and bit order
    assert np.array_equal(bits[head.size:], np.unpackbits(np.frombuffer(zlib.crc32(data).to_bytes(4, "little"), np.uint8)))
    assert P.payload_unframe(bits) == (data, True)
    assert P.payload_unframe(bits.astype(bool)) == (data, True)


def test_frame_detects_damage():
    data = b"licence 42"
    bits = P.payload_frame(data)
    for i in (32, 40, bits.size - 33, bits.size - 1):                        # payload bits and CRC bits
        bad = bits.copy(); bad[i] ^= 1
        got, ok = P.payload_unframe(bad)
        assert not ok
        assert len(got) == len(data)
    # a length header larger than the capacity: not valid, and no exception
    bad = bits.copy(); bad[:32] = np.unpackbits(np.frombuffer((1 << 30).to_bytes(4, "little"), np.uint8))
    got, ok = P.payload_unframe(bad)
    assert not ok and len(got) <= len(data)
    bad = bits.copy(); bad[:32] = np.unpackbits(np.frombuffer((len(data) - 1).to_bytes(4, "little"), np.uint8))
    assert not P.payload_unframe(bad)[1]
    assert P.payload_unframe(np.ones(8, np.uint8)) == (b"", False)
    assert P.payload_unframe(np.zeros(0, np.uint8)) == (b"", False)
    assert not P.payload_unframe(np.random.default_rng(1).integers(0, 2, 104))[1]


def test_payload_bytes_and_names(tmp_path):
    assert P.payload_bytes("héllo", "text") == "héllo".encode("utf-8")
    assert P.payload_bytes(b"\xff\x00raw", "bytes") == b"\xff\x00raw"
    assert P.payload_bytes('{ "b" : 1,\n "a" : "é" }', "json") == '{"b":1,"a":"é"}'.encode("utf-8")
    with pytest.raises(ValueError, match="^JSON không hợp lệ: "):
        P.payload_bytes("{nope", "json")
    with pytest.raises(ValueError, match="payload_type"):
        P.payload_bytes("x", "image")
    with pytest.raises(TypeError):
        P.payload_bytes(17, "text")
    f = tmp_path / "p.json"
    f.write_text('{"k": [1, 2]}', encoding="utf-8")
    assert P.payload_bytes(str(f), "json") == b'{"k":[1,2]}'
    assert P.payload_bytes(str(f), "text", allow_file=False) == str(f).encode("utf-8")
    assert P.out_name("a/b.png", "text") == "a/b_text.txt" and P.out_name("a/b.TXT", "text") == "a/b.TXT"
    assert P.out_name("a/b.png", "json") == "a/b_data.json" and P.out_name("b.json", "json") == "b.json"
    w = P.write_payload(str(tmp_path / "out.png"), b'{"k":[1,2]}', "json")
    assert w.endswith("out_data.json") and json.load(open(w, encoding="utf-8")) == {"k": [1, 2]}
    w = P.write_payload(str(tmp_path / "out.png"), "hé\xff".encode("latin-1"), "text")
    assert w.endswith("out_text.txt") and open(w, encoding="utf-8").read() == "h"     # undecodable bytes are dropped


# ---- map ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nby,nbx,n_bits", [(9, 12, 104), (9, 12, 16), (8, 8, 64), (2, 8, 1), (12, 16, 72)])
def test_map_is_the_stable_inverse(nby, nbx, n_bits):
    key = hg.derive_key("pw", bytes(range(8)))
    tbi, order, offs = P.payload_map(nby, nbx, key, n_bits)
    n = nby * nbx
    perm = np.asarray(hg.permutation_index(nby, nbx, key))
    assert np.array_equal(np.sort(perm), np.arange(n))
    assert tbi.dtype == order.dtype == offs.dtype == np.int32
    assert np.array_equal(tbi, perm % n_bits)
    assert np.array_equal(order, np.argsort(perm % n_bits, kind="stable"))
    assert offs.shape == (n_bits + 1,) and offs[0] == 0 and offs[-1] == n
    counts = np.diff(offs)
    assert counts.min() >= 1 and counts.max() - counts.min() <= 1
    for j in range(n_bits):
        mine = order[offs[j]:offs[j + 1]]
        assert np.all(tbi[mine] == j) and np.all(np.diff(mine) > 0)         # the bit's tiles, ascending
    # another key, another map; the same key, the same map
    assert not np.array_equal(P.payload_map(nby, nbx, hg.derive_key("pw2", bytes(8)), n_bits)[0], tbi) or n_bits == 1
    assert np.array_equal(P.payload_map(nby, nbx, key, n_bits)[1], order)


def test_capacity_error_names_both_counts():
    with pytest.raises(ValueError, match=r"^Payload quá dài \(112 bits\).*108 tiles"):
        P.payload_map(9, 12, bytes(32), 112)
    with pytest.raises(ValueError, match=r"^Payload quá dài \(64 bits\).*0 tiles"):
        P.check_capacity(64, P.capacity_bits(7, 7))
    with pytest.raises(ValueError):
        P.payload_map(9, 12, bytes(32), 0)


# ---- meta -----------------------------------------------------------------------------------------------------------
_IMAGE_ORDER = ["mode", "payload_type", "shape", "delta", "payload_bits", "nonce", "tile", "digest"]
_VIDEO_ORDER = ["mode", "payload_type", "shape", "delta", "payload_bits", "nonce", "tile", "frame_interval", "n_frames", "digest"]


def _sealed(H, W, n_bits=104, video=None, key=bytes(32), ptype="text", delta=16.0, nonce=bytes(range(8))):
    members = M.payload_members(ptype, H, W, delta, n_bits, nonce, *(video or ()))
    return M.sealed(members, 8, hg.hmac_digest(key, M.hmac_parts(members)))


def test_meta_layout_dtypes_and_hmac_coverage():
    img = _sealed(72, 100)
    vid = _sealed(64, 96, 80, video=(2, 5))
    assert list(img) == _IMAGE_ORDER and list(vid) == _VIDEO_ORDER
    assert str(img["mode"]) == "payload" and str(img["payload_type"]) == "text"
    assert img["delta"].dtype == np.float32 and float(img["delta"]) == 16.0
    assert img["payload_bits"].dtype == np.int32 and img["tile"].dtype == np.int32 and int(img["tile"]) == 8
    assert img["nonce"].dtype == np.uint8 and img["nonce"].shape == (8,) and img["digest"].shape == (32,)
    assert tuple(img["shape"]) == (72, 100)
    assert vid["frame_interval"].dtype == np.int32 and vid["n_frames"].dtype == np.int32
    assert not any(k in img for k in ("Sc", "Uw", "Vwt", "Sw", "alpha", "kfrac"))
    assert M.is_payload(img) and M.tile_of(img) == 8 and M.nonce_of(img) == bytes(range(8))
    # the HMAC covers every member but the digest: changing any one of them is a wrong password
    key = bytes(32)
    assert M.authentic(img, key) and M.authentic(vid, key) and not M.authentic(img, bytes([1]) * 32)
    for k, v in (("delta", np.float32(24)), ("payload_bits", np.int32(96)), ("nonce", np.zeros(8, np.uint8)),
                 ("shape", np.array((72, 104))), ("payload_type", "json"), ("tile", np.int32(0))):
        assert not M.authentic(dict(img, **{k: v}), key), k
    for k, v in (("frame_interval", np.int32(1)), ("n_frames", np.int32(6))):
        assert not M.authentic(dict(vid, **{k: v}), key), k


def test_meta_survives_a_file_and_its_size_does_not_depend_on_the_content(tmp_path):
    """The saved meta holds the rule, not the cover: the same number of bytes for a 72 x 100 and a 2160 x 3840 image, for a
    3-frame and a 3000-frame video, for every payload type.  The file is a plain .npz (np.load, no pickle) with one member whose
    fields are the layout's members in their order and dtypes."""
    sizes = {}
    for name, meta in (("img_small", _sealed(72, 100)), ("img_4k", _sealed(2160, 3840, 129600, ptype="bytes")),
                       ("vid_3", _sealed(64, 96, 80, video=(2, 3))), ("vid_3000", _sealed(64, 96, 80, video=(2, 3000), ptype="json"))):
        path = M.save_payload_meta(str(tmp_path / name), meta)
        with np.load(path, allow_pickle=False) as z:
            assert z.files == ["payload"] and list(z["payload"].dtype.names) == list(meta)
        back = M.load_payload_meta(path)
        assert list(back) == list(meta) and M.authentic(back, bytes(32))
        for k in meta:
            assert np.array_equal(np.asarray(back[k]), np.asarray(meta[k])), k
            if k not in ("mode", "payload_type"):
                assert np.asarray(back[k]).dtype == np.asarray(meta[k]).dtype, k
        assert M.is_payload(back) and int(back["payload_bits"]) == int(meta["payload_bits"]) and M.tile_of(back) == 8
        assert M.unpack_payload(back) is back
        sizes[name] = os.path.getsize(path)
    print(sizes)
    assert sizes["img_small"] == sizes["img_4k"] and sizes["vid_3"] == sizes["vid_3000"]


def test_meta_file_is_under_1_kb(tmp_path):
    """The saved file is under 1 KB for a 72 x 100 image and for a 3-frame video (512 and 584 bytes).  One member per entry of the
    layout would not be: a zip member costs 76 bytes + twice its name + a .npy header before any data, 2 096 / 2 612 bytes for
    the 8 / 10 members - which is why the file packs them as the fields of one."""
    img = os.path.getsize(M.save_payload_meta(str(tmp_path / "img"), _sealed(72, 100)))
    vid = os.path.getsize(M.save_payload_meta(str(tmp_path / "vid"), _sealed(64, 96, 80, video=(2, 3))))
    print(f"payload meta: image {img} bytes, 3-frame video {vid} bytes")
    assert img < 1024 and vid < 1024


def test_existing_extract_and_detect_refuse_a_payload_meta(tmp_path):
    """before any device call: on a box without a GPU a context would fail with another error"""
    import dct_svd_core_secure as core
    video = importlib.import_module(ge.PKG_NAME + ".video")
    meta = _sealed(72, 100)
    st = np.zeros((72, 100, 3), np.uint8)
    with pytest.raises(ValueError, match="payload"):
        core.extract_arrays(st, meta, "pw")
    with pytest.raises(ValueError, match="payload"):
        core.detect_arrays(st, meta)
    for fn in (core.extract_arrays, lambda st_, m, pw: core.detect_arrays(st_, m)):     # the file form, as np.load hands it over
        with pytest.raises(ValueError, match="payload"):
            fn(st, M.pack_payload(meta), "pw")
    ip = M.save_payload_meta(str(tmp_path / "im"), meta)
    with pytest.raises(ValueError, match="payload"):
        core.detect(str(tmp_path / "none.png"), ip)
    assert core.extract_payload_arrays.__doc__ and M.unpack_payload(M.pack_payload(meta))["mode"] == "payload"
    path = M.save_payload_meta(str(tmp_path / "m"), _sealed(64, 96, 80, video=(1, 3)))
    for fn, args in ((video.extract_watermark_video, (str(tmp_path / "w.png"), "pw")), (video.detect_watermark_video, ()),
                     (video.extract_watermark_video_color, (str(tmp_path / "w.png"), "pw")), (video.detect_watermark_video_color, ())):
        with pytest.raises(ValueError, match="payload"):
            fn(str(tmp_path / "none.y4m"), path, *args)
    # and the payload readers refuse a watermark-image meta and an unauthentic one
    z = np.zeros((1, 1, 8), np.float32)
    gray = M.sealed({"mode": "gray", **M.common_members(8, 8, 0.1, 0.6, bytes(8)), **M.image_members(8, 8),
                     **M.gray_members(z, z, z, z)}, 8, bytes(32))
    with pytest.raises(ValueError, match="embed_payload"):
        core.extract_payload_arrays(st, gray, "pw")
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        core.extract_payload_arrays(st, meta, "not the password")


def test_public_functions_refuse_before_any_device_call(tmp_path):
    import dct_svd_core_secure as core
    video = importlib.import_module(ge.PKG_NAME + ".video")
    cover = np.zeros((72, 100, 3), np.uint8)
    for delta in (7.9, float("inf"), float("nan"), 513.0, "x"):
        with pytest.raises(ValueError, match="delta"):
            core.embed_payload_arrays(cover, b"hi", "pw", bytes(8), delta=delta)
    with pytest.raises(ValueError, match="^Payload quá dài"):
        core.embed_payload_arrays(cover, b"123456", "pw", bytes(8))          # 112 bits on 108 tiles
    with pytest.raises(ValueError, match=r"^Payload quá dài \(64 bits\).*\(0 tiles"):
        core.embed_payload_arrays(np.zeros((7, 7, 3), np.uint8), b"", "pw", bytes(8))
    with pytest.raises(ValueError, match="^JSON không hợp lệ"):
        core.embed_payload_arrays(cover, "{", "pw", bytes(8), payload_type="json")
    with pytest.raises(ValueError, match="payload_type"):
        core.embed_payload_arrays(cover, b"x", "pw", bytes(8), payload_type="image")
    with pytest.raises(ValueError):
        core.embed_payload_arrays(cover, b"x", "", bytes(8))
    with pytest.raises(TypeError):
        core.embed_payload_arrays(cover, b"x", True, bytes(8))
    with pytest.raises(ValueError, match="^JSON không hợp lệ"):
        core.embed_payload(str(tmp_path / "no.png"), "{", str(tmp_path / "o.png"), str(tmp_path / "m.npz"), password="pw",
                           payload_type="json")
    with pytest.raises(ValueError, match="delta"):
        video.embed_payload_video(str(tmp_path / "no.y4m"), "x", str(tmp_path / "o.y4m"), str(tmp_path / "m.npz"),
                                  password="pw", delta=4.0)
    v = str(tmp_path / "small.y4m")
    video.write_y4m(v, np.zeros((2, 16, 16), np.uint8))
    with pytest.raises(ValueError, match="^Payload quá dài"):
        video.embed_payload_video(v, "x", str(tmp_path / "o.y4m"), str(tmp_path / "m.npz"), password="pw")


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
    st = np.zeros((72, 100), np.uint8)
    tb = np.zeros(108, np.uint8)
    _, order, offs = pr.simple_map(108, 16)
    for delta in (7.9, float("inf"), float("nan"), 1000.0):
        for call in (lambda: ctx.payload_sigma_w(st, tb, delta), lambda: ctx.embed_tiles_payload(st, tb, delta),
                     lambda: ctx.payload_metric(st, delta), lambda: ctx.payload_soft(st, order, offs, 16, delta)):
            with pytest.raises(ValueError, match="delta"):
                call()
    for bad in (tb[:-1], np.full(108, 2, np.uint8), np.zeros(109, np.uint8)):
        with pytest.raises(ValueError):
            ctx.embed_tiles_payload(st, bad, 16.0)
        with pytest.raises(ValueError):
            ctx.payload_sigma_w(st, bad, 16.0)
    with pytest.raises(ValueError):
        ctx.embed_tiles_payload(st.astype(np.float32), tb, 16.0)
    for n_bits in (0, 109):
        with pytest.raises(ValueError, match="n_bits"):
            ctx.payload_soft(st, order, offs, n_bits, 16.0)
    short = offs.copy(); short[-1] = 107
    down = offs.copy(); down[3] = down[2] - 1
    first = offs.copy(); first[0] = 1
    for bad in (short, down, first, offs[:-1]):
        with pytest.raises(ValueError):
            ctx.payload_soft(st, order, bad, 16, 16.0)
    out = order.copy(); out[5] = 108
    neg = order.copy(); neg[5] = -1
    for bad in (out, neg, order[:-1]):
        with pytest.raises(ValueError):
            ctx.payload_soft(st, bad, offs, 16, 16.0)


# ---- the value claim, on the restatement alone ----------------------------------------------------------------------
def test_payload_survives_noise_and_keeps_the_cover_on_the_restatement():
    """72 x 100 host seed 1, n_bits = 16 on 108 tiles, delta = 16: the decoded bits are exact after uniform noise in
    [-2, 2] is added to the stego, and PSNR(cover, stego) >= 45 dB (46.5 here)."""
    H, W, seed = pr.HOSTS[0]
    Y = pr.host(H, W, seed)
    bits = pr.seeded_bits(16, 11)
    tbi, order, offs = pr.simple_map(108, 16)
    r = pr.embed_ref(Y, bits[tbi], pr.DELTA)
    psnr = o.psnr(Y, r["stego"])
    clean = pr.soft_ref(pr.metric_ref(r["stego"], pr.DELTA).reshape(1, -1), order, offs)
    assert np.array_equal(clean < 0, bits != 0)
    noise = np.random.default_rng(4).integers(-2, 3, (H, W))
    noisy = np.clip(r["stego"].astype(int) + noise, 0, 255).astype(np.uint8)
    soft = pr.soft_ref(pr.metric_ref(noisy, pr.DELTA).reshape(1, -1), order, offs)
    count = np.diff(offs)
    print(f"PSNR {psnr:.2f} dB; clean worst |soft| / count {np.min(np.abs(clean) / count):.3f}, noisy {np.min(np.abs(soft) / count):.3f}")
    assert np.array_equal(soft < 0, bits != 0)
    assert psnr >= 45.0


# ---- the edge hosts and what the GPU tests may assume of them, on the restatement alone ------------------------------
def test_edge_hosts_are_what_they_say():
    Y = pr.pinned_host()
    assert Y.shape == pr.PINNED and Y.dtype == np.uint8 and len(pr.pinned_names()) == 32
    tiles = o.to_tiles(Y).reshape(32, 64)
    assert len({t.tobytes() for t in tiles}) == 32                            # one class per tile
    D = pr.document_host(*pr.DOCUMENT, pr.DOCUMENT_SEED)
    assert D.shape == pr.DOCUMENT and set(np.unique(D)) == {0, 255} and 0.02 < (D == 0).mean() < 0.2
    L = pr.letterbox_planes()
    base = pr.mr.planes_of(72, 100, 3)
    assert L.shape == (3, 72, 100) and np.array_equal(L[0], base[0])
    black = [pr.black_tiles(p) for p in L]
    assert not black[0].any() and not any(pr.black_tiles(p).any() for p in base)
    want1 = np.zeros((9, 12), bool); want1[:2] = True; want1[7:] = True
    want2 = np.zeros((9, 12), bool); want2[:, :3] = True
    assert np.array_equal(black[1], want1) and np.array_equal(black[2], want2)
    assert np.array_equal(L[1][16:56], base[1][16:56]) and np.array_equal(L[2][:, 24:], base[2][:, 24:])
    assert np.array_equal(L[2][:, 96:], base[2][:, 96:])                       # the ragged edge keeps its content


_EDGE_NAMES = [n for n, _ in pr.edge_hosts()] + ["letterbox0", "letterbox1", "letterbox2"]


@pytest.mark.parametrize("delta", pr.EDGE_DELTAS)
def test_margins_ties_and_comparable_tiles(delta):
    """For every (host, delta, bit seed) the GPU edge tests use: the share of tiles without a unique restatement or a clear
    vote (a rounding tie, s_1 = s_2, |m| within the slope bar 2 (1e-4 2040) / delta of 0) is at most 10 % of a seeded or
    letterbox host and at most half of the edge or pinned host.  Measured: seeded hosts 0..7 of 108 and 0..4 of 64 (all but 1
    of them at delta = 8, where the bar is 0.051 and the worst margin 0.005), letterbox 0..4 of 108 (a black tile counts as
    comparable: margins_of), edge 1..6 of 16, pinned 4..9 of 32; ties at most 1 of 108 / 64 and at most 6 of 16 on the edge
    host; 2 tiles of the edge host with s_1 = s_2 (the black one among them)."""
    assert np.isclose(pr.slope_bar(delta), 2 * (1e-4 * 2040) / delta)
    for seed in pr.EDGE_BIT_SEEDS:
        for name in _EDGE_NAMES:
            r = pr.margins(name, delta, seed)
            n = r["signed"].size
            out = n - int(r["comparable"].sum())
            print(f"delta {delta:g} bits {seed} {name}: left out {out} of {n} (tie {int(r['tie'].sum())}, degenerate {int(r['deg'].sum())}), "
                  f"wrong-voting comparable tiles {int((r['signed'][r['comparable']] < 0).sum())}, worst margin {float(r['signed'].min()):+.3f}, "
                  f"Yw in [{float(r['Yw'].min()):.0f}, {float(r['Yw'].max()):.0f}]")
            assert out <= pr.left_out_cap(name) * n, (name, delta, seed, out, n)
            if name == "pinned":        # the unclipped plane leaves 0..255: above at every delta, below too from delta = 16 on
                Yw = o.to_tiles(r["Yw"])[~r["tie"] & ~r["deg"]]
                assert Yw.max() > 255.5 and (delta < 16 or Yw.min() < -0.5), (delta, seed, float(Yw.min()), float(Yw.max()))
            elif name == "edge":
                assert r["tie"].sum() <= 6 and pr.degenerate_tiles(r["Sc"]).sum() == 2
            elif name != "pinned":
                assert r["tie"].sum() <= 2 and not r["deg"].any()
                assert not (r["signed"][r["comparable"]] < 0).any()          # natural and black tiles take their bit


def test_pinned_tiles_vote_against_their_bit():
    """DESIGN 14's limit, per class at delta = 16 with every tile carrying 0, then 1: a half-255 / half-0 tile (s_1 = 1442.5,
    aimed at 1460) carrying 1 has margin -0.69; a 0 / 255 checkerboard and the 4 + 4 block diagonal (s_1 = s_2 = 1020)
    carrying 0 have -1.0; the 230 / 255 checkerboard carrying 0 has 0.0.  And the embed leaves 0..255 before the clip."""
    Y = pr.pinned_host()
    r = [pr.margins_of(Y, np.full(32, b, np.uint8), 16.0) for b in (0, 1)]
    m = {nm: (float(r[0]["signed"].ravel()[i]), float(r[1]["signed"].ravel()[i])) for i, nm in enumerate(pr.pinned_names())}
    for nm, (m0, m1) in m.items():
        print(f"{nm:24s} bit 0 {m0:+.3f}  bit 1 {m1:+.3f}")
    for nm in ("half_left_255", "half_right_255", "half_top_255", "half_bottom_255", "rows_255_0", "cols_255_0"):
        assert abs(m[nm][1] + 0.6875) < 0.01 and m[nm][0] > 0.6, nm
    for nm in ("checker_0_255", "checker_255_0", "blockdiag_4_4"):
        assert abs(m[nm][0] + 1.0) < 0.01, nm
    assert abs(m["checker_230_255"][0]) < 0.01
    assert min(m["white"]) > 0.999                                            # (a white tile takes either bit)
    assert sum(min(v) < 0 for v in m.values()) >= 10
    assert min(x["Yw"].min() for x in r) < -1 and max(x["Yw"].max() for x in r) > 256


def test_document_host_repetition_does_not_cover_pinned_tiles():
    """White page with strokes, 128 x 256 (512 tiles), delta = 16, the keyed map of password "pw" and DOCUMENT_NONCE: with 80
    bits (6.4 tiles a bit) every bit decodes, with 136 bits one does not, with n_bits = n_tiles 42 do not - each wrong-voting
    tile is one wrong bit.  Measured: 43 / 39 / 42 of 512 tiles vote wrong; worst |soft| / count at 80 bits 0.35.  'sure': the
    restatement's verdict cannot be turned by the tiles a device may legitimately see otherwise."""
    Y = pr.document_host(*pr.DOCUMENT, pr.DOCUMENT_SEED)
    key = hg.derive_key("pw", pr.DOCUMENT_NONCE)
    got = {}
    for data in pr.DOCUMENT_PAYLOADS:
        bits = P.payload_frame(data)
        tbi, order, offs = P.payload_map(Y.shape[0] // 8, Y.shape[1] // 8, key, bits.size)
        v = pr.document_votes(Y, bits, tbi, order, offs)
        got[bits.size] = v
        print(f"n_bits {bits.size}: {int((v['signed'] < 0).sum())} of 512 tiles vote wrong ({int((v['signed'][v['comparable']] < 0).sum())} comparable, "
              f"{int((~v['comparable']).sum())} left out), {int(v['wrong'].sum())} bits wrong ({int((v['wrong'] & v['sure']).sum())} surely), "
              f"worst |soft| / count {float(np.min(np.abs(v['soft']) / v['count'])):.3f}")
    assert sorted(got) == [80, 136, 512]
    assert not got[80]["wrong"].any() and got[80]["sure"].all()
    assert (got[136]["wrong"] & got[136]["sure"]).sum() >= 1
    assert got[512]["wrong"].sum() >= 1 and (got[512]["wrong"] & got[512]["sure"]).sum() >= 1
    assert (~got[512]["comparable"]).sum() <= 0.10 * 512
