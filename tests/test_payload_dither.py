"""Blind payload with keyed dither, without a device: the NumPy restatement (tests/payload_dither_refs.py) against the
dither-free one at u = 0, the tile-math helpers the kernels call (a stand-alone g++ program, plain and under
AddressSanitizer + UBSan) against the restatement bit for bit, what the GPU tests may assume of their hosts, the product's
dither table, the meta member and host-side argument validation."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import payload_dither_refs as dr
import payload_refs as pr

M = importlib.import_module(ge.PKG_NAME + ".meta")
P = importlib.import_module(ge.PKG_NAME + ".payload")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
F = np.float32


def _key():
    return hg.derive_key(dr.PASSWORD, dr.NONCE)


# ---- the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", pr.EDGE_DELTAS)
def test_restatement_with_zero_words_is_the_dither_free_one(delta):
    for name, _ in pr.all_hosts():
        Sc = pr.cover_sigma(name)
        bits = pr.seeded_bits(Sc.shape[0] * Sc.shape[1], 0).reshape(Sc.shape[:2])
        z = np.zeros(Sc.shape[:2], np.uint16)
        assert np.array_equal(dr.target(Sc, bits, z, delta).view(np.uint32), pr.target(Sc, bits, delta).view(np.uint32)), name
        assert np.array_equal(dr.sigma_w_eff(Sc, bits, z, delta).view(np.uint32), pr.sigma_w_eff(Sc, bits, delta).view(np.uint32))
        assert np.array_equal(dr.metric(Sc[..., 0], z, delta).view(np.uint32), pr.metric(Sc[..., 0], delta).view(np.uint32))


def test_offset_range_and_lattice():
    for delta in dr.DELTAS:
        u = np.arange(65536, dtype=np.uint32).astype(np.uint16)
        d = dr.offset(u, delta)
        assert d.dtype == F and d[0] == 0.0 and np.all(np.diff(d) > 0) and d[-1] < 2 * delta
        assert d[32768] == F(delta)
        # a tile on its own lattice point reads +1 / -1, and the dither-free read of it reads the phase
        Sc = np.zeros((65536, 8), F); Sc[:, 0] = 700.0
        for b in (0, 1):
            q = dr.target(Sc, np.full(65536, b), u, delta) - pr.BIAS
            m = dr.metric(q, u, delta)
            assert np.all(np.abs(m - (-1.0 if b else 1.0)) <= 4 * 1100 * 2.0 ** -24 * 4 / (2 * delta) + 1e-6), (delta, b)
            assert np.all(q >= Sc[:, 1] + delta)


# ---- host build against NumPy ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request):
    return ge.build_payload_dither_harness(sanitize=request.param == "sanitized")


def _run_harness(exe, tmp_path, Sc, bits, u, delta):
    Sc = np.ascontiguousarray(Sc, F).reshape(-1, 8)
    n = Sc.shape[0]
    bits = np.ascontiguousarray(bits, np.uint8).reshape(-1); u = np.ascontiguousarray(u, np.uint16).reshape(-1)
    assert bits.size == n and u.size == n
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([n], np.int32).tobytes() + np.array([delta], F).tobytes() + Sc.tobytes() + bits.tobytes() + u.tobytes())
    r = subprocess.run([exe, "run", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout)
    out = np.fromfile(dst, F)
    assert out.size == n * 4
    return out[:n], out[n:2 * n], out[2 * n:3 * n], out[3 * n:]


def _grid(delta, seed=0):
    """(Sc [n, 8], bit [n], u [n]): s_1 near 0, near 2040, on half-integer ties of the dither-free lattice, on the lattice
    points, seeded; s_2 = 0, s_1 / 3, s_1; both bits; u in the edge words and seeded words"""
    rng = np.random.default_rng(seed)
    two = 2.0 * delta
    s1 = np.concatenate([[0.0, 1e-3, 0.5, 1.0, delta / 2, delta, 2039.0, 2039.999, 2040.0, 2040.0 - delta, 2036.0],
                         np.arange(0.0, 2040.0, two)[:40] + delta / 2, np.arange(0.0, 2040.0, two)[:40] + 3 * delta / 2,
                         np.arange(0.0, 2040.0, delta)[:60], rng.uniform(0, 2040, 200)]).astype(F)
    s1 = s1[s1 <= 2040.0]
    words = np.concatenate([np.array(dr.U_EDGES), rng.integers(0, 65536, 6)]).astype(np.uint16)
    S1, FR, B, U = np.meshgrid(s1, np.array([0.0, 1.0 / 3.0, 1.0], F), np.array([0, 1], np.uint8), words, indexing="ij")
    Sc = np.zeros((S1.size, 8), F)
    Sc[:, 0] = S1.ravel(); Sc[:, 1] = (S1 * FR).ravel().astype(F)
    return Sc, B.ravel(), U.ravel()


@pytest.mark.parametrize("delta", dr.DELTAS)
def test_host_build_agrees_with_the_restatement_bit_for_bit(harness, tmp_path, delta):
    """The offset, the metric and sigma_w_eff are equal to the bit everywhere.  The target too, except where the float32
    quotient (s_1 - b') / (2 delta) is a half-integer: both sides round it to even, so those are equal as well - no
    exception is made."""
    Sc, bit, u = _grid(delta)
    target, eff, m_s, off = _run_harness(harness, tmp_path, Sc, bit, u, delta)
    assert np.array_equal(off.view(np.uint32), dr.offset(u, delta).view(np.uint32))
    assert np.array_equal(m_s.view(np.uint32), dr.metric(Sc[:, 0], u, delta).view(np.uint32))
    want = dr.target(Sc, bit, u, delta)
    bad = np.flatnonzero(target.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (delta, bad[:5], Sc[bad[:5], :2], bit[bad[:5]], u[bad[:5]], target[bad[:5]], want[bad[:5]])
    assert np.array_equal(eff.view(np.uint32), dr.sigma_w_eff(Sc, bit, u, delta)[:, 0].view(np.uint32))
    # wherever it went: on the bit's own shifted lattice (to float32 rounding of q - d), above s_2 + delta
    m_q = dr.metric(target - pr.BIAS, u, delta)
    assert np.all(np.abs(m_q - np.where(bit != 0, -1.0, 1.0)) < 4 * 4096 * 2.0 ** -23 / (2 * delta) + 1e-6)
    assert np.all(target - pr.BIAS >= Sc[:, 1] + F(delta))


def test_host_build_on_the_hosts_with_the_products_table(harness, tmp_path):
    for name, Y in pr.all_hosts():
        Sc = pr.cover_sigma(name).reshape(-1, 8)
        u = P.dither_table(Y.shape[0] // 8, Y.shape[1] // 8, _key())
        bit = pr.seeded_bits(Sc.shape[0], 0)
        target, eff, m_s, off = _run_harness(harness, tmp_path, Sc, bit, u, 16.0)
        assert np.array_equal(target.view(np.uint32), dr.target(Sc, bit, u, 16.0).view(np.uint32)), name
        assert np.array_equal(m_s.view(np.uint32), dr.metric(Sc[:, 0], u, 16.0).view(np.uint32)), name


# ---- preconditions, on the restatement alone ------------------------------------------------------------------------
def test_preconditions_with_the_products_table():
    """With payload.dither_table under the tests' key, delta = 16: every tile of the three seeded hosts decodes right with
    margin >= 0.4 for both bit values, and the keyed mean |m| exceeds that of a dither-free read of the same stego by at
    least 0.2 on each host.  Measured: worst margins +0.50..+0.59, keyed mean |m| 0.78..0.80, keyless 0.45..0.50 (gap 0.29..0.34)."""
    key = _key()
    for H, W, seed in pr.HOSTS:
        Y = pr.host(H, W, seed)
        nt = (H // 8, W // 8)
        u = P.dither_table(nt[0], nt[1], key)
        for b in (0, 1):
            r = dr.margins_of(Y, np.full(nt, b, np.uint8), u, 16.0)
            keyed, keyless = float(np.abs(r["m"]).mean()), float(np.abs(r["keyless"]).mean())
            print(f"{H}x{W} seed {seed} bit {b}: worst margin {float(r['signed'].min()):+.3f}, mean |m| keyed {keyed:.3f}, "
                  f"dither-free read {keyless:.3f}, PSNR {pr.o.psnr(Y, r['stego']):.2f} dB")
            assert r["signed"].min() >= 0.4, (H, W, seed, b, float(r["signed"].min()))
            assert keyed - keyless >= 0.2, (H, W, seed, b, keyed, keyless)


_GPU_CASES = [(n, d) for n in ("72x100s1", "64x64s3", "edge", "pinned", "planes0", "planes1", "planes2") for d in (16.0, 24.0, 200.0)]


@pytest.mark.parametrize("name,delta", _GPU_CASES)
def test_left_out_tiles_of_the_gpu_cases_stay_within_the_cap(name, delta):
    """For every (host, delta, n_bits) the GPU tests use: tiles without a unique restatement or a clear vote (a rounding
    tie, s_1 = s_2, |m| within the slope bar of 0) are at most 10 % of a seeded host and at most half of the edge or pinned
    host."""
    for n_bits in (0, 16):
        r = dr.margins(name, delta, 0, n_bits)
        n = r["signed"].size
        out = n - int(r["comparable"].sum())
        print(f"{name} delta {delta:g} n_bits {n_bits or n}: left out {out} of {n} (tie {int(r['tie'].sum())}, degenerate "
              f"{int(r['deg'].sum())}), wrong-voting tiles {int((r['signed'] < 0).sum())}, worst margin {float(r['signed'].min()):+.3f}")
        assert out <= pr.left_out_cap(name) * n, (name, delta, n_bits, out, n)
        if name not in ("edge", "pinned"):
            assert not (r["signed"][r["comparable"]] < 0).any()


def test_flat_tiles_have_the_margin_the_design_states():
    """A constant tile stays constant, sigma_1 = 8 x an integer: under dither its margin is only >= 1 - 8 / delta"""
    Y = pr.edge_host()
    for delta in (16.0, 24.0):
        worst = 1.0
        for seed in range(4):
            for b in (0, 1):
                r = dr.margins_of(Y, np.full(16, b, np.uint8), dr.seeded_words(16, seed), delta)
                flat = np.zeros(16, bool); flat[:10] = True; flat[15] = True
                worst = min(worst, float(r["signed"].ravel()[flat].min()))
        print(f"delta {delta:g}: worst flat-tile margin {worst:+.3f}, bound {1 - 8 / delta:+.3f}")
        assert worst >= 1 - 8 / delta - pr.slope_bar(delta)


def test_document_host_under_dither():
    """DESIGN 14's limit re-measured with the product's table: white page with strokes, 128 x 256, delta = 16, n_bits =
    n_tiles under the keyed map of ("pw", DOCUMENT_NONCE).  Dither-free: mean |m| 0.89, 42 wrong-voting tiles, 46 below 0.4;
    dithered: mean |m| 0.71, 39 wrong-voting tiles, 62 below 0.4 (DESIGN.md quotes these).  Both have wrong bits - the self-check is what protects the caller."""
    Y = pr.document_host(*pr.DOCUMENT, pr.DOCUMENT_SEED)
    key = hg.derive_key("pw", pr.DOCUMENT_NONCE)
    bits = P.payload_frame(pr.DOCUMENT_PAYLOADS[2])
    tbi, order, offs = P.payload_map(16, 32, key, bits.size)
    free = pr.margins_of(Y, bits[tbi], 16.0)
    u = P.dither_table(16, 32, key)
    dith = dr.margins_of(Y, bits[tbi], u, 16.0)
    for nm, r in (("dither-free", free), ("dithered", dith)):
        print(f"{nm}: mean |m| {float(np.abs(r['m']).mean()):.3f}, wrong-voting tiles {int((r['signed'] < 0).sum())} of 512, "
              f"below 0.4: {int((r['signed'] < 0.4).sum())}")
    assert (free["signed"] < 0).sum() >= 1 and (dith["signed"] < 0).sum() >= 1
    soft = pr.soft_ref(dith["m"].reshape(1, -1), order, offs)
    assert ((soft < 0) != (bits != 0)).sum() >= 1


# ---- the product's table ----------------------------------------------------------------------------------------------
def test_dither_table_is_keyed_deterministic_and_uniform():
    key = _key()
    t = P.dither_table(64, 64, key)
    assert t.dtype == np.uint16 and t.shape == (4096,)
    assert np.array_equal(t, P.dither_table(64, 64, key)) and np.array_equal(t, P.dither_table(64, 64, key, 0))
    assert not np.array_equal(t, P.dither_table(64, 64, key, 1))
    assert not np.array_equal(t, P.dither_table(64, 64, hg.derive_key("pw2", dr.NONCE)))
    assert not np.array_equal(P.dither_table(64, 64, key, 1), P.dither_table(64, 64, key, 1 << 32))
    assert np.array_equal(P.dither_tables(64, 64, key, [0, 3])[1], P.dither_table(64, 64, key, 3))
    assert P.dither_tables(2, 3, key, []).shape == (0, 6)
    # the statement of the table, without the product: PCG64 seeded with the first 8 bytes (big endian) of the digest
    import hashlib
    seed = int.from_bytes(hashlib.sha256(key + b"payload-dither" + (3).to_bytes(8, "little")).digest()[:8], "big")
    assert np.array_equal(P.dither_table(9, 12, key, 3), np.random.default_rng(seed).integers(0, 65536, 108, dtype=np.uint16))
    # 4 096 draws in 16 bins of the top 4 bits: chi^2 with 15 degrees of freedom, 99.99 % point 44.3
    counts = np.bincount(t >> 12, minlength=16)
    chi2 = float(((counts - 256.0) ** 2 / 256.0).sum())
    print(f"chi^2 {chi2:.1f}")
    assert chi2 < 44.3
    counts = np.bincount(t & 15, minlength=16)
    assert float(((counts - 256.0) ** 2 / 256.0).sum()) < 44.3
    with pytest.raises(ValueError):
        P.dither_table(2, 2, key, -1)


# ---- meta -------------------------------------------------------------------------------------------------------------
def _sealed(H, W, n_bits=104, video=None, key=bytes(32), dither=1):
    members = M.payload_members("text", H, W, 16.0, n_bits, bytes(range(8)), *(video or (None, None)), dither=dither)
    return M.sealed(members, 8, hg.hmac_digest(key, M.hmac_parts(members)))


def test_meta_member_round_trip_hmac_and_sizes(tmp_path):
    key = bytes(32)
    img, vid = _sealed(72, 100), _sealed(64, 96, 80, video=(2, 5))
    assert list(img) == ["mode", "payload_type", "shape", "delta", "dither", "payload_bits", "nonce", "tile", "digest"]
    assert list(vid)[-3:] == ["frame_interval", "n_frames", "digest"] and "dither" in vid
    assert img["dither"].dtype == np.uint8 and int(img["dither"]) == 1 and M.payload_dither_of(img) == 1
    assert M.authentic(img, key) and M.authentic(vid, key)
    # flipped or dropped, the member is a wrong password
    assert not M.authentic(dict(img, dither=np.uint8(0)), key)
    assert not M.authentic({k: v for k, v in img.items() if k != "dither"}, key)
    plain = _sealed(72, 100, dither=0)
    assert "dither" not in plain and M.payload_dither_of(plain) == 0
    assert not M.authentic(dict(plain, dither=np.uint8(1)), key)
    with pytest.raises(ValueError, match="dither"):
        M.payload_dither_of(dict(img, dither=np.uint8(2)))
    sizes = {}
    for name, meta in (("img_small", img), ("img_4k", _sealed(2160, 3840, 129600)), ("vid_3", _sealed(64, 96, 80, video=(2, 3))),
                       ("vid_3000", _sealed(64, 96, 80, video=(2, 3000))), ("plain_img", plain),
                       ("plain_vid", _sealed(64, 96, 80, video=(2, 3), dither=0))):
        path = M.save_payload_meta(str(tmp_path / name), meta)
        back = M.load_payload_meta(path)
        assert list(back) == list(meta) and M.authentic(back, key), name
        assert M.payload_dither_of(back) == (0 if name.startswith("plain") else 1)
        for k in meta:
            assert np.array_equal(np.asarray(back[k]), np.asarray(meta[k])), k
        sizes[name] = os.path.getsize(path)
    print(sizes)
    assert sizes["plain_img"] == 512 and sizes["plain_vid"] == 584           # files written before keep their size
    assert sizes["img_small"] == sizes["img_4k"] and sizes["vid_3"] == sizes["vid_3000"]
    assert (sizes["img_small"], sizes["vid_3"]) == (577, 585)


def test_existing_readers_refuse_a_dithered_payload_meta():
    import dct_svd_core_secure as core
    meta = _sealed(72, 100)
    st = np.zeros((72, 100, 3), np.uint8)
    with pytest.raises(ValueError, match="payload"):
        core.extract_arrays(st, meta, "pw")
    with pytest.raises(ValueError, match="payload"):
        core.detect_arrays(st, M.pack_payload(meta))
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        core.extract_payload_arrays(st, meta, "not the password")


# ---- host-side validation ---------------------------------------------------------------------------------------------
class _NoCallContext:
    def __new__(cls, hostapi):
        ctx = object.__new__(hostapi.Context)
        ctx._h = None

        def _call(name, *args):
            raise AssertionError(f"{name} reached the C ABI with unvalidated arguments")
        ctx._call = _call
        return ctx


def test_context_methods_validate_the_table_before_the_c_abi(hostapi):
    ctx = _NoCallContext(hostapi)
    st = np.zeros((3, 72, 100), np.uint8)
    tb = np.zeros(108, np.uint8)
    _, order, offs = pr.simple_map(108, 16)
    for bad in (np.zeros(108, np.int32), np.zeros(107, np.uint16), np.zeros((2, 108), np.uint16), np.zeros((3, 109), np.uint16)):
        for call in (lambda: ctx.payload_sigma_w(st, tb, 16.0, dither=bad), lambda: ctx.embed_tiles_payload(st, tb, 16.0, dither=bad),
                     lambda: ctx.payload_metric(st, 16.0, dither=bad), lambda: ctx.payload_soft(st, order, offs, 16, 16.0, dither=bad)):
            with pytest.raises(ValueError, match="dither"):
                call()
    with pytest.raises(ValueError, match="delta"):
        ctx.payload_metric(st, 4.0, dither=np.zeros(108, np.uint16))
