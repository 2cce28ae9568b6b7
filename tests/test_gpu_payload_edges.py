"""Blind payload on the device, away from the defaults: the embed and the decode at delta = 8, 12, 24, 200 and 512 (rows of up
to 3 delta at alpha = 1: the unclipped plane leaves 0..255 on both sides), tiles pinned by clipping, black tiles in a
batch (plane > 0, strided, in place, with yw on a ragged width), the reduce with 0 to 300 tiles on a bit, and a document
page through the drop-in.  Every reference is the float64 / NumPy restatement of tests/payload_refs.py; what the comparisons
may assume of it (ties, s_1 = s_2, the share of tiles with a clear vote) is asserted on the CPU in tests/test_payload.py for
exactly the hosts, deltas and bit seeds used here.

A tile takes part in a vote comparison when it is "comparable": no rounding tie, s_1 != s_2, and the restatement's |m| above
the slope bar 2 (1e-4 2040) / delta.  Tie tiles are compared with the restatement evaluated on the device's own cover
singular values, s_1 = s_2 tiles in their two leading singular values (tests/test_gpu_payload.py's routes).
"""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import payload_refs as pr
from conftest import PKG_NAME
from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

SIGMA_RTOL = pr.SIGMA_RTOL
P = importlib.import_module(PKG_NAME + ".payload")
hg = importlib.import_module(PKG_NAME + ".hostglue")


def _vp(a, off=0):
    return C.c_void_p(a.ctypes.data + off)


def _restatement_stego(Y, r, sc_dev, delta):
    """(stego, Yw) of the restatement of margins dict r, a tie tile's target taken from the device's own cover singular values"""
    if not r["tie"].any():
        return r["stego"], r["Yw"]
    tie, So = r["tie"], r["Sc"]
    eff = pr.sigma_w_eff(So, r["tile_bits"], delta)
    eff[tie, 0] = pr.target(sc_dev, r["tile_bits"], delta)[tie] - So[tie, 0]
    ref = o.embed_plane(Y.astype(np.float32), None, 1.0, kfrac=0.0, tile=8, k_floor=1, wm_svd=(None, eff, None))
    return ref["stego"], ref["Yw"]


def _sigma12(tiles):
    """the two leading singular values of [n, 8, 8] tiles in float64 (those of their DCT: the transform is orthonormal)"""
    return np.linalg.svd(tiles.astype(np.float64), compute_uv=False)[:, :2]


def _check_degenerate(st, yw, ref_st, ref_yw):
    """s_1 = s_2 tiles ([n, 8, 8] each): u_1 is any unit vector of a plane, so the pixels are not unique.  What holds whatever
    the choice:
      * the unclipped tile carries (target, s_2): its two leading singular values are the restatement's to the sigma bar
        (1e-4 s_1, plus 1e-3 absolute as for sigma_c);
      * where neither unclipped tile leaves 0..255, the stegos' two leading singular values agree to the existing bar, the
        sigma bar plus 1 LSB per pixel (8 in sigma).
    Once a tile clips, the stego's singular values depend on the choice itself: on the restatement alone, turning (u_1, v_1)
    through the plane moves the stego's s_1 of the {0, 40} checkerboard at delta = 512 (target 1028) between 592 and 1026, and
    that of the 0 / 255 checkerboard at delta = 16 (target 1060) between 1020 and 1038 - no implementation meets a fixed bar
    there (the device: 516 and 12 away from NumPy's choice), so a clipped tile is held to the first property and to
    stego = clip(yw) alone.  Returns (worst stego difference on unclipped tiles, worst yw difference / s_1, unclipped count)."""
    s_yw, s_ref_yw = _sigma12(yw), _sigma12(ref_yw)
    rel = np.abs(s_yw - s_ref_yw) / np.maximum(s_ref_yw[:, :1], 1.0)
    assert np.all(np.abs(s_yw - s_ref_yw) <= SIGMA_RTOL * s_ref_yw[:, :1] + 1e-3), (s_yw.tolist(), s_ref_yw.tolist())
    inside = (yw.min((-1, -2)) >= 0) & (yw.max((-1, -2)) <= 255) & (ref_yw.min((-1, -2)) >= 0) & (ref_yw.max((-1, -2)) <= 255)
    worst = 0.0
    if inside.any():
        s_dev, s_ref = _sigma12(st[inside]), _sigma12(ref_st[inside])
        worst = float(np.abs(s_dev - s_ref).max())
        assert worst <= 8.0 + SIGMA_RTOL * float(s_ref[:, 0].max())
    return worst, float(rel.max()), int(inside.sum())


def _tile_max(d):
    return o.to_tiles(d).max((-1, -2))


# ---- 1. embed then decode off the default delta ---------------------------------------------------------------------
_CASES = [(n, d) for n, _ in pr.edge_hosts() for d in (8.0, 12.0, 24.0, 200.0, 512.0)] + [("pinned", 16.0)]


@pytest.mark.parametrize("name,delta", _CASES, ids=[f"{n}-d{d:g}" for n, d in _CASES])
def test_embed_then_decode_off_default_delta(gpu_ctx, name, delta):
    Y = dict(pr.edge_hosts())[name]
    H, W = Y.shape
    Hb, Wb = H // 8 * 8, W // 8 * 8
    nt = (H // 8) * (W // 8)
    for seed in pr.EDGE_BIT_SEEDS:
        r = pr.margins(name, delta, seed)
        _, tile_bit, _, _ = pr.edge_tile_bits(nt, seed)
        tile_bits = r["tile_bits"]
        assert np.array_equal(tile_bits.ravel(), tile_bit)
        st, sc, yw = gpu_ctx.embed_tiles_payload(Y, tile_bit, delta, want_yw=True)
        gpu_ctx.check_status()
        assert np.isfinite(yw).all() and np.isfinite(sc).all()
        assert np.array_equal(st, np.clip(yw, 0, 255).astype(np.uint8))
        # the saturation is exercised: where the restatement's unclipped plane leaves 0..255 by half a gray level on a tile
        # with a unique restatement, so does the device's (the pinned host does above at every delta and below from 16 on:
        # asserted on the CPU)
        sure = np.kron(~r["tie"] & ~r["deg"], np.ones((8, 8), bool))
        Yw_ref = r["Yw"][:Hb, :Wb][sure]
        if Yw_ref.min() < -0.5:
            assert yw.min() < 0
        if Yw_ref.max() > 255.5:
            assert yw.max() > 255
        if name == "pinned":
            assert yw.max() > 255 and (delta < 16 or yw.min() < 0)
        # outside the tile grid: passed through
        assert np.array_equal(st[:, Wb:], Y[:, Wb:]) and np.array_equal(st[Hb:], Y[Hb:])
        # the stego against the restatement's
        So, tie, deg, comp = r["Sc"], r["tie"], pr.degenerate_tiles(r["Sc"]), r["comparable"]
        assert np.all(np.abs(sc - So) <= SIGMA_RTOL * So[..., :1] + 1e-3)
        ref_st, ref_yw = _restatement_stego(Y, r, gpu_ctx.sigma_tiles(Y), delta)
        d = np.abs(st.astype(int) - ref_st.astype(int))
        dt = _tile_max(d)
        # s_1 = s_2 tiles (see _check_degenerate)
        worst_deg = worst_deg_yw = 0.0
        if deg.any():
            worst_deg, worst_deg_yw, _ = _check_degenerate(o.to_tiles(st)[deg], o.to_tiles(yw[:Hb, :Wb])[deg],
                                                           o.to_tiles(ref_st)[deg], o.to_tiles(ref_yw[:Hb, :Wb])[deg])
        # the decode
        m_dev = gpu_ctx.payload_metric(st, delta)
        gpu_ctx.check_status()
        m_own = pr.metric_ref(st, delta)
        signed = np.where(tile_bits != 0, -m_dev, m_dev)
        flips = comp & ((signed < 0) != (r["signed"] < 0))
        print(f"{name} delta {delta:g} bits {seed}: yw in [{float(yw.min()):.1f}, {float(yw.max()):.1f}]; left out of the vote comparison "
              f"{int((~comp).sum())} of {nt} (tie {int(tie.sum())}, s_1 = s_2 {int(r['deg'].sum())}; cap {pr.left_out_cap(name):.0%}); "
              f"max LSB on the other tiles {int(dt[~deg].max())}, share of pixels differing {float((d != 0).mean()):.2e}; "
              f"s_1 = s_2 tiles: worst |sigma - ref| {worst_deg:.2f} in the unclipped stegos, {worst_deg_yw:.2e} s_1 in yw; worst |m - m(own bytes)| {float(np.abs(m_dev - m_own).max()):.2e} "
              f"(bar {pr.slope_bar(delta):.2e}); wrong-voting comparable tiles {int((comp & (signed < 0)).sum())} "
              f"(restatement {int((comp & (r['signed'] < 0)).sum())}), sign flips {int(flips.sum())}")
        assert (~comp).sum() <= pr.left_out_cap(name) * nt
        assert dt[~deg].max() <= 1, np.argwhere(~deg & (dt > 1)).tolist()
        assert np.all(np.abs(m_dev - m_own) <= pr.slope_bar(delta)), np.argwhere(np.abs(m_dev - m_own) > pr.slope_bar(delta)).tolist()
        # the device is wrong exactly where the rule is wrong, and nowhere else
        assert not flips.any(), (np.argwhere(flips).tolist(), signed[flips].tolist(), r["signed"][flips].tolist())


# ---- 2. black tiles in a batch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [16.0, 12.0])
def test_black_tiles_in_a_batch(gpu_ctx, delta):
    planes = pr.letterbox_planes()
    n, H, W = planes.shape
    nby, nbx = H // 8, W // 8
    nt = nby * nbx
    seed = pr.EDGE_BIT_SEEDS[0]
    _, tile_bit, _, _ = pr.edge_tile_bits(nt, seed)
    tile_bits = tile_bit.reshape(nby, nbx)
    st3, sc3, yw3 = gpu_ctx.embed_tiles_payload(planes, tile_bit, delta, want_yw=True)
    gpu_ctx.check_status()
    assert np.isfinite(yw3).all()
    # each plane of the batch is its single-plane dense call, yw outside the grid included
    for p in range(n):
        st1, sc1, yw1 = gpu_ctx.embed_tiles_payload(planes[p], tile_bit, delta, want_yw=True)
        assert np.array_equal(st3[p], st1), p
        assert np.array_equal(sc3[p], sc1), p
        assert np.array_equal(yw3[p].view(np.uint32), yw1.view(np.uint32)), p
        assert np.array_equal(yw1[:, nbx * 8:], planes[p][:, nbx * 8:].astype(np.float32))
    # black tiles: the restatement's constant
    want_v = (pr.target(np.zeros((nby, nbx, 8), np.float32), tile_bits, delta) * np.float32(0.125)).astype(np.float32)
    m3 = gpu_ctx.payload_metric(st3, delta)
    n_black = 0
    for p in range(n):
        r = pr.margins(f"letterbox{p}", delta, seed)
        black = pr.black_tiles(planes[p])
        assert black.any() == (p > 0)
        n_black += int(black.sum())
        T, Tw = o.to_tiles(st3[p]), o.to_tiles(yw3[p])
        assert np.array_equal(T[black], np.broadcast_to(np.trunc(want_v[black]).astype(np.uint8)[:, None, None], T[black].shape)), p
        assert np.all(np.abs(Tw[black] - want_v[black][:, None, None]) <= np.spacing(want_v[black])[:, None, None]), p
        # and so says the oracle's own embed (where (q + 4) / 8 is not a whole number: its float32 inverse DCT may land an
        # ulp under one, and truncate to the level below)
        frac = black & (want_v != np.trunc(want_v))
        assert np.array_equal(o.to_tiles(r["stego"])[frac], T[frac])
        # every black tile decodes its bit
        assert np.array_equal(m3[p][black] < 0, tile_bits[black] != 0) and np.all(m3[p][black] != 0), p
        # the other tiles: within 1 LSB of the restatement's where it is unique, and the vote of every comparable tile
        ok = ~r["tie"] & ~r["deg"]
        dt = _tile_max(np.abs(st3[p].astype(int) - r["stego"].astype(int)))
        assert dt[ok].max() <= 1, (p, np.argwhere(ok & (dt > 1)).tolist())
        signed = np.where(tile_bits != 0, -m3[p], m3[p])
        assert not (r["comparable"] & ((signed < 0) != (r["signed"] < 0))).any(), p
        assert (~r["comparable"]).sum() <= pr.left_out_cap("letterbox") * nt
    print(f"delta {delta:g}: {n_black} black tiles in planes 1 and 2, constants {sorted(set(np.trunc(want_v).astype(int).ravel().tolist()))}")
    # a strided, unaligned view with sentinel bytes around it: the byte-wise paths, the host-pointer form
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, (n, H + 5, W + 12), dtype=np.uint8)
    big[:, 3:3 + H, 5:5 + W] = planes
    rs, ps, off = W + 12, (H + 5) * (W + 12), 3 * (W + 12) + 5
    inside = np.zeros(big.shape, bool); inside[:, 3:3 + H, 5:5 + W] = True
    out_big = np.full_like(big, 7)
    sc = np.empty((n, nby, nbx, 8), np.float32)
    yw = np.zeros((n, H, W), np.float32)
    gpu_ctx._call("wm_embed_tiles_payload_u8", _vp(big, off), _vp(tile_bit), _vp(out_big, off), _vp(sc), _vp(yw), n, H, W, rs, ps, delta)
    assert np.all(out_big[~inside] == 7)
    assert np.array_equal(out_big[:, 3:3 + H, 5:5 + W], st3) and np.array_equal(sc, sc3)
    assert np.array_equal(yw.view(np.uint32), yw3.view(np.uint32))
    # in place on the device, dense and through the same strided layout (stego aliases host, no yw)
    for src, args, sl in ((planes, (n, H, W, W, H * W), None), (big, (n, H, W, rs, ps), off)):
        src = np.ascontiguousarray(src)
        d_host = gpu_ctx.malloc(src.nbytes); d_bit = gpu_ctx.malloc(nt); d_sc = gpu_ctx.malloc(n * nt * 8 * 4)
        try:
            gpu_ctx.h2d(d_host, src); gpu_ctx.h2d(d_bit, tile_bit)
            gpu_ctx._call("wm_embed_tiles_payload_u8_dev", d_host + (sl or 0), d_bit, d_host + (sl or 0), d_sc, None, *args, delta)
            gpu_ctx.check_status()
            got = np.empty_like(src); gpu_ctx.d2h(got, d_host); gpu_ctx.sync()
        finally:
            for d in (d_host, d_bit, d_sc):
                gpu_ctx.free(d)
        if sl is None:
            assert np.array_equal(got, st3)
        else:
            assert np.array_equal(got[~inside], big[~inside])                 # the bytes around the view
            assert np.array_equal(got[:, 3:3 + H, 5:5 + W], st3)


# ---- 3. the reduce's trip counts -----------------------------------------------------------------------------------
_RH, _RW = 184, 352                                                         # 23 x 44 = 1012 tiles
_COUNTS = (1, 63, 0, 64, 65, 256, 257, 300, 6)                              # tiles per bit; 6 = the remainder


@pytest.mark.parametrize("n_planes", [1, 5])
def test_reduce_trip_counts(gpu_ctx, n_planes):
    """One wave per bit, a lane's loop strides by 64 under an unroll of 4: 0, 1, 63, 64, 65 (a second trip), 256, 257 (a second
    trip of the unrolled body) and 300 tiles on a bit, in a seeded order that is not ascending."""
    delta = pr.DELTA
    nt = (_RH // 8) * (_RW // 8)
    assert nt == 1012 and sum(_COUNTS) == nt
    rng = np.random.default_rng(23)
    base = rng.integers(0, 256, (_RH, _RW), dtype=np.uint8)
    planes = np.ascontiguousarray(np.stack([np.roll(base, 8 * p, axis=1) for p in range(n_planes)]))
    order = rng.permutation(nt).astype(np.int32)
    offs = np.concatenate([[0], np.cumsum(_COUNTS)]).astype(np.int32)
    n_bits = len(_COUNTS)
    m = gpu_ctx.payload_metric(planes, delta).reshape(n_planes, nt)
    m_ref = pr.metric_ref(base, delta)
    for p in range(n_planes):                                               # (a roll by whole tiles permutes the tiles)
        assert np.all(np.abs(m[p] - np.roll(m_ref, p, axis=1).ravel()) <= pr.slope_bar(delta)), p

    def check(order, offs, n_bits):
        soft = gpu_ctx.payload_soft(planes, order, offs, n_bits, delta)
        assert soft.shape == (n_bits,) and soft.dtype == np.float64
        ref = pr.soft_ref(m, order, offs)
        exact = np.array([math.fsum(float(x) for p in range(n_planes) for x in m[p, order[offs[j]:offs[j + 1]]]) for j in range(n_bits)])
        assert np.abs(soft - ref).max() < 1e-9 and np.abs(soft - exact).max() < 1e-9, (np.abs(soft - ref).max(), np.abs(soft - exact).max())
        again = gpu_ctx.payload_soft(planes, order, offs, n_bits, delta)
        assert np.array_equal(soft.view(np.uint64), again.view(np.uint64))
        soft_h = np.full(n_bits, 7.0)
        gpu_ctx._call("wm_payload_soft_tiles_u8", _vp(planes), _vp(order), _vp(offs), n_bits, _vp(soft_h), n_planes, _RH, _RW, _RW,
                      _RH * _RW, delta)
        assert np.array_equal(soft_h.view(np.uint64), soft.view(np.uint64))
        return soft

    soft = check(order, offs, n_bits)
    empty = _COUNTS.index(0)
    assert soft[empty] == 0.0 and not np.signbit(soft[empty])
    assert np.abs(soft[np.array(_COUNTS) >= 64]).min() > 0                  # (noise: no sum of 64+ terms is exactly 0)
    assert math.isfinite(P.confidence(soft, offs, n_planes)) and 0.0 <= P.confidence(soft, offs, n_planes) <= 1.0
    one = check(order, np.array([0, nt], np.int32), 1)                      # all 1012 tiles on one bit
    assert abs(one[0] - math.fsum(float(x) for x in m.ravel())) < 1e-9
    check(order, np.arange(nt + 1, dtype=np.int32), nt)                     # one tile per bit
    gpu_ctx.check_status()


# ---- 4. a document through the drop-in ------------------------------------------------------------------------------
def _document():
    Y = pr.document_host(*pr.DOCUMENT, pr.DOCUMENT_SEED)
    return Y, np.ascontiguousarray(np.stack([Y] * 3, axis=-1))             # gray BGR: Y of BGR2YCrCb is the plane itself


def _votes(Y, data):
    key = hg.derive_key("pw", pr.DOCUMENT_NONCE)
    bits = P.payload_frame(data)
    tbi, order, offs = P.payload_map(Y.shape[0] // 8, Y.shape[1] // 8, key, bits.size)
    return bits, tbi, pr.document_votes(Y, bits, tbi, order, offs)


def test_document_through_the_dropin(gpu_ctx, tmp_path):
    import dct_svd_core_secure as core
    Y, cover = _document()
    assert np.array_equal(o.bgr_to_ycrcb(cover)[..., 0], Y)
    short, nine, full = pr.DOCUMENT_PAYLOADS
    # payloads the stego does not carry are refused: 9 bytes (136 bits, 3.8 tiles a bit) and n_bits = n_tiles
    for data in (nine, full):
        bits, _, v = _votes(Y, data)
        lo, hi = int((v["wrong"] & v["sure"]).sum()), int((v["wrong"] | ~v["sure"]).sum())
        assert lo >= 1
        with pytest.raises(ValueError, match=r"^payload does not decode from its own stego: \d+ of %d bits wrong" % bits.size) as e:
            core.embed_payload_arrays(cover, data, "pw", pr.DOCUMENT_NONCE, payload_type="bytes")
        k = int(re.search(r": (\d+) of", str(e.value)).group(1))
        print(f"{len(data)} bytes: the embed reports {k} of {bits.size} bits wrong; the restatement {int(v['wrong'].sum())} ({lo} surely)")
        assert lo <= k <= hi
        assert "shorter payload" in str(e.value) and "larger delta" in str(e.value) and "larger cover" in str(e.value)
    # the file level writes neither the stego nor the meta
    cp, sp, mp = str(tmp_path / "cover.png"), str(tmp_path / "stego.png"), str(tmp_path / "meta.npz")
    assert hg.write_png(cp, cover)
    with pytest.raises(ValueError, match="^payload does not decode"):
        core.embed_payload(cp, full, sp, mp, password="pw", payload_type="bytes", nonce=pr.DOCUMENT_NONCE)
    assert not os.path.exists(sp) and not os.path.exists(mp)
    # a 2-byte payload (80 bits, 6.4 tiles a bit) embeds and extracts
    bits, tbi, v = _votes(Y, short)
    assert not v["wrong"].any() and v["sure"].all()
    core.embed_payload(cp, short, sp, mp, password="pw", payload_type="bytes", nonce=pr.DOCUMENT_NONCE)
    data, valid, conf, _ = core.extract_payload(sp, mp, password="pw")
    assert data == short and valid is True
    print(f"2 bytes: confidence {conf:.3f}; the restatement's worst |soft| / count {float(np.min(np.abs(v['soft']) / v['count'])):.3f}")
    # verify=False keeps the earlier behaviour: a stego, a sealed meta, and an extract that answers valid = False
    bits, tbi, v = _votes(Y, full)
    r = core.embed_payload_arrays(cover, full, "pw", pr.DOCUMENT_NONCE, payload_type="bytes", verify=False)
    assert core.extract_payload_arrays(r["stego"], r["meta"], "pw")[1] is False
    # array level: the stego against the restatement's, and the tiles that vote wrong
    Ys = np.ascontiguousarray(o.bgr_to_ycrcb(r["stego"])[..., 0])
    ok, comp = ~v["tie"] & ~v["deg"], v["comparable"]
    dt = _tile_max(np.abs(Ys.astype(int) - v["stego"].astype(int)))
    assert dt[ok].max() <= 1, np.argwhere(ok & (dt > 1)).tolist()
    m_dev = gpu_ctx.payload_metric(Ys, pr.DELTA)
    signed = np.where(v["tile_bits"] != 0, -m_dev, m_dev)
    print(f"n_bits = n_tiles: {int((comp & (signed < 0)).sum())} comparable tiles vote wrong on the device, "
          f"{int((comp & (v['signed'] < 0)).sum())} on the restatement; {int((~comp).sum())} of 512 left out")
    assert np.array_equal(comp & (signed < 0), comp & (v["signed"] < 0))
    assert (comp & (signed < 0)).sum() == (comp & (v["signed"] < 0)).sum() >= 1


def test_document_video_is_refused(gpu_ctx, tmp_path):
    """every frame of a still carries the same pinned tiles: repetition over frames does not cover them either"""
    v = importlib.import_module(PKG_NAME + ".video")
    Y, _ = _document()
    full, short = pr.DOCUMENT_PAYLOADS[2], pr.DOCUMENT_PAYLOADS[0]
    src, outp, metap = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "vm.npz")
    v.write_y4m(src, np.stack([Y] * 3))
    with pytest.raises(ValueError, match=r"^payload does not decode from its own stego: \d+ of 512 bits wrong"):
        v.embed_payload_video(src, full, outp, metap, password="pw", payload_type="bytes", nonce=pr.DOCUMENT_NONCE, batch=2)
    assert not os.path.exists(outp) and not os.path.exists(metap)
    v.embed_payload_video(src, full, outp, metap, password="pw", payload_type="bytes", nonce=pr.DOCUMENT_NONCE, batch=2, verify=False)
    assert os.path.exists(outp) and v.extract_payload_video(outp, metap, password="pw", batch=2)[1] is False
    v.embed_payload_video(src, short, outp, metap, password="pw", payload_type="bytes", nonce=pr.DOCUMENT_NONCE, batch=2)
    data, valid, _ = v.extract_payload_video(outp, metap, password="pw", batch=2)
    assert data == short and valid is True
