"""Blind payload with keyed dither on the device: sigma_w_eff, the stego, the metric and the soft decode against the NumPy
restatement (tests/payload_dither_refs.py) on the seeded hosts, batches with a shared and with per-plane tables, a row stride
that takes the byte-wise kernels, a table of zeros against the dither-free entry points, a keyless read, the C ABI's
refusals, and the drop-in and video round trips.  What the comparisons may assume of the restatement (ties, s_1 = s_2, the
share of tiles with a clear vote) is asserted on the CPU in tests/test_payload_dither.py for the hosts, deltas and bit counts
used here; the edge and pinned hosts are in tests/test_gpu_payload_dither_edges.py."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import payload_dither_refs as dr
import payload_refs as pr
from conftest import PKG_NAME
from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

WM_OK, WM_ERR_BADARG = 0, 1
M = importlib.import_module(PKG_NAME + ".meta")
P = importlib.import_module(PKG_NAME + ".payload")
hg = importlib.import_module(PKG_NAME + ".hostglue")


def _vp(a, off=0):
    return C.c_void_p(a.ctypes.data + off)


def _tile_max(d):
    return o.to_tiles(d).max((-1, -2))


def check_against_the_restatement(ctx, name, delta, n_bits, exact_votes):
    """One plane of a named host under dr.margins' bits and words: every check of the list, printed before it is asserted."""
    Y = dr.named_host(name)
    H, W = Y.shape
    Hb, Wb = H // 8 * 8, W // 8 * 8
    r = dr.margins(name, delta, 0, n_bits)
    nt = r["signed"].size
    tile_bit, u, order, offs = r["tile_bits"].ravel(), r["u"].ravel(), r["order"], r["offs"]
    nb = len(offs) - 1
    comp, tie = r["comparable"], r["tie"]
    assert (~comp).sum() <= pr.left_out_cap(name) * nt                       # (the CPU suite's precondition, restated)
    # sigma_w_eff
    eff = ctx.payload_sigma_w(Y, tile_bit, delta, dither=u)
    ctx.check_status()
    s1 = r["Sc"][..., 0]
    d_eff = np.abs(eff[..., 0] - r["eff"][..., 0])
    print(f"{name} delta {delta:g} n_bits {nb}: worst |sigma_w_eff - ref| / s_1 off ties {float((d_eff[~tie] / np.maximum(s1[~tie], 1e-30)).max()):.2e}")
    assert not eff[..., 1:].any()
    assert np.all(d_eff[~tie] <= pr.SIGMA_RTOL * s1[~tie]), np.argwhere(~tie & (d_eff > pr.SIGMA_RTOL * s1)).tolist()
    # the stego
    st, sc, yw = ctx.embed_tiles_payload(Y, tile_bit, delta, want_yw=True, dither=u)
    ctx.check_status()
    assert np.array_equal(st, np.clip(yw, 0, 255).astype(np.uint8))
    assert np.array_equal(st[:, Wb:], Y[:, Wb:]) and np.array_equal(st[Hb:], Y[Hb:])
    dt = _tile_max(np.abs(st.astype(int) - r["stego"].astype(int)))
    print(f"  max LSB on comparable tiles {int(dt[comp].max())}; left out {int((~comp).sum())} of {nt}")
    assert dt[comp].max() <= 1, np.argwhere(comp & (dt > 1)).tolist()
    # the metric, against the restatement on the same bytes
    m_dev = ctx.payload_metric(st, delta, dither=u)
    m_own = dr.metric_ref(st, u, delta)
    print(f"  worst |m - ref| {float(np.abs(m_dev - m_own).max()):.2e} (bar {pr.slope_bar(delta):.2e})")
    assert np.all(np.abs(m_dev - m_own) <= pr.slope_bar(delta))
    # the soft decode, twice
    soft = ctx.payload_soft(st, order, offs, nb, delta, dither=u)
    ref = pr.soft_ref(m_own.reshape(1, -1), order, offs)
    count = np.diff(offs)
    print(f"  worst |soft - ref| / count {float((np.abs(soft - ref) / count).max()):.2e}")
    assert np.all(np.abs(soft - ref) / count <= pr.slope_bar(delta))
    again = ctx.payload_soft(st, order, offs, nb, delta, dither=u)
    assert np.array_equal(soft.view(np.uint64), again.view(np.uint64))
    assert np.array_equal(ctx.payload_metric(st, delta, dither=u).view(np.uint32), m_dev.view(np.uint32))
    # the votes: the device is wrong exactly where the rule is wrong
    signed = np.where(r["tile_bits"] != 0, -m_dev, m_dev)
    flips = comp & ((signed < 0) != (r["signed"] < 0))
    print(f"  wrong-voting comparable tiles {int((comp & (signed < 0)).sum())} (restatement {int((comp & (r['signed'] < 0)).sum())})")
    assert not flips.any(), np.argwhere(flips).tolist()
    if exact_votes:
        assert not (comp & (signed < 0)).any()
        if nb < nt:                                                         # several tiles a bit: every bit decodes
            assert np.array_equal(soft < 0, r["bits"] != 0)
    # a keyless read of the dithered stego
    k_dev, k_ref = ctx.payload_metric(st, delta), pr.metric_ref(st, delta)
    print(f"  keyless mean |m| {float(np.abs(k_dev).mean()):.3f} (restatement {float(np.abs(k_ref).mean()):.3f}), keyed {float(np.abs(m_dev).mean()):.3f}")
    assert abs(float(np.abs(k_dev).mean()) - float(np.abs(k_ref).mean())) <= pr.slope_bar(delta)
    return st


@pytest.mark.parametrize("n_bits", [0, 16], ids=["n_tiles", "16"])
@pytest.mark.parametrize("delta", [16.0, 24.0, 200.0])
@pytest.mark.parametrize("name", ["72x100s1", "64x64s3"])
def test_one_plane_against_the_restatement(gpu_ctx, name, delta, n_bits):
    check_against_the_restatement(gpu_ctx, name, delta, n_bits, exact_votes=True)


@pytest.mark.parametrize("delta", [8.0, 16.0, 16.5, 24.0, 200.0, 512.0])
def test_device_rule_is_the_restatement_bit_for_bit_on_its_own_sigmas(gpu_ctx, delta):
    """The sigma pass of the payload kernels is K2's: fed the singular values the device itself reports (sigma_tiles), the
    NumPy restatement gives the device's sigma_w_eff to the bit - the offset is one multiply rounded on its own, the lattice
    point one fused multiply-add, for a delta with a long mantissa (16.5 and the words make b' one) as for 16 - and its metric
    to the bit or to the bound worked out below.  All three planes, per-plane words, the edge words among them."""
    planes, nt, tile_bit, _, _ = _planes_case()
    rows = np.stack([dr.seeded_words(nt, s) for s in (0, 1, 2)])
    rows[:, :5] = dr.U_EDGES
    Sc = gpu_ctx.sigma_tiles(planes)
    eff = gpu_ctx.payload_sigma_w(planes, tile_bit, delta, dither=rows)
    want = dr.sigma_w_eff(Sc, np.broadcast_to(tile_bit.reshape(9, 12), (3, 9, 12)), rows.reshape(3, 9, 12), delta)
    bad = np.argwhere(eff.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad[:5].tolist(), eff[tuple(bad[0])], want[tuple(bad[0])])
    st, _, _ = gpu_ctx.embed_tiles_payload(planes, tile_bit, delta, dither=rows)
    m = gpu_ctx.payload_metric(st, delta, dither=rows)
    want_m = dr.metric(gpu_ctx.sigma_tiles(st)[..., 0], rows.reshape(3, 9, 12), delta)
    # The metric: to the bit where 1 / (2 delta) is a power of two (the product x is exact).  Elsewhere the device compiler
    # contracts x - floor(x) into one fused multiply-add on the unrounded product - in the dither-free metric as well, which
    # is what keeps a table of zeros identical to the existing entry points - so f differs from the restatement's by at most
    # half an ulp of x < 64 (2^-19), m by 4 times that, plus a few ulps of m (4 x 2^-23) for the roundings of f and of
    # 2 f - 1 on either side.
    err = float(np.abs(m.astype(np.float64) - want_m.astype(np.float64)).max())
    print(f"delta {delta:g}: worst |m - restatement on the device's sigmas| {err:.2e}")
    if np.log2(2 * delta) % 1 == 0:
        assert np.array_equal(m.view(np.uint32), want_m.view(np.uint32))
    else:
        assert err <= 4 * 2.0 ** -19 + 4 * 2.0 ** -23
    # either way it is the dither-free metric's own arithmetic: the same planes read at s_1 - d = s_1
    z = np.zeros_like(rows)
    assert np.array_equal(gpu_ctx.payload_metric(st, delta, dither=z).view(np.uint32), gpu_ctx.payload_metric(st, delta).view(np.uint32))
    gpu_ctx.check_status()


def _planes_case():
    planes = pr.mr.planes_of(72, 100, 3)
    nt = 108
    _, tile_bit, order, offs = dr.case_bits(nt, 16, 0)
    return planes, nt, tile_bit, order, offs


def test_three_planes_with_a_shared_table(gpu_ctx):
    planes, nt, tile_bit, order, offs = _planes_case()
    delta = 16.0
    u = dr.seeded_words(nt, 0)
    st3, sc3, _ = gpu_ctx.embed_tiles_payload(planes, tile_bit, delta, dither=u)
    eff3 = gpu_ctx.payload_sigma_w(planes, tile_bit, delta, dither=u)
    m3 = gpu_ctx.payload_metric(st3, delta, dither=u)
    gpu_ctx.check_status()
    m_own = np.stack([dr.metric_ref(st3[p], u, delta) for p in range(3)])
    for p in range(3):
        r = dr.margins(f"planes{p}", delta, 0, 16)
        assert np.array_equal(r["tile_bits"].ravel(), tile_bit) and np.array_equal(r["u"].ravel(), u)
        comp, tie = r["comparable"], r["tie"]
        d_eff = np.abs(eff3[p][..., 0] - r["eff"][..., 0])
        assert np.all(d_eff[~tie] <= pr.SIGMA_RTOL * r["Sc"][..., 0][~tie]), p
        dt = _tile_max(np.abs(st3[p].astype(int) - r["stego"].astype(int)))
        assert dt[comp].max() <= 1, (p, np.argwhere(comp & (dt > 1)).tolist())
        assert np.all(np.abs(m3[p] - m_own[p]) <= pr.slope_bar(delta)), p
        # each plane of the batch is its single-plane call
        st1, sc1, _ = gpu_ctx.embed_tiles_payload(planes[p], tile_bit, delta, dither=u)
        assert np.array_equal(st3[p], st1) and np.array_equal(sc3[p], sc1), p
    soft = gpu_ctx.payload_soft(st3, order, offs, 16, delta, dither=u)
    ref = pr.soft_ref(m_own, order, offs)
    assert np.all(np.abs(soft - ref) / (3 * np.diff(offs)) <= pr.slope_bar(delta))
    assert np.array_equal(soft < 0, pr.seeded_bits(16, 0) != 0)
    assert np.array_equal(soft.view(np.uint64), gpu_ctx.payload_soft(st3, order, offs, 16, delta, dither=u).view(np.uint64))


def test_three_planes_with_per_plane_tables(gpu_ctx):
    planes, nt, tile_bit, order, offs = _planes_case()
    delta = 16.0
    rows = np.stack([dr.seeded_words(nt, s) for s in (0, 1, 2)])
    assert not np.array_equal(rows[0], rows[1])
    st3, sc3, yw3 = gpu_ctx.embed_tiles_payload(planes, tile_bit, delta, want_yw=True, dither=rows)
    eff3 = gpu_ctx.payload_sigma_w(planes, tile_bit, delta, dither=rows)
    m3 = gpu_ctx.payload_metric(st3, delta, dither=rows)
    gpu_ctx.check_status()
    soft_sum = np.zeros(16)
    for p in range(3):
        # a plane of the batch under its own row is the single-plane call under that row, to the byte
        st1, sc1, yw1 = gpu_ctx.embed_tiles_payload(planes[p], tile_bit, delta, want_yw=True, dither=rows[p])
        assert np.array_equal(st3[p], st1) and np.array_equal(sc3[p], sc1) and np.array_equal(yw3[p].view(np.uint32), yw1.view(np.uint32)), p
        assert np.array_equal(eff3[p].view(np.uint32), gpu_ctx.payload_sigma_w(planes[p], tile_bit, delta, dither=rows[p]).view(np.uint32))
        assert np.array_equal(m3[p].view(np.uint32), gpu_ctx.payload_metric(st3[p], delta, dither=rows[p]).view(np.uint32)), p
        # and the restatement's under that row
        r = dr.margins_of(planes[p], tile_bit, rows[p], delta)
        comp = r["comparable"]
        assert (~comp).sum() <= pr.CAP_SEEDED * nt
        dt = _tile_max(np.abs(st3[p].astype(int) - r["stego"].astype(int)))
        assert dt[comp].max() <= 1, (p, np.argwhere(comp & (dt > 1)).tolist())
        assert np.all(np.abs(m3[p] - dr.metric_ref(st3[p], rows[p], delta)) <= pr.slope_bar(delta)), p
        soft_sum += gpu_ctx.payload_soft(st3[p], order, offs, 16, delta, dither=rows[p])
        # read under another plane's row the votes are those of a stranger
        if p:
            assert float(np.abs(gpu_ctx.payload_metric(st3[p], delta, dither=rows[0])).mean()) < float(np.abs(m3[p]).mean()) - 0.2
    soft = gpu_ctx.payload_soft(st3, order, offs, 16, delta, dither=rows)
    assert np.abs(soft - soft_sum).max() < 1e-9
    assert np.array_equal(soft < 0, pr.seeded_bits(16, 0) != 0)
    # a per-plane table whose rows are all equal gives what the shared table gives
    same = np.ascontiguousarray(np.broadcast_to(rows[0], (3, nt)))
    a = gpu_ctx.embed_tiles_payload(planes, tile_bit, delta, dither=same)
    b = gpu_ctx.embed_tiles_payload(planes, tile_bit, delta, dither=rows[0])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(gpu_ctx.payload_metric(a[0], delta, dither=same).view(np.uint32),
                          gpu_ctx.payload_metric(a[0], delta, dither=rows[0]).view(np.uint32))
    assert np.array_equal(gpu_ctx.payload_soft(a[0], order, offs, 16, delta, dither=same).view(np.uint64),
                          gpu_ctx.payload_soft(a[0], order, offs, 16, delta, dither=rows[0]).view(np.uint64))
    assert np.array_equal(gpu_ctx.payload_sigma_w(planes, tile_bit, delta, dither=same).view(np.uint32),
                          gpu_ctx.payload_sigma_w(planes, tile_bit, delta, dither=rows[0]).view(np.uint32))
    # a table stride larger than n_tiles: rows 128 words apart
    wide = np.zeros((3, 128), np.uint16); wide[:, :nt] = rows
    st_w = np.empty_like(st3); sc_w = np.empty_like(sc3)
    gpu_ctx._call("wm_embed_tiles_payload_dither_u8", _vp(planes), _vp(tile_bit), _vp(wide), _vp(st_w), _vp(sc_w), None, 3, 72, 100,
                  100, 7200, 128, delta)
    assert np.array_equal(st_w, st3) and np.array_equal(sc_w, sc3)


def test_row_stride_w_plus_3_takes_the_bytewise_kernels(gpu_ctx):
    planes, nt, tile_bit, order, offs = _planes_case()
    n, H, W = planes.shape
    delta = 24.0
    rows = np.stack([dr.seeded_words(nt, s) for s in (0, 1, 2)])
    dense_st, dense_sc, dense_yw = gpu_ctx.embed_tiles_payload(planes, tile_bit, delta, want_yw=True, dither=rows)
    rs, ps = W + 3, (H + 1) * (W + 3) + 1
    big = np.random.default_rng(9).integers(0, 256, n * ps, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(big, (n, H, W), (ps, rs, 1))
    view[...] = planes
    inside = np.zeros(big.shape, bool)
    np.lib.stride_tricks.as_strided(inside, (n, H, W), (ps, rs, 1))[...] = True
    out = np.full_like(big, 7)
    sc = np.empty_like(dense_sc); yw = np.zeros_like(dense_yw)
    gpu_ctx._call("wm_embed_tiles_payload_dither_u8", _vp(big), _vp(tile_bit), _vp(rows), _vp(out), _vp(sc), _vp(yw), n, H, W, rs, ps,
                  nt, delta)
    out_view = np.lib.stride_tricks.as_strided(out, (n, H, W), (ps, rs, 1))
    assert np.all(out[~inside] == 7)
    assert np.array_equal(out_view, dense_st) and np.array_equal(sc, dense_sc) and np.array_equal(yw.view(np.uint32), dense_yw.view(np.uint32))
    # the decode through the same layout: metric, soft and sigma_w_eff equal the dense calls' to the bit
    m = np.empty((n, H // 8, W // 8), np.float32)
    gpu_ctx._call("wm_payload_metric_tiles_dither_u8", _vp(out), _vp(rows), _vp(m), n, H, W, rs, ps, nt, delta)
    assert np.array_equal(m.view(np.uint32), gpu_ctx.payload_metric(dense_st, delta, dither=rows).view(np.uint32))
    soft = np.full(16, 7.0)
    gpu_ctx._call("wm_payload_soft_tiles_dither_u8", _vp(out), _vp(rows), _vp(order), _vp(offs), 16, _vp(soft), n, H, W, rs, ps, nt, delta)
    assert np.array_equal(soft.view(np.uint64), gpu_ctx.payload_soft(dense_st, order, offs, 16, delta, dither=rows).view(np.uint64))
    eff = np.empty((n, H // 8, W // 8, 8), np.float32)
    gpu_ctx._call("wm_payload_sigma_w_tiles_dither_u8", _vp(big), _vp(tile_bit), _vp(rows), _vp(eff), n, H, W, rs, ps, nt, delta)
    assert np.array_equal(eff.view(np.uint32), gpu_ctx.payload_sigma_w(planes, tile_bit, delta, dither=rows).view(np.uint32))
    # and the restatement still holds there (plane 1 under its row)
    r = dr.margins_of(planes[1], tile_bit, rows[1], delta)
    dt = _tile_max(np.abs(out_view[1].astype(int) - r["stego"].astype(int)))
    assert (~r["comparable"]).sum() <= pr.CAP_SEEDED * nt and dt[r["comparable"]].max() <= 1


@pytest.mark.parametrize("delta", [16.0, 200.0])
def test_a_table_of_zeros_is_the_dither_free_rule(gpu_ctx, delta):
    planes, nt, tile_bit, order, offs = _planes_case()
    free_st, free_sc, free_yw = gpu_ctx.embed_tiles_payload(planes, tile_bit, delta, want_yw=True)
    free_eff = gpu_ctx.payload_sigma_w(planes, tile_bit, delta)
    free_m = gpu_ctx.payload_metric(free_st, delta)
    free_soft = gpu_ctx.payload_soft(free_st, order, offs, 16, delta)
    for z in (np.zeros(nt, np.uint16), np.zeros((3, nt), np.uint16)):
        st, sc, yw = gpu_ctx.embed_tiles_payload(planes, tile_bit, delta, want_yw=True, dither=z)
        assert np.array_equal(st, free_st) and np.array_equal(sc.view(np.uint32), free_sc.view(np.uint32))
        assert np.array_equal(yw.view(np.uint32), free_yw.view(np.uint32))
        assert np.array_equal(gpu_ctx.payload_sigma_w(planes, tile_bit, delta, dither=z).view(np.uint32), free_eff.view(np.uint32))
        assert np.array_equal(gpu_ctx.payload_metric(free_st, delta, dither=z).view(np.uint32), free_m.view(np.uint32))
        assert np.array_equal(gpu_ctx.payload_soft(free_st, order, offs, 16, delta, dither=z).view(np.uint64), free_soft.view(np.uint64))
    gpu_ctx.check_status()


def test_bad_arguments_and_empty_inputs(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx._h
    planes, nt, tile_bit, order, offs = _planes_case()
    Y = np.ascontiguousarray(planes[0])
    u = dr.seeded_words(nt, 0)
    eff = np.empty((3, nt, 8), np.float32); st = np.empty((3, 72, 100), np.uint8); sc = np.empty((3, nt, 8), np.float32)
    m = np.empty((3, nt), np.float32); soft = np.empty(16)
    p3 = planes.ctypes.data
    geo1, geo3 = (1, 72, 100, 100, 7200), (3, 72, 100, 100, 7200)

    def calls(geo, table, stride, delta=16.0, pl=p3):
        t = None if table is None else table.ctypes.data
        return [lib.wm_payload_sigma_w_tiles_dither_u8(h, pl, tile_bit.ctypes.data, t, eff.ctypes.data, *geo, stride, delta),
                lib.wm_embed_tiles_payload_dither_u8(h, pl, tile_bit.ctypes.data, t, st.ctypes.data, sc.ctypes.data, None, *geo, stride, delta),
                lib.wm_payload_metric_tiles_dither_u8(h, pl, t, m.ctypes.data, *geo, stride, delta),
                lib.wm_payload_soft_tiles_dither_u8(h, pl, t, order.ctypes.data, offs.ctypes.data, 16, soft.ctypes.data, *geo, stride, delta)]

    assert calls(geo3, u, 0) == [WM_OK] * 4
    assert calls(geo3, None, 0) == [WM_ERR_BADARG] * 4                       # a NULL table with work to do
    assert b"tile_dither" in lib.wm_last_error()
    for stride in (1, 5, nt - 1):                                           # neither 0 nor >= n_tiles
        assert calls(geo3, u, stride) == [WM_ERR_BADARG] * 4, stride
        assert calls(geo1, u, stride) == [WM_ERR_BADARG] * 4, stride
    assert b"dither_plane_stride" in lib.wm_last_error()
    assert calls(geo3, u, 0, delta=4.0) == [WM_ERR_BADARG] * 4
    # empty inputs: no planes, no tiles - WM_OK without a launch, whatever the table
    assert calls((0, 72, 100, 100, 7200), None, 0) == [WM_OK] * 4
    assert calls((1, 7, 7, 7, 49), None, 3)[:3] == [WM_OK] * 3
    assert calls((1, 0, 0, 0, 0), None, 0) == [WM_OK] * 4
    # the device forms
    d = gpu_ctx.malloc(1 << 20)
    try:
        gpu_ctx.h2d(d, Y)
        off_bit, off_u, off_out = 1 << 14, 1 << 15, 1 << 16
        gpu_ctx.h2d(d + off_bit, tile_bit); gpu_ctx.h2d(d + off_u, u)
        gpu_ctx.h2d(d + (1 << 17), order); gpu_ctx.h2d(d + (1 << 17) + 4096, offs)

        def dev_calls(table, stride):
            return [lib.wm_payload_sigma_w_tiles_dither_u8_dev(h, d, d + off_bit, table, d + off_out, *geo1, stride, 16.0),
                    lib.wm_embed_tiles_payload_dither_u8_dev(h, d, d + off_bit, table, d + (1 << 18), d + off_out, None, *geo1, stride, 16.0),
                    lib.wm_payload_metric_tiles_dither_u8_dev(h, d, table, d + off_out, *geo1, stride, 16.0),
                    lib.wm_payload_soft_tiles_dither_u8_dev(h, d, table, d + (1 << 17), d + (1 << 17) + 4096, 16, d + off_out, *geo1, stride, 16.0)]
        assert dev_calls(None, 0) == [WM_ERR_BADARG] * 4
        assert dev_calls(d + off_u, 7) == [WM_ERR_BADARG] * 4
        assert dev_calls(d + off_u + 1, 0) == [WM_ERR_BADARG] * 4            # an odd address
        assert dev_calls(d + off_u, 0) == [WM_OK] * 4
        gpu_ctx.check_status()
        assert lib.wm_payload_metric_tiles_dither_u8_dev(h, d, None, d + off_out, 0, 72, 100, 100, 7200, 0, 16.0) == WM_OK
    finally:
        gpu_ctx.free(d)
    with pytest.raises(ValueError, match="dither"):
        gpu_ctx.payload_metric(Y, 16.0, dither=u[:-1])


# ---- the drop-in and the video ----------------------------------------------------------------------------------------
def _cover(H=72, W=100):
    return np.ascontiguousarray(np.stack([pr.host(H, W, 1)] * 3, axis=-1))  # gray BGR: Y of BGR2YCrCb is the plane itself


def test_dropin_round_trip(gpu_ctx, tmp_path):
    import dct_svd_core_secure as core
    cover = _cover()
    cp, sp, mp = str(tmp_path / "cover.png"), str(tmp_path / "stego.png"), str(tmp_path / "meta.npz")
    assert hg.write_png(cp, cover)
    core.embed_payload(cp, "id 7", sp, mp, password=dr.PASSWORD, nonce=dr.NONCE, dither=True)
    assert os.path.getsize(mp) == 577
    data, valid, conf, _ = core.extract_payload(sp, mp, password=dr.PASSWORD)
    assert data == b"id 7" and valid is True and conf > 0.5
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        core.extract_payload(sp, mp, password="not the password")
    # the stego is the restatement's under the product's table, and differs from the dither-free embed's
    key = hg.derive_key(dr.PASSWORD, dr.NONCE)
    bits = P.payload_frame(b"id 7")
    tbi, order, offs = P.payload_map(9, 12, key, bits.size)
    r = dr.margins_of(cover[..., 0], bits[tbi], P.dither_table(9, 12, key), 16.0)
    Ys = np.ascontiguousarray(o.bgr_to_ycrcb(hg.read_image_bgr(sp))[..., 0])
    dt = _tile_max(np.abs(Ys.astype(int) - r["stego"].astype(int)))
    assert dt[r["comparable"]].max() <= 1 and (~r["comparable"]).sum() <= pr.CAP_SEEDED * 108
    plain = core.embed_payload_arrays(cover, "id 7", dr.PASSWORD, dr.NONCE)
    assert "dither" not in plain["meta"] and not np.array_equal(plain["stego"], hg.read_image_bgr(sp))
    # a dither-free meta forged for the same stego (the right key, no dither member) is authentic and decodes to nothing
    stego = hg.read_image_bgr(sp)
    assert core.extract_payload_arrays(stego, plain["meta"], dr.PASSWORD)[1] is False
    # and the other way round
    meta = M.load_payload_meta(mp)
    assert M.payload_dither_of(meta) == 1
    assert core.extract_payload_arrays(plain["stego"], meta, dr.PASSWORD)[1] is False
    assert core.extract_payload_arrays(plain["stego"], plain["meta"], dr.PASSWORD)[:2] == (b"id 7", True)


def test_dropin_self_check_decodes_with_the_dither(gpu_ctx):
    """verify=True raises on a payload the dithered stego does not carry: the document page with n_bits = n_tiles, which has
    wrong bits on the restatement (asserted here and in tests/test_payload_dither.py)"""
    import dct_svd_core_secure as core
    Y = pr.document_host(*pr.DOCUMENT, pr.DOCUMENT_SEED)
    cover = np.ascontiguousarray(np.stack([Y] * 3, axis=-1))
    full = pr.DOCUMENT_PAYLOADS[2]
    key = hg.derive_key("pw", pr.DOCUMENT_NONCE)
    bits = P.payload_frame(full)
    tbi, order, offs = P.payload_map(16, 32, key, bits.size)
    r = dr.margins_of(Y, bits[tbi], P.dither_table(16, 32, key), 16.0)
    soft = pr.soft_ref(r["m"].reshape(1, -1), order, offs)
    sure_wrong = ((soft < 0) != (bits != 0)) & r["comparable"].ravel()[order] & (np.abs(soft) > pr.slope_bar(16.0))
    assert sure_wrong.sum() >= 1
    with pytest.raises(ValueError, match=r"^payload does not decode from its own stego: \d+ of 512 bits wrong"):
        core.embed_payload_arrays(cover, full, "pw", pr.DOCUMENT_NONCE, payload_type="bytes", dither=True)
    out = core.embed_payload_arrays(cover, full, "pw", pr.DOCUMENT_NONCE, payload_type="bytes", dither=True, verify=False)
    assert core.extract_payload_arrays(out["stego"], out["meta"], "pw")[1] is False
    short = core.embed_payload_arrays(cover, pr.DOCUMENT_PAYLOADS[0], "pw", pr.DOCUMENT_NONCE, payload_type="bytes", dither=True)
    assert core.extract_payload_arrays(short["stego"], short["meta"], "pw")[:2] == (pr.DOCUMENT_PAYLOADS[0], True)


def test_video_round_trip(gpu_ctx, tmp_path):
    """A 3-frame .y4m with frame_interval = 1.  The frames are 64 x 96: a 32 x 48 frame has 24 tiles, and the smallest payload
    frame (no data: the length header and the CRC) has 64 bits, so no payload fits one - asserted below."""
    v = importlib.import_module(PKG_NAME + ".video")
    assert P.capacity_bits(32, 48) == 24 < P.payload_frame(b"").size == 64
    H, W = 64, 96
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = np.stack([np.clip(120 + 50 * np.sin(xx / 14.0 + f) * np.cos(yy / 10.0) + rng.normal(0, 6, (H, W)), 0, 255).astype(np.uint8)
                       for f in range(3)])
    src, outp, metap = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "vm.npz")
    v.write_y4m(src, frames)
    data = b"v1"                                                            # 80 bits on 96 tiles
    v.embed_payload_video(src, data, outp, metap, password=dr.PASSWORD, payload_type="bytes", nonce=dr.NONCE, frame_interval=1,
                          batch=2, dither=True)
    assert os.path.getsize(metap) == 585
    got, valid, conf = v.extract_payload_video(outp, metap, password=dr.PASSWORD, batch=2)
    assert got == data and valid is True
    got, valid, _ = v.extract_payload_video(outp, metap, password=dr.PASSWORD, batch=3)      # the batch size is no part of the rule
    assert got == data and valid is True
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        v.extract_payload_video(outp, metap, password="no")
    # marked frames 0 and 1 use different tables: each reads clearly under its own, not under the other's
    key = hg.derive_key(dr.PASSWORD, dr.NONCE)
    t0, t1 = P.dither_table(8, 12, key, 0), P.dither_table(8, 12, key, 1)
    assert not np.array_equal(t0, t1)
    vid = v.Y4M(outp)
    try:
        ys = [y.copy() for _, y, _ in vid]
    finally:
        vid.close()
    own0 = float(np.abs(gpu_ctx.payload_metric(ys[0], 16.0, dither=t0)).mean())
    own1 = float(np.abs(gpu_ctx.payload_metric(ys[1], 16.0, dither=t1)).mean())
    cross = float(np.abs(gpu_ctx.payload_metric(ys[1], 16.0, dither=t0)).mean())
    print(f"frame 0 under table 0: {own0:.3f}; frame 1 under table 1: {own1:.3f}, under table 0: {cross:.3f}")
    assert own0 > cross + 0.15 and own1 > cross + 0.15
