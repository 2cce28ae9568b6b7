"""Blind payload on the device: the sigma_w pass, embed then decode, batching and order, argument checks, the drop-in
and the video functions, each against the NumPy restatement of the rule composed from the unchanged oracle
(tests/payload_refs.py).  Hosts: the three seeded ones of mask_refs (72 x 100: 108 tiles, a partial wave, a ragged right
edge; 64 x 64: one wave) and the 16-tile edge host.

Two kinds of tile have no unique restatement, and the comparisons say so where they apply:
  * a rounding tie - (s_1 - b delta) / (2 delta) within 1e-4 s_1 / (2 delta) of a half-integer: a singular value that is
    right to the project's 1e-4 s_1 bar can round either way (the constants 2, 64, 128, .. of the edge host sit exactly on
    one).  Such a tile is compared with the restatement evaluated on the device's own cover singular values;
  * s_1 = s_2 (the {0, 40} checkerboard): the leading singular vector is any unit vector of a plane, np.linalg.svd returns
    one and the Jacobi another, and the two stegos differ while both carry sigma_1 = target.  Such a tile is compared in
    its singular values instead of its pixels.
Every tile takes part in every comparison; none of the seeded hosts' tiles is of either kind (asserted).
"""
import importlib
import json
import os

import numpy as np
import pytest

import payload_refs as pr
from conftest import PKG_NAME
from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

SIGMA_RTOL = pr.SIGMA_RTOL                                                  # the project's sigma bar (BASELINE.json)
DELTA = pr.DELTA
M = importlib.import_module(PKG_NAME + ".meta")
P = importlib.import_module(PKG_NAME + ".payload")
hg = importlib.import_module(PKG_NAME + ".hostglue")
WM_ERR_BADARG = 1


@pytest.fixture(scope="module", autouse=True)
def _preconditions():
    pr.check_preconditions(DELTA, 0.4)


def _hosts():
    return pr.all_hosts()


_tie_tiles = pr.tie_tiles                                                   # (shared with tests/test_gpu_payload_edges.py)
_degenerate_tiles = pr.degenerate_tiles


# ---- 1. the sigma_w pass --------------------------------------------------------------------------------------------
def _check_eff(eff, Y, bits, delta, seeded):
    """the four properties of test 1 on every tile of one plane; returns the worst |eff - restatement| / s_1"""
    So = o.stego_sigma(Y.astype(np.float32), 8)
    s1, s2 = So[..., 0].astype(np.float64), So[..., 1].astype(np.float64)
    tol = SIGMA_RTOL * s1
    assert eff.shape == So.shape and eff.dtype == np.float32
    assert np.all(eff[..., 1:] == 0)                                        # entries 1..7 are exactly 0
    q = s1 + eff[..., 0].astype(np.float64) - 4.0
    k = (q - np.where(bits != 0, delta, 0.0)) / (2 * delta)
    assert np.all(np.abs(k - np.rint(k)) * 2 * delta <= tol + 1e-9), "off the tile's lattice"
    assert np.all(q >= s2 + delta - tol - 1e-9)
    want = pr.sigma_w_eff(So, bits, delta)[..., 0]
    far = ~_tie_tiles(So, bits, delta)
    if seeded:
        assert far.all()
    err = np.abs(eff[..., 0] - want)
    assert np.all(err[far] <= tol[far] + 1e-9), np.argwhere(far & (err > tol)).tolist()
    # a tie tile went to one of the two nearest points of its lattice
    assert np.all(np.abs(err[~far] - np.round(err[~far] / (2 * delta)) * 2 * delta) <= tol[~far] + 1e-9)
    assert np.all(err[~far] <= 2 * delta + tol[~far])
    return float(np.max(err[far] / np.maximum(s1[far], 1.0)))


@pytest.mark.parametrize("case", ["72x100", "64x64", "edge", "72x100_stride_101", "three_planes"])
def test_sigma_w_eff_kernel(gpu_ctx, case):
    if case == "three_planes":
        planes = np.ascontiguousarray(pr.mr.planes_of(72, 100, 3))
    elif case == "edge":
        planes = pr.edge_host()
    elif case == "64x64":
        planes = pr.host(64, 64, 3)
    else:
        planes = pr.host(72, 100, 1)
    if case == "72x100_stride_101":                                         # a view with row stride 101: the byte-wise path
        big = np.zeros((72, 101), np.uint8); big[:, :100] = planes
        planes = big[:, :100]
        assert planes.strides == (101, 1)
    H, W = planes.shape[-2:]
    nt = (H // 8, W // 8)
    for seed in (0, 1):
        bits = pr.seeded_bits(nt[0] * nt[1], seed).reshape(nt)
        eff = gpu_ctx.payload_sigma_w(planes, bits, DELTA)
        # (the third of the three planes is a mirror image of the first, not one of the seeded hosts: it may hold a tie)
        worst = max(_check_eff(e, Y, bits, DELTA, case != "edge" and i < 2)
                    for i, (e, Y) in enumerate(zip(eff, planes) if planes.ndim == 3 else [(eff, planes)]))
        print(f"{case} bits seed {seed}: worst |eff - restatement| / s_1 = {worst:.2e} (bar {SIGMA_RTOL:.0e})")
    if case == "edge":                                                      # both bit values on every edge tile
        for b in (0, 1):
            _check_eff(gpu_ctx.payload_sigma_w(planes, np.full(nt, b, np.uint8), DELTA), planes, np.full(nt, b, np.uint8), DELTA, False)
    if case == "72x100_stride_101":
        assert np.array_equal(eff, gpu_ctx.payload_sigma_w(np.ascontiguousarray(planes), bits, DELTA))
    if case == "three_planes":                                              # one plane alone gives that plane's rows
        assert np.array_equal(gpu_ctx.payload_sigma_w(planes[1], bits, DELTA), eff[1])


@pytest.mark.parametrize("delta", [8.0, 24.0, 512.0])
def test_sigma_w_eff_other_deltas(gpu_ctx, delta):
    Y = pr.host(72, 100, 2)
    bits = pr.seeded_bits(108, 3).reshape(9, 12)
    So = o.stego_sigma(Y.astype(np.float32), 8)
    eff = gpu_ctx.payload_sigma_w(Y, bits, delta)
    far = ~_tie_tiles(So, bits, delta)
    assert far.sum() >= 100
    _check_eff(eff, Y, bits, delta, False)


# ---- 2. embed then decode -------------------------------------------------------------------------------------------
def _restatement_stego(Y, tile_bits, sc_dev, delta):
    """(restatement's stego, tie mask): a tie tile's target is taken from the device's own cover singular values - those of
    its sigma pass (K2), which the payload's sigma_w pass shares; the embed's sigma_c of a constant tile is a closed form"""
    So = o.stego_sigma(Y.astype(np.float32), 8)
    tie = _tie_tiles(So, tile_bits, delta)
    ref = pr.embed_ref(Y, tile_bits, delta)
    if tie.any():
        eff = ref["eff"].copy()
        eff[tie, 0] = pr.target(sc_dev, tile_bits, delta)[tie] - So[tie, 0]
        ref = o.embed_plane(Y.astype(np.float32), None, 1.0, kfrac=0.0, tile=8, k_floor=1, wm_svd=(None, eff, None))
    return ref["stego"], tie, So


@pytest.mark.parametrize("n_bits_mode", ["all_tiles", "16"])
@pytest.mark.parametrize("name", [n for n, _ in pr.all_hosts()])
def test_embed_then_decode(gpu_ctx, name, n_bits_mode):
    """Bits exact (n_bits = n_tiles: one wrong tile fails); stego within 1 LSB of the restatement's; soft within the sigma
    bar through the metric's slope: |soft[j] - ref[j]| <= count[j] * 2 * (1e-4 * 2040) / delta, ref = the restatement run
    on the device's own stego."""
    Y = dict(_hosts())[name]
    H, W = Y.shape
    nt = (H // 8) * (W // 8)
    n_bits = nt if n_bits_mode == "all_tiles" else 16
    seeds = (0, 1) if name != "edge" else (0, 1, "zeros", "ones")
    for seed in seeds:
        bits = (np.zeros(n_bits, np.uint8) if seed == "zeros" else np.ones(n_bits, np.uint8) if seed == "ones"
                else pr.seeded_bits(n_bits, seed))
        tbi, order, offs = pr.simple_map(nt, n_bits, seed=7)
        tile_bits = bits[tbi].reshape(H // 8, W // 8)
        st, sc, _ = gpu_ctx.embed_tiles_payload(Y, tile_bits, DELTA)
        soft = gpu_ctx.payload_soft(st, order, offs, n_bits, DELTA)
        assert soft.shape == (n_bits,) and soft.dtype == np.float64
        count = np.diff(offs)
        wrong = np.flatnonzero((soft < 0) != (bits != 0))
        assert wrong.size == 0, (name, seed, wrong.tolist(), soft[wrong].tolist())
        # stego against the restatement
        ref_st, tie, So = _restatement_stego(Y, tile_bits, gpu_ctx.sigma_tiles(Y), DELTA)
        if name != "edge":
            assert not tie.any() and not _degenerate_tiles(So).any()
        assert np.all(np.abs(sc - So) <= SIGMA_RTOL * So[..., :1] + 1e-3)      # (a black tile's sigma_c is the embed's tabulated ~1e-4)
        d = np.abs(st.astype(int) - ref_st.astype(int))
        dt = o.to_tiles(d).max((-1, -2))
        deg = _degenerate_tiles(So)
        assert dt[~deg].max() <= 1, np.argwhere(~deg & (dt > 1)).tolist()
        if deg.any():                       # s_1 = s_2: the same singular values, to the sigma bar plus 1 LSB per pixel (8 in sigma)
            s_dev, s_ref = o.stego_sigma(st.astype(np.float32), 8)[deg], o.stego_sigma(ref_st.astype(np.float32), 8)[deg]
            assert np.abs(s_dev[:, :2] - s_ref[:, :2]).max() <= 8.0 + SIGMA_RTOL * s_ref[:, 0].max()
        assert np.array_equal(st[:, (W // 8) * 8:], Y[:, (W // 8) * 8:])      # outside the grid: passed through
        # soft against the restatement on the device's own stego
        ref_soft = pr.soft_ref(pr.metric_ref(st, DELTA).reshape(1, -1), order, offs)
        bar = count * 2 * (SIGMA_RTOL * 2040) / DELTA
        assert np.all(np.abs(soft - ref_soft) <= bar), float(np.max(np.abs(soft - ref_soft) / count))
        m_dev = gpu_ctx.payload_metric(st, DELTA)
        signed = np.where(tile_bits != 0, -m_dev, m_dev)
        signed_ref = np.where(tile_bits != 0, -1, 1) * pr.metric_ref(ref_st, DELTA)
        print(f"{name} n_bits={n_bits} bits {seed}: worst |m| deficit against the restatement {float(np.max(signed_ref - signed)):.3f} "
              f"(min device margin {float(signed.min()):.3f}); worst |soft - ref| / count {float(np.max(np.abs(soft - ref_soft) / count)):.2e} "
              f"(bar {2 * SIGMA_RTOL * 2040 / DELTA:.2e}); share of stego pixels differing {float((d != 0).mean()):.2e}")
        assert signed.min() > 0 or n_bits < nt


# ---- 3. batch and order ---------------------------------------------------------------------------------------------
def test_batch_and_order(gpu_ctx):
    planes = pr.mr.planes_of(72, 100, 3)
    bits = pr.seeded_bits(16, 2)
    tbi, order, offs = pr.simple_map(108, 16)
    st, _, _ = gpu_ctx.embed_tiles_payload(planes, bits[tbi], DELTA)
    assert all(np.array_equal(st[p], gpu_ctx.embed_tiles_payload(planes[p], bits[tbi], DELTA)[0]) for p in range(3))
    soft3 = gpu_ctx.payload_soft(st, order, offs, 16, DELTA)
    ones = [gpu_ctx.payload_soft(st[p], order, offs, 16, DELTA) for p in range(3)]
    assert np.abs(soft3 - (ones[0] + ones[1] + ones[2])).max() < 1e-9
    assert np.array_equal(soft3 < 0, bits != 0)
    again = gpu_ctx.payload_soft(st, order, offs, 16, DELTA)
    assert np.array_equal(soft3.view(np.uint64), again.view(np.uint64))     # bit-identical
    # the host-pointer entry point, planes as a strided view: the same sums
    big = np.zeros((3, 75, 104), np.uint8); big[:, 2:74, 3:103] = st
    view = big[:, 2:74, 3:103]
    n, H, W, rs, ps = 3, 72, 100, 104, 75 * 104
    soft_h = np.zeros(16, np.float64)
    gpu_ctx._call("wm_payload_soft_tiles_u8", view.ctypes.data, order.ctypes.data, offs.ctypes.data, 16, soft_h.ctypes.data,
                  n, H, W, rs, ps, DELTA)
    assert np.array_equal(soft_h.view(np.uint64), soft3.view(np.uint64))
    m = gpu_ctx.payload_metric(view, DELTA)
    assert np.array_equal(m, gpu_ctx.payload_metric(st, DELTA))
    assert np.abs(pr.soft_ref(m.reshape(3, -1), order, offs) - soft3).max() < 1e-9


def test_in_place_and_yw(gpu_ctx):
    """stego may alias host (the device form, in place), and yw is the unclipped plane the stego is truncated from"""
    Y = pr.edge_host()
    bits = pr.seeded_bits(16, 4).reshape(2, 8)
    st, sc, yw = gpu_ctx.embed_tiles_payload(Y, bits, DELTA, want_yw=True)
    assert np.array_equal(np.clip(yw, 0, 255).astype(np.uint8), st)
    H, W = Y.shape
    d_host = gpu_ctx.malloc(Y.nbytes); d_bit = gpu_ctx.malloc(16); d_sc = gpu_ctx.malloc(16 * 8 * 4)
    try:
        gpu_ctx.h2d(d_host, Y); gpu_ctx.h2d(d_bit, bits)
        gpu_ctx._call("wm_embed_tiles_payload_u8_dev", d_host, d_bit, d_host, d_sc, None, 1, H, W, W, H * W, DELTA)
        gpu_ctx.check_status()
        got = np.empty_like(Y); gpu_ctx.d2h(got, d_host)
    finally:
        for d in (d_host, d_bit, d_sc):
            gpu_ctx.free(d)
    assert np.array_equal(got, st)


# ---- 4. argument checks ---------------------------------------------------------------------------------------------
def test_argument_checks(gpu_ctx, hostapi):
    Y = pr.host(72, 100, 1)
    tb = np.zeros(108, np.uint8)
    _, order, offs = pr.simple_map(108, 16)
    lib = gpu_ctx.lib
    eff = np.zeros((108, 8), np.float32); sc = np.zeros((108, 8), np.float32); st = np.zeros_like(Y)
    soft = np.full(16, 7.0); metric = np.zeros(108, np.float32)
    h = gpu_ctx._h
    d_buf = gpu_ctx.malloc(1 << 16)
    try:
        _argument_checks(gpu_ctx, lib, h, d_buf, Y, tb, order, offs, eff, sc, st, soft, metric)
    finally:
        gpu_ctx.free(d_buf)


def _argument_checks(gpu_ctx, lib, h, d_buf, Y, tb, order, offs, eff, sc, st, soft, metric):
    for delta in (7.9, float("inf"), float("nan"), 512.5):
        assert lib.wm_payload_sigma_w_tiles_u8(h, Y.ctypes.data, tb.ctypes.data, eff.ctypes.data, 1, 72, 100, 100, 7200, delta) == WM_ERR_BADARG
        assert lib.wm_embed_tiles_payload_u8(h, Y.ctypes.data, tb.ctypes.data, st.ctypes.data, sc.ctypes.data, None, 1, 72, 100, 100, 7200, delta) == WM_ERR_BADARG
        assert lib.wm_payload_metric_tiles_u8(h, Y.ctypes.data, metric.ctypes.data, 1, 72, 100, 100, 7200, delta) == WM_ERR_BADARG
        assert lib.wm_payload_soft_tiles_u8(h, Y.ctypes.data, order.ctypes.data, offs.ctypes.data, 16, soft.ctypes.data, 1, 72, 100, 100, 7200, delta) == WM_ERR_BADARG
        with pytest.raises(ValueError):
            gpu_ctx.embed_tiles_payload(Y, tb, delta)
    for n_bits in (0, 109):
        assert lib.wm_payload_soft_tiles_u8(h, Y.ctypes.data, order.ctypes.data, offs.ctypes.data, n_bits, soft.ctypes.data, 1, 72, 100, 100, 7200, DELTA) == WM_ERR_BADARG
        assert lib.wm_payload_soft_tiles_u8_dev(h, d_buf, d_buf, d_buf, n_bits, d_buf, 1, 72, 100, 100, 7200, DELTA) == WM_ERR_BADARG
        with pytest.raises(ValueError):
            gpu_ctx.payload_soft(Y, order, offs, n_bits, DELTA)
    short = offs.copy(); short[-1] = 107
    down = offs.copy(); down[3] = down[2] - 1
    first = offs.copy(); first[0] = 1
    for bad in (short, down, first):
        assert lib.wm_payload_soft_tiles_u8(h, Y.ctypes.data, order.ctypes.data, bad.ctypes.data, 16, soft.ctypes.data, 1, 72, 100, 100, 7200, DELTA) == WM_ERR_BADARG
        with pytest.raises(ValueError):
            gpu_ctx.payload_soft(Y, order, bad, 16, DELTA)
    out = order.copy(); out[5] = 108
    assert lib.wm_payload_soft_tiles_u8(h, Y.ctypes.data, out.ctypes.data, offs.ctypes.data, 16, soft.ctypes.data, 1, 72, 100, 100, 7200, DELTA) == WM_ERR_BADARG
    for args in ((None, tb.ctypes.data, eff.ctypes.data), (Y.ctypes.data, None, eff.ctypes.data), (Y.ctypes.data, tb.ctypes.data, None)):
        assert lib.wm_payload_sigma_w_tiles_u8(h, *args, 1, 72, 100, 100, 7200, DELTA) == WM_ERR_BADARG
    assert lib.wm_payload_soft_tiles_u8(h, Y.ctypes.data, order.ctypes.data, offs.ctypes.data, 16, None, 1, 72, 100, 100, 7200, DELTA) == WM_ERR_BADARG
    assert lib.wm_payload_metric_tiles_u8(h, Y.ctypes.data, None, 1, 72, 100, 100, 7200, DELTA) == WM_ERR_BADARG
    assert np.all(soft == 7.0) and not eff.any() and not st.any()           # nothing was written: no launch
    gpu_ctx.check_status()
    # a 7 x 7 image has no tiles: embed passes it through and returns WM_OK
    tiny = np.random.default_rng(2).integers(0, 256, (7, 7), dtype=np.uint8)
    st7, sc7, _ = gpu_ctx.embed_tiles_payload(tiny, np.zeros(0, np.uint8), DELTA)
    assert np.array_equal(st7, tiny) and sc7.shape == (0, 0, 8)
    assert gpu_ctx.payload_sigma_w(tiny, np.zeros(0, np.uint8), DELTA).shape == (0, 0, 8)
    assert lib.wm_payload_metric_tiles_u8(h, tiny.ctypes.data, None, 1, 7, 7, 7, 49, DELTA) == 0
    assert lib.wm_embed_tiles_payload_u8(h, None, None, st.ctypes.data, None, None, 0, 72, 100, 100, 7200, DELTA) == 0   # no planes
    import dct_svd_core_secure as core
    with pytest.raises(ValueError, match="^Payload quá dài"):
        core.embed_payload_arrays(np.zeros((7, 7, 3), np.uint8), b"", "pw", bytes(8))


# ---- 5. drop-in -----------------------------------------------------------------------------------------------------
def _colour_cover(H, W):
    """the seeded host recipe with channel offsets (-60, +10, +70)"""
    base = pr.mr.host(H, W, 5).astype(int)
    return np.clip(np.stack([base - 60, base + 10, base + 70], axis=-1), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("case", ["gray_72x100_text", "colour_96x128_json"])
def test_dropin_round_trip(gpu_ctx, tmp_path, case):
    import dct_svd_core_secure as core
    if case.startswith("gray"):
        Y = pr.host(72, 100, 1)
        cover = np.stack([Y] * 3, axis=-1)
        payload, ptype, want, suffix = "hello", "text", b"hello", "_text.txt"       # 104 bits on 108 tiles
    else:
        cover = _colour_cover(96, 128)
        payload, ptype, suffix = '{ "é" : 7 }', "json", "_data.json"       # 8 bytes once canonical: 128 bits on 192 tiles
        want = '{"é":7}'.encode("utf-8")
    cp, sp, mp = str(tmp_path / "cover.png"), str(tmp_path / "stego.png"), str(tmp_path / "meta.npz")
    assert hg.write_png(cp, cover)
    nonce = bytes(range(8))
    out, meta_path, psnr, ssim = core.embed_payload(cp, payload, sp, mp, password="pw", payload_type=ptype, nonce=nonce)
    assert out == sp and isinstance(psnr, float) and isinstance(ssim, float)
    print(f"{case}: PSNR {psnr:.2f} dB, SSIM {ssim:.4f}, meta {os.path.getsize(mp)} bytes")
    assert psnr > 40.0 and 0.0 < ssim <= 1.0
    meta = M.load_payload_meta(mp)
    assert os.path.getsize(mp) < 1024
    assert list(meta) == ["mode", "payload_type", "shape", "delta", "payload_bits", "nonce", "tile", "digest"]
    assert int(meta["payload_bits"]) == 8 * (len(want) + 8) and str(meta["payload_type"]) == ptype
    data, valid, conf, written = core.extract_payload(sp, mp, str(tmp_path / "out.png"), password="pw")
    assert data == want and valid is True and 0.5 < conf <= 1.0
    assert written == str(tmp_path / ("out" + suffix)) and os.path.isfile(written)
    text = open(written, encoding="utf-8").read()
    assert (json.loads(text) == json.loads(want.decode("utf-8"))) if ptype == "json" else (text == "hello")
    # a payload file: read when the path exists
    pf = tmp_path / ("p.json" if ptype == "json" else "p.txt")
    pf.write_text(payload, encoding="utf-8")
    r2 = core.embed_payload(cp, str(pf), str(tmp_path / "s2.png"), str(tmp_path / "m2.npz"), password="pw", payload_type=ptype, nonce=nonce)
    assert np.array_equal(hg.read_image_bgr(r2[0]), hg.read_image_bgr(sp))
    # array level, against the restatement: the Y plane of the stego is the restatement's within 1 LSB
    stego = hg.read_image_bgr(sp)
    key = hg.derive_key("pw", nonce)
    bits = P.payload_frame(want)
    tbi, order, offs = P.payload_map(cover.shape[0] // 8, cover.shape[1] // 8, key, bits.size)
    Yc = o.bgr_to_ycrcb(cover)[..., 0]
    ref = pr.embed_ref(Yc, bits[tbi], DELTA)
    d = np.abs(o.bgr_to_ycrcb(stego)[..., 0].astype(int) - ref["stego"].astype(int))
    print(f"{case}: Y of the stego against the restatement: max {d.max()} LSB on {float((d != 0).mean()):.2e} of the pixels")
    if case.startswith("gray"):             # (colour: the BGR round trip and the gamut's clipping come on top; printed)
        assert d.max() <= 1
    # a wrong password fails the HMAC
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        core.extract_payload(sp, mp, password="not pw")
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        core.extract_payload_arrays(stego, meta, "PW")
    # a stego from another key, read with this meta: not valid
    other = core.embed_payload_arrays(cover, want, "another", bytes(8), payload_type="bytes")
    data_o, valid_o, conf_o = core.extract_payload_arrays(other["stego"], meta, "pw")
    print(f"{case}: confidence {conf:.3f}; a stego from another key {conf_o:.3f}")
    assert valid_o is False                 # (with one tile per bit every tile still sits on A lattice point: the confidence says nothing here)
    # and the unmarked cover
    assert core.extract_payload_arrays(cover, meta, "pw")[1] is False
    # the existing readers refuse the meta
    with pytest.raises(ValueError, match="payload"):
        core.extract_arrays(stego, meta, "pw")
    with pytest.raises(ValueError, match="payload"):
        core.detect_arrays(stego, meta)


# ---- 6. video -------------------------------------------------------------------------------------------------------
def test_video(gpu_ctx, tmp_path):
    v = importlib.import_module(PKG_NAME + ".video")
    n, H, W = 5, 64, 96
    # the marked frames (0, 2, 4) are hosts none of whose tiles is within the sigma bar of a rounding tie, for either bit
    # value (most draws of the recipe have one such tile among 96: 2 * 1e-4 s_1 / (2 delta) of the lattice period each)
    ys = np.stack([pr.mr.host(H, W, seed) for seed in (49, 41, 52, 43, 53)])
    for i in (0, 2, 4):
        So = o.stego_sigma(ys[i].astype(np.float32), 8)
        assert not any(_tie_tiles(So, np.full(So.shape[:2], b), DELTA).any() for b in (0, 1))
    chroma = np.random.default_rng(6).integers(0, 256, (n, 2 * (H // 2) * (W // 2)), dtype=np.uint8)
    src, outp, metap = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "vm.npz")
    v.write_y4m(src, ys, chroma, chroma_tag="420")
    _, _, psnr = v.embed_payload_video(src, b"id", outp, metap, password="pw", payload_type="bytes", frame_interval=2,
                                       nonce=bytes(8), batch=2)
    assert isinstance(psnr, float) and psnr > 40.0
    vid = v.Y4M(outp); got = [(y.copy(), c.copy()) for _, y, c in vid]; vid.close()
    assert len(got) == n and vid.chroma == "420"
    for i, (y, c) in enumerate(got):
        assert np.array_equal(c, chroma[i])                                  # chroma bytes are carried through
        assert np.array_equal(y, ys[i]) == (i % 2 == 1)                      # unmarked frames are byte-identical
    data, valid, conf, soft = v.extract_payload_video(outp, metap, password="pw", batch=2, return_soft=True)
    assert data == b"id" and valid is True and conf > 0.5
    # soft is the sum of the per-frame soft vectors
    key = hg.derive_key("pw", bytes(8))
    n_bits = 8 * (2 + 8)
    tbi, order, offs = P.payload_map(H // 8, W // 8, key, n_bits)
    per_frame = [gpu_ctx.payload_soft(got[i][0], order, offs, n_bits, DELTA) for i in (0, 2, 4)]
    assert np.abs(soft - (per_frame[0] + per_frame[1] + per_frame[2])).max() < 1e-9
    assert np.abs(soft - v.payload_soft_frames(gpu_ctx, np.stack([got[i][0] for i in (0, 2, 4)]), order, offs, n_bits, DELTA, batch=3)).max() < 1e-9
    # every marked frame is the restatement's within 1 LSB
    bits = P.payload_frame(b"id")
    for i in (0, 2, 4):
        assert np.abs(got[i][0].astype(int) - pr.embed_ref(ys[i], bits[tbi], DELTA)["stego"].astype(int)).max() <= 1
    # the meta: the video layout, and the same size whatever the frame count
    assert os.path.getsize(metap) < 1024
    assert list(M.load_payload_meta(metap)) == ["mode", "payload_type", "shape", "delta", "payload_bits", "nonce", "tile",
                                          "frame_interval", "n_frames", "digest"]
    src2 = str(tmp_path / "in2.y4m")
    v.write_y4m(src2, ys[:2], chroma[:2], chroma_tag="420")
    v.embed_payload_video(src2, b"id", str(tmp_path / "out2.y4m"), str(tmp_path / "vm2.npz"), password="pw", payload_type="bytes",
                          frame_interval=2, nonce=bytes(8), batch=2)
    assert os.path.getsize(metap) == os.path.getsize(str(tmp_path / "vm2.npz"))
    with pytest.raises(ValueError, match=M.WRONG_PASSWORD):
        v.extract_payload_video(outp, metap, password="nope")
    with pytest.raises(ValueError):
        v.extract_watermark_video(outp, metap, str(tmp_path / "w.png"), password="pw")
