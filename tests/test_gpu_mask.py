"""Texture-masked strength on the device: the gain pass, the masked embed / extract / detect kernels, the drop-in and the
video functions, each against the unchanged oracle composed with the rule (tests/mask_refs.py).  The hosts are 64 x 64 (one
wave) and 72 x 100 (108 tiles: a partial wave and a ragged right edge); every regime of the gain has at least 9 tiles there,
every tile with g > 0 is full rank, and the rank-deficient ones have g = 0 (only their well-defined leading pair moves), so
no tile is left out of any comparison."""
import importlib

import numpy as np
import pytest

import mask_refs as mr
from conftest import PKG_NAME
from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

SIGMA_RTOL = 1e-4
LO, HI, CUT = mr.MASK
SIZES = [(64, 64), (72, 100)]
M = importlib.import_module(PKG_NAME + ".meta")


@pytest.fixture(scope="module", autouse=True)
def _preconditions():
    for H, W, seed in mr.HOSTS:
        mr.check_preconditions(mr.cover_sigma(H, W, seed))


@pytest.fixture(scope="module")
def masked3(gpu_ctx):
    """(planes, watermark, stego, Sc) per size: three planes masked-embedded on the device with one shared watermark"""
    out = {}
    for H, W in SIZES:
        planes = mr.planes_of(H, W, 3)
        wm = mr.watermark(H, W)
        st, sc, _ = gpu_ctx.embed_tiles(planes, wm[2], mr.ALPHA, mask=mr.MASK)
        st.setflags(write=False); sc.setflags(write=False)
        out[H, W] = (planes, wm, st, sc)
    return out


# ---- 1. the gain pass -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_mask_gain_tiles_against_numpy(gpu_ctx, H, W):
    """The < 1e-5 bar holds the FORMULA: NumPy applied to the singular values the device's own sigma pass leaves (the same
    device path as the gain pass, so its sigma error cancels).  The sigma path itself is held against the oracle's Sc by the
    looser bound SIGMA_RTOL allows (about 5e-3 in g here), and tightly, through the stego, by the embed tests below."""
    planes = mr.planes_of(H, W, 3)
    g = gpu_ctx.mask_gain_tiles(planes, LO, HI)
    assert g.shape == (3, H // 8, W // 8) and g.dtype == np.float32
    # the formula: NumPy on the singular values the same device path leaves
    S = gpu_ctx.sigma_tiles(planes)
    assert np.abs(g - M.mask_gain(S, LO, HI)).max() < 1e-5
    # against the oracle's Sc: each of the seven values may be off by SIGMA_RTOL s_1, so r by sqrt(7) of that
    So = np.stack([o.stego_sigma(p.astype(np.float32), 8) for p in planes])
    assert np.abs(g - mr.gain(So, LO, HI)[0]).max() < np.sqrt(7.0) * SIGMA_RTOL * So[..., 0].max() / (HI - LO)
    # one plane, and planes that are a strided, unaligned window of a larger array: the same values
    assert np.array_equal(gpu_ctx.mask_gain_tiles(planes[1], LO, HI), g[1])
    big = np.zeros((3, H + 5, W + 13), np.uint8)
    big[:, 3:3 + H, 5:5 + W] = planes
    assert np.array_equal(gpu_ctx.mask_gain_tiles(big[:, 3:3 + H, 5:5 + W], LO, HI), g)


# ---- 2. masked embed against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("case", ["one_plane", "three_shared", "three_per_plane"])
def test_masked_embed_against_the_oracle(gpu_ctx, case, H, W):
    """Sc within SIGMA_RTOL and stego within 1 LSB of oracle.embed_plane fed G o Sw: hard conditions.  The share of
    differing pixels and max |Yw - Yw_oracle| are held to max(the bar of test_embed_parity [2e-3, 3e-2], 2 x the figure the
    UNCHANGED uniform path shows against the uniform oracle on the same planes): nobody had measured the existing kernel on
    such low-contrast tiles, the masked perturbation is never larger than the uniform one, and the factor 2 is for another
    rounding draw.  (Observed: profiles/mask_bench.json.)"""
    planes = mr.planes_of(H, W, 1 if case == "one_plane" else 3)
    wms = [mr.watermark(H, W, 9 + p) for p in range(3)] if case == "three_per_plane" else mr.watermark(H, W)
    fig = mr.embed_figures(gpu_ctx, planes, wms)
    print(case, H, W, fig)
    uni, msk = fig["uniform"], fig["masked"]
    assert msk["sigma_rel"] < SIGMA_RTOL
    assert msk["max_lsb"] <= 1
    assert msk["share"] < max(2e-3, 2 * uni["share"])
    assert msk["max_dyw"] < max(3e-2, 2 * uni["max_dyw"])


def test_masked_embed_differs_from_uniform_where_it_should(gpu_ctx, masked3):
    """g = 1 tiles are the uniform embed bit for bit, g < 1 tiles are not it (so the tests above cannot pass on the uniform
    path), and the rows and columns outside the tile grid pass through."""
    planes, wm, st, sc = masked3[72, 100]
    st_u, sc_u, _ = gpu_ctx.embed_tiles(planes, wm[2], mr.ALPHA)
    assert np.array_equal(sc, sc_u)                                         # Sc is the cover's either way
    g = gpu_ctx.mask_gain_tiles(planes, LO, HI)
    same = np.stack([np.all(o.to_tiles(a) == o.to_tiles(b), axis=(-2, -1)) for a, b in zip(st, st_u)])
    assert same[g == 1].all() and not same[g < 0.5].any()
    assert np.array_equal(st[:, :, 96:], planes[:, :, 96:])


# ---- 3. pass-through identity ---------------------------------------------------------------------------------------
class _Dev:
    """device buffers of one test, freed together"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, arr):
        d = self.ctx.malloc(max(arr.nbytes, 16)); self.bufs.append(d)
        self.ctx.h2d(d, arr)
        return d

    def get(self, d, shape, dtype):
        out = np.empty(shape, dtype)
        self.ctx.d2h(out, d)
        return out

    def close(self):
        for d in self.bufs:
            self.ctx.free(d)


@pytest.mark.parametrize("layout", ["dense_1", "dense_3", "strided_3", "unaligned_3", "in_place_3", "in_place_unaligned_1"])
def test_pass_through_identity(gpu_ctx, layout):
    """On a uniform-random host (every tile has r > 0) lo = 0, hi = 1e-6 gives g = 1 everywhere: the masked embed must be
    the uniform embed bit for bit, in stego (every byte of the buffer, the gaps between rows and planes included) and in Sc.
    Any addressing slip of the gain kernel - tile address, strides, the sigma_w stride, a partial wave - shows here."""
    H, W, alpha = 72, 100, 0.15
    # planes, offset of the first sample, row stride, gap between planes.  Rows of 128 with 64-byte gaps take the aligned
    # byte path, everything else (W = 100 is no multiple of 8) the unaligned one.
    n, off, rs, gap = {"dense_1": (1, 0, W, 0), "dense_3": (3, 0, W, 0), "strided_3": (3, 0, 128, 64),
                       "unaligned_3": (3, 3, W + 5, 37), "in_place_3": (3, 0, 128, 64),
                       "in_place_unaligned_1": (1, 3, W + 5, 0)}[layout]
    ps = rs * H + gap
    in_place = layout.startswith("in_place")
    per_plane = layout in ("strided_3", "in_place_3")                       # sigma_w per plane there, shared elsewhere
    span = off + (n - 1) * ps + (H - 1) * rs + W
    rng = np.random.default_rng(21)
    buf = rng.integers(0, 256, span + 16, dtype=np.uint8)
    filler = rng.integers(0, 256, span + 16, dtype=np.uint8)
    nt = (H // 8) * (W // 8)
    sw = np.stack([mr.watermark(H, W, 9 + p)[2] for p in range(n if per_plane else 1)])
    dev = _Dev(gpu_ctx)
    try:
        d_sw = dev.put(sw)
        results = []
        for masked in (False, True):
            d_host = dev.put(buf)
            d_stego = d_host if in_place else dev.put(filler)
            d_sc = dev.put(np.zeros((n, nt, 8), np.float32))
            args = (d_host + off, d_sw, d_stego + off, d_sc, 0, n, H, W, rs, ps, nt * 8 if per_plane else 0, alpha, 8)
            if masked:
                gpu_ctx.embed_tiles_masked_u8_dev(*args, 0.0, 1e-6)
            else:
                gpu_ctx.embed_tiles_u8_dev(*args)
            gpu_ctx.check_status()
            results.append((dev.get(d_stego, buf.shape, np.uint8), dev.get(d_sc, (n, nt, 8), np.float32),
                            dev.get(d_host, buf.shape, np.uint8)))
        (st_u, sc_u, host_u), (st_m, sc_m, host_m) = results
    finally:
        dev.close()
    assert np.array_equal(st_m, st_u) and np.array_equal(sc_m, sc_u)
    assert not np.array_equal(st_u, buf if in_place else filler)            # something was embedded
    if not in_place:
        assert np.array_equal(host_m, buf) and np.array_equal(host_u, buf)  # the host planes are only read


# ---- 4. masked extract ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("K", [8, 3])
def test_masked_extract_against_the_restatement(gpu_ctx, masked3, H, W, K):
    """Float output within 2e-2 / cut of from_tiles(_idct_tiles(Uw diag(sw_hat) Vwt)) - the 2e-2 of
    test_sigma_extract_detect_parity scaled by the largest 1 / g; the unscrambled uint8 output within 1 level."""
    planes, wm, st, sc = masked3[H, W]
    _, Uw, Sw, Vwt = wm
    want = np.stack([mr.extract_ref(st[p], sc[p], Uw, Vwt, mr.ALPHA, mr.MASK, K) for p in range(3)])
    got = gpu_ctx.extract_tiles(st, sc, Uw, Vwt, mr.ALPHA, K, mask=mr.MASK)
    err = float(np.abs(got - want).max())
    s = gpu_ctx.extract_tiles(st, sc, Uw, Vwt, mr.ALPHA, K, sum_planes=True, mask=mr.MASK)
    err_sum = float(np.abs(s - want.sum(0)).max())
    one = gpu_ctx.extract_tiles(st[1], sc[1], Uw, Vwt, mr.ALPHA, K, mask=mr.MASK)
    print(f"extract {H}x{W} K={K}: max |d| {err:.2e}, sum of 3 planes {err_sum:.2e}")
    assert got.shape == (3, H, W) and err < 2e-2 / CUT
    assert s.shape == (H, W) and err_sum < 2e-2 / CUT
    assert np.array_equal(one, got[1])
    assert np.all(got[:, :, (W // 8) * 8:] == 0)                             # outside the tile grid
    # it is the masked rule: the plain rule's estimate is another one wherever 0 < g < 1
    assert np.abs(gpu_ctx.extract_tiles(st, sc, Uw, Vwt, mr.ALPHA, K) - want).max() > 1.0
    idx = o.permutation(H, W, o.rng_from_key(o.derive_key("mask", bytes(8))))
    for normalize in (True, False):
        u8 = gpu_ctx.extract_tiles_unscrambled_u8(st, sc, Uw, Vwt, mr.ALPHA, K, idx, normalize, mask=mr.MASK)
        ref = np.stack([mr.to_u8(o.unpermute(w, idx), normalize) for w in want])
        assert u8.dtype == np.uint8 and np.abs(u8.astype(int) - ref.astype(int)).max() <= 1
    # per-plane factors take the same path
    Uw3, Vwt3 = np.stack([Uw] * 3), np.stack([Vwt] * 3)
    assert np.array_equal(gpu_ctx.extract_tiles(st, sc, Uw3, Vwt3, mr.ALPHA, K, mask=mr.MASK), got)


@pytest.mark.parametrize("normalize", [True, False])
def test_masked_extract_unscrambled_without_a_route(gpu_ctx, masked3, monkeypatch, normalize):
    """extract_tiles_unscrambled_u8 on a plane no route addresses (more than ROUTE_MAX_N pixels; forced here by lowering the
    bound on this context): extract kernel and unscramble run apart, masked as unmasked, and give the routed chain's bytes."""
    H, W = 72, 100
    planes, wm, st, sc = masked3[H, W]
    _, Uw, Sw, Vwt = wm
    # an index of this case's own: the context keeps a route with the device copy of every index it has routed
    idx = o.permutation(H, W, o.rng_from_key(o.derive_key(f"no route {normalize}", bytes(8))))
    with monkeypatch.context() as mp:
        mp.setattr(gpu_ctx, "ROUTE_MAX_N", 0, raising=False)
        assert gpu_ctx.route_dev(idx) is None
        got = gpu_ctx.extract_tiles_unscrambled_u8(st, sc, Uw, Vwt, mr.ALPHA, 8, idx, normalize, mask=mr.MASK)
        one = gpu_ctx.extract_tiles_unscrambled_u8(st[0], sc[0], Uw, Vwt, mr.ALPHA, 8, idx, normalize, mask=mr.MASK)
        plain = gpu_ctx.extract_tiles_unscrambled_u8(st, sc, Uw, Vwt, mr.ALPHA, 8, idx, normalize)
    assert gpu_ctx.route_dev(idx) is not None                               # the bound is back: the same index, routed
    routed = gpu_ctx.extract_tiles_unscrambled_u8(st, sc, Uw, Vwt, mr.ALPHA, 8, idx, normalize, mask=mr.MASK)
    want = np.stack([mr.to_u8(o.unpermute(mr.extract_ref(st[p], sc[p], Uw, Vwt, mr.ALPHA, mr.MASK), idx), normalize)
                     for p in range(3)])
    assert got.shape == (3, H, W) and got.dtype == np.uint8
    assert np.array_equal(got, routed) and np.array_equal(one, got[0])
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    assert np.array_equal(plain, gpu_ctx.extract_tiles_unscrambled_u8(st, sc, Uw, Vwt, mr.ALPHA, 8, idx, normalize))
    assert not np.array_equal(plain, got)


def test_masked_extract_pixel_domain_factors(gpu_ctx, masked3):
    """wm_extract_tiles_px_masked_u8_dev: the same estimate from pixel-domain factors, to float32 rounding"""
    H, W = 72, 100
    planes, wm, st, sc = masked3[H, W]
    _, Uw, Sw, Vwt = wm
    want = gpu_ctx.extract_tiles(st, sc, Uw, Vwt, mr.ALPHA, 8, mask=mr.MASK)
    nt = (H // 8) * (W // 8)
    dev = _Dev(gpu_ctx)
    try:
        d_st, d_sc, d_u, d_v = (dev.put(np.ascontiguousarray(x)) for x in (st, sc, Uw, Vwt))
        d_out = dev.put(np.zeros((3, H, W), np.float32))
        gpu_ctx.tile_factors_to_pixel_dev(d_u, d_v, d_u, d_v, nt)
        gpu_ctx._call("wm_extract_tiles_px_masked_u8_dev", d_st, d_sc, d_u, d_v, d_out, 3, H, W, W, H * W, 0, mr.ALPHA, 8,
                      LO, HI, CUT)
        gpu_ctx.check_status()
        got = dev.get(d_out, (3, H, W), np.float32)
    finally:
        dev.close()
    assert np.abs(got - want).max() < 2e-2 / CUT


# ---- 5. masked detect -----------------------------------------------------------------------------------------------
def test_masked_detect(gpu_ctx, masked3):
    for H, W in SIZES:
        planes, wm, st, sc = masked3[H, W]
        scores = gpu_ctx.detect_tiles(st, sc, wm[2], mr.ALPHA, mask=mr.MASK)
        want = [mr.detect_ref(st[p], sc[p], wm[2], mr.ALPHA, mr.MASK) for p in range(3)]
        print(f"detect {H}x{W}: {scores} restatement {want}")
        assert scores.shape == (3,) and np.abs(scores - want).max() < 1e-4
        assert abs(float(gpu_ctx.detect_tiles(st[2], sc[2], wm[2], mr.ALPHA, mask=mr.MASK)[0]) - scores[2]) < 1e-12
        per_plane = gpu_ctx.detect_tiles(st, sc, np.stack([wm[2]] * 3), mr.ALPHA, mask=mr.MASK)
        assert np.array_equal(per_plane, scores)
    # 72 x 100, seed 1: the masked rule reads what the masked embed wrote; the plain rule reads it worse
    planes, wm, st, sc = masked3[72, 100]
    masked = float(gpu_ctx.detect_tiles(st[0], sc[0], wm[2], mr.ALPHA, mask=mr.MASK)[0])
    plain = float(gpu_ctx.detect_tiles(st[0], sc[0], wm[2], mr.ALPHA)[0])
    print(f"masked stego of 72x100 seed 1: masked rule {masked:.4f}, plain rule {plain:.4f}")
    assert masked > 0.99 and plain < masked
    # A stego made from another image - unrelated content, carrying the SAME watermark by the same rule - against seed 1's
    # meta: what it shares with the meta is the watermark alone, and without the cover's own Sc that is not enough.
    # ("Another image" is other content.  A second noise draw of the same host recipe is, to this statistic, nearly the same
    # image: the NC of single:284-289 runs over sorted singular values, whose profile - one large value and seven small
    # ones per tile - any marked tile shares.  The oracle scores the seed-2 stego 0.93 - 0.95 against seed 1's meta by the
    # masked rule and 0.91 - 0.92 by the plain one, and in the uniform path another watermark in the same cover 0.988: a
    # property of the reference's detector that masking neither causes nor cures; printed below, not asserted.)
    unrelated = np.random.default_rng(77).integers(0, 256, (72, 100), dtype=np.uint8)
    other, _, _ = gpu_ctx.embed_tiles(unrelated, wm[2], mr.ALPHA, mask=mr.MASK)
    s_other = float(gpu_ctx.detect_tiles(other, sc[0], wm[2], mr.ALPHA, mask=mr.MASK)[0])
    s_seed2 = float(gpu_ctx.detect_tiles(st[1], sc[0], wm[2], mr.ALPHA, mask=mr.MASK)[0])
    print(f"against seed 1's meta: stego of an unrelated image {s_other:.4f}, of the seed-2 host {s_seed2:.4f}")
    assert abs(s_other - mr.detect_ref(other, sc[0], wm[2], mr.ALPHA, mr.MASK)) < 1e-4
    assert s_other < 0.6
    assert float(gpu_ctx.detect_tiles(planes[0], sc[0], wm[2], mr.ALPHA, mask=mr.MASK)[0]) < 0.6      # the unmarked cover


# ---- 6. drop-in -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [False, True], ids=["gray_72x100", "colour_64x64"])
def test_dropin_round_trip(gpu_ctx, color):
    import dct_svd_core_secure as core
    H, W = (64, 64) if color else (72, 100)
    planes = mr.planes_of(H, W, 3)
    # gray: a cover whose three channels are the host - its Y plane IS the host, and B = G = R = Y on the way back
    cover = np.ascontiguousarray(np.moveaxis(planes, 0, -1)) if color else np.stack([planes[0]] * 3, axis=-1)
    wm = np.random.default_rng(31).integers(0, 256, (H, W, 3), dtype=np.uint8)
    nonce = bytes(range(8))
    idx = o.permutation(H, W, o.rng_from_key(o.derive_key("pw", nonce)))
    r = core.embed_arrays(cover, wm, "pw", nonce, alpha=mr.ALPHA, color=color, strength="masked")
    meta = r["meta"]
    keys = list(meta)
    assert keys[keys.index("k_floor") + 1] == "mask" and M.mask_of(meta) == mr.MASK
    chans = range(3) if color else [0]
    wys = [o.permute((wm[..., c] if color else o.bgr_to_gray(wm)).astype(np.float32), idx) for c in chans]
    names = [("S" + n, "UW" + n, "VW" + n + "t") for n in "bgr"] if color else [("Sc", "Uw", "Vwt")]
    want_wm = []
    for c, w, (ks, ku, kv) in zip(chans, wys, names):
        ref = mr.embed_ref(cover[..., c], (w,) + tuple(o.watermark_decompose(w, 8)), mr.ALPHA, mr.MASK)
        assert np.abs(r["stego"][..., c].astype(int) - ref["stego"].astype(int)).max() <= 1
        assert mr.rel_sigma(meta[ks], ref["Sc"]) < SIGMA_RTOL
        est = mr.extract_ref(r["stego"][..., c], meta[ks], meta[ku], meta[kv], mr.ALPHA, mr.MASK)
        want_wm.append(mr.to_u8(o.unpermute(est, idx)))
    if not color:
        assert np.array_equal(r["stego"][..., 0], r["stego"][..., 1]) and np.array_equal(r["stego"][..., 0], r["stego"][..., 2])
    ok, score = core.detect_arrays(r["stego"], meta)
    print("drop-in", "colour" if color else "gray", "score", score)
    assert ok
    ex = core.extract_arrays(r["stego"], meta, "pw")
    want = np.stack(want_wm, axis=-1) if color else want_wm[0]
    assert ex.shape == want.shape and np.abs(ex.astype(int) - want.astype(int)).max() <= 1
    # the same calls with the default strength: a meta without the member, read by the plain rule
    r0 = core.embed_arrays(cover, wm, "pw", nonce, alpha=mr.ALPHA, color=color)
    assert "mask" not in r0["meta"] and M.mask_of(r0["meta"]) is None
    assert [k for k in keys if k != "mask"] == list(r0["meta"])
    assert not np.array_equal(r0["stego"], r["stego"])
    assert core.detect_arrays(r0["stego"], r0["meta"])[0]


# ---- 7. video -------------------------------------------------------------------------------------------------------
def _frames_luma(n, H, W):
    return np.stack([mr.host(H, W, 40 + i) for i in range(n)])


def _frames_444(n, H, W):
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:H, 0:W]
    ys, chroma = [], []
    for i in range(n):          # a smooth colourful clip with sensor noise (random chroma would leave the BGR gamut)
        b = 90 + 60 * np.sin((xx + 3 * i) / 11.0) + rng.normal(0, 8, (H, W))
        g = 120 + 50 * np.cos((yy - 2 * i) / 7.0) + rng.normal(0, 8, (H, W))
        r = 100 + 40 * np.sin((xx + yy) / 13.0) + rng.normal(0, 8, (H, W))
        ycc = o.bgr_to_ycrcb(np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8))
        ys.append(ycc[..., 0]); chroma.append(np.concatenate([ycc[..., 2].ravel(), ycc[..., 1].ravel()]))
    return np.stack(ys), np.stack(chroma)


@pytest.mark.parametrize("color", [False, True], ids=["luma", "colour_444"])
def test_video_masked(gpu_ctx, tmp_path, color):
    v = importlib.import_module(PKG_NAME + ".video")
    hg = importlib.import_module(PKG_NAME + ".hostglue")
    n, H, W, alpha = 3, 48, 64, 0.15
    src, outp, metap = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "vm.npz")
    if color:
        ys, chroma = _frames_444(n, H, W)
        v.write_y4m(src, ys, chroma, chroma_tag="444")
    else:
        v.write_y4m(src, _frames_luma(n, H, W))
    wm = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    wp = str(tmp_path / "wm.png"); assert hg.write_png(wp, wm)
    embed, detect, extract = ((v.embed_watermark_video_color, v.detect_watermark_video_color, v.extract_watermark_video_color)
                              if color else (v.embed_watermark_video, v.detect_watermark_video, v.extract_watermark_video))
    embed(src, wp, outp, metap, alpha=alpha, password="pw", nonce=bytes(8), batch=2, strength="masked")
    data = np.load(metap, allow_pickle=False)
    keys = list(data.files)
    assert keys[keys.index("k_floor") + 1] == "mask" and M.mask_of(data) == mr.MASK
    ok, mean, scores = detect(outp, metap)
    print("video", "colour" if color else "luma", "per-frame scores", scores)
    assert ok and scores.shape == (n,) and scores.min() > 0.9
    wout = extract(outp, metap, str(tmp_path / "w.png"), password="pw")
    ex = hg.read_image_bgr(wout)
    # the restatement: every stored frame's planes by the rule, the plain mean over frames, unscramble, normalise
    idx = o.permutation(H, W, o.rng_from_key(o.derive_key("pw", bytes(8))))
    vid = v.Y4M(outp); got = [(y.copy(), c.copy()) for _, y, c in vid]; vid.close()
    if color:
        stored = [np.moveaxis(o.ycrcb_to_bgr(np.stack([y, c[H * W:].reshape(H, W), c[:H * W].reshape(H, W)], axis=-1)), -1, 0)
                  for y, c in got]
        names = [("S" + k, "UW" + k, "VW" + k + "t") for k in "bgr"]
    else:
        stored = [y[None] for y, _ in got]
        names = [("Sc", "Uw", "Vwt")]
    for ch, (ks, ku, kv) in enumerate(names):
        est = np.mean([mr.extract_ref(stored[i][ch], data[ks][i], data[ku], data[kv], alpha, mr.MASK) for i in range(n)],
                      axis=0, dtype=np.float64).astype(np.float32)
        want = mr.to_u8(o.unpermute(est, idx))
        assert np.abs(ex[..., ch].astype(int) - want.astype(int)).max() <= 1
    # the same call with the default strength writes the meta it always wrote
    embed(src, wp, str(tmp_path / "out0.y4m"), str(tmp_path / "vm0.npz"), alpha=alpha, password="pw", nonce=bytes(8), batch=2)
    assert [k for k in keys if k != "mask"] == list(np.load(str(tmp_path / "vm0.npz"), allow_pickle=False).files)
