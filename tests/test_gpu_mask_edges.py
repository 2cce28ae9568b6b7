"""Texture-masked strength on the device, at its edges: black and constant tiles (letterbox bars), rank-deficient tiles
with 0 < g < 1 (JPEG-quantised and posterised content, hand-made rank classes), off-default rules, K < 8 in the embed, tiles
on the edge of `cut`, and a detect of more than 256 waves.  The references are the unchanged oracle composed with the rule
and the rule with every operation rounded once to float32 (tests/mask_refs.py); what the comparisons assume of the hosts is
asserted on the CPU in tests/test_mask.py.

Measured on an MI355X (the prints of this module):
  * the gain pass equals gain_exact of the device's own singular values bit for bit on every host under every rule;
  * the largest |g_embed - g_reader| (the gain pass on the cover against gain_exact of the Sc the embed returned), over
    all seven hosts: 2.1e-7 for (8, 64, 0.25), 1.4e-5 for (0, 16, 0.05), 4.8e-7 for (2, 2.5, 1.0), 3.6e-43 for (8, 3e38, 0.25);
  * the masked extract at cut = 0.05 stays within 1.8e-3 of the restatement (bar 2e-2 / cut = 0.4);
  * on the build before the black-tile repair a black tile came out as a blob of 24 to 28 non-zero pixels up to 64 grey
    levels, up to 46 levels from the oracle's flat tile, and sigma_1 read back 64 % of what was embedded (worst miss 438
    against the bar of 67; 66 with the repair).
"""
import importlib

import numpy as np
import pytest
import scipy.fft

import mask_refs as mr
import payload_refs as pr
from conftest import PKG_NAME
from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

SIGMA_RTOL = 1e-4
ALPHA = mr.ALPHA
M = importlib.import_module(PKG_NAME + ".meta")


def _ptp(tiles):
    return tiles.max((-1, -2)).astype(np.float64) - tiles.min((-1, -2))


def _tiles(planes):
    return np.stack([o.to_tiles(p) for p in planes])


# ---- B. black and constant tiles ------------------------------------------------------------------------------------
def _constant_cases():
    lb, cb = pr.letterbox_planes(), mr.constant_batch()
    # the letterbox planes share one watermark; the batch has one per plane (sw_1 is a tile's own row under the per-plane stride)
    return {"letterbox": (lb, [mr.watermark(72, 100)] * 3, mr.watermark(72, 100)[2]),
            "batch": (cb, [mr.watermark(64, 64, 9 + p) for p in range(5)], np.stack([mr.watermark(64, 64, 9 + p)[2] for p in range(5)]))}


@pytest.fixture(scope="module")
def constant_embeds(gpu_ctx):
    """name -> (planes, watermarks per plane, Sw as passed, masked stego, Sc, yw): embedded once on the device"""
    out = {}
    for name, (planes, wms, Sw) in _constant_cases().items():
        st, sc, yw = gpu_ctx.embed_tiles(planes, Sw, ALPHA, K=8, want_yw=True, mask=mr.MASK)
        gpu_ctx.check_status()
        for a in (st, sc, yw):
            a.setflags(write=False)
        out[name] = (planes, wms, Sw, st, sc, yw)
    return out


@pytest.mark.parametrize("name", ["letterbox", "batch"])
def test_black_and_constant_tiles_move_along_the_flat_vector(gpu_ctx, constant_embeds, name):
    """A masked tile with g = 0 is fed (sw_1, 0, .., 0).  A black tile has no leading pair of its own: the masked embed
    gives it the flat vector (what the oracle's SVD of the zero matrix returns), so the bar of a letterboxed frame stays
    flat, within 1 LSB of the oracle composed with the rule, and sigma_1 reads back as embedded.  (With the completion
    pattern's signed leading pair instead, alpha sw_1 = 120 left a blob of 26 non-zero pixels up to 52 grey levels, and
    s^_1 read back 641 of 1000.)  Constant tiles with v > 0 move along e_0 already; Sc is the uniform embed's."""
    planes, wms, Sw, st, sc, yw = constant_embeds[name]
    n, H, W = planes.shape
    Hb, Wb = H // 8 * 8, W // 8 * 8
    _, sc_u, _ = gpu_ctx.embed_tiles(planes, Sw, ALPHA)
    assert np.array_equal(sc, sc_u)                                         # Sc (the meta) does not move
    assert np.isfinite(yw).all() and np.isfinite(sc).all()
    assert np.array_equal(st[:, :Hb, :Wb], np.clip(yw, 0, 255).astype(np.uint8)[:, :Hb, :Wb])
    assert np.array_equal(st[:, :, Wb:], planes[:, :, Wb:]) and np.array_equal(st[:, Hb:], planes[:, Hb:])
    s_st = gpu_ctx.sigma_tiles(st)
    n_black = n_const = n_read = 0
    worst_flat = worst_ref = worst_const = worst_read = 0.0
    for p in range(n):
        black, const = pr.black_tiles(planes[p]), mr.constant_tiles(planes[p])
        ref = mr.embed_ref(planes[p], wms[p])
        t_st, t_ref, t_yw = o.to_tiles(st[p]), o.to_tiles(ref["stego"]), o.to_tiles(yw[p])
        sw1 = wms[p][2][..., 0]
        if black.any():
            n_black += int(black.sum())
            worst_flat = max(worst_flat, float(_ptp(t_st)[black].max()))
            worst_ref = max(worst_ref, float(np.abs(t_st[black].astype(int) - t_ref[black].astype(int)).max()))
            assert np.all(_ptp(t_ref)[black] == 0)                          # the reference's black tiles are flat
        pos = const & ~black
        if pos.any():
            n_const += int(pos.sum())
            d = t_st[pos].astype(int) - o.to_tiles(planes[p])[pos].astype(int)
            worst_const = max(worst_const, float(_ptp(d).max()))
        # sigma_1 read back from the stored tile, where nothing clipped
        inside = const & (t_yw.min((-1, -2)) >= 0) & (t_yw.max((-1, -2)) <= 255)
        if inside.any():
            n_read += int(inside.sum())
            s1_hat = (s_st[p][..., 0].astype(np.float64) - sc[p][..., 0]) / ALPHA
            worst_read = max(worst_read, float(np.abs(s1_hat - sw1)[inside].max()))
    print(f"{name}: {n_black} black tiles, max spread within one {worst_flat:g}, max |stego - oracle| on them {worst_ref:g} LSB; "
          f"{n_const} constant tiles v > 0, max spread of stego - cover {worst_const:g}; sigma_1 read back on {n_read} tiles, "
          f"worst miss {worst_read:.1f} (bar {8 / ALPHA:.1f})")
    assert n_black >= 48 and n_read >= 48
    assert worst_flat == 0
    assert worst_ref <= 1
    assert worst_const <= 1
    assert worst_read <= 8 / ALPHA
    gpu_ctx.check_status()


def test_masked_embed_of_black_tiles_with_small_K(gpu_ctx):
    """K = 0 leaves a black tile untouched; K = 1 moves it as K = 8 does (only sw_1 reaches a g = 0 tile)."""
    planes = pr.letterbox_planes()
    Sw = mr.watermark(72, 100)[2]
    st8, sc8, _ = gpu_ctx.embed_tiles(planes, Sw, ALPHA, K=8, mask=mr.MASK)
    st1, sc1, yw1 = gpu_ctx.embed_tiles(planes, Sw, ALPHA, K=1, want_yw=True, mask=mr.MASK)
    st0, sc0, yw0 = gpu_ctx.embed_tiles(planes, Sw, ALPHA, K=0, want_yw=True, mask=mr.MASK)
    assert np.array_equal(st0, planes) and np.array_equal(yw0, planes.astype(np.float32))
    assert np.array_equal(sc0, sc8) and np.array_equal(sc1, sc8)
    for p in range(3):
        black = pr.black_tiles(planes[p])
        assert np.array_equal(o.to_tiles(st1[p])[black], o.to_tiles(st8[p])[black])
        if black.any():
            want = ALPHA * Sw[..., 0][black] / 8
            assert np.abs(o.to_tiles(yw1[p])[black] - want[:, None, None]).max() < 1e-3
    gpu_ctx.check_status()


@pytest.mark.parametrize("name", ["letterbox", "batch"])
def test_masked_detect_on_black_and_constant_planes(gpu_ctx, constant_embeds, name):
    """Per plane within 1e-4 of the restatement and finite - the all-white plane included, whose stego is its cover (every
    s^ is the same, the variance is 0 and the + 1e-8 of the NC decides) - and no plane bleeds into another."""
    planes, wms, Sw, st, sc, yw = constant_embeds[name]
    n = planes.shape[0]
    scores = gpu_ctx.detect_tiles(st, sc, Sw, ALPHA, mask=mr.MASK)
    want = np.array([mr.detect_ref(st[p], sc[p], wms[p][2], ALPHA, mr.MASK) for p in range(n)])
    print(f"{name}: detect {scores} restatement {want}")
    assert scores.shape == (n,) and np.isfinite(scores).all()
    assert np.abs(scores - want).max() < 1e-4
    if name == "batch":
        assert np.array_equal(st[1], planes[1])                             # white + anything clips back to white
    for p in range(n):
        alone = float(gpu_ctx.detect_tiles(st[p], sc[p], wms[p][2], ALPHA, mask=mr.MASK)[0])
        assert abs(alone - scores[p]) < 1e-12
    gpu_ctx.check_status()


def test_video_masked_letterboxed(gpu_ctx, tmp_path):
    """Three letterboxed 48 x 64 frames (top and bottom tile row black) through embed_watermark_video(strength="masked"):
    the bars of the stored frames are flat per tile, detect says ok, and extract is within 1 level of the restatement."""
    v = importlib.import_module(PKG_NAME + ".video")
    hg = importlib.import_module(PKG_NAME + ".hostglue")
    n, H, W, alpha = 3, 48, 64, 0.15
    frames = np.stack([mr.host(H, W, 40 + i) for i in range(n)])
    frames[:, :8] = 0; frames[:, 40:] = 0
    src, outp, metap = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "vm.npz")
    v.write_y4m(src, frames)
    wm = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    wp = str(tmp_path / "wm.png"); assert hg.write_png(wp, wm)
    v.embed_watermark_video(src, wp, outp, metap, alpha=alpha, password="pw", nonce=bytes(8), batch=2, strength="masked")
    data = np.load(metap, allow_pickle=False)
    assert M.mask_of(data) == mr.MASK
    vid = v.Y4M(outp); stored = [y.copy() for _, y, _ in vid]; vid.close()
    for i, y in enumerate(stored):
        t = o.to_tiles(y)
        bars = pr.black_tiles(frames[i])
        assert bars.sum() == 16 and np.all(_ptp(t)[bars] == 0)
        want = np.clip(alpha * data["Sw"][..., 0] / 8, 0, 255).astype(np.uint8)       # the flat vector, truncated
        assert np.abs(t[bars][:, 0, 0].astype(int) - want[bars].astype(int)).max() <= 1
    ok, mean, scores = v.detect_watermark_video(outp, metap)
    print("letterboxed video: per-frame scores", scores)
    assert ok and scores.shape == (n,)
    ex = hg.read_image_bgr(v.extract_watermark_video(outp, metap, str(tmp_path / "w.png"), password="pw"))
    idx = o.permutation(H, W, o.rng_from_key(o.derive_key("pw", bytes(8))))
    est = np.mean([mr.extract_ref(stored[i], data["Sc"][i], data["Uw"], data["Vwt"], alpha, mr.MASK) for i in range(n)],
                  axis=0, dtype=np.float64).astype(np.float32)
    want = mr.to_u8(o.unpermute(est, idx))
    assert np.abs(ex[..., 0].astype(int) - want.astype(int)).max() <= 1
    gpu_ctx.check_status()


# ---- C. flagged tiles with g > 0, off-default rules, K < 8 ----------------------------------------------------------
_HOSTS = [f"{k}_{s}" for k in ("quantised", "posterised", "natural") for s in ("64x64", "72x100")] + ["handmade_64x64"]
_G_SPREAD = {}                                                             # rule -> largest |g_embed - g_reader| seen


def _embed_checks(host, wm, G, K, st, sc, yw, label):
    """the bars of tests/test_gpu_scaled_rotation.py against the oracle fed G o Sw with the first K values"""
    wys, Uw, Sw, Vwt = wm
    H, W = host.shape
    Hb, Wb = H // 8 * 8, W // 8 * 8
    eff = (Sw * G).astype(np.float32)
    ref = o.embed_plane(host.astype(np.float32), wys, ALPHA, kfrac=0.0, tile=8, k_floor=K, wm_svd=(Uw, eff, Vwt))
    assert ref["K"] == K
    d = o.to_tiles(np.abs(st.astype(np.int32) - ref["stego"].astype(np.int32))).max((-1, -2))
    S = np.linalg.svd(o.to_tiles(host).astype(np.float64), compute_uv=False)
    gaps = np.min(-np.diff(S, axis=-1) / np.maximum(S[..., :1], 1e-30), axis=-1)
    unique = (S[..., 7] > 1e-9 * S[..., 0]) & (gaps > 1e-4)
    got = np.linalg.svd(o.to_tiles(yw).astype(np.float64), compute_uv=False)
    add = ALPHA * eff.astype(np.float64)
    add[..., K:] = 0
    want = np.sort(sc.astype(np.float64) + add, axis=-1)[..., ::-1]
    svd_err = float(np.max(np.abs(got - want) / np.maximum(want[..., :1], 1.0)))
    sc_err = mr.rel_sigma(sc, ref["Sc"])
    print(f"{label} K={K}: {int(unique.sum())} of {unique.size} tiles with unique vectors, stego max "
          f"{int(d[unique].max()) if unique.any() else 0} LSB on them ({int(d.max())} on all), Sc {sc_err:.2e} s_1, "
          f"svd(Yw) {svd_err:.2e} s_1")
    assert not unique.any() or d[unique].max() <= 1
    assert np.isfinite(yw).all() and np.array_equal(st[:Hb, :Wb], np.clip(yw, 0, 255).astype(np.uint8)[:Hb, :Wb])
    assert svd_err < 5e-4
    assert sc_err < SIGMA_RTOL
    assert np.array_equal(st[Hb:], host[Hb:]) and np.array_equal(st[:, Wb:], host[:, Wb:])


@pytest.mark.parametrize("rule", mr.RULES, ids=["-".join(f"{x:g}" for x in r) for r in mr.RULES])
@pytest.mark.parametrize("name", _HOSTS)
def test_flagged_tiles_and_off_default_rules(gpu_ctx, name, rule):
    lo, hi, cut = rule
    host = mr.flagged_hosts()[name]
    H, W = host.shape
    wm = mr.watermark(H, W)
    _, Uw, Sw, Vwt = wm
    label = f"{name} ({lo:g}, {hi:g}, {cut:g})"
    # 1. the gain pass: the formula bit for bit on the device's own singular values; the oracle's g within the sigma bound
    g = gpu_ctx.mask_gain_tiles(host, lo, hi)
    S_dev = gpu_ctx.sigma_tiles(host)
    g_exact = mr.gain_exact(S_dev, lo, hi)
    n_diff = int((g.view(np.uint32) != g_exact.view(np.uint32)).sum())
    So = mr.flagged_sigma(name)
    bound = np.sqrt(7.0) * SIGMA_RTOL * float(So[..., 0].max()) / (np.float32(hi) - np.float32(lo))
    print(f"{label}: gain pass differs from gain_exact on {n_diff} tiles (max {np.abs(g - g_exact).max():.2e}); against the "
          f"oracle's g {np.abs(g - mr.gain(So, lo, hi)[0]).max():.2e} (bound {bound:.2e})")
    assert n_diff == 0
    assert np.abs(g - mr.gain(So, lo, hi)[0]).max() < bound
    # 2. the embed against the oracle fed G o Sw, G from the device's g (for hi - lo = 0.5 the sigma tolerance alone moves
    #    g by up to 0.5: the oracle's own g is no reference there)
    G = np.ones(Sw.shape, np.float32)
    G[..., 1:] = g[..., None]
    st, sc, yw = gpu_ctx.embed_tiles(host, Sw, ALPHA, K=8, want_yw=True, mask=rule)
    _embed_checks(host, wm, G, 8, st, sc, yw, label)
    # the reader's g, from the Sc the embed returned
    g_reader = mr.gain_exact(sc, lo, hi)
    spread = float(np.abs(g - g_reader).max())
    _G_SPREAD[rule] = max(_G_SPREAD.get(rule, 0.0), spread)
    print(f"{label}: |g_embed - g_reader| max {spread:.2e} (largest so far under this rule {_G_SPREAD[rule]:.2e})")
    assert np.abs(g_reader - mr.gain(So, lo, hi)[0]).max() < bound
    # 3. extract against the restatement on the device's own stego and Sc
    for K in (8, 3):
        want = mr.extract_ref(st, sc, Uw, Vwt, ALPHA, rule, K)
        got = gpu_ctx.extract_tiles(st, sc, Uw, Vwt, ALPHA, K, mask=rule)
        err = float(np.abs(got - want).max())
        print(f"{label}: extract K={K} max |d| {err:.2e} (bar {2e-2 / cut:.2e})")
        assert err < 2e-2 / cut
    # 4. detect
    score = float(gpu_ctx.detect_tiles(st, sc, Sw, ALPHA, mask=rule)[0])
    want = mr.detect_ref(st, sc, Sw, ALPHA, rule)
    print(f"{label}: detect {score:.6f} restatement {want:.6f}")
    assert np.isfinite(score) and abs(score - want) < 1e-4
    # 5. K in the embed: K = 1 and K = 0 are the uniform embed byte for byte (G only scales the values from the second on;
    #    these hosts hold no black tile), K = 3 goes against the oracle
    for K in (1, 0):
        st_m, sc_m, yw_m = gpu_ctx.embed_tiles(host, Sw, ALPHA, K=K, want_yw=True, mask=rule)
        st_u, sc_u, yw_u = gpu_ctx.embed_tiles(host, Sw, ALPHA, K=K, want_yw=True)
        assert np.array_equal(st_m, st_u) and np.array_equal(sc_m, sc_u) and np.array_equal(yw_m, yw_u)
    assert np.array_equal(st_m, host)                                       # K = 0 embeds nothing
    st3, sc3, yw3 = gpu_ctx.embed_tiles(host, Sw, ALPHA, K=3, want_yw=True, mask=rule)
    _embed_checks(host, wm, G, 3, st3, sc3, yw3, label)
    gpu_ctx.check_status()


# ---- D. the edge of `cut` --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", mr.RULES[:2], ids=["-".join(f"{x:g}" for x in r) for r in mr.RULES[:2]])
def test_tiles_on_the_edge_of_cut(gpu_ctx, rule):
    """128 synthetic sigma_c rows within 3e-7 of `cut` (mask_refs.near_cut_rows; 72 of them put on different sides by the
    exact fused sum and by a pairwise sum) against a noise stego, Uw = Vwt = I, K = 2: the forward DCT of an output tile is
    diag(s^_1, s^_2, 0, ..), so s^_2 shows whether the device carried the tile and by which g.  The device's mask_keep must
    agree with carried_exact on every row, and the detect score with the restatement over that carried set (which the
    pairwise set misses by more than 1e-3: asserted on the CPU)."""
    lo, hi, cut = rule
    sc, stego, Sw, score_exact, score_pairwise = mr.near_cut_case(lo, hi, cut)
    g = mr.gain_exact(sc, lo, hi)
    carried = g >= np.float32(cut)
    eye = np.broadcast_to(np.eye(8, dtype=np.float32), (8, 16, 8, 8)).copy()
    out = gpu_ctx.extract_tiles(stego, sc, eye, eye, ALPHA, 2, mask=rule)
    D = scipy.fft.dctn(o.to_tiles(out).astype(np.float64), type=2, norm="ortho", axes=(-2, -1))
    s2_hat = D[..., 1, 1]
    S = gpu_ctx.sigma_tiles(stego).astype(np.float64)
    assert (S[..., 1] - sc[..., 1]).min() > 100
    want = (S[..., 1] - sc[..., 1]) / (ALPHA * g.astype(np.float64))
    left_out = np.abs(s2_hat) < 1e-3
    err = float(np.abs(s2_hat - want)[carried].max())
    print(f"{rule}: device leaves out {int(left_out.sum())} tiles, carried_exact {int((~carried).sum())}, differing "
          f"{int((left_out != ~carried).sum())}; s^_2 on carried tiles max |d| {err:.2e} (bar {2e-2 / cut:.2e})")
    assert np.array_equal(left_out, ~carried)
    assert err < 2e-2 / cut
    assert np.abs(D[..., 0, 0] - (S[..., 0] - sc[..., 0]) / ALPHA).max() < 2e-2
    score = float(gpu_ctx.detect_tiles(stego, sc, Sw, ALPHA, mask=rule)[0])
    print(f"{rule}: detect {score:.6f}, restatement with carried_exact {score_exact:.6f}, with the pairwise set {score_pairwise:.6f}")
    assert abs(score - score_exact) < 1e-4
    gpu_ctx.check_status()


# ---- E. detect beyond 256 waves per plane ---------------------------------------------------------------------------
def test_detect_beyond_256_waves(gpu_ctx):
    """1024 x 1032: 128 x 129 tiles = 258 waves a plane, so k_detect_finalize's 256 threads take a second turn through
    their strided loop.  The host is the mask host recipe (every regime of the gain), tiled; masked and uniform embed on the
    device, detect by both rules against the restatement / the oracle.  In a second stego the last tile row - waves 257
    and 258 - is unrelated noise, which moves the score by far more than the bar: a finalize that stops at 256 waves shows.
    In a batch of three the second plane is the cover itself and the third the stego with the noise row: each scores what
    it scores alone (to 1e-12), not the first plane's.
    The cover's score has no reference to 1e-4: with s~ = sc up to the rounding of two SVDs, s^ = (s~ - sc) / alpha IS that
    rounding (|s^| below SIGMA_RTOL s_1 / alpha), and an NC of it is as good as any other - on an MI355X the device scores the
    masked cover 0.111 where the restatement, with LAPACK's rounding in s~, scores 0.273.  It is printed and held to the
    detect threshold 0.6, as tests/test_gpu_mask.py holds the unmarked cover; the two marked planes carry the 1e-4 bar."""
    H, W = 1024, 1032
    cover = np.ascontiguousarray(np.tile(mr.host(256, 344, 6), (4, 3)))
    assert cover.shape == (H, W) and ((H // 8) * (W // 8) + 63) // 64 == 258
    wm = mr.watermark(H, W)
    Sw = wm[2]
    noise = np.random.default_rng(61).integers(0, 256, (8, W), dtype=np.uint8)
    for mask in (mr.MASK, None):
        st, sc, _ = gpu_ctx.embed_tiles(cover, Sw, ALPHA, mask=mask)
        ref = (lambda y: mr.detect_ref(y, sc, Sw, ALPHA, mask)) if mask else (lambda y: o.detect_plane(y.astype(np.float32), sc, Sw, ALPHA, 8))
        tail = st.copy()
        tail[H - 8:] = noise
        want = [ref(st), ref(tail), ref(cover)]
        got = [float(gpu_ctx.detect_tiles(y, sc, Sw, ALPHA, mask=mask)[0]) for y in (st, tail, cover)]
        print(f"{'masked' if mask else 'uniform'}: stego {got[0]:.6f} / {want[0]:.6f}, noise in the last tile row {got[1]:.6f} / "
              f"{want[1]:.6f}, cover {got[2]:.6f} / {want[2]:.6f}")
        assert np.abs(np.array(got) - np.array(want))[:2].max() < 1e-4
        assert abs(want[1] - want[0]) > 1e-2                                # the last two waves matter
        assert np.isfinite(got[2]) and got[2] < 0.6 and want[2] < 0.6
        batch = gpu_ctx.detect_tiles(np.stack([st, cover, tail]), np.stack([sc, sc, sc]), Sw, ALPHA, mask=mask)
        assert abs(batch[0] - want[0]) < 1e-4 and abs(batch[2] - want[1]) < 1e-4
        assert np.abs(batch - np.array([got[0], got[2], got[1]])).max() < 1e-12
    gpu_ctx.check_status()
