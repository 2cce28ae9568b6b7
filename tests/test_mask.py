"""Texture-masked strength without a device: the tile-math helpers the kernels call (a stand-alone g++ program, plain
and under AddressSanitizer + UBSan), the meta member and its checks, host-side argument validation, and the value claim on
the oracle alone."""
import importlib
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import mask_refs as mr
from oracle import wm_oracle as o

M = importlib.import_module(ge.PKG_NAME + ".meta")


# ---- tile math ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request):
    return ge.build_mask_harness(sanitize=request.param == "sanitized")


def _run_harness(exe, tmp_path, Sc, lo, hi, cut, K):
    Sc = np.ascontiguousarray(Sc, np.float32).reshape(-1, 8)
    n = Sc.shape[0]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([n, K], np.int32).tobytes() + np.array([lo, hi, cut], np.float32).tobytes() + Sc.tobytes())
    r = subprocess.run([exe, "run", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = np.fromfile(dst, np.float32)
    assert out.size == n * 18
    return out[:n], out[n:2 * n] != 0, out[2 * n:10 * n].reshape(n, 8), out[10 * n:].reshape(n, 8)


def test_tile_math_edges(harness):
    """all-zero sc, r == lo, r == hi, lo = 0, a very large hi, K < 8: asserted inside the program"""
    r = subprocess.run([harness, "edges"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


@pytest.mark.parametrize("K", [8, 3])
def test_tile_math_against_numpy_on_the_test_hosts(harness, tmp_path, K):
    """mask_gain / mask_keep on the oracle's Sc of the three test hosts.  Bounds: the program sums the seven squares in a
    chain of fused multiply-adds, NumPy pairwise - a few ulp of r, which only matters below hi = 64, so
    |dg| <= 64 * 4 * 2^-24 / 56 < 1e-6; a carried tile has g >= cut = 0.25, so |d(1/g)| <= |dg| / cut^2 < 2e-5."""
    lo, hi, cut = mr.MASK
    for H, W, seed in mr.HOSTS:
        Sc = mr.cover_sigma(H, W, seed).reshape(-1, 8)
        mr.check_preconditions(Sc)
        g, carried, keep, eff = _run_harness(harness, tmp_path, Sc, lo, hi, cut, K)
        g_np, G_np = mr.gain(Sc, lo, hi)
        carried_np, keep_np = mr.keep(Sc, lo, hi, cut, K)
        assert np.abs(g - g_np).max() < 1e-6
        assert np.array_equal(g == 0, g_np == 0) and np.array_equal(g == 1, g_np == 1)
        assert np.array_equal(carried, carried_np)
        assert np.abs(keep - keep_np).max() < 2e-5
        assert np.array_equal(keep == 0, keep_np == 0)
        assert np.abs(eff - G_np).max() < 1e-6 and np.all(eff[:, 0] == 1)
    # the product's own NumPy statement of the gain is the same formula
    assert np.array_equal(M.mask_gain(Sc, lo, hi), g_np)


def test_tile_math_edge_rows_against_numpy(harness, tmp_path):
    rows = mr.edge_rows()
    for lo, hi, cut, K in ((8.0, 64.0, 0.25, 8), (0.0, 1e-6, 1.0, 8), (8.0, 3.0e38, 0.25, 8), (0.0, 64.0, 0.5, 5), (8.0, 64.0, 1.0, 0)):
        g, carried, keep, _ = _run_harness(harness, tmp_path, rows, lo, hi, cut, K)
        g_np, _ = mr.gain(rows, lo, hi)
        carried_np, keep_np = mr.keep(rows, lo, hi, cut, K)
        assert np.abs(g - g_np).max() < 1e-6 and np.array_equal(carried, carried_np)
        assert np.allclose(keep, keep_np, rtol=1e-5, atol=0) and np.array_equal(keep == 0, keep_np == 0)


# ---- the exact restatement and the hosts of tests/test_gpu_mask_edges.py --------------------------------------------
_EDGE_RULES = [r for r in mr.RULES if r[2] < 1 and r[1] < 1e30]             # the rules whose cut a row with s_1 = 500 can sit on
_RULE_IDS = ["-".join(f"{x:g}" for x in r) for r in mr.RULES]


@pytest.mark.parametrize("rule", mr.RULES, ids=_RULE_IDS)
def test_gain_exact_is_the_harness_bit_for_bit(harness, tmp_path, rule):
    """mask_refs.gain_exact / carried_exact - the rule with every operation rounded once to float32, the squares added in
    rational arithmetic - against mask_gain / mask_keep of the g++ program, on the three test hosts' Sc, the edge rows and
    the rows on the edge of both cuts: the same bits, under every rule of the table."""
    lo, hi, cut = rule
    Sc = np.concatenate([mr.cover_sigma(H, W, seed).reshape(-1, 8) for H, W, seed in mr.HOSTS] + [mr.edge_rows()]
                        + [mr.near_cut_rows(*r) for r in _EDGE_RULES])
    g, carried, keep, _ = _run_harness(harness, tmp_path, Sc, lo, hi, cut, 8)
    ge = mr.gain_exact(Sc, lo, hi)
    assert np.array_equal(g.view(np.uint32), ge.view(np.uint32))
    assert np.array_equal(carried, mr.carried_exact(Sc, lo, hi, cut))
    with np.errstate(divide="ignore", over="ignore"):
        inv = np.where(carried, np.float32(1.0) / ge, np.float32(0.0)).astype(np.float32)
    assert np.array_equal(keep[:, 1].view(np.uint32), inv.view(np.uint32)) and np.all(keep[:, 0] == 1)


@pytest.mark.parametrize("rule", _EDGE_RULES, ids=["-".join(f"{x:g}" for x in r) for r in _EDGE_RULES])
def test_near_cut_rows_split_the_two_sums(rule):
    """near_cut_rows asserts its own composition (the three single-component rows at, below and above the cut; everything
    within 3e-7 of it); here: the exact fused sum and NumPy's pairwise sum disagree on at least 64 rows, both carried
    classes hold at least 16, and the detect restatement tells the two carried sets apart by more than 1e-3."""
    lo, hi, cut = rule
    rows = mr.near_cut_rows(lo, hi, cut)
    assert rows.shape == (128, 8) and np.all(rows[:, 0] == 500) and np.all(np.diff(rows, axis=-1) <= 0)
    ce, cp = mr.carried_exact(rows, lo, hi, cut), mr.keep(rows, lo, hi, cut)[0]
    print(rule, "carried exact", int(ce.sum()), "pairwise", int(cp.sum()), "disagree", int((ce != cp).sum()))
    assert (ce != cp).sum() >= 64
    assert min(ce.sum(), (~ce).sum()) >= 16
    assert ce[0] and not ce[1] and ce[2]
    _, _, _, exact, pairwise = mr.near_cut_case(lo, hi, cut)
    print(rule, "detect restatement: carried_exact", exact, "pairwise", pairwise)
    assert abs(exact - pairwise) > 1e-3


def test_flagged_hosts_hold_what_the_device_tests_need():
    """From the oracle's Sc: JPEG-quantised and posterised content is rich in rank-deficient tiles (s_8 <= 1e-5 s_1) that
    the rule gives 0 < g < 1 (measured: 20 / 68 of quantised under the default rule / (0, 16, 0.05), 99 of posterised), the
    hand-made plane holds every class, and no tile of any host lies within 1e-4 of the cut of a rule with cut < 1: no tile
    is left out of any comparison."""
    def count(name, rule):
        Sc = mr.flagged_sigma(name)
        g, _ = mr.gain(Sc, rule[0], rule[1])
        return int((~(Sc[..., 7] > 1e-5 * Sc[..., 0]) & (g > 0) & (g < 1)).sum())
    assert count("quantised_72x100", mr.RULES[0]) >= 15
    assert count("quantised_72x100", mr.RULES[1]) >= 60
    assert count("posterised_72x100", mr.RULES[0]) >= 90
    hosts = mr.flagged_hosts()
    assert sorted(hosts) == sorted([f"{k}_{s}" for k in ("quantised", "posterised", "natural") for s in ("64x64", "72x100")]
                                   + ["handmade_64x64"])
    for name in hosts:
        assert hosts[name].reshape(-1).max() > 0 and not (o.to_tiles(hosts[name]).max((-1, -2)) == 0).any()    # no black tile
        Sc = mr.flagged_sigma(name)
        for lo, hi, cut in mr.RULES:
            if cut < 1:
                assert np.abs(mr.gain(Sc, lo, hi)[0] - np.float32(cut)).min() > 1e-4, (name, lo, hi, cut)
    # the hand-made plane: ranks 7, 2, 4, 0 + constant, 1, and near-deficient full-rank tiles
    S = np.linalg.svd(o.to_tiles(hosts["handmade_64x64"]).astype(np.float64), compute_uv=False).reshape(64, 8)
    rank = (S > 1e-9 * S[:, :1]).sum(-1)
    assert all((rank == k).sum() >= 4 for k in (1, 2, 4, 7, 8))
    assert ((rank == 8) & (S[:, 7] < 1e-5 * S[:, 0])).sum() >= 8
    assert mr.constant_tiles(hosts["handmade_64x64"]).sum() == 4


def test_constant_batch_and_letterbox_hold_black_tiles():
    import payload_refs as pr
    lb = pr.letterbox_planes()
    assert [int(pr.black_tiles(p).sum()) for p in lb] == [0, 48, 27]
    cb = mr.constant_batch()
    assert [int(pr.black_tiles(p).sum()) for p in cb] == [64, 0, 0, 0, 63]
    assert [int(mr.constant_tiles(p).sum()) for p in cb] == [64, 64, 64, 0, 63]
    # the oracle composed with the rule moves a black or constant tile along the flat vector: the reference of the device test
    wm = mr.watermark(64, 64)
    for p in (0, 2, 4):
        ref = mr.embed_ref(cb[p], wm)
        t, c = o.to_tiles(ref["Yw"]), mr.constant_tiles(cb[p])
        assert np.all((t.max((-1, -2)) - t.min((-1, -2)))[c] < 1e-3)
        assert np.abs(t[c][:, 0, 0] - (float(cb[p, 0, 0]) + mr.ALPHA * wm[2][c][:, 0] / 8)).max() < 1e-3


# ---- meta -----------------------------------------------------------------------------------------------------------
# the member lists of an unmasked meta, as they were before masking existed
_UNMASKED = {
    "gray": ["mode", "Sc", "Uw", "Vwt", "Sw", "payload_type", "shape", "alpha", "kfrac", "nonce", "tile", "k_floor", "digest"],
    "color": ["mode", "payload_type", "shape", "alpha", "kfrac", "nonce", "tile", "k_floor",
              "Sb", "UWb", "VWbt", "SWb", "Sg", "UWg", "VWgt", "SWg", "Sr", "UWr", "VWrt", "SWr", "digest"],
    "video_gray": ["mode", "payload_type", "Sc", "Uw", "Vwt", "Sw", "shape", "alpha", "kfrac", "frame_interval", "n_frames",
                   "tile", "k_floor", "nonce", "digest"],
    "video_color": ["mode", "payload_type", "shape", "alpha", "kfrac", "frame_interval", "n_frames", "tile", "k_floor", "nonce",
                    "digest", "Sb", "UWb", "VWbt", "SWb", "Sg", "UWg", "VWgt", "SWg", "Sr", "UWr", "VWrt", "SWr"],
}


def _members(mode, mask):
    z = np.zeros((1, 1, 8), np.float32)
    factors = M.gray_members(z, z, z, z) if "gray" in mode else M.channel_members([z] * 3, [z] * 3, [z] * 3, [z] * 3)
    extra = M.video_members(1, 3, 8, 8) if mode.startswith("video") else M.image_members(8, 8)
    return {"mode": mode, **M.common_members(8, 8, 0.1, 0.6, bytes(8)), **extra, **M.mask_members(mask), **factors}


@pytest.mark.parametrize("mode", sorted(_UNMASKED))
def test_meta_mask_member_sits_after_k_floor_and_only_when_masked(mode):
    plain = M.sealed(_members(mode, None), 8, bytes(32))
    assert list(plain) == _UNMASKED[mode] and M.mask_of(plain) is None
    mask = M.check_strength("masked", (4.0, 32.5, 0.5), 8)
    masked = M.sealed(_members(mode, mask), 8, bytes(32))
    want = list(_UNMASKED[mode]); want.insert(want.index("k_floor") + 1, "mask")
    assert list(masked) == want
    assert masked["mask"].dtype == np.float32 and masked["mask"].shape == (3,)
    assert M.mask_of(masked) == (4.0, 32.5, 0.5)
    # the HMAC covers what it covered: the parameters, like alpha, are not part of it
    assert len(M.hmac_parts(masked)) == len(M.hmac_parts(plain)) and not any(x is masked["mask"] for x in M.hmac_parts(masked))


def test_mask_of_round_trips_through_a_file(tmp_path):
    mask = M.check_strength("masked", M.MASK_DEFAULT, 8)
    assert mask == (8.0, 64.0, 0.25)
    np.savez(tmp_path / "m.npz", **M.sealed(_members("gray", mask), 8, bytes(32)))
    with np.load(tmp_path / "m.npz", allow_pickle=False) as data:
        assert M.mask_of(data) == mask
    with pytest.raises(ValueError):
        M.mask_of({"mask": np.array([8.0, 4.0, 0.25], np.float32)})        # a meta whose rule is not one


_BAD_MASKS = [(8.0, 8.0, 0.25), (9.0, 8.0, 0.25), (-1.0, 8.0, 0.25), (8.0, 64.0, 0.0), (8.0, 64.0, -0.1), (8.0, 64.0, 1.5),
              (float("nan"), 64.0, 0.25), (8.0, float("inf"), 0.25), (8.0, 64.0, float("nan")), (8.0, 64.0), "masked"]


@pytest.mark.parametrize("mask", _BAD_MASKS)
def test_bad_mask_parameters_are_value_errors(mask):
    with pytest.raises(ValueError):
        M.check_strength("masked", mask, 8)


def test_check_strength():
    assert M.check_strength("uniform", M.MASK_DEFAULT, 8) is None
    assert M.check_strength("uniform", M.MASK_DEFAULT, None) is None
    assert M.check_strength("uniform", "ignored", 8) is None              # the parameters only matter when masking
    assert M.check_strength("masked", (0.0, 1e-6, 1.0), 8) == (0.0, float(np.float32(1e-6)), 1.0)
    with pytest.raises(ValueError, match="full-frame"):
        M.check_strength("masked", M.MASK_DEFAULT, None)
    for bad in ("Masked", "texture", None, 1):
        with pytest.raises(ValueError, match="strength"):
            M.check_strength(bad, M.MASK_DEFAULT, 8)


def test_public_functions_refuse_before_any_device_call(tmp_path):
    """strength="masked" with tile=None, a bad rule and an unknown strength raise ValueError before a context exists (the
    messages are the checks' own: on a box without a GPU a context would fail with another error)."""
    import dct_svd_core_secure as core
    video = importlib.import_module(ge.PKG_NAME + ".video")
    cover = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="full-frame"):
        core.embed_arrays(cover, cover, "pw", bytes(8), tile=None, strength="masked")
    with pytest.raises(ValueError, match="lo < hi"):
        core.embed_arrays(cover, cover, "pw", bytes(8), strength="masked", mask=(64.0, 8.0, 0.25))
    with pytest.raises(ValueError, match="cut"):
        core.embed_arrays(cover, cover, "pw", bytes(8), strength="masked", mask=(8.0, 64.0, 0.0))
    with pytest.raises(ValueError, match="strength"):
        core.embed_arrays(cover, cover, "pw", bytes(8), strength="adaptive")
    with pytest.raises(ValueError, match="full-frame"):
        core.embed(str(tmp_path / "no.png"), str(tmp_path / "no.png"), str(tmp_path / "o.png"), str(tmp_path / "m.npz"),
                   password="pw", tile=None, strength="masked")
    for fn in (video.embed_watermark_video, video.embed_watermark_video_color):
        with pytest.raises(ValueError, match="full-frame"):
            fn(str(tmp_path / "no.y4m"), str(tmp_path / "no.png"), str(tmp_path / "o.y4m"), str(tmp_path / "m.npz"),
               password="pw", tile=None, strength="masked")
        with pytest.raises(ValueError, match="strength"):
            fn(str(tmp_path / "no.y4m"), str(tmp_path / "no.png"), str(tmp_path / "o.y4m"), str(tmp_path / "m.npz"),
               password="pw", strength="bogus")
    frames = np.zeros((2, 16, 16), np.uint8)
    for call in (lambda: video.embed_frames(None, frames, np.zeros(16, np.float32), 0.1, tile=None, mask=mr.MASK),
                 lambda: video.extract_frames_mean(None, frames, None, None, None, 0.1, tile=None, mask=mr.MASK),
                 lambda: video.detect_frames(None, frames, None, None, 0.1, tile=None, mask=mr.MASK)):
        with pytest.raises(ValueError, match="full-frame"):
            call()


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
    st = np.zeros((64, 96), np.uint8)
    nby, nbx = 8, 12
    sw = np.zeros((nby, nbx, 8), np.float32)
    U = np.zeros((nby, nbx, 8, 8), np.float32)
    idx = np.arange(64 * 96)
    for bad in _BAD_MASKS:                                                  # the rule itself, on every method that takes it
        for call in (lambda: ctx.embed_tiles(st, sw, 0.1, mask=bad), lambda: ctx.extract_tiles(st, sw, U, U, 0.1, mask=bad),
                     lambda: ctx.detect_tiles(st, sw, sw, 0.1, mask=bad),
                     lambda: ctx.extract_tiles_unscrambled_u8(st, sw, U, U, 0.1, 8, idx, mask=bad)):
            with pytest.raises(ValueError):
                call()
    for lo, hi in ((8.0, 8.0), (-1.0, 8.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError):
            ctx.mask_gain_tiles(st, lo, hi)
    # shapes, with a good rule
    with pytest.raises(ValueError):
        ctx.mask_gain_tiles(st.astype(np.float32), 8.0, 64.0)
    with pytest.raises(ValueError):
        ctx.mask_gain_tiles(np.zeros((2, 2, 64, 96), np.uint8), 8.0, 64.0)
    with pytest.raises(ValueError):
        ctx.embed_tiles(st, sw[:, :-1], 0.1, mask=mr.MASK)
    with pytest.raises(ValueError):
        ctx.embed_tiles(st, np.zeros((2, nby, nbx, 8), np.float32), 0.1, mask=mr.MASK)   # per-plane sigma_w for 1 plane
    with pytest.raises(ValueError):
        ctx.embed_tiles(st.astype(np.int16), sw, 0.1, mask=mr.MASK)
    with pytest.raises(ValueError):
        ctx.extract_tiles(st, sw[:4], U, U, 0.1, mask=mr.MASK)
    with pytest.raises(ValueError):
        ctx.extract_tiles(st, sw, U, U[:, :5], 0.1, mask=mr.MASK)
    with pytest.raises(ValueError):
        ctx.detect_tiles(st, sw, sw[:, :-1], 0.1, mask=mr.MASK)
    with pytest.raises(ValueError):
        ctx.extract_tiles_unscrambled_u8(st, sw[:4], U, U, 0.1, 8, idx, mask=mr.MASK)


class _RecordingLib:
    """stands in for libwmhip.so: every entry point succeeds, writes nothing and is recorded"""

    def __init__(self):
        self.calls, self._next = [], 0x1000

    def wm_last_error(self):
        return b""

    def __getattr__(self, name):
        if not name.startswith("wm_"):
            raise AttributeError(name)

        def fn(h, *args):
            self.calls.append(name)
            if name in ("wm_malloc", "wm_route_create_dev"):               # both hand a handle back through their last argument
                self._next += 0x100000
                args[-1]._obj.value = self._next
            return 0
        return fn


@pytest.mark.parametrize("routed", [True, False])
@pytest.mark.parametrize("masked", [True, False])
def test_unscrambled_extract_returns_on_every_branch(hostapi, routed, masked):
    """extract_tiles_unscrambled_u8 with and without a route (a plane of more than ROUTE_MAX_N pixels has none), masked and
    unmasked: each reaches its own extract entry point, the route-less ones then unscramble, and all four return planes."""
    ctx = object.__new__(hostapi.Context)
    ctx.lib, ctx._h, ctx.device = _RecordingLib(), 1, 0
    if not routed:
        ctx.ROUTE_MAX_N = 0
    H = W = 16
    st = np.zeros((2, H, W), np.uint8); sc = np.zeros((2, 2, 2, 8), np.float32); U = np.zeros((2, 2, 8, 8), np.float32)
    try:
        out = ctx.extract_tiles_unscrambled_u8(st, sc, U, U, 0.1, 8, np.arange(H * W), mask=mr.MASK if masked else None)
        calls = ctx.lib.calls
    finally:
        ctx._h = None
    assert out.shape == (2, H, W) and out.dtype == np.uint8
    stem = "wm_extract_unscrambled" if routed else "wm_extract_tiles"
    assert (stem + ("_masked_u8_dev" if masked else "_u8_dev")) in calls
    assert (stem + ("_u8_dev" if masked else "_masked_u8_dev")) not in calls
    assert ("wm_unpermute_f32_dev" in calls) == (not routed)
    assert calls[-1] == "wm_free" and "wm_check_status" in calls


# ---- the value claim, on the oracle alone ---------------------------------------------------------------------------
def test_masked_strength_keeps_smooth_content_clean_on_the_oracle():
    """A 128 x 192 cover, left half a ramp, right half the ramp plus noise of std 35; a logo of 16 x 24 cells of 8 x 8
    pixels; alpha = 0.12.  Deviation = RMS of stego - cover about its mean over the half (the mean is the brightness shift of
    the leading component, which stays uniform by design).  The masked deviation in the smooth half is at most a quarter of
    the uniform one (7.8 x here: 1.7 against 13.4 gray levels), the textured half is untouched, and every logo cell
    decodes from the masked stego by the masked rule."""
    rng = np.random.default_rng(7)
    H, W = 128, 192
    yy, xx = np.mgrid[0:H, 0:W]
    cover = (60 + 0.5 * xx + 0.3 * yy).astype(np.float64)
    cover[:, W // 2:] += rng.normal(0, 35, (H, W))[:, W // 2:]
    Y = np.clip(np.round(cover), 0, 255).astype(np.uint8)
    logo = (rng.integers(0, 2, (16, 24)) * 255).astype(np.uint8)
    idx = o.permutation(H, W, o.rng_from_key(o.derive_key("pw", bytes(8))))
    wy_s = o.permute(np.kron(logo, np.ones((8, 8), np.uint8)).astype(np.float32), idx)
    wm = (wy_s,) + tuple(o.watermark_decompose(wy_s, 8))
    uni = mr.embed_ref(Y, wm, mr.ALPHA, None)
    msk = mr.embed_ref(Y, wm, mr.ALPHA, mr.MASK)
    dev = lambda r, half: float(np.std((r["stego"].astype(np.float64) - Y)[:, half]))
    smooth, textured = slice(0, W // 2), slice(W // 2, W)
    print(f"smooth half: uniform {dev(uni, smooth):.2f}, masked {dev(msk, smooth):.2f}; "
          f"textured half: uniform {dev(uni, textured):.2f}, masked {dev(msk, textured):.2f}")
    assert dev(msk, smooth) <= 0.25 * dev(uni, smooth)
    assert abs(dev(msk, textured) - dev(uni, textured)) < 0.05 * dev(uni, textured)
    rec = o.unpermute(mr.extract_ref(msk["stego"], msk["Sc"], wm[1], wm[3], mr.ALPHA, mr.MASK), idx)
    cells = rec.reshape(16, 8, 24, 8).mean((1, 3))
    assert np.array_equal(cells > cells.mean(), logo > 127)
