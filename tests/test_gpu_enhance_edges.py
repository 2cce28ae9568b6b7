"""GPU: the extract post-processing kernels (csrc/wm_enhance.hip) at their edges, against tests/enhance_oracle.py bit
for bit - tile seams of NL-means (64 x 26) and unsharp (64 x 16), single rows and columns, 4K widths (k_clahe_apply's
column loop past 2048, the Lab kernels' grid-stride loops past 524 288 px), the CLAHE grid / clip space, the NL-means h
range up to the longest LDS weight table and the context's four table slots, every 8-bit input of the Lab and YCrCb
conversions, the device entry points' in-place use and refusals, and enhance calls on one long-lived context."""
import ctypes as C

import numpy as np
import pytest

import enhance_oracle as eo
from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


def _contents(H, W, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    return {
        "noise": rng.integers(0, 256, (H, W), dtype=np.uint8),
        "gradient": ((xx + yy) * 255 // max(H + W - 2, 1)).astype(np.uint8),
        "constant": np.full((H, W), 93, np.uint8),
        "blocks": np.where(((yy // 9) + (xx // 13)) % 2 == 0, 15, 240).astype(np.uint8),
    }


def _pair(c, a, b):
    return np.ascontiguousarray(np.stack([c[a], c[b]], axis=-1))


def _smooth(H, W, seed):
    """textured content whose template distances spread over the whole weight table"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    v = 128 + 50 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + rng.normal(0, 10, (H, W))
    return np.clip(v, 0, 255).astype(np.uint8)


def _all_triples():
    """every 8-bit triple once, as one 4096 x 4096 x 3 image: byte 0 = v & 255, byte 1 = (v >> 8) & 255, byte 2 = v >> 16"""
    v = np.arange(1 << 24, dtype=np.uint32)
    img = np.empty((1 << 24, 3), np.uint8)
    img[:, 0] = v & 255
    img[:, 1] = (v >> 8) & 255
    img[:, 2] = v >> 16
    return img.reshape(4096, 4096, 3)


# ---- shape seams ---------------------------------------------------------------------------------------------------
NLM_H = (1, 2, 25, 26, 27, 52, 53)          # k_nlmeans tiles are 64 x 26
NLM_W = (1, 2, 63, 64, 65, 128, 129)
NLM_SHAPES = sorted({(h, w) for h in NLM_H for w in (1, 64, 65)} | {(h, w) for h in (1, 26, 53) for w in NLM_W}
                    | {(1, 300), (300, 1)})


@pytest.mark.parametrize("shape", NLM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nlmeans_tile_seams(gpu_ctx, shape):
    c = _contents(*shape, seed=shape[0] * 131 + shape[1])
    for name, img in c.items():
        assert np.array_equal(gpu_ctx.nlmeans_u8(img, 7.0), eo.nlmeans(img, 7.0)), (name, 7.0)
    assert np.array_equal(gpu_ctx.nlmeans_u8(c["noise"], 3.0), eo.nlmeans(c["noise"], 3.0))
    for a, b, h in (("noise", "gradient", 3.0), ("blocks", "noise", 7.0)):
        ab = _pair(c, a, b)
        assert np.array_equal(gpu_ctx.nlmeans_u8(ab, h), eo.nlmeans(ab, h)), (a, b, h)


@pytest.mark.parametrize("H", [1, 2, 15, 16, 17])             # k_unsharp tiles are 64 x 16
def test_unsharp_tile_seams(gpu_ctx, H):
    rng = np.random.default_rng(H)
    for W in (1, 3, 63, 64, 65):
        for name, img in _contents(H, W, seed=W).items():
            assert np.array_equal(gpu_ctx.unsharp_u8(img, 0.25), eo.unsharp(img, 0.25)), (W, name)
        bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert np.array_equal(gpu_ctx.unsharp_u8(bgr, 0.15), eo.unsharp(bgr, 0.15)), W


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (1, 300), (9, 1), (300, 1), (2, 2)])
def test_clahe_single_rows_and_columns(gpu_ctx, shape):
    for name, img in _contents(*shape, seed=7).items():
        for tiles in ((8, 8), (1, 1), (16, 16), (3, 5)):
            got = gpu_ctx.clahe_u8(img, 2.0, tiles)
            assert np.array_equal(got, eo.clahe(img, 2.0, *tiles)), (name, tiles)


# ---- 4K widths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 2049), (8, 3840), (11, 4097), (2160, 3840)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_clahe_wide(gpu_ctx, shape):
    """k_clahe_apply's grid is capped at 8 x 256 threads per row: its column loop only turns past 2048 columns"""
    c = _contents(*shape, seed=shape[1])
    for name in (("noise", "gradient") if shape[0] > 1000 else c):
        img = c[name]
        assert np.array_equal(gpu_ctx.clahe_u8(img, 2.0, (8, 8)), eo.clahe(img, 2.0)), name
    if shape[0] < 1000:
        img = c["blocks"]
        assert np.array_equal(gpu_ctx.clahe_u8(img, 40.0, (16, 3)), eo.clahe(img, 40.0, 16, 3))


def test_unsharp_4k(gpu_ctx):
    rng = np.random.default_rng(40)
    g = _smooth(2160, 3840, 1)
    assert np.array_equal(gpu_ctx.unsharp_u8(g, 0.25), eo.unsharp(g, 0.25))
    bgr = rng.integers(0, 256, (2160, 3840, 3), dtype=np.uint8)
    assert np.array_equal(gpu_ctx.unsharp_u8(bgr, 0.15), eo.unsharp(bgr, 0.15))


def test_nlmeans_4k_band(gpu_ctx):
    g = _smooth(60, 3840, 2)
    assert np.array_equal(gpu_ctx.nlmeans_u8(g, 7.0), eo.nlmeans(g, 7.0))
    ab = np.ascontiguousarray(np.stack([g, g[::-1]], axis=-1) // 2 + 64)
    assert np.array_equal(gpu_ctx.nlmeans_u8(ab, 3.0), eo.nlmeans(ab, 3.0))


def test_gray_chain_4k_band(gpu_ctx):
    g = _smooth(270, 3840, 3)
    assert np.array_equal(gpu_ctx.enhance_extract_u8(g), eo.enhance_gray(g))


def test_color_chain_wide_band(gpu_ctx):
    """240 x 2304: more than 524 288 px (the Lab kernels' grid-stride loops turn) and wider than 2048 (the in-place CLAHE
    on the Y byte of interleaved YCrCb runs its column loop)"""
    H, W = 240, 2304
    assert H * W > 256 * 8 * 256 and W > 2048
    rng = np.random.default_rng(5)
    base = _smooth(H, W, 4).astype(np.int64)
    c = np.clip(np.stack([base, base[::-1], base[:, ::-1]], -1) + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)
    assert np.array_equal(gpu_ctx.enhance_extract_u8(c), eo.enhance_color(c))


# ---- CLAHE parameters ----------------------------------------------------------------------------------------------
GRIDS = [(1, 1), (2, 2), (3, 5), (16, 1), (1, 16), (16, 16)]


@pytest.mark.parametrize("tiles", GRIDS, ids=lambda t: f"{t[0]}x{t[1]}")
def test_clahe_grids_and_clips(gpu_ctx, tiles):
    # (80, 48) is divisible by every grid here, (37, 61) by none but 1, (3, 5) is smaller than most (reflected padding)
    for shape in ((80, 48), (37, 61), (3, 5)):
        for name, img in _contents(*shape, seed=shape[1]).items():
            none = gpu_ctx.clahe_u8(img, 0.0, tiles)
            assert np.array_equal(none, eo.clahe(img, 0.0, *tiles)), (shape, name)
            for clip in (-1.0, 0.01, 2.0, 40.0, 1e9):
                got = gpu_ctx.clahe_u8(img, clip, tiles)
                assert np.array_equal(got, eo.clahe(img, clip, *tiles)), (shape, name, clip)
            assert np.array_equal(gpu_ctx.clahe_u8(img, 1e9, tiles), none), (shape, name)
            assert np.array_equal(gpu_ctx.clahe_u8(img, -1.0, tiles), none), (shape, name)


def test_clahe_huge_clip_is_no_clip(gpu_ctx):
    """clip 1e9 on one 17 x 33 tile: 1e9 * 561 / 256 is past INT_MAX; the count saturates and clips nothing (it used to
    wrap to a count of 1, maximal equalisation)"""
    assert eo.clahe_clip_count(1e9, 17 * 33) == INT_MAX
    for name, img in _contents(17, 33, seed=3).items():
        none = eo.clahe(img, 0.0, 1, 1)
        for clip in (1e9, 1e30):
            assert np.array_equal(gpu_ctx.clahe_u8(img, clip, (1, 1)), none), (name, clip)
            assert np.array_equal(eo.clahe(img, clip, 1, 1), none), (name, clip)
        if name != "constant":
            assert not np.array_equal(eo.clahe(img, 0.01, 1, 1), none), name


def test_clahe_residual_off_grid(gpu_ctx):
    """a 3 x 5 grid at clip 40 on high-contrast blocks: the excess is not a multiple of 256, so the residual spread runs"""
    img = _contents(80, 48)["blocks"]
    th, tw = 80 // 5, 48 // 3
    clip = eo.clahe_clip_count(40.0, th * tw)
    hist = np.bincount(img[:th, :tw].ravel(), minlength=256)
    excess = int(np.maximum(hist - clip, 0).sum())
    assert excess > 0 and excess % 256 != 0
    assert np.array_equal(gpu_ctx.clahe_u8(img, 40.0, (3, 5)), eo.clahe(img, 40.0, 3, 5))


# ---- NL-means h ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch,h", [(1, 0.05), (1, 0.3), (1, 10.0), (1, 15.0), (2, 0.05), (2, 0.3), (2, 1.0), (2, 5.0)])
def test_nlmeans_h_range(gpu_ctx, ch, h):
    c = _contents(53, 129, seed=int(h * 100) + ch)
    c["smooth"] = _smooth(53, 129, 6)
    imgs = c.values() if ch == 1 else (_pair(c, "noise", "gradient"), _pair(c, "smooth", "blocks"), _pair(c, "smooth", "smooth"))
    for img in imgs:
        assert np.array_equal(gpu_ctx.nlmeans_u8(img, h), eo.nlmeans(img, h))


@pytest.mark.parametrize("ch", [1, 2])
def test_nlmeans_longest_weight_table(hostapi, ch):
    """the largest h whose table fits the kernels' 2048 LDS entries is bit-exact; one float32 step up is refused, and the
    context is still clean and exact afterwards"""
    h = eo.nlm_boundary_h(ch)
    assert len(eo.nlm_weights(h, ch)) - 1 == 2047
    up = float(np.nextafter(np.float32(h), np.float32(np.inf)))
    g = _smooth(52, 128, 7)
    img = g if ch == 1 else np.ascontiguousarray(np.stack([g, g[::-1]], axis=-1))
    want = eo.nlmeans(img, h)
    with hostapi.Context(0) as ctx:
        assert np.array_equal(ctx.nlmeans_u8(img, h), want)
        with pytest.raises(ValueError):
            ctx.nlmeans_u8(img, up)
        ctx.check_status()
        assert np.array_equal(ctx.nlmeans_u8(img, h), want)


def test_nlmeans_table_slots_evict_and_reuse(hostapi):
    """six (h, channels) keys of its own, twice round, between gray and colour chains (three keys of theirs): the four
    table slots of one context are evicted and refilled and every result stays exact"""
    c = _contents(30, 70, seed=12)
    g, ab = c["noise"] // 2 + c["gradient"] // 2, _pair(c, "noise", "blocks")
    keys = [(2.0, 1), (4.0, 1), (2.5, 2), (5.5, 1), (4.0, 2), (9.0, 1), (3.0, 1), (3.0, 2)]
    want = {k: eo.nlmeans(g if k[1] == 1 else ab, k[0]) for k in keys}
    bgr = np.ascontiguousarray(np.stack([c["noise"], c["gradient"], c["blocks"]], -1) // 2 + 40)
    want_gray, want_color = eo.enhance_gray(g), eo.enhance_color(bgr)
    with hostapi.Context(0) as ctx:
        for rnd in range(2):
            for i, k in enumerate(keys):
                assert np.array_equal(ctx.nlmeans_u8(g if k[1] == 1 else ab, k[0]), want[k]), (rnd, k)
                if i % 3 == 1:
                    assert np.array_equal(ctx.enhance_extract_u8(g), want_gray), (rnd, k)
                if i % 3 == 2:
                    assert np.array_equal(ctx.enhance_extract_u8(bgr), want_color), (rnd, k)
        ctx.check_status()


# ---- every 8-bit input of the per-pixel conversions ----------------------------------------------------------------
def test_lab_exhaustive(gpu_ctx):
    every = _all_triples()
    assert np.array_equal(gpu_ctx.lab_u8(every), eo.bgr_to_lab(every))
    assert np.array_equal(gpu_ctx.lab_u8(every, inverse=True), eo.lab_to_bgr(every))


def test_colour_conversions_exhaustive(gpu_ctx):
    every = _all_triples()
    ycc = o.bgr_to_ycrcb(every)
    assert np.array_equal(gpu_ctx.color("bgr2ycrcb", every), ycc)
    assert np.array_equal(gpu_ctx.color("bgr2y", every), ycc[..., 0])
    assert np.array_equal(gpu_ctx.color("ycrcb2bgr", every), o.ycrcb_to_bgr(every))
    assert np.array_equal(gpu_ctx.color("bgr2gray", every), o.bgr_to_gray(every))
    ynew = np.random.default_rng(9).integers(0, 256, every.shape[:2], dtype=np.uint8)
    ycc[..., 0] = ynew
    assert np.array_equal(gpu_ctx.color("replace_y", every, ynew), o.ycrcb_to_bgr(ycc))


# ---- unsharp amounts -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amount", [-1.0, 0.0, 3.0, 1e6])
def test_unsharp_amounts(gpu_ctx, amount):
    rng = np.random.default_rng(int(abs(amount)) % 97)
    for img in (_smooth(37, 70, 8), rng.integers(0, 256, (37, 70, 3), dtype=np.uint8)):
        got = gpu_ctx.unsharp_u8(img, amount)
        assert np.array_equal(got, eo.unsharp(img, amount))
        if amount == 0.0:
            assert np.array_equal(got, img)


# ---- device entry points -------------------------------------------------------------------------------------------
def _vp(p):
    return C.c_void_p(p) if p else None


def _dev_run(ctx, fn, img, *args, in_place=False):
    """img -> device, fn(ctx, src, dst, *args), device -> host"""
    a = ctx.malloc(img.nbytes)
    b = a if in_place else ctx.malloc(img.nbytes)
    try:
        ctx.h2d(a, img)
        ctx._call(fn, _vp(a), _vp(b), *args)
        out = np.empty_like(img)
        ctx.d2h(out, b)
        ctx.sync()
        return out
    finally:
        ctx.free(a)
        if b != a:
            ctx.free(b)


@pytest.mark.parametrize("color", [False, True], ids=["gray", "color"])
def test_enhance_extract_dev_in_place(gpu_ctx, color):
    c = _contents(45, 300, seed=2)
    img = (np.ascontiguousarray(np.stack([c["noise"], c["gradient"], c["blocks"]], -1) // 2 + 40) if color
           else c["noise"] // 3 + c["gradient"] // 2)
    ch = 3 if color else 1
    out = _dev_run(gpu_ctx, "wm_enhance_extract_u8_dev", img, 45, 300, ch)
    assert np.array_equal(out, eo.enhance(img))
    assert np.array_equal(_dev_run(gpu_ctx, "wm_enhance_extract_u8_dev", img, 45, 300, ch, in_place=True), out)


def test_dev_entry_points_refuse_bad_arguments(hostapi):
    H, W = 20, 70
    nb = H * W * 3
    nan, inf = float("nan"), float("inf")
    img = _contents(H, W, seed=4)["noise"]
    with hostapi.Context(0) as ctx:
        a, b = ctx.malloc(2 * nb), ctx.malloc(nb)          # a + offset stays inside its allocation
        try:
            ctx.h2d(a, np.zeros(nb, np.uint8))
            bad = [
                ("wm_nlmeans_u8_dev", (a, a, H, W, 1, 7.0, 7, 21)),            # in place
                ("wm_nlmeans_u8_dev", (a, a + 64, H, W, 1, 7.0, 7, 21)),       # overlapping
                ("wm_nlmeans_u8_dev", (a + 64, a, H, W, 2, 3.0, 7, 21)),
                ("wm_nlmeans_u8_dev", (a, b, H, W, 3, 7.0, 7, 21)),
                ("wm_nlmeans_u8_dev", (a, b, H, W, 0, 7.0, 7, 21)),
                ("wm_nlmeans_u8_dev", (a, b, 0, W, 1, 7.0, 7, 21)),
                ("wm_nlmeans_u8_dev", (a, b, H, -1, 1, 7.0, 7, 21)),
                ("wm_nlmeans_u8_dev", (0, b, H, W, 1, 7.0, 7, 21)),
                ("wm_nlmeans_u8_dev", (a, 0, H, W, 1, 7.0, 7, 21)),
                ("wm_nlmeans_u8_dev", (a, b, H, W, 1, nan, 7, 21)),
                ("wm_nlmeans_u8_dev", (a, b, H, W, 1, inf, 7, 21)),
                ("wm_nlmeans_u8_dev", (a, b, H, W, 1, -3.0, 7, 21)),
                ("wm_nlmeans_u8_dev", (a, b, H, W, 1, 7.0, 7, 19)),
                ("wm_clahe_u8_dev", (a, b, H, W, 2.0, 0, 8)),
                ("wm_clahe_u8_dev", (a, b, H, W, 2.0, 8, 0)),
                ("wm_clahe_u8_dev", (a, b, H, W, 2.0, 17, 8)),
                ("wm_clahe_u8_dev", (a, b, H, W, 2.0, 8, 17)),
                ("wm_clahe_u8_dev", (a, b, H, W, nan, 8, 8)),
                ("wm_clahe_u8_dev", (a, b, H, W, inf, 8, 8)),
                ("wm_clahe_u8_dev", (a, b, H, W, -inf, 8, 8)),
                ("wm_clahe_u8_dev", (a, b, 0, W, 2.0, 8, 8)),
                ("wm_clahe_u8_dev", (a, b, H, -5, 2.0, 8, 8)),
                ("wm_clahe_u8_dev", (0, b, H, W, 2.0, 8, 8)),
                ("wm_clahe_u8_dev", (a, 0, H, W, 2.0, 8, 8)),
                ("wm_unsharp_u8_dev", (a, a, H, W, 1, 0.25)),
                ("wm_unsharp_u8_dev", (a + 100, a, H, W, 3, 0.25)),
                ("wm_unsharp_u8_dev", (a, b, H, W, 2, 0.25)),
                ("wm_unsharp_u8_dev", (a, b, H, W, 1, nan)),
                ("wm_unsharp_u8_dev", (a, b, H, W, 1, -inf)),
                ("wm_unsharp_u8_dev", (a, b, -1, W, 1, 0.25)),
                ("wm_unsharp_u8_dev", (a, b, H, 0, 1, 0.25)),
                ("wm_unsharp_u8_dev", (0, b, H, W, 1, 0.25)),
                ("wm_unsharp_u8_dev", (a, 0, H, W, 1, 0.25)),
                ("wm_bgr_to_lab_u8_dev", (0, b, H * W)),
                ("wm_bgr_to_lab_u8_dev", (a, 0, H * W)),
                ("wm_lab_to_bgr_u8_dev", (0, b, H * W)),
                ("wm_lab_to_bgr_u8_dev", (a, 0, H * W)),
                ("wm_enhance_extract_u8_dev", (a, b, H, W, 2)),
                ("wm_enhance_extract_u8_dev", (a, b, H, W, 0)),
                ("wm_enhance_extract_u8_dev", (a, b, 0, W, 1)),
                ("wm_enhance_extract_u8_dev", (a, b, H, -2, 3)),
                ("wm_enhance_extract_u8_dev", (0, b, H, W, 1)),
                ("wm_enhance_extract_u8_dev", (a, 0, H, W, 3)),
            ]
            for fn, args in bad:
                with pytest.raises((ValueError, RuntimeError)):
                    ctx._call(fn, _vp(args[0]), _vp(args[1]), *args[2:])
                ctx.check_status()
            # n_px == 0 is a no-op: the destination keeps its bytes
            marker = np.arange(nb, dtype=np.uint8)
            ctx.h2d(b, marker)
            for fn in ("wm_bgr_to_lab_u8_dev", "wm_lab_to_bgr_u8_dev"):
                ctx._call(fn, _vp(a), _vp(b), 0)
            back = np.empty_like(marker)
            ctx.d2h(back, b)
            ctx.sync()
            assert np.array_equal(back, marker)
        finally:
            ctx.free(a)
            ctx.free(b)
        ctx.check_status()
        assert np.array_equal(ctx.nlmeans_u8(img, 7.0), eo.nlmeans(img, 7.0))
        assert np.array_equal(ctx.clahe_u8(img, 2.0), eo.clahe(img, 2.0))
        assert np.array_equal(ctx.unsharp_u8(img, 0.25), eo.unsharp(img, 0.25))
        assert np.array_equal(ctx.enhance_extract_u8(img), eo.enhance_gray(img))


# ---- state reuse ---------------------------------------------------------------------------------------------------
REUSE_SHAPES = [(1, 1), (5, 300), (64, 96), (130, 260), (27, 65), (300, 7), (16, 16), (53, 129), (200, 320), (2, 2)]


def test_enhance_calls_on_a_long_lived_context_match_fresh_contexts(hostapi):
    """random enhance calls of growing and shrinking shapes, with tile-mode and full-frame calls between them (they share
    the context's scratch): each result equals the same call on a brand-new context, bit for bit"""
    rng = np.random.default_rng(77)
    long_lived = hostapi.Context(0)
    try:
        for step in range(40):
            H, W = REUSE_SHAPES[rng.integers(len(REUSE_SHAPES))]
            g = rng.integers(0, 256, (H, W), dtype=np.uint8)
            bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            op = int(rng.integers(8))
            h = float(rng.choice([3.0, 7.0, 0.3, 12.0, 5.0, 9.0]))
            clip = float(rng.choice([0.0, 2.0, 40.0, 1e9]))
            tiles = (int(rng.integers(1, 17)), int(rng.integers(1, 17)))
            amount = float(rng.choice([0.25, 0.15, 3.0]))

            def run(ctx):
                if op == 0:
                    return ctx.nlmeans_u8(g, h)
                if op == 1:
                    return ctx.nlmeans_u8(np.ascontiguousarray(bgr[..., :2]), h)
                if op == 2:
                    return ctx.clahe_u8(g, clip, tiles)
                if op == 3:
                    return ctx.unsharp_u8(bgr if step % 2 else g, amount)
                if op == 4:
                    lab = ctx.lab_u8(bgr)
                    return lab, ctx.lab_u8(lab, inverse=True)
                if op == 5:
                    return ctx.enhance_extract_u8(g), ctx.enhance_extract_u8(bgr)
                if op == 6:                                             # tile mode (H, W >= 8) or full frame
                    planes = np.stack([g, bgr[..., 0]])
                    if H >= 8 and W >= 8:
                        return ctx.sigma_tiles(planes)
                    return ctx.ref_sigma_planes(planes)
                return ctx.ref_sigma_planes(np.stack([g, bgr[..., 1]])), ctx.enhance_extract_u8(g)

            got = run(long_lived)
            with hostapi.Context(0) as fresh:
                want = run(fresh)
            got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
            assert all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(got, want)), \
                f"step {step}: op {op} on {H}x{W} differs from a fresh context"
        long_lived.check_status()
    finally:
        long_lived.close()
