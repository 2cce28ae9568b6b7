"""k_extract_tiles with shared factors staged through LDS (csrc/wmhip.hip, k_extract_tiles<SH>, stage_fetch .. stage_read):
every form of the kernel at the smallest shapes that take each of its paths, against the float64 product
Uw diag((s - sc) / alpha * keep) Vwt (idct2 of it) built from the GPU's own sigma, at the bound of
tests/test_gpu_watermark_side.py: 2e-6 max|y| + 1e-6.

Planes that share their factors (two or more, stride 0) go four to a workgroup that fetches a tile group's factors once;
one plane, or factors per plane, keep the one-wave workgroup.  What can go wrong is a tile that gets another tile's matrix
(or another plane's), a row or a column out of place, a plane count that does not fill the last workgroup, and the clamp of
the fetch in a plane's last, partial group.  The factors of every tile are therefore different full matrices, the plane
counts run over 1 .. 5 and 9, and each factor array is followed IN ITS ALLOCATION by a guard of NaNs: a fetch that runs past
the last tile and uses what it read shows up as NaN."""
import numpy as np
import pytest
from scipy.fft import idctn

import mask_refs as mr
from oracle import wm_oracle as o

pytestmark = pytest.mark.gpu

ALPHA = 0.15
GUARD = 64 * 256                   # bytes of NaN behind each factor array: a whole wave's block
# the masked form's rule: noise tiles have r = |s_2..8| of 500 .. 800, so 0 < g < 1 and every tile is carried, far from cut
MASK = (0.0, 2000.0, 0.05)
SHAPES = [(8, 8), (16, 24), (64, 64), (8, 520), (52, 83)]     # 1 tile, 6 tiles, one wave, one lane of a second wave, ragged


class _Dev:
    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes):
        p = self.ctx.malloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def put(self, arr, offset=0, guard=0):
        """a copy of arr `offset` bytes into an allocation of its own, `guard` bytes of NaN right behind it"""
        arr = np.ascontiguousarray(arr)
        p = self.alloc(offset + arr.nbytes + guard)
        self.ctx.h2d(p + offset, arr)
        if guard:
            self.ctx.h2d(p + offset + arr.nbytes, np.full(guard // 4, np.nan, np.float32))
        return p + offset

    def get(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        self.ctx.sync(); self.ctx.d2h(out, p); self.ctx.sync()
        return out

    def close(self):
        self.ctx.sync()
        for p in reversed(self.ptrs):
            self.ctx.free(p)


_CASES = {}


def _case(gpu_ctx, n, H, W, per_plane):
    """(stego [n, H, W], s, sc [n, nby, nbx, 8], U, Vt [nby, nbx, 8, 8] or [n, ..]): made once per shape and shared, unchanged"""
    key = (n, H, W, per_plane)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * H + W + n)
        st = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
        s = gpu_ctx.sigma_tiles(st).reshape(n, H // 8, W // 8, 8)
        sc = (s - np.float32(ALPHA) * rng.uniform(0, 255, s.shape).astype(np.float32)).astype(np.float32)
        f = [gpu_ctx.svd_tiles(rng.uniform(0, 255, (H, W)).astype(np.float32)) for _ in range(n if per_plane else 1)]
        U = np.stack([a[0] for a in f]) if per_plane else f[0][0]
        Vt = np.stack([a[2] for a in f]) if per_plane else f[0][2]
        _CASES[key] = (st, s, sc, U, Vt)
    return _CASES[key]


def _want(s, sc, U, Vt, H, W, K=8, mask=None):
    """(float64 estimate [n, H, W] with the zero border, max|y|): y as the kernel computes it in float32, the product in float64"""
    inv = np.float32(1.0) / np.float32(ALPHA)
    keep = mr.keep(sc, *mask, K)[1] if mask else (np.arange(8) < K).astype(np.float32)
    y = ((s - sc) * inv * keep).astype(np.float64)                                    # [n, nby, nbx, 8]
    t = idctn((U.astype(np.float64) * y[..., None, :]) @ Vt.astype(np.float64), axes=(-2, -1), norm="ortho")
    n, nby, nbx = y.shape[:3]
    out = np.zeros((n, H, W))
    out[:, :nby * 8, :nbx * 8] = t.transpose(0, 1, 3, 2, 4).reshape(n, nby * 8, nbx * 8)
    return out, float(np.abs(y).max())


def _check(got, want, ymax, H, W, what):
    assert not np.isnan(got).any(), f"{what}: NaN in the output (guard data used)"
    e = float(np.abs(got - want).max())
    print(f"{what}: error {e:.3e} at max|y| {ymax:.1f}, bound {2e-6 * ymax + 1e-6:.3e}")
    assert e <= 2e-6 * ymax + 1e-6, what
    assert not got[:, (H // 8) * 8:].any() and not got[:, :, (W // 8) * 8:].any(), f"{what}: border not zero"


def _extract_dev(gpu_ctx, st, sc, U, Vt, K=8, px=True, mask=None, st_off=0, out_off=0):
    """the *_dev entry points on buffers of the test's own: factors with a NaN guard, stego and out at a byte offset"""
    n, H, W = st.shape
    nt = (H // 8) * (W // 8)
    uv_stride = nt if U.ndim == 5 else 0
    dv = _Dev(gpu_ctx)
    try:
        d_u, d_v = dv.put(U, guard=GUARD), dv.put(Vt, guard=GUARD)
        d_st, d_sc = dv.put(st, offset=st_off), dv.put(sc)
        d_out = dv.put(np.full((n, H, W), np.nan, np.float32), offset=out_off)
        if px:
            gpu_ctx.tile_factors_to_pixel_dev(d_u, d_v, d_u, d_v, nt * (n if uv_stride else 1))
        name = "wm_extract_tiles" + ("_px" if px else "") + ("_masked" if mask else "") + "_u8_dev"
        gpu_ctx._call(name, d_st, d_sc, d_u, d_v, d_out, n, H, W, W, H * W, uv_stride, ALPHA, K, *(mask or ()))
        gpu_ctx.check_status()
        return dv.get(d_out, (n, H, W), np.float32)
    finally:
        dv.close()


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("n", [1, 3])
def test_staged_extract_pixel_factors_at_every_wave_shape(gpu_ctx, H, W, n):
    """one plane (its own loads) and three planes that share the factors (staged, one wave of the workgroup without a plane)"""
    st, s, sc, U, Vt = _case(gpu_ctx, n, H, W, False)
    want, ymax = _want(s, sc, U, Vt, H, W)
    _check(_extract_dev(gpu_ctx, st, sc, U, Vt), want, ymax, H, W, f"px {n} x {H}x{W}")


@pytest.mark.parametrize("n", [2, 4, 5, 9])
def test_staged_extract_plane_counts(gpu_ctx, n):
    """shared factors at plane counts around the workgroup's four; 65 tiles: the second group has one tile"""
    H, W = 8, 520
    st, s, sc, U, Vt = _case(gpu_ctx, n, H, W, False)
    want, ymax = _want(s, sc, U, Vt, H, W)
    _check(_extract_dev(gpu_ctx, st, sc, U, Vt), want, ymax, H, W, f"px {n} planes shared")


@pytest.mark.parametrize("H,W", [(8, 520), (52, 83)])
def test_staged_extract_of_three_planes_with_factors_of_their_own(gpu_ctx, H, W):
    """stride n_tiles: with 65 and 60 tiles a plane's factors start in the middle of the previous plane's last group"""
    st, s, sc, U, Vt = _case(gpu_ctx, 3, H, W, True)
    want, ymax = _want(s, sc, U, Vt, H, W)
    _check(_extract_dev(gpu_ctx, st, sc, U, Vt), want, ymax, H, W, f"px 3 planes {H}x{W} per plane")


@pytest.mark.parametrize("H,W", [(64, 64), (8, 520)])
@pytest.mark.parametrize("n", [1, 3])
def test_staged_extract_at_unaligned_bases(gpu_ctx, H, W, n):
    """stego at an odd byte offset (ALIGNED false), out 4 but not 16 bytes into its allocation (VECF false)"""
    st, s, sc, U, Vt = _case(gpu_ctx, n, H, W, False)
    want, ymax = _want(s, sc, U, Vt, H, W)
    _check(_extract_dev(gpu_ctx, st, sc, U, Vt, st_off=1, out_off=4), want, ymax, H, W, f"px unaligned {n} x {H}x{W}")


@pytest.mark.parametrize("px", [True, False])
def test_staged_extract_truncated_rank(gpu_ctx, px):
    H, W = 8, 520
    st, s, sc, U, Vt = _case(gpu_ctx, 3, H, W, False)
    want, ymax = _want(s, sc, U, Vt, H, W, K=5)
    _check(_extract_dev(gpu_ctx, st, sc, U, Vt, K=5, px=px), want, ymax, H, W, f"K=5 px={px}")


@pytest.mark.parametrize("H,W", [(8, 520), (52, 83)])
@pytest.mark.parametrize("per_plane", [False, True])
def test_staged_extract_dct_domain_entry(gpu_ctx, H, W, per_plane):
    st, s, sc, U, Vt = _case(gpu_ctx, 3, H, W, per_plane)
    want, ymax = _want(s, sc, U, Vt, H, W)
    _check(_extract_dev(gpu_ctx, st, sc, U, Vt, px=False), want, ymax, H, W, f"dct {H}x{W} per_plane={per_plane}")


@pytest.mark.parametrize("px", [True, False])
def test_staged_extract_masked(gpu_ctx, px):
    H, W = 52, 83
    st, s, sc, U, Vt = _case(gpu_ctx, 3, H, W, False)
    g = mr.gain(sc, MASK[0], MASK[1])[0]
    assert g.min() > 2 * MASK[2] and g.max() < 1            # every tile carried, none on the edge, 1 / g at work
    want, ymax = _want(s, sc, U, Vt, H, W, mask=MASK)
    _check(_extract_dev(gpu_ctx, st, sc, U, Vt, px=px, mask=MASK), want, ymax, H, W, f"masked px={px}")


@pytest.mark.parametrize("H,W", [(8, 520), (52, 83)])
@pytest.mark.parametrize("per_plane", [False, True])
@pytest.mark.parametrize("mask", [None, MASK])
def test_staged_extract_one_call_unscrambled(gpu_ctx, H, W, per_plane, mask):
    """wm_extract_unscrambled_u8_dev (the MM form: the kernel's own min / max feed the normalise).  Its output is uint8: the
    float estimate is within 2e-6 max|y| of the float64 one, which moves the normalised value by far less than 1, so after
    the truncation to uint8 the two differ by at most 1."""
    st, s, sc, U, Vt = _case(gpu_ctx, 3, H, W, per_plane)
    want, _ = _want(s, sc, U, Vt, H, W, mask=mask)
    idx = o.permutation(H, W, o.rng_from_key(o.derive_key("staging", bytes(8))))
    got = gpu_ctx.extract_tiles_unscrambled_u8(st, sc, U, Vt, ALPHA, 8, idx, True, mask=mask)
    ref = np.stack([mr.to_u8(o.unpermute(w.astype(np.float32), idx), True) for w in want])
    d = int(np.abs(got.astype(int) - ref.astype(int)).max())
    print(f"one-call {H}x{W} per_plane={per_plane} mask={mask}: max |d| {d} LSB")
    assert got.shape == (3, H, W) and got.dtype == np.uint8 and d <= 1
