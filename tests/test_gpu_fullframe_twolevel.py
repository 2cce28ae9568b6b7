"""The two-level (super-block) block Jacobi of the full-frame mode (csrc/wm_ref_hier.inc).

From 20 planes per call on it is the library's default; below that the flat tournament runs.  Here it is FORCED
(WM_RF_HIER=1, read by the library on every call) and held against
  * float64 LAPACK and the flat tournament directly (singular values, sweep counts), for every super-block size, on
    shapes that exercise 1, 2 and 3 row panels, byes of the level-1 tournament, unequal super-blocks, transposed
    (portrait) planes, rank-deficient planes and a batch;
  * the whole existing full-frame suite: the parity tests of tests/test_gpu_fullframe.py are collected a second
    time in this module under the forced scheme (embed / sigma / detect / extract / watermark-side SVD with its
    accumulated left factor / rank-deficient planes and their null-space completion / smooth content / 1080p).
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _force_two_level(monkeypatch):
    monkeypatch.setenv("WM_RF_HIER", "1")
    yield


def _load_base():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_fullframe.py")
    spec = importlib.util.spec_from_file_location("_ff_base_for_two_level", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_base = _load_base()
# the existing parity tests, run again under the forced two-level scheme
test_two_level_embed_sigma_detect = _base.test_fullframe_embed_sigma_detect
test_two_level_watermark_svd_and_extract = _base.test_fullframe_watermark_svd_and_extract
test_two_level_batched_planes_equal_single = _base.test_fullframe_batched_planes_equal_single
test_two_level_rank_deficient_planes = _base.test_fullframe_rank_deficient_planes
test_two_level_parity_on_smooth_content = _base.test_fullframe_parity_on_smooth_content
test_two_level_batch_of_mixed_content = _base.test_fullframe_batch_of_mixed_content
test_two_level_cfg2_1080p_against_float64_lapack = _base.test_fullframe_cfg2_1080p_against_float64_lapack
test_two_level_random_geometries = _base.test_fullframe_random_geometries


def _planes(B, H, W, seed=5):
    rng = np.random.default_rng(seed)
    planes = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    if B >= 3:      # a smooth plane and a half-empty one in the batch
        planes[1] = (np.outer(np.linspace(0, 200, H), np.ones(W)) + 20 * np.sin(np.arange(W) / 9.0)[None, :]).astype(np.uint8)
        planes[2, :, W // 2:] = 0
    return planes


@pytest.mark.parametrize("f16", [3, 0, 1])
@pytest.mark.parametrize("sb", [6, 4, 2])
@pytest.mark.parametrize("B,H,W", [(1, 64, 96), (2, 128, 200), (1, 200, 136), (3, 320, 480), (1, 448, 448), (1, 832, 900)])
def test_two_level_against_lapack_and_the_flat_tournament(gpu_ctx, monkeypatch, sb, B, H, W, f16):
    """f16 = 3: Gram tiles and rotation products from split-f16 operands on the f16 matrix pipe (the default for uint8 planes),
    1: the Gram tiles only, 0: the f32 kernels - the same bars for all three."""
    monkeypatch.setenv("WM_RF_HIER_F16", str(f16))
    planes = _planes(B, H, W)
    ref = np.stack([np.linalg.svd(p.astype(np.float64), compute_uv=False) for p in planes])
    monkeypatch.setenv("WM_RF_HIER", "0")
    s_flat = gpu_ctx.ref_sigma_planes(planes)
    n_flat = gpu_ctx.ref_last_sweeps()
    assert gpu_ctx.ref_last_flops()[1] is False
    monkeypatch.setenv("WM_RF_HIER", "1")
    monkeypatch.setenv("WM_RF_HIER_SB", str(sb))
    s = gpu_ctx.ref_sigma_planes(planes)
    n = gpu_ctx.ref_last_sweeps()
    flops, two_level = gpu_ctx.ref_last_flops()
    assert two_level is True and flops > 0
    assert np.max(np.abs(s - ref) / ref[:, :1]) < 2e-6           # the bar of tests/test_gpu_fullframe.py
    assert np.max(np.abs(s - s_flat) / ref[:, :1]) < 1e-6
    assert n <= n_flat + 3                                       # the ordering converges like the flat one (measured: -2 .. +2)
    gpu_ctx.check_status()


_OFF_GRID = [(H, W, f16, h3) for H, W in [(64, 97), (128, 130), (320, 323), (97, 64)] for f16 in (3, 0)
             for h3 in ((0, 1) if (H, W) == (320, 323) else (None,))]


@pytest.mark.parametrize("H,W,f16,hgram3", _OFF_GRID)
def test_two_level_row_lengths_off_the_float4_grid(gpu_ctx, monkeypatch, H, W, f16, hgram3):
    """Row lengths M = 1, 2, 3 (mod 4): the last 16-byte load of a row is masked element by element (every other shape of the
    suite has M = 0 (mod 4)).  One panel (64 rows), two, three (ten blocks: a 6 + 4 super-pair, with both Gram kernels) and a
    transposed plane; the module's bars against float64 LAPACK and the flat tournament, and two runs bit for bit."""
    monkeypatch.setenv("WM_RF_HIER_F16", str(f16))
    if hgram3 is None:
        monkeypatch.delenv("WM_RF_HGRAM3", raising=False)
    else:
        monkeypatch.setenv("WM_RF_HGRAM3", str(hgram3))
    planes = _planes(2, H, W)
    ref = np.stack([np.linalg.svd(p.astype(np.float64), compute_uv=False) for p in planes])
    monkeypatch.setenv("WM_RF_HIER", "0")
    s_flat = gpu_ctx.ref_sigma_planes(planes)
    assert gpu_ctx.ref_last_flops()[1] is False
    monkeypatch.setenv("WM_RF_HIER", "1")
    a = gpu_ctx.ref_sigma_planes(planes)
    assert gpu_ctx.ref_last_flops()[1] is True
    b = gpu_ctx.ref_sigma_planes(planes)
    print(f"off-grid {H}x{W} f16={f16} hgram3={hgram3}: vs LAPACK {np.max(np.abs(a - ref) / ref[:, :1]):.2e}, "
          f"vs flat {np.max(np.abs(a - s_flat) / ref[:, :1]):.2e} sigma_1")
    assert np.max(np.abs(a - ref) / ref[:, :1]) < 2e-6
    assert np.max(np.abs(a - s_flat) / ref[:, :1]) < 1e-6
    assert a.tobytes() == b.tobytes()
    gpu_ctx.check_status()


def test_two_level_is_deterministic_and_batch_independent(gpu_ctx):
    """Bit for bit: the same plane alone, twice, and inside a batch (fixed summation orders, no float atomics)."""
    planes = _planes(3, 256, 384, seed=11)
    a = gpu_ctx.ref_sigma_planes(planes[:1])
    b = gpu_ctx.ref_sigma_planes(planes[:1])
    c = gpu_ctx.ref_sigma_planes(planes)
    assert np.array_equal(a, b)
    # a batch sweeps until its slowest plane has converged, so a plane may see extra (skipped or tiny) rotations: equal to
    # the accuracy of the values, not bit for bit
    assert np.max(np.abs(c[0] - a[0])) / a[0, 0] < 5e-7


def test_default_scheme_follows_the_batch_size(gpu_ctx, monkeypatch):
    """uint8 planes (split-f16 kernels apply): two-level from 3 planes per call on; float inputs (the watermark-side SVD keeps
    the f32 kernels): from 20."""
    monkeypatch.delenv("WM_RF_HIER", raising=False)
    monkeypatch.delenv("WM_RF_HIER_F16", raising=False)
    small = _planes(2, 64, 96)
    gpu_ctx.ref_sigma_planes(small)
    assert gpu_ctx.ref_last_flops()[1] is False
    big = np.repeat(_planes(1, 64, 96), 5, axis=0)
    s = gpu_ctx.ref_sigma_planes(big)
    assert gpu_ctx.ref_last_flops()[1] is True
    ref = np.linalg.svd(big[0].astype(np.float64), compute_uv=False)
    assert np.max(np.abs(s - ref[None, :])) / ref[0] < 2e-6
    wm = np.random.default_rng(3).integers(0, 256, (3, 64, 96)).astype(np.float32)
    gpu_ctx.ref_svd_planes(wm, apply_dct=True)
    assert gpu_ctx.ref_last_flops()[1] is False


def test_split_f16_keeps_the_embed_within_the_bars_on_extreme_planes(gpu_ctx, monkeypatch):
    """The split-f16 products see rows whose entries reach 255 sqrt(L) (a saturated plane: sigma_1 = 255 sqrt(H W)) and rows of
    tiny magnitude (a plane of zeros and ones): the singular values stay within the suite's bar of float64 LAPACK and the embed
    within 1 LSB of the f32 kernels' result."""
    rng = np.random.default_rng(2)
    H, W = 256, 416
    planes = np.stack([np.full((H, W), 255, np.uint8), rng.integers(0, 2, (H, W)).astype(np.uint8),
                       rng.integers(250, 256, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8)])
    planes[0, ::7, ::5] = 254                                   # (not exactly rank 1)
    ref = np.stack([np.linalg.svd(p.astype(np.float64), compute_uv=False) for p in planes])
    sw = np.linspace(300.0, 1.0, H).astype(np.float32)
    out = {}
    for f16 in (0, 3):
        monkeypatch.setenv("WM_RF_HIER_F16", str(f16))
        s = gpu_ctx.ref_sigma_planes(planes)
        assert np.max(np.abs(s - ref) / ref[:, :1]) < 2e-6, f16
        out[f16] = gpu_ctx.ref_embed_planes(planes, sw, 0.15, int(0.6 * H))
    # plane 0 is rank-deficient (2 of 256 directions): its missing ranks go along an arbitrary orthonormal completion that
    # depends on the rotated rows' last bits - like LAPACK's - so pixels are only comparable on the full-rank planes
    d = np.abs(out[0][0][1:].astype(int) - out[3][0][1:].astype(int))
    assert d.max() <= 1 and np.mean(d != 0) < 2e-3
    assert np.max(np.abs(out[0][1] - out[3][1]) / ref[:, :1]) < 1e-6


def test_two_level_is_reproducible_at_1080p(gpu_ctx, monkeypatch):
    """Three 1080p planes, default kernels (split-f16 Gram and rotation products), three runs: bit-identical singular values,
    every run within the suite's bar of float64 LAPACK.  (Round 4: two co-resident workgroups of the split-f16 Gram kernel per
    CU gave run-to-run differences of up to 7e-5 sigma_1 at this size - small planes never showed it.)"""
    monkeypatch.delenv("WM_RF_HIER_F16", raising=False)
    rng = np.random.default_rng(21)
    planes = rng.integers(0, 256, (3, 1080, 1920), dtype=np.uint8)
    ref = np.stack([np.linalg.svd(p.astype(np.float64), compute_uv=False) for p in planes])
    runs = [gpu_ctx.ref_sigma_planes(planes) for _ in range(3)]
    assert gpu_ctx.ref_last_flops()[1] is True
    for s in runs:
        assert np.max(np.abs(s - ref) / ref[:, :1]) < 2e-6
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


def test_two_level_on_one_two_and_three_queues(gpu_ctx, monkeypatch):
    """The plane groups of a batch run on 1 - 3 HIP queues (WM_RF_QUEUES, read per call): the same singular values to 1e-6 sigma_1
    whatever the grouping (a group's column splits differ with its size, so not bit for bit), every grouping reproducible."""
    planes = _planes(6, 320, 480, seed=23)
    ref = np.stack([np.linalg.svd(p.astype(np.float64), compute_uv=False) for p in planes])
    got = {}
    for q in ("1", "2", "3"):
        monkeypatch.setenv("WM_RF_QUEUES", q)
        a = gpu_ctx.ref_sigma_planes(planes)
        b = gpu_ctx.ref_sigma_planes(planes)
        assert np.array_equal(a, b), q
        assert np.max(np.abs(a - ref) / ref[:, :1]) < 2e-6, q
        got[q] = a
    assert np.max(np.abs(got["1"] - got["3"]) / ref[:, :1]) < 1e-6 and np.max(np.abs(got["2"] - got["3"]) / ref[:, :1]) < 1e-6


@pytest.mark.parametrize("H,W", [(832, 900), (1080, 1920), (400, 1000)])
def test_three_panel_gram_kernel(gpu_ctx, monkeypatch, H, W):
    """k_hgram_h3 (one workgroup per super-pair, plane and column split: all <= 384 rows of a chunk fetched once, the 78 blocks of the
    upper triangle shared out over 12 waves) is the default from 11 planes per launch on; forced here on two planes: the same
    singular values as the two-panel kernel to 5e-7 sigma_1, within the suite's bar of float64 LAPACK, bit-reproducible, also for
    super-pairs of 10 blocks (832 rows: 26 blocks) and row lengths that are no multiple of the chunk (W = 900, 1000)."""
    planes = _planes(2, H, W, seed=31)
    ref = np.stack([np.linalg.svd(p.astype(np.float64), compute_uv=False) for p in planes])
    monkeypatch.setenv("WM_RF_HGRAM3", "0")
    a = gpu_ctx.ref_sigma_planes(planes)
    monkeypatch.setenv("WM_RF_HGRAM3", "1")
    b = gpu_ctx.ref_sigma_planes(planes)
    c = gpu_ctx.ref_sigma_planes(planes)
    assert gpu_ctx.ref_last_flops()[1] is True
    assert np.array_equal(b, c)
    assert np.max(np.abs(b - ref) / ref[:, :1]) < 2e-6
    assert np.max(np.abs(a - b) / ref[:, :1]) < 5e-7
