"""The LQ prelude of the V-free tile iteration (B0 = X Q: Householder LQ with greedy row pivoting, applied from the right,
ahead of the Jacobi sweeps) checked WITHOUT a GPU, in both of its forms: the generated gfx950 stream through
tools/emu_jacobi_asm.py (64-tile waves, wave-uniform sweep control) and the C++ form of csrc/wm_tile_math.h built
with g++ (tests/lq_harness.cpp, one tile at a time), in the two configurations the kernels run:
embed (conv 1e-7, three untested sweeps, pairs skipped from the 4th) and sigma-only (conv 1e-2 next to the stream's
norm-move test, JAC_MOVE2 of wm_tile_math.h)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import emu_jacobi_asm as emu          # noqa: E402

CSRC = os.path.join(ROOT, "digital-watermarking-for-image-video-using-dct-svd-singular-value-decomposition_amd", "csrc")

# (conv2, skip2, min_sweeps, skip_from): what embed_group (csrc/wmhip.hip) / sigma_tile_dev (csrc/wm_tile_pass.h) pass to the stream; the
# fifth entry chooses the generated stream (1) or the baseline the test generates for itself (0)
EMBED = (1e-7, 1e-12, 4, 3, 1)
SIGMA = (1e-2, 1e-8, 3, 2, 1)
# the stream without the prelude and without the norm-move test (gen_jacobi_asm.build(move_test=False, lq=False), never
# compiled into a kernel), with the sweep control it had before: the iteration before the prelude
EMBED_BEFORE = (1e-7, 1e-12, 4, 4, 0)
SIGMA_BEFORE = (1e-3, 1e-8, 3, 2, 0)


def _wave(seed):
    """64 tiles: every special kind the prelude can trip over, between noise and smooth tiles"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (64, 8, 8), dtype=np.uint8)
    yy, xx = np.mgrid[0:8, 0:8]
    k = 0

    def put(x):
        nonlocal k
        t[k] = np.clip(x, 0, 255); k += 1
    for _ in range(12):                                                   # smooth + sensor noise: steep spectrum
        put(rng.uniform(40, 200) + rng.uniform(-6, 6) * xx + rng.uniform(-6, 6) * yy + rng.normal(0, 2, (8, 8)))
    put(np.zeros((8, 8)))                                                 # zero
    put(np.full((8, 8), 9)); put(np.full((8, 8), 255))                    # flat
    put(np.equal(yy, xx) * 255)                                           # 255 * identity: equal row norms, equal sigma
    put((yy + xx) % 2 * 255)                                              # checkerboard
    put((xx % 2) * 255); put((xx % 2 == 0) * rng.integers(1, 256, (8, 8)))   # alternating zero columns
    for rows in ((0,), (7,), (2, 5), (0, 1, 2, 3, 4, 5, 6)):              # zero rows
        a = rng.integers(0, 256, (8, 8)); a[list(rows)] = 0; put(a)
    for _ in range(3):
        put(np.outer(rng.integers(0, 16, 8), rng.integers(0, 16, 8)))     # rank 1
    for _ in range(3):                                                    # rank 2
        put(np.outer(rng.integers(0, 12, 8), rng.integers(0, 12, 8)) + np.outer(rng.integers(0, 8, 8), np.ones(8, int)))
    a = rng.integers(0, 256, (8, 8)); a[5] = a[2]; put(a)                 # two equal rows
    a = rng.integers(0, 256, (8, 8)); a[6] = a[1]; a[:, 3] = a[:, 0]; put(a)
    return t


WAVES = [_wave(s) for s in (5, 6)]
REF = [np.linalg.svd(w.astype(np.float64), compute_uv=False) for w in WAVES]


def _rows(a):
    """[n][rp][c][half] -> [n][row][column], float64"""
    return a.transpose(0, 1, 3, 2).reshape(-1, 8, 8).astype(np.float64)


@pytest.fixture(scope="module")
def host_form():
    out = os.path.join(ROOT, "tests", "_build", "liblq_harness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "lq_harness.cpp")
    deps = [src, os.path.join(CSRC, "wm_tile_math.h"), os.path.join(CSRC, "wm_completion_tables.inc")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", out, src], check=True)
    lib = C.CDLL(out)
    u8, f32, i32 = (np.ctypeslib.ndpointer(dt, flags="C_CONTIGUOUS") for dt in (np.uint8, np.float32, np.int32))
    lib.lq_prelude_host.argtypes = [u8, C.c_int, f32]
    lib.lq_jacobi_host.argtypes = [u8, C.c_int, C.c_int, f32, f32, i32]
    lib.lq_prelude_host.restype = lib.lq_jacobi_host.restype = None
    return lib


def _check_prelude(tiles, b0):
    """(b): B0 B0^T = X X^T to 1e-5 |X|_F^2, and B0 is a row permutation of a lower-triangular matrix: the pivot row of
    step k has nothing above rounding beyond column k, so the rows' last non-zero columns, sorted, stay below 0, 1, .. 7"""
    x = tiles.astype(np.float64)
    fro2 = np.maximum((x ** 2).sum(axis=(1, 2)), 1.0)
    assert np.isfinite(b0).all()
    err = np.abs(np.einsum("nrc,nsc->nrs", b0, b0) - np.einsum("nrc,nsc->nrs", x, x)).max(axis=(1, 2))
    print("prelude: max |B0 B0^T - X X^T| / |X|_F^2 = %.2e" % (err / fro2).max())
    assert (err / fro2).max() < 1e-5
    big = np.abs(b0) > 1e-5 * np.sqrt(fro2)[:, None, None]
    last = np.where(big.any(axis=2), 7 - np.argmax(big[:, :, ::-1], axis=2), -1)       # [tile][row]
    assert np.all(np.sort(last, axis=1) <= np.arange(8)), np.sort(last, axis=1).max(axis=0)


def _check_result(tiles, ref, b, n2, conv2):
    """(a), (c), (d), (e) on one wave's B = X V and |b_i|^2"""
    assert np.isfinite(b).all() and np.isfinite(n2).all()
    s1 = np.maximum(ref[:, :1], 1.0)
    s = np.sqrt(np.maximum(n2, 0)).astype(np.float64)
    err = np.abs(s - ref) / s1
    print("conv2 %g: max sigma error %.2e sigma_1" % (conv2, err.max()))
    assert err.max() < 2e-6
    assert np.all(np.diff(s, axis=1) <= 2e-3 * s1)
    x = tiles.astype(np.float64)
    fro2 = np.maximum((x ** 2).sum(axis=(1, 2)), 1.0)
    d = np.abs(np.einsum("nrc,nsc->nrs", b, b) - np.einsum("nrc,nsc->nrs", x, x)).max(axis=(1, 2))
    assert (d / fro2).max() < 1e-5
    good = ref > 1e-5 * np.maximum(ref[:, :1], 1e-30)                     # de Rijk keeps them in front
    gram = np.einsum("nrc,nrd->ncd", b, b)
    pair_good = good[:, :, None] & good[:, None, :] & ~np.eye(8, dtype=bool)
    off = np.where(pair_good, np.abs(gram), 0.0).max(axis=(1, 2)) / s1[:, 0] ** 2
    print("conv2 %g: max off-diagonal Gram %.2e sigma_1^2" % (conv2, off.max()))
    assert off.max() < (1e-6 if conv2 < 1e-5 else 2e-3)


@pytest.mark.parametrize("w", range(len(WAVES)))
def test_prelude_of_the_generated_stream(w):
    _check_prelude(WAVES[w], _rows(emu.run_prelude(WAVES[w])))


@pytest.mark.parametrize("w", range(len(WAVES)))
def test_prelude_of_the_cpp_form(host_form, w):
    b0 = np.zeros((64, 8, 8), np.float32)
    host_form.lq_prelude_host(np.ascontiguousarray(WAVES[w]), 64, b0)
    _check_prelude(WAVES[w], b0.astype(np.float64))


@pytest.mark.parametrize("cfg", [EMBED, SIGMA], ids=["embed", "sigma"])
@pytest.mark.parametrize("w", range(len(WAVES)))
def test_generated_stream_behind_the_prelude_against_lapack(w, cfg):
    a, n2, more, sweeps = emu.run(WAVES[w], *cfg[:4], lq=cfg[4])
    assert not np.any(more) and sweeps <= 8, sweeps
    _check_result(WAVES[w], REF[w], _rows(a), n2, cfg[0])


@pytest.mark.parametrize("sigma_only", [0, 1], ids=["embed", "sigma"])
@pytest.mark.parametrize("w", range(len(WAVES)))
def test_cpp_form_behind_the_prelude_against_lapack(host_form, w, sigma_only):
    b = np.zeros((64, 8, 8), np.float32); n2 = np.zeros((64, 8), np.float32); sweeps = np.zeros(64, np.int32)
    host_form.lq_jacobi_host(np.ascontiguousarray(WAVES[w]), 64, sigma_only, b, n2, sweeps)
    assert np.all(sweeps > 0) and sweeps.max() <= 8, sweeps                # > 0: converged (more == 0)
    _check_result(WAVES[w], REF[w], b.astype(np.float64), n2, 1e-2 if sigma_only else 1e-7)


NOISE_WAVES = [np.random.default_rng(2025).integers(0, 256, (40, 64, 8, 8), dtype=np.uint8)]


def _mean_sweeps_and_cost(cfg):
    sw, cost = [], []
    for t in NOISE_WAVES[0]:
        st = {}
        _, _, more, k = emu.run(t, *cfg[:4], lq=cfg[4], stats=st, move_test=bool(cfg[4]))
        assert not np.any(more)
        sw.append(k); cost.append(2 * st.get("pk", 0) + st.get("valu", 0) + st.get("trans", 0))
    return float(np.mean(sw)), float(np.mean(cost))


@pytest.mark.parametrize("name,new,old,gain", [("embed", EMBED, EMBED_BEFORE, 0.5), ("sigma", SIGMA, SIGMA_BEFORE, 0.8)],
                         ids=["embed", "sigma"])
def test_the_prelude_saves_most_of_a_sweep_per_wave(name, new, old, gain):
    """(f) 40 noise waves: sweeps per wave below those of the iteration without the prelude by at least 0.5 (embed) and
    0.8 (sigma-only) - from the CPU model's 5.00 -> 4.25 and 4.12 -> 3.12 - and fewer VALU instructions executed per
    wave in both (a packed instruction counted as two: profiles/r02_embed_variants.md section 2).
    Measured: embed 5.000 -> 4.250 sweeps, 8 034 -> 7 641 weighted instructions; sigma-only 4.100 -> 3.275, 7 095 -> 6 672."""
    (s_new, c_new), (s_old, c_old) = _mean_sweeps_and_cost(new), _mean_sweeps_and_cost(old)
    print(f"{name}: sweeps per wave {s_old:.3f} -> {s_new:.3f}, weighted VALU instructions per wave {c_old:.0f} -> {c_new:.0f}")
    assert c_new < c_old
    assert s_new <= s_old - gain
