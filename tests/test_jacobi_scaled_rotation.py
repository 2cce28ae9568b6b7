"""The scaled rotations of the V-free tile iteration's untested sweeps (rotation_scaled() of tools/gen_jacobi_asm.py,
jacobi_rot_scaled_pk of csrc/wm_tile_math.h) checked WITHOUT a GPU: the generated stream through tools/emu_jacobi_asm.py on 64-tile waves, the
C++ form built with g++ (tests/lq_harness.cpp, one tile at a time: the "wave" is the tile), both against float64 LAPACK,
in the embed configuration (conv 1e-7) and the sigma-only one (conv 1e-2 next to the norm-move test)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import emu_jacobi_asm as emu          # noqa: E402
import jacobi_stream_cost as cost     # noqa: E402
import scaled_rotation_inputs as inp  # noqa: E402

CSRC = os.path.join(ROOT, "digital-watermarking-for-image-video-using-dct-svd-singular-value-decomposition_amd", "csrc")
EMBED = (1e-7, 1e-12, 4, 3)           # (conv2, skip2, min_sweeps, skip_from) of embed_group (csrc/wmhip.hip) / sigma_tile_dev (csrc/wm_tile_pass.h)
SIGMA = (1e-2, 1e-8, 3, 2)
CFG = {"embed": EMBED, "sigma": SIGMA}


@pytest.fixture(scope="module")
def host_form():
    out = os.path.join(ROOT, "tests", "_build", "libscaled_rot_harness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "lq_harness.cpp")
    deps = [src, os.path.join(CSRC, "wm_tile_math.h"), os.path.join(CSRC, "wm_completion_tables.inc")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", out, src], check=True)
    lib = C.CDLL(out)
    u8, f32, i32 = (np.ctypeslib.ndpointer(dt, flags="C_CONTIGUOUS") for dt in (np.uint8, np.float32, np.int32))
    lib.lq_jacobi_host.argtypes = [u8, C.c_int, C.c_int, f32, f32, i32]
    lib.lq_jacobi_host.restype = None
    return lib


def _rows(a):
    """[n][rp][c][half] -> [n][row][column], float64"""
    return a.transpose(0, 1, 3, 2).reshape(-1, 8, 8).astype(np.float64)


def _check(tiles, b, n2, embed):
    """sigma <= 1e-4 sigma_1 (the project bar; the figure is printed), descending order, B B^T = X X^T, and B's columns
    orthogonal to the criterion the configuration stops on (the columns of singular values above 1e-5 sigma_1: a
    rank-deficient tile's null columns are rounding residue, the kernels complete such tiles from the good ones)."""
    assert np.isfinite(b).all() and np.isfinite(n2).all()
    x = tiles.astype(np.float64)
    ref = np.linalg.svd(x, compute_uv=False)
    s1 = np.maximum(ref[:, :1], 1.0)
    s = np.sqrt(np.maximum(n2, 0)).astype(np.float64)
    err = (np.abs(s - ref) / s1).max()
    good = ref > 1e-5 * np.maximum(ref[:, :1], 1e-30)
    gram = np.einsum("nrc,nrd->ncd", b, b)
    pair_good = good[:, :, None] & good[:, None, :] & ~np.eye(8, dtype=bool)
    off = (np.where(pair_good, np.abs(gram), 0.0).max(axis=(1, 2)) / s1[:, 0] ** 2).max()
    print("max sigma error %.2e sigma_1, max off-diagonal Gram %.2e sigma_1^2" % (err, off))
    assert err < 1e-4
    assert np.all(np.diff(s, axis=1) <= 2e-3 * s1)                       # descending like LAPACK
    fro2 = np.maximum((x ** 2).sum(axis=(1, 2)), 1.0)
    assert (np.abs(np.einsum("nrc,nsc->nrs", b, b) - np.einsum("nrc,nsc->nrs", x, x)).max(axis=(1, 2)) / fro2).max() < 1e-5
    assert off < (1e-6 if embed else 2e-3)


WAVES = {kind: inp.tiles(kind, 64, 40 + i) for i, kind in enumerate(inp.KINDS)}
WAVES.update(one_late_swap=inp.one_late_swap_wave(), every_lane_swaps=inp.every_lane_swaps_wave(), degenerate=inp.degenerate_wave())
_RUNS = {}


def _run(name, cfg):
    """one emulator run per (wave, configuration), shared by the tests"""
    if (name, cfg) not in _RUNS:
        st, sc = {}, []
        a, n2, more, sweeps = emu.run(WAVES[name], *CFG[cfg], stats=st, scales=sc)
        _RUNS[name, cfg] = (_rows(a), n2, more, sweeps, st, sc[0])
    return _RUNS[name, cfg]


@pytest.mark.parametrize("cfg", ["embed", "sigma"])
@pytest.mark.parametrize("name", list(WAVES))
def test_generated_stream_against_lapack(name, cfg):
    b, n2, more, sweeps, st, w2 = _run(name, cfg)
    assert not np.any(more) and sweeps <= 8, sweeps
    _check(WAVES[name], b, n2, cfg == "embed")
    # the squared scales (as they are when they are folded back into B) stay finite, positive and far inside the float32
    # range, zero and rank-1 tiles included
    print("squared scales in [%.2e, %.2e]" % (w2.min(), w2.max()))
    assert np.isfinite(w2).all() and w2.min() > 1e-6 and w2.max() < 1e6


@pytest.mark.parametrize("sigma_only", [0, 1], ids=["embed", "sigma"])
@pytest.mark.parametrize("name", list(WAVES))
def test_cpp_form_against_lapack(host_form, name, sigma_only):
    t = np.ascontiguousarray(WAVES[name])
    b = np.zeros((64, 8, 8), np.float32); n2 = np.zeros((64, 8), np.float32); sweeps = np.zeros(64, np.int32)
    host_form.lq_jacobi_host(t, 64, sigma_only, b, n2, sweeps)
    assert np.all(sweeps > 0) and sweeps.max() <= 8, sweeps                # > 0: converged
    _check(t, b.astype(np.float64), n2, not sigma_only)


def test_one_lane_alone_sends_its_wave_through_the_swap_branch_at_a_late_pair():
    """one_late_swap_wave(): in the embed's third sweep, the last one on scaled columns, exactly one lane (the tile with
    near-equal singular values) wants the de Rijk swap at a pair, the wave takes the swap branch there, and the 63 other
    tiles come out right all the same (test_generated_stream_against_lapack checks every lane of this wave)."""
    st = _run("one_late_swap", "embed")[4]
    late = st.get(("swap_lanes", 2), [])
    assert late.count(1) >= 1 and max(late) == 1, late
    assert st.get(("swap", 2), 0) == late.count(1)


def test_a_wave_in_which_every_lane_swaps():
    st = _run("every_lane_swaps", "embed")[4]
    lanes = [n for k in range(8) for n in st.get(("swap_lanes", k), [])]
    assert lanes.count(64) >= 1, lanes


# Executed VALU instructions per 64-tile wave of the stream of commit 6281a71 (every pair through the unscaled
# rotation), mean over the 40 noise waves of tools/jacobi_stream_cost.py: (scalar VALU, v_pk_mul_f32, v_pk_fma_f32, v_rsq_f32)
PARENT = {"embed": (2745.825, 894.4, 1456.4, 193.35), "sigma": (2467.75, 757.7, 1261.1, 166.5)}


@pytest.mark.parametrize("cfg", ["embed", "sigma"])
def test_fewer_instruction_cycles_than_the_unscaled_stream(cfg):
    """The scaled rotations trade 8 v_pk_mul_f32 per swap-free rotation for a few scalar products, so the packed classes
    fall and the scalar class rises; what must fall is the sum priced with the costs measured on the part
    (profiles/r02_embed_variants.md section 2) and the count with a packed instruction taken as two.  The embed
    configuration, which runs three of its 4.25 sweeps on scaled columns, must be at least 5 % below the parent; the
    sigma-only one runs two of its 3.3 and is only required to be below it.
    Measured: embed 19 564 -> 18 392 priced cycles (-6.0 %), sigma-only 17 073 -> 16 591 (-2.8 %)."""
    names = ("valu", "v_pk_mul_f32", "v_pk_fma_f32", "trans")
    old = dict(zip(names, PARENT[cfg]))
    new, sweeps, per_sweep = cost.count(CFG[cfg], scaled=True)
    print(cfg, "parent", old, "now", {k: round(v, 1) for k, v in new.items()}, "sweeps per wave %.3f" % sweeps, per_sweep)
    assert new["v_pk_mul_f32"] < old["v_pk_mul_f32"] and new["v_pk_fma_f32"] <= old["v_pk_fma_f32"] + 1.0
    assert cost.cycles(new) <= (0.95 if cfg == "embed" else 1.0) * cost.cycles(old)
    simple = lambda d: 2 * (d["v_pk_mul_f32"] + d["v_pk_fma_f32"]) + d["valu"] + d["trans"]
    assert simple(new) < simple(old)
    # the baseline the generator still builds (build(scaled=False)) is the parent's stream: same counts
    if cfg == "sigma":
        base = cost.count(CFG[cfg], scaled=False)[0]
        assert all(abs(base[k] - old[k]) < 0.01 for k in names), base
