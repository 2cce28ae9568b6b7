"""1 / c^2 of the swap-free scaled rotation from one v_rcp_f32 (build(rcp=True)) and the sigma-only stream whose columns
stay scaled to the end (build(sigma_only=True), written to csrc/wm_jacobi_sigma_gfx950.inc when the library is built), checked WITHOUT a GPU through
tools/emu_jacobi_asm.py against float64 LAPACK and against the streams with the keywords off: every singular value
within the float32 floor of 2e-6 sigma_1 wherever the old stream's is, no fold of the scales in the sigma-only stream
(but the one that keeps them in range on the way to the sweep bound), scales finite at that bound, and the
not-converged mask of rank-deficient lanes as before."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import emu_jacobi_asm as emu          # noqa: E402
import gen_jacobi_asm as gen          # noqa: E402
import jacobi_stream_cost as cost     # noqa: E402
import scaled_rotation_inputs as inp  # noqa: E402
import tile_diet_inputs as diet       # noqa: E402

WAVES = dict(diet.waves(), quantised=inp.tiles("quantised", 64, 5), posterised=inp.tiles("posterised", 64, 6))
RANK_DEFICIENT = ("constant", "rank1", "zero", "all255")
# (configuration, keywords of the old stream, keywords of the new one)
# C is committed in the sigma-only stream alone; on the stream that hands out B it is only interpreted here
BUILDS = {"embed, C": ("embed", dict(), dict(rcp=True)),
          "sigma, C": ("sigma", dict(), dict(rcp=True)),
          "sigma, C + D": ("sigma", dict(), dict(sigma_only=True))}
_RUNS, _REF = {}, {}


def _run(name, cfg, **kw):
    key = (name, cfg) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        st, end = {}, []
        a, n2, more, sweeps = emu.run(WAVES[name], *cost.CONFIGS[cfg], stats=st, end_scales=end, **kw)
        _RUNS[key] = (n2, more, sweeps, st, end[0])
    return _RUNS[key]


def _err(name, n2):
    """|sigma - LAPACK's| / sigma_1 per value (sigma_1 at least one grey level), [64, 8]"""
    if name not in _REF:
        _REF[name] = np.linalg.svd(WAVES[name].astype(np.float64), compute_uv=False)
    ref = _REF[name]
    return np.abs(np.sqrt(np.maximum(n2.astype(np.float64), 0)) - ref) / ref[:, :1].clip(1)


# csrc/wm_jacobi_sigma_gfx950.inc is generated when the library is built and not committed (gen_jacobi_asm.write_sigma says
# why).  Its fingerprint is: whoever changes the generator so that the sigma-only kernels run other instructions changes
# these two values in the same diff.
SIGMA_STREAM_INSTRUCTIONS = 5826
SIGMA_STREAM_SHA256 = "f387d9e847fa0c402632332e8367b879f2886df3327f9a5b8e164b3ac253c4f2"


def test_the_sigma_stream_as_generated():
    import hashlib
    st, body = gen.render_sigma()
    assert st.nops() == 0 and "jacobi_sigma_gfx950" in body
    assert gen.n_instructions(st) == SIGMA_STREAM_INSTRUCTIONS
    assert hashlib.sha256(body.encode()).hexdigest() == SIGMA_STREAM_SHA256
    out = gen.csrc_path("wm_jacobi_sigma_gfx950.inc")
    if os.path.exists(out):                                # a built tree: what was compiled is what the generator gives
        assert open(out).read() == body
    assert sum(1 for ln in st.lines if ln.startswith("v_rcp_f32")) == 2 * 28      # untested and tested bodies
    assert not any(ln.startswith("v_rcp_f32") for ln in gen.build().lines)         # the stream that hands out B: as it was


@pytest.mark.parametrize("build", list(BUILDS))
def test_singular_values_against_lapack(build):
    cfg, off, on = BUILDS[build]
    for name in WAVES:
        e0, e1 = _err(name, _run(name, cfg, **off)[0]), _err(name, _run(name, cfg, **on)[0])
        print(f"{build:13s} {name:10s} worst error / sigma_1: keyword off {e0.max():.2e}, on {e1.max():.2e}; sweeps "
              f"{_run(name, cfg, **off)[2]} / {_run(name, cfg, **on)[2]}")
        assert np.isfinite(_run(name, cfg, **on)[0]).all(), name
        assert np.all(e1[e0 <= 2e-6] <= 2e-6), (name, float(e1.max()))
        assert not _run(name, cfg, **on)[1].any(), name                   # converged within the bound, as before


def test_rcp_saves_one_instruction_per_swapfree_scaled_rotation():
    for cfg in cost.CONFIGS:
        untested = cost.CONFIGS[cfg][2] - 1
        old, new = _run("noise", cfg)[3], _run("noise", cfg, rcp=True)[3]
        if all(old.get((w, k), 0) == new.get((w, k), 0) for w in ("rot", "swap") for k in range(12)):   # same path taken
            free = sum(new.get(("rot", k), 0) - new.get(("swap", k), 0) for k in range(untested))
            swaps = sum(new.get(("swap", k), 0) for k in range(untested))
            assert old["valu"] - new["valu"] == free and new["trans"] - old["trans"] == swaps


def test_both_paths_of_the_tested_scaled_rotation_run():
    """from the emulator's branch trace, on the wave whose circulant tiles want a swap in a tested sweep: ("rot", k)
    rotations carried out in sweep k, ("swap", k) those of them that entered the four-product swap branch"""
    st = _run("late_swap", "sigma", sigma_only=True)[3]
    tested = range(cost.CONFIGS["sigma"][2] - 1, 12)
    rot, swap = (sum(st.get((w, k), 0) for k in tested) for w in ("rot", "swap"))
    print(f"{rot} tested rotations carried out on the late-swap wave, {swap} of them through the swap branch")
    assert swap >= 1 and rot - swap >= 1


def test_the_sigma_only_stream_never_folds():
    for name in WAVES:
        n2, more, sweeps, st, end = _run(name, "sigma", sigma_only=True)
        assert sweeps <= gen.SIGMA_FOLD_AT and st.get("fold", 0) == 0, (name, sweeps)
        assert np.isfinite(end).all() and (end > 0).all(), name
        assert _run(name, "sigma")[3].get("fold", 0) == 1                      # the stream that hands out B folds once
    w = _run("noise", "sigma", sigma_only=True)[4]
    assert w.min() < 0.9 and w.max() > 1.1                                     # the scales really are left in place


@pytest.mark.parametrize("name", RANK_DEFICIENT + ("noise",))
def test_scales_stay_finite_at_the_sweep_bound(name):
    """all 12 sweeps forced: eleven untested ones and a tested one (min_sweeps = 12), and, on the noise wave, ten tested
    ones that can never pass (conv2 = 0).  The scales are folded into B once, ahead of the 7th sweep's norms."""
    runs = [(1e-2, 1e-8, 12, 2)] + ([(0.0, 0.0, 3, 2)] if name == "noise" else [])
    for conv2, skip2, minsw, skipfrom in runs:
        st, end = {}, []
        a, n2, more, sweeps = emu.run(WAVES[name], conv2, skip2, minsw, skipfrom, stats=st, end_scales=end, sigma_only=True)
        assert sweeps == 12 and st["fold"] == 1, (sweeps, st.get("fold"))
        assert np.isfinite(end[0]).all() and (end[0] > 0).all() and np.isfinite(a).all() and np.isfinite(n2).all()
        assert 2.0 ** -42 <= end[0].min() and end[0].max() <= 2.0 ** 42
        e = _err(name, n2)
        print(f"{name}: 12 sweeps (conv2 {conv2:g}, min_sweeps {minsw}), scales in [{end[0].min():.2e}, {end[0].max():.2e}], "
              f"worst error {e.max():.2e} sigma_1")
        assert e.max() <= 2e-6


@pytest.mark.parametrize("name", RANK_DEFICIENT + ("posterised", "noise"))
def test_rank_deficient_lanes_leave_the_mask_from_the_sixth_sweep_on(name):
    """conv2 = 0 keeps every lane with a non-zero dot product 'not converged'.  The stream that hands out B and the
    sigma-only one then stop after the same sweep with the same mask: the rank-1 wave, whose null columns are rounding
    residue, exactly when DEFI_FROM sweeps are done; the full-rank noise wave at the bound with its lanes still in the
    mask; the posterised wave (both kinds of tile) at the bound with only its full-rank stragglers in it."""
    out = {}
    for tag, kw in (("old", dict()), ("sigma_only", dict(sigma_only=True))):
        a, n2, more, sweeps = emu.run(WAVES[name], 0.0, 0.0, 3, 2, **kw)
        out[tag] = (sweeps, more.copy())
    assert out["old"][0] == out["sigma_only"][0] and np.array_equal(out["old"][1], out["sigma_only"][1]), out
    sweeps, more = out["sigma_only"]
    if name == "rank1":
        assert sweeps == gen.DEFI_FROM and not more.any()
    if name in RANK_DEFICIENT:
        assert sweeps <= gen.DEFI_FROM and not more.any()
    if name == "noise":
        assert sweeps == gen.MAX_SWEEPS and more.sum() > 32
    if name == "posterised":
        full_rank = np.linalg.matrix_rank(WAVES[name].astype(np.float64)) == 8
        assert sweeps == gen.MAX_SWEEPS and not more[~full_rank].any()
