"""The swap-free path of the scaled rotation updates the two tracked norms in place (rotation_scaled(swapfree=True) of
tools/gen_jacobi_asm.py): it runs only where n2[q] - n2[p] <= 0 in every lane of the wave, so max(n2[p], n2[q]) is n2[p]
and the min is n2[q], and the two instructions that took them move into the swap branch.  Checked WITHOUT a GPU through
tools/emu_jacobi_asm.py: the committed stream against the one the generator still builds with max / min ahead of the
branch (build(swapfree=False)) - the same bits out, exactly two scalar VALU instructions fewer per swap-free scaled
rotation, nothing else moved."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import emu_jacobi_asm as emu          # noqa: E402
import jacobi_stream_cost as cost     # noqa: E402
import scaled_rotation_inputs as inp  # noqa: E402


def _waves():
    """the 40 noise waves of the cost tool, then one wave each of smooth, constant, rank-1 and all-zero tiles"""
    rng = np.random.default_rng(77)
    w = {f"noise{i}": t for i, t in enumerate(cost.noise_waves())}
    w["smooth"] = inp.tiles("natural", 64, 7)
    w["constant"] = np.repeat(rng.integers(1, 256, 64).astype(np.uint8), 64).reshape(64, 8, 8)
    w["rank1"] = np.stack([np.outer(rng.integers(1, 16, 8), rng.integers(1, 16, 8)) for _ in range(64)]).astype(np.uint8)
    w["zero"] = np.zeros((64, 8, 8), np.uint8)
    return w


WAVES = _waves()
_RUNS = {}


def _run(name, cfg, swapfree):
    """one emulator run per (wave, configuration, body), shared by the tests"""
    key = (name, cfg, swapfree)
    if key not in _RUNS:
        st = {}
        a, n2, more, sweeps = emu.run(WAVES[name], *cost.CONFIGS[cfg], stats=st, swapfree=swapfree)
        _RUNS[key] = (a, n2, more, sweeps, st)
    return _RUNS[key]


def test_the_inputs_are_what_they_claim():
    assert len(WAVES) == 44 and all(t.shape == (64, 8, 8) and t.dtype == np.uint8 for t in WAVES.values())
    rank = lambda t: np.linalg.matrix_rank(t.astype(np.float64))
    assert all(rank(t) == 1 for t in WAVES["rank1"]) and all(rank(t) == 1 and t.min() == t.max() for t in WAVES["constant"])
    assert not WAVES["zero"].any() and all(rank(t) == 8 for t in WAVES["smooth"][:8])


@pytest.mark.parametrize("cfg", list(cost.CONFIGS))
def test_same_bits_as_the_stream_with_max_and_min_ahead_of_the_branch(cfg):
    for name in WAVES:
        a0, n0, more0, sw0, _ = _run(name, cfg, False)
        a1, n1, more1, sw1, _ = _run(name, cfg, True)
        assert a0.tobytes() == a1.tobytes(), name              # B, bit for bit (NaN and the sign of zero included)
        assert n0.tobytes() == n1.tobytes(), name              # n2
        assert sw0 == sw1 and np.array_equal(more0, more1), name


@pytest.mark.parametrize("cfg", list(cost.CONFIGS))
def test_two_scalar_instructions_fewer_per_swapfree_scaled_rotation(cfg):
    """Counted from the emulator's own statistics: ("rot", k) rotations carried out in sweep k, ("swap", k) those of
    them that took the swap branch; the scaled rotations are those of the untested sweeps, the first min_sweeps - 1."""
    untested = cost.CONFIGS[cfg][2] - 1
    total = 0
    for name in WAVES:
        old, new = _run(name, cfg, False)[4], _run(name, cfg, True)[4]
        swapfree = sum(new.get(("rot", k), 0) - new.get(("swap", k), 0) for k in range(untested))
        assert all(old.get((w, k), 0) == new.get((w, k), 0) for w in ("rot", "swap") for k in range(12)), name
        assert old["valu"] - new["valu"] == 2 * swapfree, (name, old["valu"], new["valu"], swapfree)
        assert all(old.get(k, 0) == new.get(k, 0) for k in ("pk", "v_pk_mul_f32", "v_pk_fma_f32", "trans")), name
        total += swapfree if name.startswith("noise") else 0
    print(f"{cfg}: {total / 40:.1f} swap-free scaled rotations per noise wave of {28 * untested}")
    assert total / 40 > 0.75 * 28 * untested                   # the path the change is about is the common one
