"""Waves shared by tests/test_jacobi_byte_norms.py, tests/test_jacobi_sigma_scaled.py and tests/test_gpu_tile_diet.py:
one wave (64 tiles) per content kind, and a wave in which some lane wants the de Rijk swap inside a TESTED sweep, so that
both paths of the sigma-only stream's tested rotation run."""
import numpy as np

import scaled_rotation_inputs as inp


def late_swap_wave():
    """Lanes 0 .. 31: circulant tiles.  A real circulant's singular values come in exactly equal pairs (|DFT| of its first
    row, bins k and 8 - k), the tracked norms of such a pair differ by rounding only, and in the first tested sweep of both
    the embed and the sigma-only configuration some lane finds the later column the larger one.  Lanes 32 .. 63: noise
    tiles whose two leading columns are equal up to one grey level - behind the LQ prelude these alone never swap that
    late (the prelude grades the columns), they are the company the swapping lanes keep in the wave."""
    rng = np.random.default_rng(0)
    t = np.zeros((64, 8, 8), np.uint8)
    for i in range(32):
        c = rng.integers(0, 256, 8)
        t[i] = np.array([np.roll(c, k) for k in range(8)], dtype=np.uint8)
    t[32:] = rng.integers(0, 256, (32, 8, 8), dtype=np.uint8)
    t[32:, :, 1] = t[32:, :, 0]
    t[np.arange(32, 64), rng.integers(0, 8, 32), 1] ^= 1
    return t


def waves():
    """name -> uint8 [64, 8, 8]"""
    rng = np.random.default_rng(77)
    w = {"noise": inp.tiles("noise", 64, 3), "smooth": inp.tiles("natural", 64, 7)}
    w["constant"] = np.repeat(rng.integers(1, 256, 64).astype(np.uint8), 64).reshape(64, 8, 8)
    w["rank1"] = np.stack([np.outer(rng.integers(1, 16, 8), rng.integers(1, 16, 8)) for _ in range(64)]).astype(np.uint8)
    w["zero"] = np.zeros((64, 8, 8), np.uint8)
    w["all255"] = np.full((64, 8, 8), 255, np.uint8)
    w["late_swap"] = late_swap_wave()
    return w
