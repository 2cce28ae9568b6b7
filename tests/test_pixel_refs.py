"""CPU: the tools of tests/test_gpu_pixel_edges.py (tests/pixel_refs.py) checked on their own - the permutation builders
are bijections and produce the route cells they exist for, the float64 SSIM agrees with the oracle on the flat and
two-level inputs, the reference normalise gives the 0 / 255 patterns the include_zero cases rely on."""
import numpy as np
import pytest

import pixel_refs as pr
from oracle import wm_oracle as o

S = pr.S


@pytest.mark.parametrize("n", pr.ROUTE_SIZES)
def test_every_builder_returns_a_bijection(n):
    perms = pr.permutations_for(n)
    assert len(perms) >= 6
    for name, idx in perms:
        assert idx.dtype == np.int64 and pr.is_bijection(idx), (n, name)
        inv = pr.inverse(idx)
        assert np.array_equal(inv[idx], np.arange(n)) and np.array_equal(idx[inv], np.arange(n)), (n, name)
    names = {name for name, _ in perms}
    assert ("block-transpose" in names) == (n % S == 0 and n > S)
    assert ("fill-last" in names) == ("fill-last-inverse" in names) == (n % S != 0 and n > S)


def test_is_bijection_refuses_what_is_not_one():
    bad = np.arange(10); bad[3] = 4
    assert not pr.is_bijection(bad)
    assert not pr.is_bijection(np.arange(1, 11))
    assert pr.is_bijection(np.array([0]))


def test_builders_produce_the_cells_they_are_there_for():
    n = 3 * S + 5
    r, nb = n % S, pr.n_blocks(n)
    full = np.array([S] * (nb - 1) + [r])

    c = pr.cell_counts(pr.perm_identity(n))                     # whole blocks stay: cells of S, n mod S and 0
    assert np.array_equal(np.diag(c), full) and c.sum() == n and np.count_nonzero(c) == nb
    assert np.array_equal(pr.cell_counts(pr.perm_block_local(n, 1)), c)

    c = pr.cell_counts(pr.perm_reversal(n))                     # block a lands on blocks nb-1-a and nb-2-a: cells of r and S - r
    assert c[0, nb - 1] == r and c[0, nb - 2] == S - r and c[nb - 1, 0] == r and c[0, 0] == 0

    c = pr.cell_counts(pr.perm_rotation(n, 1))                  # one element per block crosses over: cells of 1 and S - 1
    assert c[0, 1] == 1 and c[0, 0] == S - 1 and c[nb - 1, 0] == 1 and c[nb - 1, nb - 1] == r - 1 and c[0, 2] == 0

    c = pr.cell_counts(pr.perm_rotation(n, S - 1))              # all but one element move on one block
    assert c[0, 1] == S - 1 and c[0, 0] == 1

    k = pr.coprime_above(n)
    assert k > S and np.gcd(k, n) == 1
    c = pr.cell_counts(pr.perm_multiply(n))                     # a stride above S: every full block is spread over all full blocks,
    assert c[:nb - 1, :nb - 1].min() > S // 4 and c.max() < S // 2      # the 5-element last block gets and gives cells of 0 .. 3
    assert c[nb - 1].max() <= 3 and c[:, nb - 1].max() <= 3 and 0 in c[:, nb - 1]

    f = pr.perm_fill_last_block(n)                              # the last block is filled from ONE source block
    c = pr.cell_counts(f)
    assert c[0, nb - 1] == r and c[1:, nb - 1].sum() == 0 and c[0].sum() == S and c[nb - 1, nb - 1] == 0
    ci = pr.cell_counts(pr.inverse(f))                          # ... and in the inverse it empties into one block
    assert np.array_equal(ci, c.T) and ci[nb - 1, 0] == r and np.count_nonzero(ci[nb - 1]) == 1

    c = pr.cell_counts(pr.perm_block_transpose(3))              # n = 3 S: i -> (i mod 3) S + i // 3
    assert c.shape == (3, 3) and c.min() >= S // 3 and c.max() <= S // 3 + 1
    t = pr.perm_block_transpose(3)
    assert t[0] == 0 and t[1] == S and t[2] == 2 * S and t[3] == 1

    for n1 in (S - 1, S, 17, 1):                                # one block: one cell with everything in it
        for name, idx in pr.permutations_for(n1):
            assert pr.cell_counts(idx).tolist() == [[n1]], (n1, name)
    c = pr.cell_counts(pr.perm_rotation(S + 1, 1))              # a last block of ONE element
    assert c.tolist() == [[S - 1, 1], [1, 0]]
    c = pr.cell_counts(pr.perm_fill_last_block(S + 1))
    assert c.tolist() == [[S - 1, 1], [1, 0]]
    c = pr.cell_counts(pr.perm_fill_last_block(2 * S - 1))      # S - 1 of S elements of block 0 go to the last block
    assert c.tolist() == [[1, S - 1], [S - 1, 0]]


def test_scramble_and_unscramble_are_inverse_statements():
    rng = np.random.default_rng(3)
    for name, idx in pr.permutations_for(2 * S + 1):
        x = rng.normal(0, 50, idx.size).astype(np.float32)
        g = rng.integers(0, 256, idx.size, dtype=np.uint8)
        assert np.array_equal(pr.unscramble(pr.scramble(x, idx), idx), x), name
        s = pr.scramble(g, idx)
        assert s.dtype == np.float32 and np.array_equal(s, o.permute(g.reshape(1, -1).astype(np.float32), idx).ravel()), name
        assert np.array_equal(pr.unscramble(x, idx), o.unpermute(x.reshape(1, -1), idx).ravel()), name


def test_float64_ssim_agrees_with_the_oracle_on_every_ssim_input():
    pairs = pr.ssim_pairs(200, 300)
    assert len(pairs) == 9
    for name, a, b in pairs:
        combos = pr.dtype_combinations(a, b)
        assert len(combos) == (4 if b.dtype == np.uint8 else 2)
        for x, y in combos:
            assert np.array_equal(x.astype(np.float64), a.astype(np.float64)) and np.array_equal(y.astype(np.float64), b.astype(np.float64))
        want = pr.ssim64(a, b)
        assert abs(o.ssim(a, b) - want) < 1e-5, (name, o.ssim(a, b), want)
    named = dict((p[0], p[1:]) for p in pairs)
    assert pr.ssim64(*named["white-white"]) == pytest.approx(1.0, abs=1e-12)
    assert pr.ssim64(*named["logo-logo"]) == pytest.approx(1.0, abs=1e-12)
    assert pr.ssim64(*named["checker-inverse"]) < -0.5
    assert 0.0 < pr.ssim64(*named["black-white"]) < 1e-3
    assert set(np.unique(named["logo-logo"][0])) == {0, 255}
    assert np.count_nonzero(named["logo-lsb"][0] != named["logo-lsb"][1]) == 40
    # random content: the two forms are the same statement
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (45, 70), dtype=np.uint8); b = rng.integers(0, 256, (45, 70), dtype=np.uint8)
    assert abs(o.ssim(a, b) - pr.ssim64(a, b)) < 1e-5
    small = rng.integers(0, 256, (7, 9), dtype=np.uint8)        # smaller than the window: reflect-101 folds more than once
    assert abs(o.ssim(small, small[::-1].copy()) - pr.ssim64(small, small[::-1].copy())) < 1e-5


@pytest.mark.parametrize("shape", [(1080, 1920), (2160, 3840)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_float64_ssim_agrees_with_the_oracle_on_the_large_inputs(shape):
    pairs = pr.ssim_large_pairs(*shape)
    assert [p[0] for p in pairs] == ["logo-logo", "logo-lsb", "white-noisy"]
    for name, a, b in pairs:
        assert abs(o.ssim(a, b) - pr.ssim64(a, b)) < 1e-5, name


def test_reference_normalise_gives_the_include_zero_patterns():
    for (H, W) in ((8, 9), (15, 15), (70, 101), (64, 101), (70, 96)):
        m = pr.grid_mask(H, W)
        assert m.sum() == (H // 8) * (W // 8) * 64 and not m.all()
        for v in (64.0, 3.0, 1600.0, 0.5):
            pos = pr.normalize_u8(pr.constant_grid_estimate(H, W, v))
            assert (pos[m] == 255).all() and (pos[~m] == 0).all(), (H, W, v)
            neg = pr.normalize_u8(pr.constant_grid_estimate(H, W, -v))
            assert (neg[m] == 0).all() and (neg[~m] == 255).all(), (H, W, v)
        # whatever the constant, float32 rounding of v * (255 / v) costs at most the last byte
        for v in np.random.default_rng(H).uniform(1, 5000, 50).astype(np.float32):
            pos = pr.normalize_u8(pr.constant_grid_estimate(H, W, v))
            assert (pos[m] >= 254).all() and (pos[~m] == 0).all() and np.unique(pos[m]).size == 1
    # without the border a constant plane has range 0: zeros
    assert not pr.normalize_u8(pr.constant_grid_estimate(16, 24, 64.0)).any()
    assert pr.grid_mask(16, 24).all() and not pr.grid_mask(7, 40).any()


def test_reference_normalise_edge_values():
    f = np.float32
    assert pr.normalize_u8(np.array([-3e38, 3e38], f)).tolist() == [0, 255]         # float32 subtraction overflows: inf * scale
    assert pr.normalize_u8(np.array([-0.0, 0.0], f)).tolist() == [0, 0]
    assert pr.normalize_u8(np.array([-5, -1, -3], f)).tolist() == [0, 255, 127]
    assert pr.normalize_u8(np.array([7.5] * 5, f)).tolist() == [0] * 5
    assert pr.normalize_u8(np.array([0, 1e-40], f)).tolist() == [0, 0]              # a denormal range is below the epsilon
    assert pr.normalize_u8(np.array([0, 2.0e-16], f)).tolist() == [0, 0]
    assert pr.normalize_u8(np.array([0, 2.5e-16], f)).tolist()[0] == 0 and pr.normalize_u8(np.array([0, 2.5e-16], f))[1] >= 254
    assert pr.normalize_u8(np.array([-2.0 ** 100, 0, 2.0 ** 100], f)).tolist() == [0, 127, 255]
    assert pr.normalize_u8(np.array([-1e30, 0, 1e30], f)).tolist() == [0, 127, 254]  # 2e30 * float32(255 / 2e30) rounds below 255
    assert pr.normalize_u8(np.array([-4, 300.7, 12.9], f), False).tolist() == [0, 255, 12]


def test_single_entry_factors_make_constant_tiles():
    """the oracle's own extract on such factors: one constant per tile, its sign that of Uw[0][0], zeros outside the grid"""
    H, W = 18, 27
    nby, nbx = H // 8, W // 8
    stego = np.full((H, W), 200, np.float32)
    sc = 0.5 * o.stego_sigma(stego, 8)
    for sign in (1.0, -1.0):
        U, V = pr.single_entry_factors(nby, nbx, sign)
        assert np.count_nonzero(U) == nby * nbx == np.count_nonzero(V)
        w = o.extract_plane(stego, sc, U, V, 0.5, 0.0, H, W, 8, k_floor=1)
        m = pr.grid_mask(H, W)
        assert not w[~m].any() and (np.sign(w[m]) == sign).all()
        assert np.abs(w[m] - w[0, 0]).max() <= 1e-4 * abs(w[0, 0])
        out = pr.normalize_u8(w)
        assert (out[m] >= 254).all() if sign > 0 else (out[~m] >= 254).all()
        assert not (out[~m].any() if sign > 0 else out[m].any())
