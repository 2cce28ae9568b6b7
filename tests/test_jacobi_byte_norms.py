"""The LQ prelude takes its eight row norms from the raw bytes (lq_prelude(byte_norms=True) of tools/gen_jacobi_asm.py:
v_dot4_u32_u8 twice and v_cvt_f32_u32 per row) and is meant to deliver the bits of the packed float chain it replaces.
Checked WITHOUT a GPU through tools/emu_jacobi_asm.py against the stream the generator still builds with the keyword
off: the same row norms, and the same B, n2, sweep count and not-converged mask on every wave."""
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
import tile_diet_inputs as diet       # noqa: E402

WAVES = diet.waves()


def test_the_inputs_are_what_they_claim():
    assert all(t.shape == (64, 8, 8) and t.dtype == np.uint8 for t in WAVES.values())
    assert set(WAVES) == {"noise", "smooth", "constant", "rank1", "zero", "all255", "late_swap"}
    rank = lambda t: np.linalg.matrix_rank(t.astype(np.float64))
    assert all(rank(t) == 1 for t in WAVES["rank1"]) and all(rank(t) == 1 and t.min() == t.max() for t in WAVES["constant"])
    assert not WAVES["zero"].any() and WAVES["all255"].min() == 255
    s = np.linalg.svd(WAVES["late_swap"][:32].astype(np.float64), compute_uv=False)
    assert np.all((np.abs(np.diff(s, axis=1)) < 1e-9 * s[:, :1]).sum(axis=1) >= 3)   # a circulant's singular values pair up
    two = WAVES["late_swap"][32:].astype(np.int32)
    assert np.all(np.abs(two[:, :, 0] - two[:, :, 1]).sum(axis=1) == 1)   # leading columns equal up to one grey level


def test_keyword_off_gives_the_stream_as_it_was():
    """4819 instructions and no s_nop: the stream before the change (its own tests keep running on it unchanged)"""
    old = gen.build(byte_norms=False)
    assert gen.n_instructions(old) == 4819 and old.nops() == 0
    assert not any(ln.startswith(("v_dot4", "v_cvt_f32_u32")) for ln in old.lines)
    st, body = gen.render()
    assert st.nops() == 0 and body == open(gen.csrc_path("wm_jacobi_gfx950.inc")).read()
    assert sum(1 for ln in st.lines if ln.startswith("v_dot4_u32_u8")) == 16


def test_row_norms_from_the_bytes_equal_the_packed_chain():
    for name, t in WAVES.items():
        packed, dot = emu.run_row_norms(t, byte_norms=False), emu.run_row_norms(t, byte_norms=True)
        assert packed.tobytes() == dot.tobytes(), name
        assert np.array_equal(dot.astype(np.int64), (t.astype(np.int64) ** 2).sum(axis=2)), name


@pytest.mark.parametrize("cfg", list(cost.CONFIGS))
def test_same_bits_as_the_stream_with_the_keyword_off(cfg):
    for name, t in WAVES.items():
        s0, s1 = {}, {}
        a0, n0, more0, sw0 = emu.run(t, *cost.CONFIGS[cfg], stats=s0, byte_norms=False)
        a1, n1, more1, sw1 = emu.run(t, *cost.CONFIGS[cfg], stats=s1)
        assert a0.tobytes() == a1.tobytes(), name              # B, bit for bit (NaN and the sign of zero included)
        assert n0.tobytes() == n1.tobytes(), name              # n2
        assert sw0 == sw1 and np.array_equal(more0, more1), name
        # 32 packed instructions become 16 dot products and 8 conversions (one class of the emulator's statistics)
        assert s0["pk"] - s1["pk"] == 32 and s1["dot4"] == 24 and s1["valu"] == s0["valu"], name
