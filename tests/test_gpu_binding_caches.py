"""The binding's device caches on the device: one Context cycles three keys of each kind - permutation index (with its
route), payload CSR map, shared dither table - twice, so that every entry is uploaded, used, evicted and uploaded again,
with a per-plane dither table (staged for the one call) beside them.  Every result equals, byte for byte, the same call on
a Context that has seen nothing else.  The index passes move values without arithmetic, and payload_soft is a fixed-order
float64 reduction without atomics, so two runs of the one kernel on the same bytes may be compared with ==."""
import importlib

import numpy as np
import pytest

import payload_refs as pr
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

hg = importlib.import_module(PKG_NAME + ".hostglue")

H, W = 64, 96                     # 96 tiles: the smallest frame that holds the 64-bit minimum payload frame
N_TILES, N_BITS, DELTA = 96, 64, 16.0
PASSWORDS = ("first", "second", "third")
NAMES = ("scrambled", "unscrambled", "stego/shared", "sigma_c/shared", "soft/shared", "stego/rows", "sigma_c/rows", "soft/rows")


def _visit(ctx, planes, k):
    """what key k gives on these planes, through the index cache, the CSR cache and the dither cache"""
    n = planes.shape[0]
    idx = hg.permutation_index(H, W, hg.derive_key(PASSWORDS[k], bytes(8)))
    scrambled = ctx.permute_planes(planes, idx)
    back = ctx.unpermute_normalize_u8(scrambled, idx, normalize=False)
    tbi, order, offs = pr.simple_map(N_TILES, N_BITS, seed=5 + k)
    tile_bit = pr.seeded_bits(N_BITS, k)[tbi]
    rng = np.random.default_rng(20 + k)
    out = [scrambled, back]
    for shape in ((N_TILES,), (n, N_TILES)):                                # shared by the planes (cached); a row per plane
        table = rng.integers(0, 1 << 16, shape).astype(np.uint16)
        stego, sc, _ = ctx.embed_tiles_payload(planes, tile_bit, DELTA, dither=table)
        out += [stego, sc, ctx.payload_soft(stego, order, offs, N_BITS, DELTA, dither=table)]
    return out


@pytest.mark.parametrize("n", [1, 3])
def test_evicted_and_rebuilt_entries_give_what_a_fresh_context_gives(hostapi, n):
    planes = np.random.default_rng(n).integers(0, 256, (n, H, W), dtype=np.uint8)
    fresh = []
    for k in range(3):
        with hostapi.Context(0) as ctx:
            fresh.append(_visit(ctx, planes, k))
        assert fresh[k][0].dtype == np.float32 and np.array_equal(fresh[k][1], planes)     # the index passes invert
        assert not np.array_equal(fresh[k][0], planes) and np.any(fresh[k][4] != 0) and np.any(fresh[k][7] != 0)
    assert not np.array_equal(fresh[0][0], fresh[1][0]) and not np.array_equal(fresh[0][4], fresh[1][4])
    with hostapi.Context(0) as ctx:
        for visit in range(2):                                              # two entries a kind: every visit is a miss
            for k in range(3):
                for name, got, want in zip(NAMES, _visit(ctx, planes, k), fresh[k]):
                    assert got.dtype == want.dtype and got.shape == want.shape, (visit, k, name)
                    assert got.tobytes() == want.tobytes(), (visit, k, name)
