"""Blind payload with keyed dither on the device, on the edge host (constant tiles, s_1 = s_2, ramps, a black tile) and the
host of tiles pinned by clipping: the checks of tests/test_gpu_payload_dither.py, with the decoded bits wrong exactly where
the restatement's are and nowhere else (the pattern of tests/test_gpu_payload_edges.py).  The left-out tiles are capped at
half of these hosts; tests/test_payload_dither.py asserts on the restatement that the inputs stay within it."""
import numpy as np
import pytest

import payload_dither_refs as dr
import payload_refs as pr
from test_gpu_payload_dither import check_against_the_restatement

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_bits", [0, 16], ids=["n_tiles", "16"])
@pytest.mark.parametrize("delta", [16.0, 24.0, 200.0])
@pytest.mark.parametrize("name", ["edge", "pinned"])
def test_edge_and_pinned_hosts_against_the_restatement(gpu_ctx, name, delta, n_bits):
    st = check_against_the_restatement(gpu_ctx, name, delta, n_bits, exact_votes=False)
    r = dr.margins(name, delta, 0, n_bits)
    if name == "pinned":
        # pinned tiles vote wrong with dither as without: the restatement has such tiles here, and the device the same ones
        assert (r["signed"][r["comparable"]] < 0).any()
    else:
        # a constant tile stays constant: sigma_1 of its stego is 8 x a gray level
        flat = np.zeros(16, bool); flat[:10] = True; flat[15] = True
        T = pr.o.to_tiles(st).reshape(16, 64)
        assert np.all(T[flat] == T[flat][:, :1])
