"""GPU tests: the drop-in's files through the reference program, and the reference's files through the drop-in.

They read only tests/golden/reference/ (written by the reference's own embed / extract / detect) and, for the live
part, the byte-compiled program under oracle/_ref/ - never the reference tree.

Bars.  Nothing here is derived from the device's output:

* stego, psnr, ssim, Sc / Sw, detect score, the un-enhanced estimate: the full-frame bars of tests/test_gpu_dropin.py
  (test_fullframe_golden_fixture_through_the_dropin): stego off by at most 1 (colour) / 2 (gray, through YCrCb -> BGR) on
  less than 1e-2 of the pixels, psnr 5e-2, ssim 1e-3, sigma 1e-4 of the largest, score 5e-3, share of estimate pixels off
  by more than 2 below 5e-2;
* watermark factors: U diag(S) Vt within 2e-4 of the largest coefficient and orthonormal to 1e-4
  (tests/test_gpu_fullframe.py), never member by member - the signs are free;
* the ENHANCED watermark image (all the reference writes): the device's chain equals the oracle's bit for bit on equal
  input (tests/test_gpu_enhance.py), but here its input is the device's estimate, and NL-means / CLAHE / unsharp amplify a
  1-LSB difference.  The bar is the oracle chain's own sensitivity, measured on the CPU on these fixtures
  (tests/ref_program.py: enhance(x) against enhance(x +- 1 LSB on 5e-2 of the pixels), 8 seeds x 8 cases; worst mean
  absolute difference 1.8281 grey levels, worst share of pixels off by more than 8 grey levels 0.0451), doubled:
  mean absolute difference <= 3.6562, share off by more than 8 <= 0.0902.

The live part compares CPU with CPU on identical decoded input, so it is bit for bit.
"""
import os

import numpy as np
import pytest

import ref_program as rp
from oracle import wm_oracle as o
from test_reference_program import CASES, RES, WRONG, assert_meta_layout, factor_names, fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core(gpu_ctx):
    import dct_svd_core_secure as c
    return c


@pytest.fixture(scope="module")
def ref():
    return rp.load()


def share_off_by_more_than_2(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8, (a.shape, b.shape)
    return float(np.mean(np.abs(a.astype(int) - b.astype(int)) > 2))


def test_pillow_is_there():
    import PIL
    assert PIL.__version__


@pytest.mark.parametrize("case", CASES)
def test_reference_written_files_through_the_gpu_dropin(core, case, tmp_path):
    """extract(enhance="reference"), extract(normalize=False) and detect of the file-level drop-in on what the reference
    wrote, against the reference's own watermark image and score (and, for the stages the reference does not write, the
    oracle, which tests/test_reference_program.py holds to the reference bit for bit)."""
    c, cover, logo, stego, meta, wm = fixture(case)
    sp, mp = rp.case_path(case, c["stego_file"]), rp.case_path(case, c["meta_file"])
    # what the reference writes: same file name rule, the enhanced image
    out = core.extract(sp, mp, str(tmp_path / c["wm_arg"]), c["password"], c["normalize"], enhance="reference")
    assert os.path.basename(out) == c["wm_file"]
    got = rp.wm_image(out, c["color"])
    rp.assert_enhanced_close(got, wm, case + " vs the reference's file")
    # the stage before the chain, both normalize settings, against the oracle on the same files
    for normalize in (True, False):
        raw = rp.wm_image(core.extract(sp, mp, str(tmp_path / f"raw{int(normalize)}.png"), c["password"], normalize), c["color"])
        want = o.extract_arrays(stego, meta, c["password"], normalize, None)
        share = share_off_by_more_than_2(raw, want)
        print(f"{case} normalize={normalize}: share of estimate pixels off by > 2: {share:.4f}")
        assert share < 5e-2, (case, normalize, share)
        enh = rp.wm_image(core.extract(sp, mp, str(tmp_path / f"enh{int(normalize)}.png"), c["password"], normalize,
                                       enhance="reference"), c["color"])
        rp.assert_enhanced_close(enh, rp.oracle_chain(stego, meta, c["password"], normalize), f"{case} normalize={normalize}")
    ok, score = core.detect(sp, mp)
    print(f"{case}: detect {score:.6f}, reference {c['score']:.6f}")
    assert ok == c["detect"] and abs(score - c["score"]) < 5e-3
    with pytest.raises(ValueError, match=WRONG):
        core.extract(sp, mp, str(tmp_path / "x.png"), c["password"] + "x")
    assert not os.path.exists(str(tmp_path / "x.png"))


@pytest.mark.parametrize("compress_meta", [True, False], ids=["deflated", "stored"])
@pytest.mark.parametrize("case", CASES)
def test_gpu_embed_against_the_reference_embed(core, case, compress_meta, tmp_path):
    """File-level embed(tile=None) with the fixture's nonce against what the reference's embed wrote from the same two
    files: meta layout exactly, the plain members exactly, the numbers under the existing full-frame bars, the returned
    paths the reference's (renaming included)."""
    c, cover, logo, stego, meta, wm = fixture(case)
    color = c["color"]
    sp, mp, ps, ss = core.embed(rp.case_path(case, "cover.png"), rp.case_path(case, "logo.png"), str(tmp_path / c["stego_arg"]),
                                str(tmp_path / "meta.npz"), alpha=c["alpha"], color=color, password=c["password"],
                                kfrac=c["kfrac"], tile=None, nonce=bytes.fromhex(c["nonce"]), compress_meta=compress_meta)
    assert (os.path.basename(sp), os.path.basename(mp)) == (c["stego_file"], c["meta_file"])
    assert os.path.dirname(sp) == os.path.dirname(mp) == str(tmp_path)
    got = rp.load_meta(mp)                                               # np.load(allow_pickle=False), the reference's reader
    assert_meta_layout(got, meta)
    for k in ("shape", "alpha", "kfrac", "nonce", "mode", "payload_type"):
        assert got[k].tobytes() == meta[k].tobytes(), k
    assert str(got["mode"]) == str(meta["mode"]) and str(got["payload_type"]) == "image"
    H, W = c["cover"]
    L = min(H, W)
    for s, u, v, sw in factor_names(color):
        for k in (s, sw):
            a, b = got[k], meta[k]
            rel = float(np.max(np.abs(a - b)) / b[0])
            print(f"{case} {k}: max |d sigma| / sigma_0 = {rel:.2e}")
            assert a.shape == b.shape and rel < 1e-4, (k, rel)
        rec = (got[u] * got[sw]) @ got[v]
        want = (meta[u] * meta[sw]) @ meta[v]
        assert np.abs(rec - want).max() < 2e-4 * np.abs(want).max(), u
        assert np.abs(got[u].T @ got[u] - np.eye(L)).max() < 1e-4 and np.abs(got[v] @ got[v].T - np.eye(L)).max() < 1e-4
    st = rp.read_png(sp)
    d = np.abs(st.astype(int) - stego.astype(int))
    print(f"{case}: stego max diff {int(d.max())}, share {float(np.mean(d != 0)):.4f}, psnr {ps:.4f} vs {c['psnr']:.4f}, "
          f"ssim {ss:.6f} vs {c['ssim']:.6f}")
    assert d.max() <= (1 if color else 2) and np.mean(d != 0) < 1e-2
    assert abs(ps - c["psnr"]) < 5e-2 and abs(ss - c["ssim"]) < 1e-3
    # the digest the drop-in stored authenticates ITS factors under the reference's rule (order and bytes of the parts)
    key = o.derive_key(c["password"], bytes.fromhex(c["nonce"]))
    f = factor_names(color)
    parts = [got[t[0]] for t in f] + [got[t[1]] for t in f] + [got[t[2]] for t in f]
    assert o.hmac_digest(key, [p.tobytes() for p in parts]) == got["digest"].tobytes()


@rp.needs_program
@pytest.mark.parametrize("compress_meta", [True, False], ids=["deflated", "stored"])
@pytest.mark.parametrize("case", CASES)
def test_gpu_written_files_through_the_reference_program(core, ref, case, compress_meta, tmp_path):
    """The reference's extract and detect open the drop-in's stego.png + meta.npz (both meta forms).  They must not
    raise - the HMAC check passing proves the byte layout of the factors - and must equal, bit for bit, what the oracle
    gives on the same decoded arrays (CPU against CPU on identical input).  The score also stays within the existing
    bar of the reference's own on its own files."""
    c = RES["cases"][case]
    sp, mp, _, _ = core.embed(rp.case_path(case, "cover.png"), rp.case_path(case, "logo.png"), str(tmp_path / c["stego_arg"]),
                              str(tmp_path / "meta.npz"), alpha=c["alpha"], color=c["color"], password=c["password"],
                              kfrac=c["kfrac"], tile=None, nonce=bytes.fromhex(c["nonce"]), compress_meta=compress_meta)
    ref.log.clear()
    wp = ref.extract(sp, mp, str(tmp_path / c["wm_arg"]), c["password"], c["normalize"])
    ok, score = ref.detect(sp, mp)
    assert ref.log.errors == []
    assert os.path.basename(wp) == c["wm_file"]
    stego, meta = rp.read_png(sp), rp.load_meta(mp)
    assert np.array_equal(rp.wm_image(wp, c["color"]), rp.oracle_chain(stego, meta, c["password"], c["normalize"]))
    assert (ok, score) == o.detect_arrays(stego, meta, 0.6, None)
    assert ok == c["detect"] and abs(score - c["score"]) < 5e-3
    with pytest.raises(ValueError, match=WRONG):
        ref.extract(sp, mp, str(tmp_path / "x.png"), c["password"] + "x")


@rp.needs_program
@pytest.mark.parametrize("color", [False, True], ids=["gray", "colour"])
def test_tile_mode_meta_is_not_a_reference_file(core, ref, color, tmp_path):
    """tile=8 is the project's own formulation: its meta holds per-tile factors ([nby, nbx, 8] sigmas).  The reference
    authenticates it (the digest rule is the same) and then fails on the shapes with NumPy's broadcasting ValueError -
    it neither reads it nor mistakes it for a wrong password.  The drop-in's documentation says so."""
    case = "color_32x48_x2" if color else "gray_40x56_mixed"
    c = RES["cases"][case]
    sp, mp, _, _ = core.embed(rp.case_path(case, "cover.png"), rp.case_path(case, "logo.png"), str(tmp_path / "stego.png"),
                              str(tmp_path / "meta.npz"), alpha=c["alpha"], color=color, password=c["password"],
                              kfrac=c["kfrac"], tile=8, nonce=bytes.fromhex(c["nonce"]))
    assert int(rp.load_meta(mp)["tile"]) == 8
    with pytest.raises(ValueError, match="broadcast") as e:
        ref.extract(sp, mp, str(tmp_path / "w.png"), c["password"])
    assert WRONG not in str(e.value)
    with pytest.raises(ValueError, match="broadcast"):
        ref.detect(sp, mp)
    with pytest.raises(ValueError, match=WRONG):                             # authentication still comes first
        ref.extract(sp, mp, str(tmp_path / "w.png"), c["password"] + "x")
    assert "not readable by the reference" in " ".join(core._impl.__doc__.split())
    assert core.detect(sp, mp)[0]                                            # the drop-in reads its own tile-mode files
