"""The oracle, the host glue and the file formats held to the REFERENCE PROGRAM itself (no GPU).

Two halves:

* from the committed fixtures alone (tests/golden/reference/, written by the reference's own embed / extract / detect:
  tests/golden/make_reference_golden.py) - these run everywhere;
* live, where oracle/_ref/ holds the byte-compiled reference module (oracle/ref_build.py; ``build()`` makes it where the
  reference tree is present): the program runs in this process over the stand-in cv2 (tests/cv2_standin.py), both
  sides call the same np.linalg.svd on identical bytes, so every comparison is BIT FOR BIT.  Skipped only when the
  compiled file is absent.

What this pins: the reference's program logic (everything that is not a cv2.* call) and its file formats.  What it
does not: OpenCV's own arithmetic - the stand-in IS the project's restatements of it.
"""
import importlib
import os
import sys

import numpy as np
import pytest

import enhance_oracle as eo
import ref_program as rp
from conftest import PKG_NAME
from oracle import wm_oracle as o

hg = importlib.import_module(PKG_NAME + ".hostglue")

RES = rp.results()
CASES = rp.case_names()
WRONG = "Sai mật khẩu hoặc meta không khớp."

GRAY_KEYS = {"mode", "payload_type", "Sc", "Uw", "Vwt", "Sw", "shape", "alpha", "kfrac", "nonce", "digest"}
COLOR_KEYS = {"mode", "payload_type", "shape", "alpha", "kfrac", "nonce", "digest",
              "Sb", "Sg", "Sr", "UWb", "VWbt", "SWb", "UWg", "VWgt", "SWg", "UWr", "VWrt", "SWr"}


def factor_names(color: bool):
    """(host sigma, watermark U, watermark Vt, watermark sigma) member names per plane."""
    if color:
        return [("S" + n, "UW" + n, "VW" + n + "t", "SW" + n) for n in "bgr"]
    return [("Sc", "Uw", "Vwt", "Sw")]


def hmac_parts(meta: dict, color: bool):
    """The members the digest covers, in the reference's order: all host sigmas, all U, all Vt."""
    f = factor_names(color)
    return [meta[t[0]] for t in f] + [meta[t[1]] for t in f] + [meta[t[2]] for t in f]


def fixture(case: str):
    c = RES["cases"][case]
    meta = rp.load_meta(rp.case_path(case, c["meta_file"]))
    return c, rp.read_png(rp.case_path(case, "cover.png")), rp.read_png(rp.case_path(case, "logo.png")), \
        rp.read_png(rp.case_path(case, c["stego_file"])), meta, rp.wm_image(rp.case_path(case, c["wm_file"]), c["color"])


def assert_meta_layout(got: dict, want: dict):
    """Key set, and every member's dtype and shape, exactly."""
    assert set(got) == set(want)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)


def assert_meta_bits(got: dict, want: dict):
    assert_meta_layout(got, want)
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k


# =====================================================================================================================
# from the committed fixtures alone
# =====================================================================================================================
def test_fixture_set_is_the_documented_one():
    assert len(CASES) == 8 and len(RES["source_sha256"]) == 64
    for case in CASES:
        c = RES["cases"][case]
        for f in ("cover.png", "logo.png", c["stego_file"], c["meta_file"], c["wm_file"]):
            p = rp.case_path(case, f)
            assert os.path.isfile(p) and os.path.getsize(p) <= 100 * 1024, p
    c = RES["cases"]["gray_40x56_nonorm_rename"]                          # single:148-149,178-179,225-226
    assert (c["stego_arg"], c["stego_file"], c["wm_arg"], c["wm_file"]) == ("out.jpg", "out_stego.png", "mark", "mark_wm.png")


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_reference_fixture(case):
    """o.embed_arrays / extract_arrays (+ enhance) / detect_arrays against what the reference wrote.  Layout and the
    integer / byte members exactly; float members, stego, scores under the comparisons tests/test_oracle.py applies to
    the oracle-generated fixtures (another host's LAPACK may differ in the last bit); singular vectors through
    U diag(S) Vt and orthonormality (tests/test_gpu_parity.py), never member by member: their signs are free.  The
    enhanced watermark under rp.assert_enhanced_close (the oracle chain's measured sensitivity; bit-equal on the
    generating host, which test_regenerating_the_fixtures_gives_them_back checks)."""
    c, cover, logo, stego, meta, wm = fixture(case)
    color = c["color"]
    nonce = bytes.fromhex(c["nonce"])
    H, W = c["cover"]
    assert cover.shape == (H, W, 3) and logo.shape == tuple(c["logo"]) + (3,)
    r = o.embed_arrays(cover, logo, c["password"], nonce, c["alpha"], color, c["kfrac"], None)
    assert set(meta) == (COLOR_KEYS if color else GRAY_KEYS)
    assert_meta_layout(r["meta"], meta)
    # integer and byte members exactly
    assert meta["shape"].tolist() == [H, W] and np.array_equal(np.asarray(r["meta"]["shape"]), meta["shape"])
    assert meta["nonce"].tobytes() == nonce == np.asarray(r["meta"]["nonce"]).tobytes()
    assert str(meta["mode"]) == ("color" if color else "gray") == str(r["meta"]["mode"])
    assert str(meta["payload_type"]) == "image" == str(r["meta"]["payload_type"])
    assert float(meta["alpha"]) == c["alpha"] == float(r["meta"]["alpha"])
    assert float(meta["kfrac"]) == c["kfrac"] == float(r["meta"]["kfrac"])
    key = o.derive_key(c["password"], nonce)
    assert o.hmac_digest(key, [a.tobytes() for a in hmac_parts(meta, color)]) == meta["digest"].tobytes()
    # shapes the reference's thin SVD gives: U (H, L), S (L,), Vt (L, W)
    L = min(H, W)
    for s, u, v, sw in factor_names(color):
        assert meta[u].shape == (H, L) and meta[v].shape == (L, W) and meta[s].shape == meta[sw].shape == (L,)
        assert meta[u].dtype == meta[v].dtype == meta[s].dtype == meta[sw].dtype == np.float32
    # float members
    for s, u, v, sw in factor_names(color):
        for k in (s, sw):
            a, b = r["meta"][k], meta[k]
            assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), k
        rec = (r["meta"][u] * r["meta"][sw]) @ r["meta"][v]
        want = (meta[u] * meta[sw]) @ meta[v]
        assert np.abs(rec - want).max() <= 1e-5 * np.abs(want).max(), u
        for m in (meta, r["meta"]):
            assert np.abs(m[u].T @ m[u] - np.eye(L, dtype=np.float32)).max() < 1e-5
            assert np.abs(m[v] @ m[v].T - np.eye(L, dtype=np.float32)).max() < 1e-5
    assert np.abs(r["stego"].astype(int) - stego.astype(int)).max() <= 1
    assert np.mean(r["stego"] != stego) < 1e-3
    assert abs(r["psnr"] - c["psnr"]) < 1e-2 and abs(r["ssim"] - c["ssim"]) < 1e-4
    ok, score = o.detect_arrays(stego, meta, 0.6, None)
    assert ok == c["detect"] and abs(score - c["score"]) < 1e-4
    rp.assert_enhanced_close(rp.oracle_chain(stego, meta, c["password"], c["normalize"]), wm, case)
    with pytest.raises(ValueError, match=WRONG):
        o.extract_arrays(stego, meta, c["password"] + "x", c["normalize"], None)


@pytest.mark.parametrize("case", CASES)
def test_hostglue_reads_the_reference_files(case, tmp_path):
    """hostglue's readers and security glue on files the reference wrote: the PNG decode equals Pillow's, load_npz equals
    np.load, the key / HMAC glue verifies the reference's digest and reproduces its permutation; a tampered member
    and a wrong password raise the reference's message from the drop-in before any device work."""
    c, cover, logo, stego, meta, wm = fixture(case)
    color = c["color"]
    for f, want in (("cover.png", cover), ("logo.png", logo), (c["stego_file"], stego)):
        got = hg.read_image_bgr(rp.case_path(case, f))
        assert got.dtype == np.uint8 and np.array_equal(got, want), f
    got = hg.read_image_bgr(rp.case_path(case, c["wm_file"]))
    assert np.array_equal(got if color else got[..., 0], wm)
    assert_meta_bits(hg.load_npz(rp.case_path(case, c["meta_file"])), meta)
    # ... and its writers on the same content, read back by NumPy and Pillow: the reference's meta and stego come back bit for bit
    for compressed in (True, False):
        mp = hg.save_npz(str(tmp_path / f"again{int(compressed)}"), meta, compressed=compressed)
        assert_meta_bits(rp.load_meta(mp), meta)
    for level in (0, 1):
        assert hg.write_png(str(tmp_path / "again.png"), stego, level) and np.array_equal(rp.read_png(str(tmp_path / "again.png")), stego)
    assert hg.write_png(str(tmp_path / "again_wm.png"), wm, 1) and np.array_equal(rp.wm_image(str(tmp_path / "again_wm.png"), color), wm)
    nonce = bytes.fromhex(c["nonce"])
    key = hg.derive_key(c["password"], nonce)
    assert hg.digests_equal(hg.hmac_digest(key, hmac_parts(meta, color)), meta["digest"].tobytes())
    assert not hg.digests_equal(hg.hmac_digest(hg.derive_key(c["password"] + "x", nonce), hmac_parts(meta, color)),
                                meta["digest"].tobytes())
    H, W = c["cover"]
    assert np.array_equal(hg.permutation_index(H, W, key), o.permutation(H, W, o.rng_from_key(key)))
    # the drop-in (file level): the reference's message, raised before any device work
    core = importlib.import_module("dct_svd_core_secure")
    with pytest.raises(ValueError, match=WRONG):
        core.extract(rp.case_path(case, c["stego_file"]), rp.case_path(case, c["meta_file"]), str(tmp_path / "w.png"),
                     c["password"] + "x", enhance="reference")
    bad = {k: v.copy() for k, v in meta.items()}
    u = factor_names(color)[-1][1]
    bad[u].view(np.uint8).reshape(-1)[5] ^= 1
    np.savez_compressed(str(tmp_path / "bad.npz"), **bad)
    with pytest.raises(ValueError, match=WRONG):
        core.extract(rp.case_path(case, c["stego_file"]), str(tmp_path / "bad.npz"), str(tmp_path / "w.png"), c["password"])
    with pytest.raises(ValueError, match=WRONG):
        o.extract_arrays(stego, bad, c["password"], True, None)
    assert not os.path.exists(str(tmp_path / "w.png"))


def test_recipe_compiles_once_and_a_damaged_product_fails_to_load(tmp_path, monkeypatch):
    """oracle/ref_build.py on a stand-in source tree: one compiled file + the build record, nothing rewritten while the
    source and the interpreter stay the same, rebuilt when the source changes, nothing done where the tree is absent.
    A compiled file that is present but is not this interpreter's is an ImportError from the loader - which the live
    tests do not turn into a skip."""
    import hashlib
    from oracle import ref_build
    src_dir, out = tmp_path / "tree", tmp_path / "out"
    src_dir.mkdir()
    text = "import cv2\nfrom PySide6.QtWidgets import QWidget\nimport os\nclass App(QWidget): pass\ndef embed(): return os.urandom(8)\n"
    (src_dir / ref_build.SOURCE_NAME).write_text(text)
    compiled = ref_build.build_reference(str(src_dir), out_dir=str(out))
    assert sorted(os.listdir(out)) == sorted(os.path.basename(p) for p in (ref_build.COMPILED, ref_build.INFO))
    assert not compiled.endswith((".pyc", ".py"))                          # a build product that travels, not a cache
    info = ref_build.read_info(os.path.join(out, os.path.basename(ref_build.INFO)))
    assert info == dict(source=ref_build.SOURCE_NAME, sha256=hashlib.sha256(text.encode()).hexdigest(),
                        python="%d.%d.%d" % sys.version_info[:3])
    stamp = os.stat(compiled).st_mtime_ns
    assert ref_build.build_reference(str(src_dir), out_dir=str(out)) == compiled and os.stat(compiled).st_mtime_ns == stamp
    prog = rp.load(compiled)
    assert prog.mod.cv2 is prog.cv2 and "cv2" not in sys.modules and "PySide6" not in sys.modules
    prog.next_nonce = b"12345678"
    assert prog.mod.embed() == b"12345678" and prog.next_nonce is None    # os.urandom inside the module only
    assert len(os.urandom(8)) == 8
    (src_dir / ref_build.SOURCE_NAME).write_text(text + "X = 1\n")
    ref_build.build_reference(str(src_dir), out_dir=str(out))
    assert rp.load(compiled).mod.X == 1
    monkeypatch.setattr(ref_build, "DEFAULT_REF_DIRS", (str(tmp_path / "nowhere"),))
    assert ref_build.find_reference() is None and ref_build.build_reference(out_dir=str(tmp_path / "untouched")) is None
    assert not os.path.exists(tmp_path / "untouched")
    with open(compiled, "r+b") as f:
        f.write(b"\x00\x00\x00\x00")                                      # another interpreter's magic number
    with pytest.raises(ImportError):
        rp.load(compiled)
    assert "cv2" not in sys.modules                                        # taken out again on failure too


def test_fixture_files_are_what_the_documents_say():
    """8-bit gray or RGB PNGs only (alpha, palette and 16-bit handling is OpenCV's and not pinned); the meta is an
    ordinary compressed .npz that np.load(allow_pickle=False) reads; 0-d string members render as the reference's
    str(data['mode']) expects."""
    from PIL import Image
    import zipfile
    for case in CASES:
        c = RES["cases"][case]
        for f in ("cover.png", "logo.png", c["stego_file"], c["wm_file"]):
            with Image.open(rp.case_path(case, f)) as im:
                assert im.mode in ("L", "RGB"), (case, f, im.mode)
        with zipfile.ZipFile(rp.case_path(case, c["meta_file"])) as z:
            assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in z.infolist())
        meta = rp.load_meta(rp.case_path(case, c["meta_file"]))
        assert meta["mode"].shape == () and meta["mode"].dtype.kind == "U" and meta["alpha"].dtype == np.float64
        assert meta["shape"].dtype == np.int64 and meta["nonce"].dtype == meta["digest"].dtype == np.uint8
        assert meta["nonce"].shape == (8,) and meta["digest"].shape == (32,)
    with Image.open(rp.case_path("gray_56x40_shrink", "cover.png")) as im:
        assert im.mode == "L"                                            # a gray file read as 3 equal channels


# =====================================================================================================================
# live: the reference program in this process
# =====================================================================================================================
@pytest.fixture(scope="module")
def ref():
    return rp.load()


@rp.needs_program
def test_program_loads_cleanly_and_is_the_fixtures_source(ref):
    """The stand-ins are in sys.modules only while the module runs; the compiled program is the one the committed
    fixtures were made from (a changed source is a failure, not a skip)."""
    assert "cv2" not in sys.modules and "PySide6" not in sys.modules and "wm_reference_single" not in sys.modules
    assert ref.mod.cv2.__doc__.startswith("stand-in")
    info = rp.build_info()
    assert info["sha256"] == RES["source_sha256"], "oracle/_ref/ was built from another source than the fixtures"
    assert info["python"] == "%d.%d.%d" % sys.version_info[:3]
    assert all(callable(getattr(ref.mod, f)) for f in ("embed", "extract", "detect"))
    importlib.import_module(PKG_NAME + ".hostglue")                        # the product imports as before
    assert "cv2" not in sys.modules


def run_reference(ref, d, cover_file, logo_file, c, stego_arg="stego.png", wm_arg="wm.png"):
    """embed -> extract -> detect through the reference; returns paths and results."""
    p = lambda f: os.path.join(str(d), f)
    ref.log.clear()
    sp, mp, ps, ss = ref.embed(cover_file, logo_file, p(stego_arg), p("meta.npz"), alpha=c["alpha"], color=c["color"],
                               password=c["password"], kfrac=c["kfrac"], nonce=bytes.fromhex(c["nonce"]))
    wp = ref.extract(sp, mp, p(wm_arg), c["password"], c["normalize"])
    ok, score = ref.detect(sp, mp)
    assert not ref.log.errors, ref.log.errors
    return sp, mp, wp, ps, ss, ok, score


@rp.needs_program
@pytest.mark.parametrize("case", CASES)
def test_regenerating_the_fixtures_gives_them_back(ref, case, tmp_path):
    """The fixtures cannot drift from the program: run again, every array and figure comes back bit for bit - and the
    oracle equals them bit for bit in the same process."""
    c, cover, logo, stego, meta, wm = fixture(case)
    sp, mp, wp, ps, ss, ok, score = run_reference(ref, tmp_path, rp.case_path(case, "cover.png"), rp.case_path(case, "logo.png"),
                                                  c, c["stego_arg"], c["wm_arg"])
    assert (os.path.basename(sp), os.path.basename(mp), os.path.basename(wp)) == (c["stego_file"], c["meta_file"], c["wm_file"])
    assert np.array_equal(rp.read_png(sp), stego)
    assert_meta_bits(rp.load_meta(mp), meta)
    assert np.array_equal(rp.wm_image(wp, c["color"]), wm)
    assert (ps, ss, ok, score) == (c["psnr"], c["ssim"], c["detect"], c["score"])
    r = o.embed_arrays(cover, logo, c["password"], bytes.fromhex(c["nonce"]), c["alpha"], c["color"], c["kfrac"], None)
    assert np.array_equal(r["stego"], stego) and (r["psnr"], r["ssim"]) == (ps, ss)
    assert_meta_bits(r["meta"], meta)
    assert np.array_equal(rp.oracle_chain(stego, meta, c["password"], c["normalize"]), wm)
    assert o.detect_arrays(stego, meta, 0.6, None) == (ok, score)


def _sweep_cases(n=44):
    """Seeded: H, W in 6...96 independently, gray / colour, logos covering same size, integer and fractional shrink and
    enlargement and mixed axes, kfrac in [0, 1] with both ends, alpha from 1e-9 (below the max(alpha, 1e-8) guard) to
    0.5, normalize both ways."""
    rng = np.random.default_rng(20240607)
    kinds = ["same", "int_shrink", "int_enlarge", "frac_shrink", "frac_enlarge", "mixed"]
    out = []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        H, W = int(rng.integers(6, 97)), int(rng.integers(6, 97))
        if kind == "same":
            h, w = H, W
        elif kind == "int_shrink":
            H, W = int(rng.integers(6, 33)), int(rng.integers(6, 33))
            h, w = H * int(rng.integers(1, 4)), W * int(rng.integers(2, 4))
        elif kind == "int_enlarge":
            h, w = int(rng.integers(3, 17)), int(rng.integers(3, 17))
            H, W = h * int(rng.integers(2, 6)), w * int(rng.integers(2, 6))
        elif kind == "frac_shrink":
            h, w = H + int(rng.integers(1, H)), W + int(rng.integers(1, W))
        elif kind == "frac_enlarge":
            h, w = max(2, H - int(rng.integers(1, H - 2))), max(2, W - int(rng.integers(1, W - 2)))
        else:
            h, w = H + int(rng.integers(1, H)), max(2, W - int(rng.integers(1, W - 2)))
        kfrac = [0.0, 1.0, 0.33, 0.6][i] if i < 4 else float(rng.uniform(0, 1))
        alpha = [1e-9, 0.5, 1e-8, 0.1][i] if i < 4 else float(10 ** rng.uniform(-9, np.log10(0.5)))
        out.append(dict(i=i, kind=kind, cover=(H, W), logo=(h, w), color=bool(i % 3 == 1), kfrac=kfrac, alpha=alpha,
                        normalize=bool(i % 4 != 2), password=f"sweep-{i}", nonce=rng.bytes(8).hex()))
    return out


SWEEP = _sweep_cases()


def _sweep_images(c):
    rng = np.random.default_rng(c["i"] + 99)
    H, W = c["cover"]
    yy, xx = np.mgrid[0:H, 0:W]
    base = 120 + 50 * np.sin(xx / 6.0 + c["i"]) * np.cos(yy / 5.0)
    cover = np.clip(base[..., None] + rng.normal(0, 15, (H, W, 3)), 0, 255).astype(np.uint8)
    h, w = c["logo"]
    logo = np.full((h, w, 3), 230, np.uint8)
    logo[h // 4:max(h // 4 + 1, 3 * h // 4), w // 5:max(w // 5 + 1, 4 * w // 5)] = (25, 60, 200)
    logo[::4, ::3] = 0
    logo = np.clip(logo.astype(int) + rng.integers(-8, 9, logo.shape), 0, 255).astype(np.uint8)
    return cover, logo


def test_sweep_covers_what_it_claims():
    assert len(SWEEP) >= 40
    assert {c["kind"] for c in SWEEP} == {"same", "int_shrink", "int_enlarge", "frac_shrink", "frac_enlarge", "mixed"}
    assert any(c["color"] for c in SWEEP) and any(not c["color"] for c in SWEEP)
    assert any(not c["normalize"] for c in SWEEP)
    assert min(c["alpha"] for c in SWEEP) == 1e-9 and max(c["alpha"] for c in SWEEP) == 0.5
    assert min(c["kfrac"] for c in SWEEP) == 0.0 and max(c["kfrac"] for c in SWEEP) == 1.0
    assert all(6 <= v <= 96 for c in SWEEP for v in c["cover"])
    assert any(min(c["cover"]) < 8 for c in SWEEP)                       # L < 8: K = max(8, ...) exceeds L
    assert any(c["cover"][0] > c["cover"][1] for c in SWEEP) and any(c["cover"][0] < c["cover"][1] for c in SWEEP)


@rp.needs_program
@pytest.mark.parametrize("c", SWEEP, ids=[f"{c['i']:02d}-{c['kind']}-{'colour' if c['color'] else 'gray'}" for c in SWEEP])
def test_sweep_reference_against_oracle_bit_for_bit(ref, c, tmp_path):
    from PIL import Image
    cover, logo = _sweep_images(c)
    cp, lp = str(tmp_path / "cover.png"), str(tmp_path / "logo.png")
    Image.fromarray(np.ascontiguousarray(cover[..., ::-1])).save(cp)
    Image.fromarray(np.ascontiguousarray(logo[..., ::-1])).save(lp)
    sp, mp, wp, ps, ss, ok, score = run_reference(ref, tmp_path, cp, lp, c)
    r = o.embed_arrays(cover, logo, c["password"], bytes.fromhex(c["nonce"]), c["alpha"], c["color"], c["kfrac"], None)
    stego, meta = rp.read_png(sp), rp.load_meta(mp)
    assert np.array_equal(stego, r["stego"])
    assert_meta_bits(r["meta"], meta)
    assert (ps, ss) == (r["psnr"], r["ssim"])
    assert np.array_equal(rp.wm_image(wp, c["color"]), rp.oracle_chain(stego, meta, c["password"], c["normalize"]))
    assert (ok, score) == o.detect_arrays(stego, meta, 0.6, None)
    # the host glue's restatements of the same steps
    assert np.array_equal(hg.resize_area(logo, c["cover"][1], c["cover"][0]), o.resize_area(logo, c["cover"][1], c["cover"][0]))
    key = hg.derive_key(c["password"], bytes.fromhex(c["nonce"]))
    assert hg.digests_equal(hg.hmac_digest(key, hmac_parts(meta, c["color"])), meta["digest"].tobytes())


@rp.needs_program
def test_refusals_and_odd_inputs_follow_the_reference(ref, tmp_path):
    """Wrong password, one byte of Uw changed, detect on an unrelated image, a gray stego cropped below meta['shape']:
    whatever the reference does - result or exception type and message - the oracle does, and the host glue's check
    agrees."""
    from PIL import Image
    case = "gray_40x56_mixed"
    c, cover, logo, stego, meta, wm = fixture(case)
    sp, mp = rp.case_path(case, c["stego_file"]), rp.case_path(case, c["meta_file"])
    out = str(tmp_path / "w.png")
    # wrong / empty password
    with pytest.raises(ValueError) as e_ref:
        ref.extract(sp, mp, out, "not-" + c["password"])
    with pytest.raises(ValueError) as e_o:
        o.extract_arrays(stego, meta, "not-" + c["password"], True, None)
    assert str(e_ref.value) == str(e_o.value) == WRONG
    with pytest.raises(ValueError) as e_ref:
        ref.extract(sp, mp, out, "")
    with pytest.raises(ValueError) as e_o:
        o.extract_arrays(stego, meta, "", True, None)
    assert str(e_ref.value) == str(e_o.value)
    with pytest.raises(ValueError) as e_ref:
        ref.embed(rp.case_path(case, "cover.png"), rp.case_path(case, "logo.png"), out, str(tmp_path / "m.npz"), password="", nonce=bytes(8))
    with pytest.raises(ValueError) as e_o:
        o.embed_arrays(cover, logo, "", bytes(8))
    assert str(e_ref.value) == str(e_o.value)
    # one byte of Uw changed
    bad = {k: v.copy() for k, v in meta.items()}
    bad["Uw"].view(np.uint8).reshape(-1)[123] ^= 0x40
    bp = str(tmp_path / "bad.npz")
    np.savez_compressed(bp, **bad)
    with pytest.raises(ValueError) as e_ref:
        ref.extract(sp, bp, out, c["password"])
    with pytest.raises(ValueError) as e_o:
        o.extract_arrays(stego, bad, c["password"], True, None)
    assert str(e_ref.value) == str(e_o.value) == WRONG
    key = hg.derive_key(c["password"], bytes.fromhex(c["nonce"]))
    assert not hg.digests_equal(hg.hmac_digest(key, hmac_parts(bad, False)), bad["digest"].tobytes())
    assert ref.detect(sp, bp) == o.detect_arrays(stego, bad, 0.6, None)      # detect does not authenticate: Sc, Sw untouched
    assert not os.path.exists(out)
    # a missing file: the reference's own ValueError
    with pytest.raises(ValueError, match="Không mở được ảnh"):
        ref.detect(str(tmp_path / "missing.png"), mp)
    with pytest.raises(ValueError, match="Không mở được ảnh"):
        hg.read_image_bgr(str(tmp_path / "missing.png"))
    # detect on an unrelated image of the same size
    other = np.random.default_rng(5).integers(0, 256, stego.shape, dtype=np.uint8)
    op = str(tmp_path / "other.png")
    Image.fromarray(np.ascontiguousarray(other[..., ::-1])).save(op)
    got = ref.detect(op, mp)
    assert got == o.detect_arrays(other, meta, 0.6, None) and got[0] is False
    # a gray stego cropped from 40 x 56 to 33 x 47 (and to an even 32 x 46): accepted, L = 33, scored like the oracle
    for (hh, ww) in ((33, 47), (32, 46)):
        crop = np.ascontiguousarray(stego[:hh, :ww])
        cpth = str(tmp_path / f"crop{hh}.png")
        Image.fromarray(np.ascontiguousarray(crop[..., ::-1])).save(cpth)
        ref.log.clear()
        wp = ref.extract(cpth, mp, str(tmp_path / f"wcrop{hh}.png"), c["password"])
        assert not ref.log.errors
        got_wm = rp.wm_image(wp, False)
        assert got_wm.shape == (40, 56)                                      # the META's size
        assert np.array_equal(got_wm, rp.oracle_chain(crop, meta, c["password"], True))
        got = ref.detect(cpth, mp)
        assert got == o.detect_arrays(crop, meta, 0.6, None)
    assert ref.detect(str(tmp_path / "crop33.png"), mp)[1] < 0                # what the reference does: accepted, scored negative


@rp.needs_program
@pytest.mark.parametrize("case", ["gray_40x56_mixed", "gray_56x40_shrink", "color_32x48_x2", "gray_6x10_tiny"])
@pytest.mark.parametrize("compressed", [True, False], ids=["deflated", "stored"])
@pytest.mark.parametrize("png_level", [0, 1])
def test_hostglue_writers_against_the_reference_readers(ref, case, compressed, png_level, tmp_path):
    """Meta written by hostglue.save_npz (compressed and not) and stego written by hostglue.write_png (levels 0 and 1)
    from oracle-made arrays, read by the reference's extract and detect: bit for bit what the oracle gives on the same
    arrays."""
    c, cover, logo, _, _, _ = fixture(case)
    r = o.embed_arrays(cover, logo, c["password"], bytes.fromhex(c["nonce"]), c["alpha"], c["color"], c["kfrac"], None)
    sp = str(tmp_path / "stego.png")
    assert hg.write_png(sp, r["stego"], png_level)
    mp = hg.save_npz(str(tmp_path / "meta"), r["meta"], compressed=compressed)
    assert mp.endswith("meta.npz")
    assert np.array_equal(rp.read_png(sp), r["stego"])
    assert_meta_bits(rp.load_meta(mp), r["meta"])
    ref.log.clear()
    wp = ref.extract(sp, mp, str(tmp_path / "wm.png"), c["password"], c["normalize"])
    assert not ref.log.errors
    assert np.array_equal(rp.wm_image(wp, c["color"]), rp.oracle_chain(r["stego"], r["meta"], c["password"], c["normalize"]))
    assert ref.detect(sp, mp) == o.detect_arrays(r["stego"], r["meta"], 0.6, None)
    # a watermark image written by hostglue.write_png, read by the stand-in's (Pillow's) decoder
    w = rp.oracle_chain(r["stego"], r["meta"], c["password"], c["normalize"])
    assert hg.write_png(str(tmp_path / "w2.png"), w, 1)
    assert np.array_equal(rp.wm_image(str(tmp_path / "w2.png"), c["color"]), w)


@rp.needs_program
@pytest.mark.parametrize("case", ["gray_40x56_mixed", "color_32x48_x2"])
def test_call_log_shows_the_whole_post_processing_chain(ref, case, tmp_path):
    """The reference wraps NL-means and CLAHE in try/except: a stand-in entry that raised there would be swallowed and
    change the output silently.  After an extract the log shows each step called and nothing raised."""
    c = RES["cases"][case]
    ref.log.clear()
    ref.extract(rp.case_path(case, c["stego_file"]), rp.case_path(case, c["meta_file"]), str(tmp_path / "w.png"), c["password"])
    nlm = "fastNlMeansDenoisingColored" if c["color"] else "fastNlMeansDenoising"
    for name in (nlm, "createCLAHE", "CLAHE.apply", "GaussianBlur", "addWeighted", "imwrite"):
        assert ref.log.count(name) == 1, (name, ref.log.calls)
    assert ref.log.count("normalize") == (3 if c["color"] else 1)
    assert ref.log.count("idct") == (3 if c["color"] else 1) and ref.log.count("dct") == (3 if c["color"] else 1)
    assert ref.log.errors == []


@rp.needs_program
def test_call_log_catches_an_exception_the_reference_swallows(ref, tmp_path, monkeypatch):
    """The log is what makes a swallowed failure visible: with NL-means made to raise, the reference's extract still
    returns (single:223-224) and the log holds the exception.  The written image cannot be relied on to show it: on a
    noise-like estimate NL-means finds no similar patches and changes nothing, so the output is the same either way."""
    case = "gray_40x56_mixed"
    c = RES["cases"][case]

    def boom(*a, **k):
        raise RuntimeError("nlmeans unavailable")
    monkeypatch.setattr(eo, "nlmeans", boom)
    ref.log.clear()
    wp = ref.extract(rp.case_path(case, c["stego_file"]), rp.case_path(case, c["meta_file"]), str(tmp_path / "w.png"), c["password"])
    assert os.path.exists(wp)
    assert [n for n, _ in ref.log.errors] == ["fastNlMeansDenoising"]
    assert isinstance(ref.log.errors[0][1], RuntimeError)
    # and a call outside what an entry was written for is refused, not approximated
    ref.log.clear()
    with pytest.raises(TypeError, match="cv2 stand-in"):
        ref.cv2.GaussianBlur(np.zeros((8, 8), np.float32), (5, 5), 1.0)
    with pytest.raises(TypeError, match="cv2 stand-in"):
        ref.cv2.cvtColor(np.zeros((8, 8), np.uint8), ref.cv2.COLOR_BGR2GRAY)
    assert len(ref.log.errors) == 2
    ref.log.clear()
