"""CPU tests of the package's ``meta`` module: the one statement of the .npz layout.

* The HMAC coverage and order, the nonce / digest readers and the key derivation, held to files the reference program
  itself wrote (tests/golden/reference/): ``hmac_parts`` of the stored meta under ``derive_key(password, nonce)`` is the
  stored digest, and is not once a covered member is tampered with.
* The tile rule on both meta forms (explicit ``tile`` key, inferred from the rank of Sc / Sb) and on ``tile = 0``.
* ``k_of`` against the literal ``max(k_floor, int(kfrac * L))`` of single:174, capped at L.
"""
import importlib
import json
import os

import numpy as np
import pytest

from conftest import PKG_NAME

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
with open(os.path.join(GOLDEN, "results.json")) as _f:
    RESULTS = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def M():
    return importlib.import_module(PKG_NAME + ".meta")


@pytest.fixture(scope="module")
def hg():
    return importlib.import_module(PKG_NAME + ".hostglue")


def test_the_fixtures_are_there():
    assert len(RESULTS) == 8 and any(c["color"] for c in RESULTS.values())


@pytest.mark.parametrize("case", sorted(RESULTS))
def test_hmac_parts_reproduce_the_reference_digest(M, hg, case):
    c = RESULTS[case]
    with np.load(os.path.join(GOLDEN, case, c["meta_file"]), allow_pickle=False) as z:
        meta = {k: z[k] for k in z.files}
    assert M.is_color(meta) == c["color"]
    assert M.nonce_of(meta) == bytes.fromhex(c["nonce"])
    stored = M.digest_of(meta)
    assert isinstance(stored, bytes) and len(stored) == 32
    key = hg.derive_key(c["password"], bytes.fromhex(c["nonce"]))
    parts = M.hmac_parts(meta)
    assert len(parts) == (9 if c["color"] else 3)
    assert hg.hmac_digest(key, parts) == stored
    assert M.authentic(meta, key)
    assert not M.authentic(meta, hg.derive_key(c["password"] + "x", bytes.fromhex(c["nonce"])))
    # the order is part of the coverage
    assert hg.hmac_digest(key, parts[::-1]) != stored
    # every covered member, tampered with in its last value, makes the digest differ
    names = (["Sc", "Uw", "Vwt"] if not c["color"] else
             ["Sb", "Sg", "Sr", "UWb", "UWg", "UWr", "VWbt", "VWgt", "VWrt"])
    for i, name in enumerate(names):
        assert parts[i] is meta[name]
        bad = dict(meta)
        bad[name] = meta[name].copy()
        bad[name].reshape(-1)[-1] += np.float32(1.0)
        assert hg.hmac_digest(key, M.hmac_parts(bad)) != stored, name
        assert not M.authentic(bad, key), name
    # the members the HMAC does not cover (single:152-156, 182) leave it alone
    free = dict(meta)
    sw = "SWb" if c["color"] else "Sw"
    free[sw] = meta[sw] + np.float32(1.0)
    assert M.authentic(free, key)
    # the reference's files are full-frame and name neither tile nor k_floor
    assert M.tile_of(meta) is None and M.k_floor_of(meta) == 8 and M.kfrac_of(meta) == c["kfrac"]


def test_key_names(M):
    assert M.CHANNELS == "bgr"
    assert [(M.s_key(n), M.uw_key(n), M.vwt_key(n), M.sw_key(n)) for n in M.CHANNELS] == [
        ("Sb", "UWb", "VWbt", "SWb"), ("Sg", "UWg", "VWgt", "SWg"), ("Sr", "UWr", "VWrt", "SWr")]
    meta = {k: np.full((2,), i, np.float32) for i, k in enumerate(("Sb", "Sg", "Sr", "SWb", "SWg", "SWr"))}
    assert M.stacked(meta, M.s_key).tolist() == [[0, 0], [1, 1], [2, 2]]
    assert M.stacked(meta, M.sw_key).tolist() == [[3, 3], [4, 4], [5, 5]]
    for mode, want in (("gray", False), ("video_gray", False), ("color", True), ("video_color", True)):
        assert M.is_color({"mode": np.array(mode)}) is want


def test_tile_rule(M):
    f32 = np.float32
    # explicit key: 8, 0 (the video metas' full-frame), anything else refused with the argument check's text
    assert M.tile_of({"tile": np.int32(8), "Sc": np.zeros(5, f32)}) == 8
    assert M.tile_of({"tile": np.int32(0), "Sc": np.zeros((2, 3, 4, 8), f32)}) is None
    assert M.tile_of({"tile": np.int32(0), "Sb": np.zeros((2, 5), f32)}) is None
    for bad in (4, 16, -8):
        with pytest.raises(ValueError, match="^tile must be 8 or None$"):
            M.tile_of({"tile": np.int32(bad), "Sc": np.zeros((3, 4, 8), f32)})
    # no key: per-tile [nby, nbx, 8] against full-frame [L], gray and colour
    assert M.tile_of({"Sc": np.zeros((3, 4, 8), f32)}) == 8
    assert M.tile_of({"Sc": np.zeros(24, f32)}) is None
    assert M.tile_of({"Sb": np.zeros((3, 4, 8), f32)}) == 8
    assert M.tile_of({"Sb": np.zeros(24, f32)}) is None
    # an .npz as np.load hands it over
    import io
    buf = io.BytesIO()
    np.savez(buf, tile=np.int32(0), Sc=np.zeros((1, 6), f32))
    buf.seek(0)
    with np.load(buf) as z:
        assert M.tile_of(z) is None
    # the argument check of the public functions
    M.check_tile(8); M.check_tile(None)
    with pytest.raises(ValueError, match="^tile must be 8 or None$"):
        M.check_tile(16)


@pytest.mark.parametrize("L", (6, 8, 64))
@pytest.mark.parametrize("kfrac", (0.0, 0.6, 1.0))
@pytest.mark.parametrize("k_floor", (3, 8))
def test_k_of(M, L, kfrac, k_floor):
    want = max(k_floor, int(kfrac * L))                                    # single:174
    if want > L:
        want = L
    got = M.k_of(L, kfrac, k_floor)
    assert isinstance(got, int) and got == want


def test_readers_defaults_and_small_rules(M):
    assert M.kfrac_of({}) == 0.6 and M.k_floor_of({}) == 8
    assert M.kfrac_of({"kfrac": np.array(0.25)}) == 0.25 and M.k_floor_of({"k_floor": np.int32(5)}) == 5
    assert M.nonce_of({"nonce": np.arange(8, dtype=np.uint8)}) == bytes(range(8))
    assert M.out_name("a/b.PNG", "_stego.png") == "a/b.PNG"                # single:148-149
    assert M.out_name("a/b.jpg", "_stego.png") == "a/b_stego.png"
    assert M.out_name("a/mark", "_wm.png") == "a/mark_wm.png"              # single:225-226
    with pytest.raises(ValueError, match="^Vui lòng nhập mật khẩu để nhúng.$"):
        M.require_password("", "embed")
    with pytest.raises(ValueError, match="^Vui lòng nhập mật khẩu để giải trích.$"):
        M.require_password(None, "extract")
    M.require_password("pw", "embed")
    with pytest.raises(TypeError, match="password must be a str, got bool: extract"):
        M.check_password_type(True, "extract")
    M.check_password_type(None, "embed")
    assert M.WRONG_PASSWORD == "Sai mật khẩu hoặc meta không khớp."
    for ok in (False, True, "reference"):
        M.check_enhance(ok)
    with pytest.raises(ValueError, match="enhance must be False, True or 'reference'"):
        M.check_enhance("yes")
