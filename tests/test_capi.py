"""The C-ABI library loads on a box without a GPU and exports every symbol
include/wmhip.h declares (no compute calls here)."""
import importlib
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge


def _header_functions():
    txt = open(os.path.join(ge.ROOT, "include", "wmhip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(wm_[a-z0-9_]+)\s*\(", txt)))


def test_header_binding_and_library_agree(hostapi):
    ge.build_hip()
    names = _header_functions()
    assert len(names) >= 25
    assert sorted(hostapi.SIGNATURES) == names            # binding types every declared entry point
    lib = hostapi.load_library()
    for n in names:
        assert hasattr(lib, n), f"libwmhip.so does not export {n}"
    assert lib.wm_abi_version() == hostapi.ABI_VERSION == 1


def test_no_gpu_fails_loudly_not_silently(hostapi):
    """Without a device the product raises; it never computes on the host."""
    if hostapi.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises((hostapi.WmError, ValueError)):
        hostapi.Context(0)
    import dct_svd_core_secure as core
    with pytest.raises((hostapi.WmError, ValueError)):
        core.embed_arrays(np.zeros((16, 16, 3), np.uint8), np.zeros((4, 4, 3), np.uint8), "pw", bytes(8))


def test_missing_library_is_an_import_error(hostapi, tmp_path):
    with pytest.raises(hostapi.WmLibraryError):
        hostapi.load_library(str(tmp_path / "nope.so"))


def test_product_does_not_import_the_oracle():
    pkg_dir = os.path.join(ge.ROOT, ge.PKG_NAME)
    for root, _, files in os.walk(pkg_dir):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(root, f), errors="replace").read()
                assert "wm_oracle" not in src and "from oracle" not in src and "import oracle" not in src, f
    assert "oracle" not in open(os.path.join(ge.ROOT, "dct_svd_core_secure.py")).read()


class _NoCallContext:
    """hostapi.Context without a device: any attempt to cross the C ABI fails the test."""

    def __new__(cls, hostapi):
        ctx = object.__new__(hostapi.Context)
        ctx._h = None

        def _call(name, *args):
            raise AssertionError(f"{name} reached the C ABI with unvalidated shapes")
        ctx._call = _call
        return ctx


def test_meta_shapes_are_validated_before_the_c_abi(hostapi):
    """a meta that does not belong to the stego (short Sc / Sw, wrong tile grid, per-plane
    factor batch of another size) must raise ValueError on the host - the C side would read
    min(H, W) or n_tiles * 8 floats from whatever buffer it is given."""
    ctx = _NoCallContext(hostapi)
    st = np.zeros((64, 96), np.uint8)
    good_sc = np.zeros(64, np.float32)
    for sc, sw in ((np.zeros(32, np.float32), good_sc), (good_sc, np.zeros(63, np.float32)),
                   (np.zeros((2, 64), np.float32), good_sc)):
        with pytest.raises(ValueError):
            ctx.ref_detect(st, sc, sw, 0.1)
    nby, nbx = 8, 12
    sc_t = np.zeros((nby, nbx, 8), np.float32)
    with pytest.raises(ValueError):
        ctx.detect_tiles(st, sc_t, np.zeros((nby, nbx - 1, 8), np.float32), 0.1)
    with pytest.raises(ValueError):
        ctx.detect_tiles(st, sc_t[:-1], sc_t, 0.1)
    with pytest.raises(ValueError):
        ctx.detect_tiles(st, sc_t, np.zeros((2, nby, nbx, 8), np.float32), 0.1)       # per-plane Sw for 1 plane
    U = np.zeros((nby, nbx, 8, 8), np.float32)
    with pytest.raises(ValueError):
        ctx.extract_tiles(st, sc_t, np.zeros((2, nby, nbx, 8, 8), np.float32),
                          np.zeros((2, nby, nbx, 8, 8), np.float32), 0.1)             # 5-D Uw with shape[0] != n
    with pytest.raises(ValueError):
        ctx.extract_tiles(st, sc_t[:4], U, U, 0.1)
    with pytest.raises(ValueError):
        ctx.extract_tiles(st, sc_t, U, U[:, :5], 0.1)
    with pytest.raises(ValueError):
        ctx.reconstruct_tiles(U, np.zeros((nby, nbx, 4), np.float32), U, 64, 96)
    # the scramble index is gathered / scattered through unchecked on the device: range-checked before the upload
    bad = np.arange(64 * 96); bad[7] = 64 * 96
    with pytest.raises(ValueError):
        ctx.permute_planes(st, bad)
    bad[7] = -1
    with pytest.raises(ValueError):
        ctx.permute_planes(st, bad)
    with pytest.raises(ValueError):
        ctx.permute_planes(st, np.arange(64 * 96 - 1))


def test_meta_tile_and_stego_size_are_checked():
    import dct_svd_core_secure as core
    mod = core.embed_arrays.__globals__
    tile_of = importlib.import_module(core._impl.__package__ + ".meta").tile_of
    meta = {"tile": np.int32(16), "Sc": np.zeros((2, 2, 8), np.float32), "shape": np.array((16, 16))}
    with pytest.raises(ValueError, match="tile must be 8 or None"):
        tile_of(meta)
    assert tile_of({"tile": np.int32(0), "Sc": np.zeros(4)}) is None
    assert tile_of({"tile": np.int32(8), "Sc": np.zeros(4)}) == 8
    assert tile_of({"Sc": np.zeros((2, 2, 8))}) == 8 and tile_of({"Sb": np.zeros(16)}) is None
    with pytest.raises(ValueError, match="meta was written for"):
        mod["_check_stego_shape"](np.zeros((16, 24, 3), np.uint8), meta)
    mod["_check_stego_shape"](np.zeros((16, 16, 3), np.uint8), meta)


class _FakeLib:
    """Stands in for libwmhip.so on a box without a GPU: every entry point succeeds and writes nothing, except
    wm_check_status, which reports the sticky status bit (set -> WM_ERR_NOCONV).  Records the calls.
    ``routes``: wm_route_create_dev hands a handle back (without it the binding sees no route and takes the index
    passes).  ``fail_malloc=k``: the k-th wm_malloc returns WM_ERR_NOMEM.  ``mallocs`` / ``routed`` hold the addresses
    and handles handed out, ``freed`` those released, in order, and ``freed_at`` where in ``calls`` each one was."""

    def __init__(self, status_rc=0, routes=False, fail_malloc=0):
        self.status_rc, self.routes, self.fail_malloc = status_rc, routes, fail_malloc
        self.calls = []
        self.mallocs, self.routed, self.freed, self.freed_at = [], [], [], {}
        self._next = 0x1000

    def wm_last_error(self):
        return b"SVD did not converge"

    def __getattr__(self, name):
        if not name.startswith("wm_"):
            raise AttributeError(name)

        def fn(h, *args):
            self.calls.append(name)
            if name == "wm_check_status":
                return self.status_rc
            if name == "wm_malloc":
                if self.calls.count("wm_malloc") == self.fail_malloc:
                    return 4                                                # WM_ERR_NOMEM
                self._next += 0x100000
                args[1]._obj.value = self._next
                self.mallocs.append(self._next)
            if name == "wm_route_create_dev" and self.routes:
                self._next += 0x100000
                args[2]._obj.value = self._next
                self.routed.append(self._next)
            if name in ("wm_free", "wm_route_destroy"):
                self.freed.append(args[0].value)
                self.freed_at[args[0].value] = len(self.calls) - 1
            return 0
        return fn


def _fake_ctx(hostapi, status_rc=0, **kw):
    ctx = object.__new__(hostapi.Context)
    ctx.lib = _FakeLib(status_rc, **kw)
    ctx._h = None                       # close() / __del__ do nothing
    ctx.__dict__["_h"] = 1
    ctx.device = 0
    return ctx


def test_device_resident_extract_reports_a_set_status_bit(hostapi):
    """extract_tiles_unscrambled_u8 drives the *_dev entry points, which only SET the sticky status bit: the wrapper
    must end in wm_check_status so that a Jacobi that hit its sweep bound raises LinAlgError here, not in
    some later unrelated call (round-2 advisor finding)."""
    H = W = 16
    st = np.zeros((H, W), np.uint8); sc = np.zeros((2, 2, 8), np.float32)
    U = np.zeros((2, 2, 8, 8), np.float32)
    idx = np.arange(H * W)
    ctx = _fake_ctx(hostapi, status_rc=hostapi.WM_ERR_NOCONV)
    with pytest.raises(np.linalg.LinAlgError):
        ctx.extract_tiles_unscrambled_u8(st, sc, U, U, 0.1, 8, idx)
    calls = ctx.lib.calls
    assert "wm_check_status" in calls and calls.index("wm_check_status") > calls.index("wm_extract_tiles_u8_dev")
    assert calls.count("wm_free") == calls.count("wm_malloc") - 1          # everything but the cached index is released
    ok = _fake_ctx(hostapi, status_rc=0)
    out = ok.extract_tiles_unscrambled_u8(st, sc, U, U, 0.1, 8, idx)
    assert out.shape == (H, W) and out.dtype == np.uint8
    ctx.__dict__["_h"] = None; ok.__dict__["_h"] = None


def test_device_index_cache_is_keyed_by_identity_not_address(hostapi):
    """The device copy of a permutation is cached on what the index IS - (H, W, sha256(key)) for
    hostglue.permutation_index, a content digest otherwise - never on its address (NumPy reuses a freed index's
    address for the next arange of the same size).  Non-bijective indices are refused before the upload."""
    import importlib
    hg = importlib.import_module(ge.PKG_NAME + ".hostglue")
    ctx = _fake_ctx(hostapi)
    a = hg.permutation_index(8, 8, b"k" * 32)
    assert a.tag == ("perm", 8, 8, __import__("hashlib").sha256(b"k" * 32).digest()) and a[::2].tag is None
    d1 = ctx.index_dev(a)
    assert ctx.index_dev(a) == d1 and ctx.lib.calls.count("wm_malloc") == 1
    b = hg.permutation_index(8, 8, b"q" * 32)
    assert ctx.index_dev(b) != d1
    # same contents at a different address: one device copy; different contents in the SAME buffer: another
    x = np.arange(64)[::-1].copy()
    dx = ctx.index_dev(x)
    assert ctx.index_dev(x.copy()) == dx
    x[0], x[1] = x[1], x[0]
    assert ctx.index_dev(x) != dx
    with pytest.raises(ValueError):
        ctx.index_dev(np.zeros(16, np.int64))                   # in range, but not a permutation
    with pytest.raises(ValueError):
        ctx.index_dev(np.arange(16) + 1)
    ctx.__dict__["_h"] = None


def test_extract_checks_the_hmac_before_anything_else_counts():
    """The HMAC over the meta's factors runs on a worker thread under the device work; the reference checks it first
    (single:206-209), so a mismatch must win over whatever else went wrong, and the other error must surface when the
    password is right.  No device needed: a tile-mode meta for another stego size fails before any device call."""
    import importlib
    import dct_svd_core_secure as core
    hg = importlib.import_module(core._impl.__package__ + ".hostglue")
    rng = np.random.default_rng(3)
    nonce = bytes(range(8))
    Sc = rng.normal(0, 1, (2, 2, 8)).astype(np.float32)
    Uw = rng.normal(0, 1, (2, 2, 8, 8)).astype(np.float32); Vwt = rng.normal(0, 1, (2, 2, 8, 8)).astype(np.float32)
    digest = hg.hmac_digest(hg.derive_key("right", nonce), [Sc, Uw, Vwt])
    meta = dict(mode="gray", alpha=0.1, shape=np.array((16, 16)), nonce=np.frombuffer(nonce, dtype=np.uint8),
                digest=np.frombuffer(digest, dtype=np.uint8), Sc=Sc, Uw=Uw, Vwt=Vwt, tile=np.int32(8), kfrac=0.6)
    stego_other_size = np.zeros((16, 24, 3), np.uint8)
    with pytest.raises(ValueError, match="Sai mật khẩu"):
        core.extract_arrays(stego_other_size, meta, "wrong")
    with pytest.raises(ValueError, match="meta was written for"):
        core.extract_arrays(stego_other_size, meta, "right")


# ---- the binding's staging scope, device cache and payload call, on the fake library ----------------------------------
def _header_prototypes():
    """name -> parameter kinds ("ptr", "int", "size_t", "float") of every prototype of include/wmhip.h"""
    txt = open(os.path.join(ge.ROOT, "include", "wmhip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {}
    for name, params in re.findall(r"\b(wm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        kinds = []
        for p in (q.strip() for q in params.split(",")):
            if p == "void":
                continue
            kinds.append("ptr" if "*" in p else " ".join(w for w in p.split()[:-1] if w != "const"))
        assert name not in protos, name
        protos[name] = kinds
    return protos


def test_signatures_match_the_header_parameter_by_parameter(hostapi):
    """SIGNATURES is written by hand; an int where the header says size_t would pass every test without a device and
    corrupt an argument on one.  Every parameter of every prototype, the leading wm_ctx* included (a pointer like any
    other: _call supplies it)."""
    import ctypes as C
    protos = _header_prototypes()
    assert sorted(protos) == _header_functions() == sorted(hostapi.SIGNATURES)
    exact = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    for name, kinds in protos.items():
        argtypes = hostapi.SIGNATURES[name]
        assert len(argtypes) == len(kinds), f"{name}: {len(argtypes)} argtypes for {len(kinds)} parameters"
        for k, (kind, t) in enumerate(zip(kinds, argtypes)):
            if kind == "ptr":
                assert t is C.c_void_p or issubclass(t, C._Pointer), f"{name} parameter {k}: {t} for a pointer"
            else:
                assert t is exact[kind], f"{name} parameter {k}: {t} for {kind}"


_TH, _TW = 16, 24                                                          # 2 x 3 tiles
_MASK = (8.0, 64.0, 0.5)


def _trace_runs():
    """name -> (needs routes?, call on a context): the methods whose C calls the traces below pin"""
    u8 = np.zeros((2, _TH, _TW), np.uint8); f32 = np.zeros((2, _TH, _TW), np.float32)
    idx = np.arange(_TH * _TW)[::-1].copy()
    sc = np.zeros((2, 2, 3, 8), np.float32); sw = np.zeros((2, 3, 8), np.float32); U = np.zeros((2, 3, 8, 8), np.float32)
    tb = np.zeros(6, np.uint8); order = np.arange(6); offs = np.array([0, 2, 4, 6])
    shared = np.zeros(6, np.uint16); rows = np.zeros((2, 6), np.uint16)
    runs = {
        "permute_u8": lambda c: c.permute_planes(u8, idx),
        "permute_f32": lambda c: c.permute_planes(f32, idx),
        "unpermute": lambda c: c.unpermute_normalize_u8(f32, idx),
        "unscrambled": lambda c: c.extract_tiles_unscrambled_u8(u8, sc, U, U, 0.1, 8, idx),
        "unscrambled_mask": lambda c: c.extract_tiles_unscrambled_u8(u8, sc, U, U, 0.1, 8, idx, mask=_MASK),
        "soft": lambda c: c.payload_soft(u8, order, offs, 3, 16.0),
        "soft_shared": lambda c: c.payload_soft(u8, order, offs, 3, 16.0, dither=shared),
        "soft_rows": lambda c: c.payload_soft(u8, order, offs, 3, 16.0, dither=rows),
        "sigma_w": lambda c: c.payload_sigma_w(u8, tb, 16.0),
        "sigma_w_dither": lambda c: c.payload_sigma_w(u8, tb, 16.0, dither=shared),
        "embed_payload": lambda c: c.embed_tiles_payload(u8, tb, 16.0, want_yw=True),
        "embed_payload_dither": lambda c: c.embed_tiles_payload(u8[0], tb, 16.0, dither=rows[:1]),
        "metric": lambda c: c.payload_metric(u8, 16.0),
        "metric_dither": lambda c: c.payload_metric(u8, 16.0, dither=rows),
        "embed": lambda c: c.embed_tiles(u8, sw, 0.1),
        "embed_mask": lambda c: c.embed_tiles(u8[0], sw, 0.1, want_yw=True, mask=_MASK),
        "extract": lambda c: c.extract_tiles(u8, sc, U, U, 0.1),
        "extract_mask": lambda c: c.extract_tiles(u8, sc, U, U, 0.1, sum_planes=True, mask=_MASK),
        "detect": lambda c: c.detect_tiles(u8, sc, sw, 0.1),
        "detect_mask": lambda c: c.detect_tiles(u8, sc, sw, 0.1, mask=_MASK),
    }
    # one context through the index, CSR and dither caches, so that close() has all three to release
    runs["session"] = lambda c: [runs[k](c) for k in ("permute_u8", "unscrambled", "soft_shared", "soft_rows", "unpermute")]
    routed = ("permute_u8", "permute_f32", "unpermute", "unscrambled", "unscrambled_mask", "session")
    return {**{k: (False, r) for k, r in runs.items()}, **{k + "+route": (True, runs[k]) for k in routed}}


def _trace(hostapi, routes, run):
    """the C calls of one run and of the close() after it, as one string without the wm_ prefixes"""
    ctx = _fake_ctx(hostapi, routes=routes)
    run(ctx)
    ctx.close()
    assert ctx._h is None
    return " ".join(c[3:] for c in ctx.lib.calls)


# recorded on the commit before the binding was folded (its own staging blocks, three caches and call pairs)
_PARENT_TRACES = {
    "permute_u8":
        "malloc memcpy_h2d sync malloc malloc memcpy_h2d sync route_create_dev permute_u8_f32_dev memcpy_d2h "
        "free free free free free destroy",
    "permute_f32":
        "malloc memcpy_h2d sync malloc malloc memcpy_h2d sync permute_f32_dev memcpy_d2h free free free free "
        "free destroy",
    "unpermute":
        "malloc memcpy_h2d sync malloc memcpy_h2d sync route_create_dev malloc malloc unpermute_f32_dev "
        "normalize_u8_dev memcpy_d2h unpermute_f32_dev normalize_u8_dev memcpy_d2h free free free free free "
        "free destroy",
    "unscrambled":
        "malloc memcpy_h2d sync route_create_dev malloc malloc malloc malloc malloc memcpy_h2d sync "
        "memcpy_h2d sync memcpy_h2d sync memcpy_h2d sync extract_tiles_u8_dev route_create_dev malloc malloc "
        "unpermute_f32_dev normalize_u8_dev memcpy_d2h unpermute_f32_dev normalize_u8_dev memcpy_d2h free "
        "free check_status free free free free free free free free destroy",
    "unscrambled_mask":
        "malloc memcpy_h2d sync route_create_dev malloc malloc malloc malloc malloc memcpy_h2d sync "
        "memcpy_h2d sync memcpy_h2d sync memcpy_h2d sync extract_tiles_masked_u8_dev route_create_dev malloc "
        "malloc unpermute_f32_dev normalize_u8_dev memcpy_d2h unpermute_f32_dev normalize_u8_dev memcpy_d2h "
        "free free check_status free free free free free free free free destroy",
    "soft":
        "malloc memcpy_h2d sync memcpy_h2d sync malloc malloc memcpy_h2d sync payload_soft_tiles_u8_dev "
        "memcpy_d2h check_status free free free free free destroy",
    "soft_shared":
        "malloc memcpy_h2d sync memcpy_h2d sync malloc malloc memcpy_h2d sync malloc memcpy_h2d sync "
        "payload_soft_tiles_dither_u8_dev memcpy_d2h check_status free free free free free free destroy",
    "soft_rows":
        "malloc memcpy_h2d sync memcpy_h2d sync malloc malloc memcpy_h2d sync malloc memcpy_h2d sync "
        "payload_soft_tiles_dither_u8_dev memcpy_d2h check_status free free free free free free destroy",
    "sigma_w":
        "payload_sigma_w_tiles_u8 free free destroy",
    "sigma_w_dither":
        "payload_sigma_w_tiles_dither_u8 free free destroy",
    "embed_payload":
        "embed_tiles_payload_u8 free free destroy",
    "embed_payload_dither":
        "embed_tiles_payload_dither_u8 free free destroy",
    "metric":
        "payload_metric_tiles_u8 free free destroy",
    "metric_dither":
        "payload_metric_tiles_dither_u8 free free destroy",
    "embed":
        "embed_tiles_u8 free free destroy",
    "embed_mask":
        "embed_tiles_masked_u8 free free destroy",
    "extract":
        "extract_tiles_u8 free free destroy",
    "extract_mask":
        "extract_tiles_sum_masked_u8 free free destroy",
    "detect":
        "detect_tiles_u8 free free destroy",
    "detect_mask":
        "detect_tiles_masked_u8 free free destroy",
    "session":
        "malloc memcpy_h2d sync malloc malloc memcpy_h2d sync route_create_dev permute_u8_f32_dev memcpy_d2h "
        "free free route_create_dev malloc malloc malloc malloc malloc memcpy_h2d sync memcpy_h2d sync "
        "memcpy_h2d sync memcpy_h2d sync extract_tiles_u8_dev route_create_dev malloc malloc "
        "unpermute_f32_dev normalize_u8_dev memcpy_d2h unpermute_f32_dev normalize_u8_dev memcpy_d2h free "
        "free check_status free free free free free malloc memcpy_h2d sync memcpy_h2d sync malloc malloc "
        "memcpy_h2d sync malloc memcpy_h2d sync payload_soft_tiles_dither_u8_dev memcpy_d2h check_status free "
        "free malloc malloc memcpy_h2d sync malloc memcpy_h2d sync payload_soft_tiles_dither_u8_dev "
        "memcpy_d2h check_status free free free malloc memcpy_h2d sync route_create_dev malloc malloc "
        "unpermute_f32_dev normalize_u8_dev memcpy_d2h unpermute_f32_dev normalize_u8_dev memcpy_d2h free "
        "free free free free free free free destroy",
    "permute_u8+route":
        "malloc memcpy_h2d sync malloc malloc memcpy_h2d sync route_create_dev permute_u8_f32_routed_dev "
        "memcpy_d2h free free route_destroy free free free destroy",
    "permute_f32+route":
        "malloc memcpy_h2d sync malloc malloc memcpy_h2d sync permute_f32_dev memcpy_d2h free free free free "
        "free destroy",
    "unpermute+route":
        "malloc memcpy_h2d sync malloc memcpy_h2d sync route_create_dev malloc unpermute_normalize_u8_dev "
        "memcpy_d2h free free route_destroy free free free destroy",
    "unscrambled+route":
        "malloc memcpy_h2d sync route_create_dev malloc malloc malloc malloc malloc memcpy_h2d sync "
        "memcpy_h2d sync memcpy_h2d sync memcpy_h2d sync extract_unscrambled_u8_dev memcpy_d2h check_status "
        "free free free free free route_destroy free free free destroy",
    "unscrambled_mask+route":
        "malloc memcpy_h2d sync route_create_dev malloc malloc malloc malloc malloc memcpy_h2d sync "
        "memcpy_h2d sync memcpy_h2d sync memcpy_h2d sync extract_unscrambled_masked_u8_dev memcpy_d2h "
        "check_status free free free free free route_destroy free free free destroy",
    "session+route":
        "malloc memcpy_h2d sync malloc malloc memcpy_h2d sync route_create_dev permute_u8_f32_routed_dev "
        "memcpy_d2h free free malloc malloc malloc malloc malloc memcpy_h2d sync memcpy_h2d sync memcpy_h2d "
        "sync memcpy_h2d sync extract_unscrambled_u8_dev memcpy_d2h check_status free free free free free "
        "malloc memcpy_h2d sync memcpy_h2d sync malloc malloc memcpy_h2d sync malloc memcpy_h2d sync "
        "payload_soft_tiles_dither_u8_dev memcpy_d2h check_status free free malloc malloc memcpy_h2d sync "
        "malloc memcpy_h2d sync payload_soft_tiles_dither_u8_dev memcpy_d2h check_status free free free "
        "malloc memcpy_h2d sync malloc unpermute_normalize_u8_dev memcpy_d2h free free route_destroy free "
        "free free free free destroy",
}


@pytest.mark.parametrize("name", sorted(_PARENT_TRACES))
def test_same_c_calls_as_before_the_fold(hostapi, name):
    """Every call of the C ABI, in order, that a method and the close() after it made before the staging scope, the keyed
    cache and the one payload call replaced the copies: the same now.  (All wm_free calls carry one name, so their order
    among themselves is not held; which buffer each releases is the cache test's matter.)"""
    routes, run = _trace_runs()[name]
    got = _trace(hostapi, routes, run)
    assert sorted(got.split()) == sorted(_PARENT_TRACES[name].split())
    assert got == _PARENT_TRACES[name]


def _staged_runs():
    runs = _trace_runs()
    return {k: runs[k] for k in ("permute_u8", "permute_u8+route", "permute_f32", "unpermute", "unpermute+route", "unscrambled",
                                 "unscrambled+route", "unscrambled_mask+route", "soft", "soft_shared", "soft_rows")}


@pytest.mark.parametrize("name", sorted(_staged_runs()))
def test_a_failed_allocation_leaks_nothing(hostapi, name):
    """The k-th wm_malloc of a staged method fails, for every k the method reaches: MemoryError, and by the time it is
    raised every buffer handed out before it is released again, except what a cache keeps - which close() releases."""
    routes, run = _staged_runs()[name]

    def released(lib):
        return [a for a in lib.freed if a in lib.mallocs]
    ok = _fake_ctx(hostapi, routes=routes)
    run(ok)
    cached = set(ok.lib.mallocs) - set(released(ok.lib))                   # the same addresses in every run below
    n_alloc = len(ok.lib.mallocs)
    ok.close()
    assert n_alloc >= 3 and 1 <= len(cached) <= 2 and sorted(released(ok.lib)) == sorted(ok.lib.mallocs)
    for k in range(1, n_alloc + 1):
        ctx = _fake_ctx(hostapi, routes=routes, fail_malloc=k)
        with pytest.raises(MemoryError):
            run(ctx)
        lib = ctx.lib
        assert len(lib.mallocs) == k - 1
        before = released(lib)
        ctx.close()
        kept = released(lib)[len(before):]
        assert set(kept) <= cached, (k, "close() released what no cache holds")
        assert len(before) == len(lib.mallocs) - len(kept), (k, "buffers leaked", len(lib.mallocs) - len(kept) - len(before))
        assert sorted(before + kept) == sorted(lib.mallocs), (k, "a buffer released twice")


def test_device_caches_keep_two_entries_and_release_each_once(hostapi):
    """Three keys through each cache of one context - the permutation index (with its route), the payload's CSR map, the
    shared dither table: the third releases the first one's buffer (and route) and nothing else, after a wm_sync (work
    still queued may read them); the second key again allocates nothing beyond the call's own staging; close() releases
    what is left, once."""
    ctx = _fake_ctx(hostapi, routes=True)
    lib = ctx.lib
    u8 = np.zeros((_TH, _TW), np.uint8)

    def held():
        return [a for a in lib.mallocs + lib.routed if a not in lib.freed]

    def step(call, *args):
        """(handles the call left held, handles held before that it released, its wm_malloc count)"""
        had, n = held(), len(lib.mallocs)
        call(*args)
        now = held()
        return [a for a in now if a not in had], [a for a in had if a not in now], len(lib.mallocs) - n

    def index(k):
        idx = np.roll(np.arange(_TH * _TW), k)
        assert ctx.route_dev(idx) in lib.routed and ctx.index_dev(idx) in lib.mallocs

    def soft(map_k, table_k):
        ctx.payload_soft(u8, np.roll(np.arange(6), map_k), np.array([0, 2, 4, 6]), 3, 16.0, dither=np.full(6, table_k, np.uint16))

    def evicted_after_a_sync(gone):
        at = min(lib.freed_at[a] for a in gone)
        return lib.calls[at - 2:at] == ["wm_sync", "wm_sync"]             # the upload's own, then the eviction's

    i0, gone, _ = step(index, 0)
    assert len(i0) == 2 and not gone                                        # the device index and its route
    assert step(index, 1)[1] == []
    new, gone, _ = step(index, 2)
    assert len(new) == 2 and sorted(gone) == sorted(i0) and evicted_after_a_sync(gone)
    assert lib.calls[lib.freed_at[i0[1]]] == "wm_route_destroy" and lib.freed_at[i0[1]] < lib.freed_at[i0[0]]
    assert step(index, 1) == ([], [], 0)
    (csr0, table0), gone, n = step(soft, 0, 0)                              # the first map and the first table; 2 staged
    assert not gone and n == 4
    assert step(soft, 1, 0)[1:] == ([], 3)
    new, gone, n = step(soft, 2, 0)
    assert len(new) == 1 and gone == [csr0] and n == 3 and evicted_after_a_sync(gone)
    assert step(soft, 1, 0) == ([], [], 2)
    assert step(soft, 1, 1)[1:] == ([], 3)
    new, gone, n = step(soft, 1, 2)
    assert len(new) == 1 and gone == [table0] and n == 3 and evicted_after_a_sync(gone)
    assert step(soft, 1, 1) == ([], [], 2)
    assert len(held()) == 2 * 2 + 2 + 2                                     # two entries a kind; an index entry is two handles
    ctx.close()
    freed = [a for a in lib.freed if a is not None]
    assert held() == [] and len(set(freed)) == len(freed)
