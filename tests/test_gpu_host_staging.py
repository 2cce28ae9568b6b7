"""The host-pointer entry points stage their arrays through grow-only buffers of the context, each with ONE statement of
its layout (wmi::staged).  Every such entry point must return, bit for bit, what its `_dev` form returns on buffers the
caller allocated, at the shapes where a layout can go wrong: planes cut out of a larger array (ragged border, a base
that is not 8-byte aligned, odd byte counts), a single tile, no tile at all, shared and per-plane sigma_w / factors.
The results must not depend on what the buffers held or how large they already were."""
import ctypes as C
import math

import numpy as np
import pytest

import payload_refs as pr

pytestmark = pytest.mark.gpu

ALPHA, K = 0.15, 6
LO, HI, MCUT = 8.0, 64.0, 0.25        # the texture-masked rule's defaults (meta.MASK_DEFAULT)
DELTA = pr.DELTA                      # the payload rule's default step
# bits: the payload bits the case's tiles are dealt to
CUT = dict(n=3, H=19, W=27, base=(3, 21, 32), at=(1, 3), bits=3)      # 2 x 3 tiles, rows of 32 from element 35 on
ONE_TILE = dict(n=1, H=8, W=8, base=None, at=None, bits=1)
NO_TILE = dict(n=1, H=7, W=13, base=None, at=None, bits=1)
DENSE = dict(n=2, H=40, W=104, base=None, at=None, bits=5)            # 65 tiles: the second wave has one live lane
LARGE = dict(n=2, H=64, W=96, base=None, at=None, bits=5)
CASES = {"cut_shared": (CUT, True), "cut_per_plane": (CUT, False), "one_tile": (ONE_TILE, False), "no_tile": (NO_TILE, True),
         "dense": (DENSE, False)}


def _vp(x):
    return C.c_void_p(int(x)) if x else None


class Planes:
    """n planes of H x W inside `base` (dense, or a cut out of a larger array whose other bytes belong to the caller)"""

    def __init__(self, case, dtype, rng, fill=None):
        n, H, W = case["n"], case["H"], case["W"]
        shape = case["base"] or (n, H, W)
        y, x = case["at"] or (0, 0)
        if fill is None:
            self.base = (rng.integers(0, 256, shape).astype(dtype) if dtype == np.uint8
                         else rng.normal(100.0, 60.0, shape).astype(dtype))
        else:
            self.base = np.full(shape, fill, dtype)
        self.view = self.base[:, y:y + H, x:x + W]
        self.off = y * shape[2] + x                   # elements from the base to the first sample
        self.rs, self.ps = shape[2], shape[1] * shape[2]
        self.span = (n - 1) * self.ps + (H - 1) * self.rs + W      # elements from the first sample to the last
        self.inside = np.zeros(shape, bool)
        self.inside[:, y:y + H, x:x + W] = True

    def like(self, base):
        p = object.__new__(Planes)
        p.__dict__.update(self.__dict__)
        p.base = base
        y, x = np.argwhere(self.inside[0])[0]
        p.view = base[:, y:y + self.view.shape[1], x:x + self.view.shape[2]]
        return p


def make_inputs(case, shared, seed):
    rng = np.random.default_rng(seed)
    n, H, W = case["n"], case["H"], case["W"]
    nby, nbx = H // 8, W // 8
    nt = nby * nbx
    host = Planes(case, np.uint8, rng)
    if case is CUT:  # the flagged-tile lists of the embed: a constant tile, a rank-1 tile, a tile of rank 2
        host.view[0, :8, :8] = 77
        host.view[1, 8:16, 16:24] = np.outer(np.arange(1, 9), np.arange(3, 11)).astype(np.uint8)
        host.view[2, :8, 8:16] = host.view[2, :2, 8:16].repeat(4, axis=0)
        host.view[0, 8:16, 8:16] = 0     # and a black tile, which the payload embed rewrites on its own (k_embed_black)
    lead = () if shared else (n,)
    sw = np.sort(np.abs(rng.normal(0, 300, lead + (nby, nbx, 8))).astype(np.float32), axis=-1)[..., ::-1].copy()
    idx = rng.permutation(H * W).astype(np.int32)
    I = dict(
        n=n, H=H, W=W, nt=nt, shared=shared, case=case, host=host,
        stego_fill=Planes(case, np.uint8, rng, fill=0xA5),
        fplanes=Planes(case, np.float32, rng),
        sw=sw, sw_ps=0 if shared else nt * 8,
        sc=np.abs(rng.normal(0, 300, (n, nby, nbx, 8))).astype(np.float32),
        U=rng.normal(0, 0.4, lead + (nby, nbx, 8, 8)).astype(np.float32),
        Vt=rng.normal(0, 0.4, lead + (nby, nbx, 8, 8)).astype(np.float32),
        uv_ps=0 if shared else nt,
        U_all=rng.normal(0, 0.4, (n, nby, nbx, 8, 8)).astype(np.float32),
        Vt_all=rng.normal(0, 0.4, (n, nby, nbx, 8, 8)).astype(np.float32),
        sw_hat=np.abs(rng.normal(0, 300, (n, nby, nbx, 8))).astype(np.float32),
        idx=idx,
        bgr=rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
        y_new=rng.integers(0, 256, (H, W), dtype=np.uint8),
        a8=rng.integers(0, 256, n * H * W, dtype=np.uint8), b8=rng.integers(0, 256, n * H * W, dtype=np.uint8),
        img8=rng.integers(0, 256, (H, W), dtype=np.uint8), img8b=rng.integers(0, 256, (H, W), dtype=np.uint8),
        imgf=rng.normal(120, 50, (H, W)).astype(np.float32), imgfb=rng.normal(120, 50, (H, W)).astype(np.float32),
        xf=rng.normal(10, 200, n * H * W).astype(np.float32),
    )
    # payload: a bit per tile, and the tile-to-bit map in CSR form (a bit's tiles in ascending order)
    n_bits = case["bits"]
    I["tile_bit"] = rng.integers(0, 2, nt).astype(np.uint8)
    bit_of = rng.permutation(nt) % n_bits
    I["order"] = np.argsort(bit_of, kind="stable").astype(np.int32)
    I["offs"] = np.concatenate(([0], np.cumsum(np.bincount(bit_of, minlength=n_bits)))).astype(np.int32)
    I["n_bits"] = n_bits
    return I


COLOR_OPS = ("wm_bgr_to_ycrcb_u8_dev", "wm_ycrcb_to_bgr_u8_dev", "wm_bgr_to_gray_u8_dev", "wm_bgr_to_y_u8_dev", "wm_replace_y_u8_dev")


def _ssim_pair(I, kind):
    return (I["imgf"] if kind & 1 else I["img8"]), (I["imgfb"] if kind & 2 else I["img8b"])


def _psnr_of(ssd, n):        # the library's own expression, in the same double arithmetic
    mse = float(ssd) / float(n)
    return 99.0 if mse <= 1e-12 else 20.0 * math.log10(255.0 / max(math.sqrt(mse), 1e-12))


def run_host(ctx, I):
    """every converted entry point through its host-pointer form (wm_extract_unscrambled_u8_dev: the one call)"""
    n, H, W, nt = I["n"], I["H"], I["W"], I["nt"]
    hp, fp = I["host"], I["fplanes"]
    nby, nbx = H // 8, W // 8
    R = {}
    call = ctx._call
    ptr = lambda a: _vp(a.ctypes.data)
    # embed with yw into a separate stego array whose other bytes are the caller's; without yw in place
    st = hp.like(I["stego_fill"].base.copy())
    sc = np.zeros((n, nby, nbx, 8), np.float32); yw = np.zeros((n, H, W), np.float32)
    call("wm_embed_tiles_u8", ptr(hp.view), ptr(I["sw"]), ptr(st.view), ptr(sc), ptr(yw), n, H, W, hp.rs, hp.ps, I["sw_ps"], ALPHA, K)
    R["embed_yw"] = (st.base, sc, yw)
    ip = hp.like(hp.base.copy())
    sc = np.zeros((n, nby, nbx, 8), np.float32)
    call("wm_embed_tiles_u8", ptr(ip.view), ptr(I["sw"]), ptr(ip.view), ptr(sc), None, n, H, W, hp.rs, hp.ps, I["sw_ps"], ALPHA, K)
    R["embed_inplace"] = (ip.base, sc)
    s = np.zeros((n, nby, nbx, 8), np.float32)
    call("wm_sigma_tiles_u8", ptr(hp.view), ptr(s), n, H, W, hp.rs, hp.ps)
    R["sigma"] = s
    U = np.zeros((n, nby, nbx, 8, 8), np.float32); S = np.zeros((n, nby, nbx, 8), np.float32); Vt = np.zeros_like(U)
    call("wm_svd_tiles_f32", ptr(fp.view), ptr(U), ptr(S), ptr(Vt), n, H, W, fp.rs, fp.ps)
    R["svd"] = (U, S, Vt)
    out = np.zeros((n, H, W), np.float32)
    call("wm_extract_tiles_u8", ptr(hp.view), ptr(I["sc"]), ptr(I["U"]), ptr(I["Vt"]), ptr(out), n, H, W, hp.rs, hp.ps, I["uv_ps"], ALPHA, K)
    R["extract"] = out
    tot = np.zeros((H, W), np.float32)
    call("wm_extract_tiles_sum_u8", ptr(hp.view), ptr(I["sc"]), ptr(I["U"]), ptr(I["Vt"]), ptr(tot), n, H, W, hp.rs, hp.ps, I["uv_ps"], ALPHA, K)
    R["extract_sum"] = tot
    out = np.zeros((n, H, W), np.float32)
    call("wm_reconstruct_tiles", ptr(I["U_all"]), ptr(I["sw_hat"]), ptr(I["Vt_all"]), ptr(out), n, H, W)
    R["reconstruct"] = out
    scores = np.zeros(n, np.float64)
    call("wm_detect_tiles_u8", ptr(hp.view), ptr(I["sc"]), ptr(I["sw"]), ptr(scores), n, H, W, hp.rs, hp.ps, I["sw_ps"], ALPHA)
    R["detect"] = scores
    for op in range(5):
        plane_out = op in (2, 3)
        o = np.zeros((H, W) if plane_out else (H, W, 3), np.uint8)
        call("wm_color_u8", op, ptr(I["bgr"]), ptr(I["y_new"]) if op == 4 else None, None if plane_out else ptr(o),
             ptr(o) if plane_out else None, H * W)
        R[f"color{op}"] = o
    v = C.c_double(0.0)
    call("wm_psnr_u8", ptr(I["a8"]), ptr(I["b8"]), I["a8"].size, C.byref(v))
    R["psnr"] = v.value
    for kind in range(4):
        x, y = _ssim_pair(I, kind)
        v = C.c_double(0.0)
        call("wm_ssim", ptr(x), ptr(y), H, W, kind, C.byref(v))
        R[f"ssim{kind}"] = v.value
    for dn in (0, 1):
        o = np.zeros(I["xf"].size, np.uint8)
        call("wm_normalize_u8", ptr(I["xf"]), I["xf"].size, dn, ptr(o))
        R[f"normalize{dn}"] = o
    for ch, img in ((1, I["img8"]), (3, I["bgr"])):
        o = np.zeros_like(img)
        call("wm_enhance_extract_u8", ptr(img), ptr(o), H, W, ch)
        R[f"enhance{ch}"] = o
    R.update(_unscrambled(ctx, I, fused=True))
    # texture-masked strength
    eff = np.zeros((n, nby, nbx, 8), np.float32); g = np.zeros((n, nby, nbx), np.float32)
    call("wm_mask_sigma_w_tiles_u8", ptr(hp.view), ptr(I["sw"]), ptr(eff), ptr(g), n, H, W, hp.rs, hp.ps, I["sw_ps"], LO, HI)
    R["mask_sw"] = (eff, g)
    g = np.zeros((n, nby, nbx), np.float32)
    call("wm_mask_sigma_w_tiles_u8", ptr(hp.view), None, None, ptr(g), n, H, W, hp.rs, hp.ps, 0, LO, HI)
    R["mask_gain"] = g
    st = hp.like(I["stego_fill"].base.copy())
    sc = np.zeros((n, nby, nbx, 8), np.float32); yw = np.zeros((n, H, W), np.float32)
    call("wm_embed_tiles_masked_u8", ptr(hp.view), ptr(I["sw"]), ptr(st.view), ptr(sc), ptr(yw), n, H, W, hp.rs, hp.ps, I["sw_ps"],
         ALPHA, K, LO, HI)
    R["masked_embed_yw"] = (st.base, sc, yw)
    ip = hp.like(hp.base.copy())
    sc = np.zeros((n, nby, nbx, 8), np.float32)
    call("wm_embed_tiles_masked_u8", ptr(ip.view), ptr(I["sw"]), ptr(ip.view), ptr(sc), None, n, H, W, hp.rs, hp.ps, I["sw_ps"],
         ALPHA, K, LO, HI)
    R["masked_embed_inplace"] = (ip.base, sc)
    out = np.zeros((n, H, W), np.float32)
    call("wm_extract_tiles_masked_u8", ptr(hp.view), ptr(I["sc"]), ptr(I["U"]), ptr(I["Vt"]), ptr(out), n, H, W, hp.rs, hp.ps,
         I["uv_ps"], ALPHA, K, LO, HI, MCUT)
    R["masked_extract"] = out
    tot = np.zeros((H, W), np.float32)
    call("wm_extract_tiles_sum_masked_u8", ptr(hp.view), ptr(I["sc"]), ptr(I["U"]), ptr(I["Vt"]), ptr(tot), n, H, W, hp.rs, hp.ps,
         I["uv_ps"], ALPHA, K, LO, HI, MCUT)
    R["masked_extract_sum"] = tot
    scores = np.zeros(n, np.float64)
    call("wm_detect_tiles_masked_u8", ptr(hp.view), ptr(I["sc"]), ptr(I["sw"]), ptr(scores), n, H, W, hp.rs, hp.ps, I["sw_ps"],
         ALPHA, LO, HI, MCUT)
    R["masked_detect"] = scores
    # blind payload
    eff = np.zeros((n, nby, nbx, 8), np.float32)
    call("wm_payload_sigma_w_tiles_u8", ptr(hp.view), ptr(I["tile_bit"]), ptr(eff), n, H, W, hp.rs, hp.ps, DELTA)
    R["payload_sw"] = eff
    st = hp.like(I["stego_fill"].base.copy())
    sc = np.zeros((n, nby, nbx, 8), np.float32); yw = np.zeros((n, H, W), np.float32)
    call("wm_embed_tiles_payload_u8", ptr(hp.view), ptr(I["tile_bit"]), ptr(st.view), ptr(sc), ptr(yw), n, H, W, hp.rs, hp.ps, DELTA)
    R["payload_embed_yw"] = (st.base, sc, yw)
    ip = hp.like(hp.base.copy())
    sc = np.zeros((n, nby, nbx, 8), np.float32)
    call("wm_embed_tiles_payload_u8", ptr(ip.view), ptr(I["tile_bit"]), ptr(ip.view), ptr(sc), None, n, H, W, hp.rs, hp.ps, DELTA)
    R["payload_embed_inplace"] = (ip.base, sc)
    m = np.zeros((n, nby, nbx), np.float32)
    call("wm_payload_metric_tiles_u8", ptr(hp.view), ptr(m), n, H, W, hp.rs, hp.ps, DELTA)
    R["payload_metric"] = m
    soft = np.zeros(I["n_bits"], np.float64)
    rc = ctx.lib.wm_payload_soft_tiles_u8(ctx._h, ptr(hp.view), ptr(I["order"]), ptr(I["offs"]), I["n_bits"], ptr(soft),
                                          n, H, W, hp.rs, hp.ps, DELTA)
    R["payload_soft"] = (np.int32(rc), soft)         # (no tile: both forms refuse, and with the same code)
    return R


class Dev:
    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def new(self, nbytes):
        self.ptrs.append(self.ctx.malloc(max(int(nbytes), 16)))
        return self.ptrs[-1]

    def put(self, arr):
        d = self.new(arr.nbytes)
        self.ctx.h2d(d, arr)
        return d

    def get(self, d, shape, dtype):
        out = np.zeros(shape, dtype)
        self.ctx.d2h(out, d)
        self.ctx.sync()
        return out

    def put_planes(self, p, base=None):
        """the planes from their first sample on, on a 256-byte line as the wrappers stage them -> pointer to that sample"""
        flat = (p.base if base is None else base).reshape(-1)
        return self.put(flat[p.off:p.off + p.span])

    def get_planes(self, d, p, base):
        """`base` with what the device holds from the first sample to the last"""
        out = base.copy()
        out.reshape(-1)[p.off:p.off + p.span] = self.get(d, p.span, base.dtype)
        return out

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)


def _unscrambled(ctx, I, fused):
    """fused: wm_extract_unscrambled_u8_dev; else the extract, then the routed unscramble + normalise, as two calls"""
    n, H, W = I["n"], I["H"], I["W"]
    hp = I["host"]
    R = {}
    d = Dev(ctx)
    try:
        d_idx = d.put(I["idx"])
        route = C.c_void_p()
        ctx._call("wm_route_create_dev", _vp(d_idx), H * W, C.byref(route))
        try:
            d_st, d_sc, d_u, d_v = d.put(hp.base), d.put(I["sc"]), d.put(I["U"]), d.put(I["Vt"])
            d_w, d_o = d.new(n * H * W * 4), d.new(n * H * W)
            for dn in (0, 1):
                if fused:
                    ctx._call("wm_extract_unscrambled_u8_dev", _vp(d_st + hp.off), _vp(d_sc), _vp(d_u), _vp(d_v), route, _vp(d_o),
                              n, H, W, hp.rs, hp.ps, I["uv_ps"], ALPHA, K, 0, dn)
                else:
                    ctx.extract_tiles_u8_dev(d_st + hp.off, d_sc, d_u, d_v, d_w, n, H, W, hp.rs, hp.ps, I["uv_ps"], ALPHA, K)
                    ctx._call("wm_unpermute_normalize_u8_dev", _vp(d_w), route, _vp(d_o), H * W, n, dn)
                ctx.check_status()
                R[f"unscrambled{dn}"] = d.get(d_o, (n, H, W), np.uint8)
        finally:
            ctx._call("wm_route_destroy", route)
    finally:
        d.close()
    return R


def run_dev(ctx, I):
    """The same calls through the `_dev` forms on buffers of the test's own.  Planes go to the device as the wrappers put
    them there, from their first sample on at the start of an allocation, so that both forms run the same instantiation
    of each kernel: the 8-byte and the byte-wise tile I/O variants are separate machine code, and a layout is not
    judged by whether two compilations of the fallback chain round yw alike."""
    n, H, W, nt = I["n"], I["H"], I["W"], I["nt"]
    hp, fp = I["host"], I["fplanes"]
    nby, nbx = H // 8, W // 8
    R = {}
    d = Dev(ctx)
    call = ctx._call
    try:
        d_host, d_sw, d_scin = d.put_planes(hp), d.put(I["sw"]), d.put(I["sc"])
        d_st, d_sc, d_yw = d.put_planes(hp, I["stego_fill"].base), d.new(n * nt * 32), d.new(n * H * W * 4)
        ctx.memset(d_sc, 0, n * nt * 32); ctx.memset(d_yw, 0, n * H * W * 4)
        ctx.embed_tiles_u8_dev(d_host, d_sw, d_st, d_sc, d_yw, n, H, W, hp.rs, hp.ps, I["sw_ps"], ALPHA, K)
        ctx.check_status()
        R["embed_yw"] = (d.get_planes(d_st, hp, I["stego_fill"].base), d.get(d_sc, (n, nby, nbx, 8), np.float32),
                         d.get(d_yw, (n, H, W), np.float32))
        d_ip = d.put_planes(hp)
        ctx.memset(d_sc, 0, n * nt * 32)
        ctx.embed_tiles_u8_dev(d_ip, d_sw, d_ip, d_sc, 0, n, H, W, hp.rs, hp.ps, I["sw_ps"], ALPHA, K)
        ctx.check_status()
        R["embed_inplace"] = (d.get_planes(d_ip, hp, hp.base), d.get(d_sc, (n, nby, nbx, 8), np.float32))
        ctx.memset(d_sc, 0, n * nt * 32)
        ctx.sigma_tiles_u8_dev(d_host, d_sc, n, H, W, hp.rs, hp.ps)
        ctx.check_status()
        R["sigma"] = d.get(d_sc, (n, nby, nbx, 8), np.float32)
        d_f, d_U, d_V = d.put_planes(fp), d.new(n * nt * 256), d.new(n * nt * 256)
        for p, b in ((d_U, n * nt * 256), (d_V, n * nt * 256), (d_sc, n * nt * 32)):
            ctx.memset(p, 0, b)
        ctx.svd_tiles_f32_dev(d_f, d_U, d_sc, d_V, n, H, W, fp.rs, fp.ps)
        ctx.check_status()
        R["svd"] = (d.get(d_U, (n, nby, nbx, 8, 8), np.float32), d.get(d_sc, (n, nby, nbx, 8), np.float32),
                    d.get(d_V, (n, nby, nbx, 8, 8), np.float32))
        d_u, d_v, d_out = d.put(I["U"]), d.put(I["Vt"]), d.new(n * H * W * 4)
        ctx.extract_tiles_u8_dev(d_host, d_scin, d_u, d_v, d_out, n, H, W, hp.rs, hp.ps, I["uv_ps"], ALPHA, K)
        ctx.check_status()
        R["extract"] = d.get(d_out, (n, H, W), np.float32)
        tot = np.zeros((H, W), np.float32)          # k_sum_planes: planes added in ascending order, in float32
        for z in range(n):
            tot = tot + R["extract"][z]
        R["extract_sum"] = tot
        d_ua, d_va, d_sh = d.put(I["U_all"]), d.put(I["Vt_all"]), d.put(I["sw_hat"])
        ctx.reconstruct_tiles_dev(d_ua, d_sh, d_va, d_out, n, H, W)
        R["reconstruct"] = d.get(d_out, (n, H, W), np.float32)
        d_scores = d.new(n * 8)
        ctx.detect_tiles_u8_dev(d_host, d_scin, d_sw, d_scores, n, H, W, hp.rs, hp.ps, I["sw_ps"], ALPHA)
        ctx.check_status()
        R["detect"] = d.get(d_scores, n, np.float64)
        d_bgr, d_y, d_o3, d_o1 = d.put(I["bgr"]), d.put(I["y_new"]), d.new(H * W * 3), d.new(H * W)
        for op, fn in enumerate(COLOR_OPS):
            plane_out = op in (2, 3)
            args = (_vp(d_bgr),) + ((_vp(d_y),) if op == 4 else ()) + (_vp(d_o1 if plane_out else d_o3), H * W)
            call(fn, *args)
            R[f"color{op}"] = d.get(d_o1, (H, W), np.uint8) if plane_out else d.get(d_o3, (H, W, 3), np.uint8)
        d_a, d_b, d_ssd = d.put(I["a8"]), d.put(I["b8"]), d.new(8)
        call("wm_sqdiff_u8_dev", _vp(d_a), _vp(d_b), I["a8"].size, _vp(d_ssd))
        R["psnr"] = _psnr_of(int(d.get(d_ssd, 1, np.uint64)[0]), I["a8"].size)
        d_res = d.new(8)
        for kind in range(4):
            x, y = _ssim_pair(I, kind)
            d_x, d_yy = d.put(x), d.put(y)
            call("wm_ssim_dev", _vp(d_x), W, _vp(d_yy), W, H, W, kind, _vp(d_res))
            R[f"ssim{kind}"] = float(d.get(d_res, 1, np.float64)[0])
        d_xf, d_q = d.put(I["xf"]), d.new(I["xf"].size)
        for dn in (0, 1):
            call("wm_normalize_u8_dev", _vp(d_xf), I["xf"].size, dn, _vp(d_q))
            R[f"normalize{dn}"] = d.get(d_q, I["xf"].size, np.uint8)
        for ch, img in ((1, I["img8"]), (3, I["bgr"])):
            d_i, d_e = d.put(img), d.new(img.nbytes)
            call("wm_enhance_extract_u8_dev", _vp(d_i), _vp(d_e), H, W, ch)
            R[f"enhance{ch}"] = d.get(d_e, img.shape, np.uint8)
        # texture-masked strength
        d_eff, d_g = d.new(n * nt * 32), d.new(n * nt * 4)
        ctx.memset(d_eff, 0, n * nt * 32); ctx.memset(d_g, 0, n * nt * 4)
        ctx.mask_sigma_w_tiles_u8_dev(d_host, d_sw, d_eff, d_g, n, H, W, hp.rs, hp.ps, I["sw_ps"], LO, HI)
        ctx.check_status()
        R["mask_sw"] = (d.get(d_eff, (n, nby, nbx, 8), np.float32), d.get(d_g, (n, nby, nbx), np.float32))
        ctx.memset(d_g, 0, n * nt * 4)
        ctx.mask_sigma_w_tiles_u8_dev(d_host, 0, 0, d_g, n, H, W, hp.rs, hp.ps, 0, LO, HI)
        ctx.check_status()
        R["mask_gain"] = d.get(d_g, (n, nby, nbx), np.float32)

        def embed_pair(key, embed):
            """embed(host, stego, sigma_c, yw): with yw into the caller's stego array, then in place without"""
            d_st = d.put_planes(hp, I["stego_fill"].base)
            ctx.memset(d_sc, 0, n * nt * 32); ctx.memset(d_yw, 0, n * H * W * 4)
            embed(d_host, d_st, d_sc, d_yw)
            ctx.check_status()
            R[key + "_yw"] = (d.get_planes(d_st, hp, I["stego_fill"].base), d.get(d_sc, (n, nby, nbx, 8), np.float32),
                              d.get(d_yw, (n, H, W), np.float32))
            d_ip = d.put_planes(hp)
            ctx.memset(d_sc, 0, n * nt * 32)
            embed(d_ip, d_ip, d_sc, 0)
            ctx.check_status()
            R[key + "_inplace"] = (d.get_planes(d_ip, hp, hp.base), d.get(d_sc, (n, nby, nbx, 8), np.float32))

        embed_pair("masked_embed", lambda h, s, c, y: ctx.embed_tiles_masked_u8_dev(
            h, d_sw, s, c, y, n, H, W, hp.rs, hp.ps, I["sw_ps"], ALPHA, K, LO, HI))
        call("wm_extract_tiles_masked_u8_dev", _vp(d_host), _vp(d_scin), _vp(d_u), _vp(d_v), _vp(d_out), n, H, W, hp.rs, hp.ps,
             I["uv_ps"], ALPHA, K, LO, HI, MCUT)
        ctx.check_status()
        R["masked_extract"] = d.get(d_out, (n, H, W), np.float32)
        tot = np.zeros((H, W), np.float32)
        for z in range(n):
            tot = tot + R["masked_extract"][z]
        R["masked_extract_sum"] = tot
        call("wm_detect_tiles_masked_u8_dev", _vp(d_host), _vp(d_scin), _vp(d_sw), _vp(d_scores), n, H, W, hp.rs, hp.ps,
             I["sw_ps"], ALPHA, LO, HI, MCUT)
        ctx.check_status()
        R["masked_detect"] = d.get(d_scores, n, np.float64)
        # blind payload
        d_bit = d.put(I["tile_bit"])
        ctx.memset(d_eff, 0, n * nt * 32)
        call("wm_payload_sigma_w_tiles_u8_dev", _vp(d_host), _vp(d_bit), _vp(d_eff), n, H, W, hp.rs, hp.ps, DELTA)
        ctx.check_status()
        R["payload_sw"] = d.get(d_eff, (n, nby, nbx, 8), np.float32)
        embed_pair("payload_embed", lambda h, s, c, y: call(
            "wm_embed_tiles_payload_u8_dev", _vp(h), _vp(d_bit), _vp(s), _vp(c), _vp(y), n, H, W, hp.rs, hp.ps, DELTA))
        ctx.memset(d_g, 0, n * nt * 4)
        call("wm_payload_metric_tiles_u8_dev", _vp(d_host), _vp(d_g), n, H, W, hp.rs, hp.ps, DELTA)
        ctx.check_status()
        R["payload_metric"] = d.get(d_g, (n, nby, nbx), np.float32)
        d_order, d_offs, d_soft = d.put(I["order"]), d.put(I["offs"]), d.new(I["n_bits"] * 8)
        ctx.memset(d_soft, 0, I["n_bits"] * 8)
        rc = ctx.lib.wm_payload_soft_tiles_u8_dev(ctx._h, _vp(d_host), _vp(d_order), _vp(d_offs), I["n_bits"], _vp(d_soft),
                                                  n, H, W, hp.rs, hp.ps, DELTA)
        ctx.check_status()
        R["payload_soft"] = (np.int32(rc), d.get(d_soft, I["n_bits"], np.float64))
    finally:
        d.close()
    R.update(_unscrambled(ctx, I, fused=False))
    return R


def _differences(a, b):
    bad = []
    assert a.keys() == b.keys()
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], tuple) else ((a[k],), (b[k],))
        for j, (x, y) in enumerate(zip(xs, ys)):
            x, y = np.asarray(x), np.asarray(y)
            # bit for bit: the same bytes, so a NaN equals itself and -0.0 differs from 0.0
            if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                bad.append(f"{k}[{j}]")
    return bad


@pytest.fixture(scope="module")
def host_results(gpu_ctx):
    """the host-pointer forms of every case, computed once on the session's context"""
    return {name: run_host(gpu_ctx, make_inputs(case, shared, 11)) for name, (case, shared) in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_host_form_equals_dev_form(gpu_ctx, host_results, name):
    case, shared = CASES[name]
    I = make_inputs(case, shared, 11)
    assert _differences(host_results[name], run_dev(gpu_ctx, I)) == []
    # what the caller owns around the planes comes back as it went in, the planes themselves are written
    hp, fill = I["host"], I["stego_fill"]
    for embed in ("embed", "masked_embed", "payload_embed"):
        st = host_results[name][embed + "_yw"][0]
        assert np.array_equal(st[~hp.inside], fill.base[~hp.inside]), embed
        assert not np.array_equal(st[hp.inside], fill.base[hp.inside]), embed
        ip = host_results[name][embed + "_inplace"][0]
        assert np.array_equal(ip[~hp.inside], hp.base[~hp.inside]), embed
        if I["nt"] == 0:         # no tile: the border copy alone
            assert np.array_equal(st[hp.inside], hp.base[hp.inside]) and np.array_equal(ip, hp.base), embed
    # payload_soft: answered where the case has a tile, refused (by both forms, with the compared code) where it has none
    assert (int(host_results[name]["payload_soft"][0]) != 0) == (I["nt"] == 0)
    if case is CUT:          # the black tile takes the payload embed's flat form: a constant tile, no longer black
        t = host_results[name]["payload_embed_yw"][0][hp.inside].reshape(hp.view.shape)[0, 8:16, 8:16]
        assert t.min() == t.max() and t.max() > 0


def test_layouts_do_not_depend_on_the_buffers_history(hostapi, host_results):
    """19 x 27, 8 x 8, 19 x 27 on one context; the same after a larger first call.  Every run of a case must give the
    bytes the session's context gave (which had run other shapes before)."""
    seq = ("cut_per_plane", "one_tile", "cut_per_plane")
    for warm_up in (False, True):
        with hostapi.Context(0) as ctx:
            if warm_up:
                run_host(ctx, make_inputs(LARGE, False, 5))
            runs = [run_host(ctx, make_inputs(*CASES[name], 11)) for name in seq]
        assert _differences(runs[0], runs[2]) == [], f"warm_up={warm_up}"
        for name, r in zip(seq, runs):
            assert _differences(r, host_results[name]) == [], f"warm_up={warm_up} {name}"
