"""A/B of TWO builds of libwmhip.so in ONE process on one device (no torch).

Tile kernels (default): embed and extract (pixel-domain factors, what bench.py runs) at the bench shape, the variants
interleaved round by round, HIP events on each context's stream.  Prints per variant the median over the rounds and the
spread (max - min) of the round values, and the parity of b against a (stego LSB differences, Sc relative to sigma_1,
extracted watermark).

    python tools/ab_libs.py --a /path/to/parent/libwmhip.so --b <package>/csrc/libwmhip.so [--content natural]

Full-frame mode (--ref): the BYTES of both builds' singular values, embed (stego, Sc), watermark-side SVD (U, S, Vt),
extract and detect on seeded planes, under every combination of WM_RF_HIER, WM_RF_HIER_F16, WM_RF_HGRAM3 and
WM_RF_FINAL_F16 (read by the library on every call).  Extract and detect of both builds get a's stego and factors, so a
difference is that call's own.  The mode is deterministic, so any differing byte is a change of behaviour.

    python tools/ab_libs.py --ref --a /path/to/parent/libwmhip.so --b <package>/csrc/libwmhip.so

Sigma passes of the tile mode (--sigma-pass): the BYTES of both builds' sigma_tiles, mask_sigma_w, payload_sigma_w,
payload_metric, masked embed, payload embed and payload_soft on seeded planes (noise with a constant, a black and a rank-1
tile) at an aligned and a misaligned base.  These kernels are deterministic too: any differing byte is a change of behaviour.

    python tools/ab_libs.py --sigma-pass --a /path/to/parent/libwmhip.so --b <package>/csrc/libwmhip.so

Development aid; bench.py is the contract benchmark."""
import argparse
import ctypes as C
import importlib
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
api = importlib.import_module(
    "digital-watermarking-for-image-video-using-dct-svd-singular-value-decomposition_amd.hostapi")


class LibContext(api.Context):
    """a Context on an explicitly loaded library"""

    def __init__(self, lib):
        self.lib = lib
        h = C.c_void_p()
        assert lib.wm_create(0, None, C.byref(h)) == 0
        self._h = h
        self.device = 0


def make_frames(content, F, H, W, rng):
    if content == "noise":
        return rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    low = rng.uniform(20, 235, (F, H // 16 + 2, W // 16 + 2)).astype(np.float32)     # quick_bench.py's "natural"
    up = np.kron(low, np.ones((16, 16), np.float32))[:, 8:8 + H, 8:8 + W]
    for ax in (1, 2):
        c = np.cumsum(up, axis=ax)
        up = (np.take(c, np.arange(16, c.shape[ax]), axis=ax) - np.take(c, np.arange(0, c.shape[ax] - 16), axis=ax)) / 16
        pad = [(0, 0)] * 3; pad[ax] = (8, 8); up = np.pad(up, pad, mode="edge")
    return np.clip(up + rng.normal(0, 2.0, up.shape), 0, 255).astype(np.uint8)


class Side:
    def __init__(self, path, host, wys, alpha):
        self.ctx = ctx = LibContext(api.load_library(path))
        F, H, W = host.shape
        self.dims = (F, H, W)
        self.alpha = alpha
        nt = (H // 8) * (W // 8)
        self.d_host = ctx.malloc(host.nbytes); ctx.h2d(self.d_host, host)
        self.d_stego = ctx.malloc(host.nbytes)
        d_wys = ctx.malloc(wys.nbytes); ctx.h2d(d_wys, wys)
        d_U = ctx.malloc(nt * 256); d_V = ctx.malloc(nt * 256)
        self.d_S = ctx.malloc(nt * 32)
        self.d_Ux = ctx.malloc(nt * 256); self.d_Vx = ctx.malloc(nt * 256)
        self.d_sc = ctx.malloc(F * nt * 32)
        self.d_out = ctx.malloc(F * H * W * 4)
        ctx.svd_tiles_f32_dev(d_wys, d_U, self.d_S, d_V, 1, H, W, W, H * W)
        ctx.tile_factors_to_pixel_dev(d_U, d_V, self.d_Ux, self.d_Vx, nt)
        self.embed(); self.extract(); ctx.sync()

    def embed(self):
        F, H, W = self.dims
        self.ctx.embed_tiles_u8_dev(self.d_host, self.d_S, self.d_stego, self.d_sc, None, F, H, W, W, H * W, 0, self.alpha, 8)

    def extract(self):
        F, H, W = self.dims
        self.ctx.extract_tiles_px_u8_dev(self.d_stego, self.d_sc, self.d_Ux, self.d_Vx, self.d_out, F, H, W, W, H * W, 0,
                                         self.alpha, 8)

    def time_us(self, fn, launches):
        self.ctx.sync()
        self.ctx.event_record(0)
        for _ in range(launches):
            fn()
        self.ctx.event_record(1)
        self.ctx.sync()
        return self.ctx.event_elapsed_ms(0, 1) * 1e3 / launches

    def results(self):
        F, H, W = self.dims
        nt = (H // 8) * (W // 8)
        st = np.empty((F, H, W), np.uint8); sc = np.empty((F, nt, 8), np.float32); out = np.empty((F, H, W), np.float32)
        self.ctx.sync()
        self.ctx.d2h(st, self.d_stego); self.ctx.d2h(sc, self.d_sc); self.ctx.d2h(out, self.d_out)
        self.ctx.sync()
        self.ctx.check_status()
        return st, sc, out


def seeded_planes(B, H, W, seed=5):
    """tests/test_gpu_fullframe_twolevel.py's planes: noise, from three planes on a smooth and a half-empty one as well"""
    rng = np.random.default_rng(seed)
    planes = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    if B >= 3:
        planes[1] = (np.outer(np.linspace(0, 200, H), np.ones(W)) + 20 * np.sin(np.arange(W) / 9.0)[None, :]).astype(np.uint8)
        planes[2, :, W // 2:] = 0
    return planes


def ref_bits(path_a, path_b, alpha=0.15):
    ctx = {"a": LibContext(api.load_library(path_a)), "b": LibContext(api.load_library(path_b))}
    inputs = [("3x320x480", seeded_planes(3, 320, 480)), ("2x832x900", seeded_planes(2, 832, 900)),
              ("3x1080x1920", np.random.default_rng(21).integers(0, 256, (3, 1080, 1920), dtype=np.uint8))]
    inputs += [(f"2x{H}x{W}", seeded_planes(2, H, W)) for H, W in ((64, 97), (128, 130), (320, 323), (97, 64))]
    n_diff = n_cmp = 0
    for hier, f16, h3, fin in itertools.product((0, 1), (3, 1, 0), (0, 1), (1, 0)):
        os.environ.update(WM_RF_HIER=str(hier), WM_RF_HIER_F16=str(f16), WM_RF_HGRAM3=str(h3), WM_RF_FINAL_F16=str(fin))
        for name, planes in inputs:
            _, H, W = planes.shape
            K = int(0.6 * min(H, W))
            wm = np.random.default_rng(H * 10000 + W).integers(0, 256, (1, H, W)).astype(np.float32)
            got = {}
            for k, c in ctx.items():
                U, S, Vt = c.ref_svd_planes(wm, apply_dct=True)
                got[k] = {"sigma": c.ref_sigma_planes(planes), "U": U, "S": S, "Vt": Vt}
                got[k]["two_level"] = c.ref_last_flops()[1]
            for k, c in ctx.items():            # the same watermark factors (a's) for both builds from here on
                emb = c.ref_embed_planes(planes, got["a"]["S"][0], alpha, K)
                got[k]["stego"], got[k]["Sc"] = emb[0], emb[1]
            ga = got["a"]
            for k, c in ctx.items():
                got[k]["extract"] = c.ref_extract_planes(ga["stego"], ga["Sc"], ga["U"][0], ga["Vt"][0], alpha, K)
                got[k]["detect"] = c.ref_detect_planes(ga["stego"], ga["Sc"], ga["S"][0], alpha)
                c.check_status()
            keys = ("sigma", "stego", "Sc", "U", "S", "Vt", "extract", "detect")
            diff = [q for q in keys if np.asarray(got["a"][q]).tobytes() != np.asarray(got["b"][q]).tobytes()]
            n_cmp += len(keys); n_diff += len(diff)
            print(f"HIER={hier} HIER_F16={f16} HGRAM3={h3} FINAL_F16={fin}  {name:12s} sigma two-level={got['a']['two_level']}:  "
                  + ("all %d results equal bytes" % len(keys) if not diff else "DIFFERENT: " + ", ".join(diff)), flush=True)
    print(f"{n_cmp} results compared, {n_diff} differ")
    for c in ctx.values():
        c.close()
    return 1 if n_diff else 0


def sigma_pass_bits(path_a, path_b, alpha=0.15, mask=(8.0, 64.0), delta=16.0):
    """Tile mode, everything that runs a sigma pass: the BYTES of both builds' sigma_tiles, mask_sigma_w (eff + gain),
    payload_sigma_w, payload_metric, masked embed, payload embed (stego with the caller's bytes around it, Sc, yw) and
    payload_soft, on 3 planes of 72 x 136 (153 tiles: the third wave is partial) of noise with a constant, a black and a
    rank-1 tile, cut out of a larger array at an aligned and at a misaligned base."""
    ctx = {"a": LibContext(api.load_library(path_a)), "b": LibContext(api.load_library(path_b))}
    n, H, W = 3, 72, 136
    nt = (H // 8) * (W // 8)
    rng = np.random.default_rng(31)
    sw = np.sort(np.abs(rng.normal(0, 300, (nt, 8))).astype(np.float32), axis=-1)[:, ::-1].copy()
    tile_bit = rng.integers(0, 2, nt).astype(np.uint8)
    bit_of = rng.permutation(nt) % 16
    order = np.argsort(bit_of, kind="stable").astype(np.int32)
    offs = np.concatenate(([0], np.cumsum(np.bincount(bit_of, minlength=16)))).astype(np.int32)
    n_diff = n_cmp = 0
    for name, rs, (y0, x0) in (("aligned", 144, (0, 0)), ("misaligned", 139, (1, 3))):
        base = rng.integers(0, 256, (n, H + 2, rs), dtype=np.uint8)
        view = base[:, y0:y0 + H, x0:x0 + W]
        view[0, 8:16, 16:24] = 77
        view[1, 16:24, 8:16] = 0
        view[2, 24:32, 40:48] = np.outer(np.arange(1, 9), np.arange(3, 11)).astype(np.uint8)
        off, ps = y0 * rs + x0, (H + 2) * rs
        plane = (n, H, W, rs, ps)
        got = {}
        for k, c in ctx.items():
            d = {q: c.malloc(b) for q, b in dict(p=base.nbytes, st=base.nbytes, s=n * nt * 32, eff=n * nt * 32, g=n * nt * 4, sc=n * nt * 32,
                                                 yw=n * H * W * 4, sw=sw.nbytes, bit=nt, order=order.nbytes, offs=offs.nbytes, soft=128).items()}
            for q, arr in (("p", base), ("sw", sw), ("bit", tile_bit), ("order", order), ("offs", offs)):
                c.h2d(d[q], arr)
            R = got[k] = {}

            def get(q, shape, dtype):
                out = np.empty(shape, dtype); c.sync(); c.d2h(out, d[q]); c.sync()
                return out

            c.sigma_tiles_u8_dev(d["p"] + off, d["s"], *plane)
            R["sigma_tiles"] = get("s", (n, nt, 8), np.float32)
            c.mask_sigma_w_tiles_u8_dev(d["p"] + off, d["sw"], d["eff"], d["g"], *plane, 0, *mask)
            R["mask_sigma_w"] = get("eff", (n, nt, 8), np.float32); R["mask_gain"] = get("g", (n, nt), np.float32)
            c._call("wm_payload_sigma_w_tiles_u8_dev", d["p"] + off, d["bit"], d["eff"], *plane, delta)
            R["payload_sigma_w"] = get("eff", (n, nt, 8), np.float32)
            c._call("wm_payload_metric_tiles_u8_dev", d["p"] + off, d["g"], *plane, delta)
            R["payload_metric"] = get("g", (n, nt), np.float32)
            for what, embed in (("masked_embed", lambda: c.embed_tiles_masked_u8_dev(d["p"] + off, d["sw"], d["st"] + off, d["sc"], d["yw"], *plane,
                                                                                      0, alpha, 6, *mask)),
                                ("payload_embed", lambda: c._call("wm_embed_tiles_payload_u8_dev", d["p"] + off, d["bit"], d["st"] + off, d["sc"],
                                                                  d["yw"], *plane, delta))):
                c.memset(d["st"], 0xA5, base.nbytes); c.memset(d["sc"], 0, n * nt * 32); c.memset(d["yw"], 0, n * H * W * 4)
                embed()
                R[what + "_stego"], R[what + "_Sc"] = get("st", base.shape, np.uint8), get("sc", (n, nt, 8), np.float32)
                R[what + "_yw"] = get("yw", (n, H, W), np.float32)
            c._call("wm_payload_soft_tiles_u8_dev", d["st"] + off, d["order"], d["offs"], 16, d["soft"], *plane, delta)   # (of the payload stego)
            R["payload_soft"] = get("soft", 16, np.float64)
            c.check_status()
            for q in d.values():
                c.free(q)
        diff = [q for q in got["a"] if got["a"][q].tobytes() != got["b"][q].tobytes()]
        n_cmp += len(got["a"]); n_diff += len(diff)
        st = got["a"]["payload_embed_stego"][:, y0:y0 + H, x0:x0 + W]
        print(f"{name:10s} base offset {off}, row stride {rs}: " + ("all %d results equal bytes" % len(got["a"]) if not diff else
              "DIFFERENT: " + ", ".join(diff)) + f"  (payload stego: black tile -> {int(st[1, 16, 8])}, soft[:4] "
              f"{np.round(got['a']['payload_soft'][:4], 3).tolist()})", flush=True)
    print(f"{n_cmp} results compared, {n_diff} differ")
    for c in ctx.values():
        c.close()
    return 1 if n_diff else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", action="store_true", help="full-frame mode: compare the bytes of both builds' results")
    ap.add_argument("--sigma-pass", action="store_true", help="tile mode: compare the bytes of everything that runs a sigma pass")
    ap.add_argument("--a", required=True, help="libwmhip.so of the baseline")
    ap.add_argument("--b", required=True, help="libwmhip.so of the variant")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--H", type=int, default=2160)
    ap.add_argument("--W", type=int, default=3840)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup-rounds", type=int, default=2, help="rounds run first and left out (clocks settle)")
    ap.add_argument("--alpha", type=float, default=0.15)
    ap.add_argument("--content", default="noise", choices=["noise", "natural"])
    a = ap.parse_args()
    if a.ref:
        sys.exit(ref_bits(a.a, a.b, a.alpha))
    if a.sigma_pass:
        sys.exit(sigma_pass_bits(a.a, a.b, a.alpha))
    rng = np.random.default_rng(1234)
    host = np.ascontiguousarray(make_frames(a.content, a.frames, a.H, a.W, rng))
    wys = rng.integers(0, 256, (a.H, a.W)).astype(np.float32)
    sides = {"a": Side(a.a, host, wys, a.alpha), "b": Side(a.b, host, wys, a.alpha)}
    t = {(k, w): [] for k in sides for w in ("embed", "extract")}
    for r in range(-a.warmup_rounds, a.rounds):
        for k in (("a", "b") if r % 2 == 0 else ("b", "a")):
            s = sides[k]
            te, tx = s.time_us(s.embed, a.launches), s.time_us(s.extract, a.launches)
            if r >= 0:
                t[k, "embed"].append(te); t[k, "extract"].append(tx)
        if r < 0:
            continue
        print("round %d  " % r + "  ".join(f"{k}.{w} {t[k, w][-1]:8.1f}" for k in "ab" for w in ("embed", "extract")), flush=True)
    print(f"content={a.content}, {a.frames} frames {a.W}x{a.H}, {a.rounds} rounds x {a.launches} launches, us per launch")
    for w in ("embed", "extract"):
        ma, mb = np.median(t["a", w]), np.median(t["b", w])
        spread = max(np.ptp(t["a", w]), np.ptp(t["b", w]))
        print(f"{w:8s} a {ma:9.1f}  b {mb:9.1f}  delta {100 * (mb / ma - 1):+6.2f} %  ({ma - mb:+.1f} us; round-to-round spread "
              f"{spread:.1f} us, delta / spread {abs(ma - mb) / max(spread, 1e-9):.1f})")
    (st_a, sc_a, w_a), (st_b, sc_b, w_b) = sides["a"].results(), sides["b"].results()
    d = np.abs(st_a.astype(np.int16) - st_b.astype(np.int16))
    print(f"parity b vs a: stego max {int(d.max())} LSB on {float((d != 0).mean()):.2e} of the pixels, "
          f"Sc max {float(np.max(np.abs(sc_a - sc_b) / np.maximum(sc_a[..., :1], 1.0))):.2e} sigma_1, "
          f"extract max |diff| {float(np.max(np.abs(w_a - w_b))):.3e} (values up to {float(np.max(np.abs(w_a))):.1f})")
    # the sigma-only kernel of both builds on IDENTICAL input (a's stego)
    F, H, W = host.shape
    sig = {}
    sides["b"].ctx.h2d(sides["b"].d_host, st_a)
    for k, s in sides.items():
        s.ctx.sigma_tiles_u8_dev(s.d_stego if k == "a" else s.d_host, s.d_sc, F, H, W, W, H * W)
        sig[k] = np.empty_like(sc_a); s.ctx.sync(); s.ctx.d2h(sig[k], s.d_sc); s.ctx.sync(); s.ctx.check_status()
    rel = np.abs(sig["a"] - sig["b"]) / np.maximum(sig["a"][..., :1], 1.0)
    print(f"sigma-only kernel on the same stego: max |b - a| {float(rel.max()):.2e} sigma_1, tiles above 2e-6: "
          f"{int((rel.max(axis=-1) > 2e-6).sum())} of {rel.shape[0] * rel.shape[1]}, above 1e-5: {int((rel.max(axis=-1) > 1e-5).sum())}")
    for s in sides.values():
        s.ctx.close()


if __name__ == "__main__":
    main()
