"""What texture-masked strength costs on the device, and what it leaves alone (no torch, no fallback without a GPU).

Per frame size (1080p and 4K, 64 frames per launch) the variants are timed interleaved in ONE process, HIP events on the
context's stream, after warm-up rounds that are left out:

    embed_uniform / embed_masked / mask_sigma_w (the gain pass alone)
    extract_plain / extract_masked (pixel-domain factors, what bench.py runs)      detect_plain / detect_masked
    extract_plain_on_masked_stego / detect_plain_on_masked_stego (the plain rule on the masked stego: same tiles, no flag)

The expectation to confirm or correct: embed_masked = embed_uniform + mask_sigma_w.  With --parent-lib the unmasked
variants of ANOTHER build of libwmhip.so (the parent commit's) run in the same rounds, so a difference beyond the
round-to-round spread on embed_uniform / extract_plain / detect_plain would mean the change is not free for them.  A
parent that has the gain pass also runs its sigma_tiles and mask_sigma_w there, and --sigma-pass-out records this build's
against the parent's own round-to-round spread (sigma_pass_record).

Also records the parity figures of the masked embed against the oracle on the test hosts (tests/mask_refs.py: what
tests/test_gpu_mask.py holds to its bars), uniform and masked.

--content letterbox: the textured frames with black bars (an eighth of the height at the top and at the bottom), whose
tiles the masked embed redoes along the flat vector (k_embed_black); a parent build that has the masked embed runs its
masked variants in the same rounds, and derived.embed_masked_new_over_parent is what the repair costs.

    python tools/mask_bench.py [--parent-lib /path/to/parent/libwmhip.so] [--out profiles/mask_bench.json]
    python tools/mask_bench.py --parent-lib ... --content letterbox --sizes 1080p --out profiles/mask_bench_letterbox.json

Development aid; bench.py is the contract benchmark."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
api = importlib.import_module(
    "digital-watermarking-for-image-video-using-dct-svd-singular-value-decomposition_amd.hostapi")

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}
MASK = (8.0, 64.0, 0.25)


def load_build(path):
    """another build of the library, typed like hostapi.load_library but tolerant of entry points it predates"""
    lib = C.CDLL(path)
    for name, argtypes in api.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes = argtypes
            fn.restype = C.c_char_p if name == "wm_last_error" else C.c_int
    return lib


class LibContext(api.Context):
    def __init__(self, lib):
        self.lib = lib
        h = C.c_void_p()
        if lib.wm_create(0, None, C.byref(h)) != 0:
            raise RuntimeError((lib.wm_last_error() or b"wm_create failed").decode())
        self._h = h
        self.device = 0


def sigma_pass_record(path, entries):
    """entries: name -> (this build's round values, the parent's, both in us, same interleaved rounds).  Adds to the JSON at
    ``path``, per name, both medians and whether this build's lies within the parent's OWN round-to-round spread
    (max - min) above the parent's median - the bar a refactor of the sigma passes is held to - and prints it."""
    rec = json.load(open(path)) if os.path.exists(path) else {}
    for name, (new, par) in entries.items():
        spread, diff = float(np.ptp(par)), float(np.median(new) - np.median(par))
        rec[name] = dict(unit="us per launch", rounds=len(new), new_median=float(np.median(new)), new_min=float(np.min(new)),
                         new_max=float(np.max(new)), parent_median=float(np.median(par)), parent_min=float(np.min(par)),
                         parent_max=float(np.max(par)), parent_spread=spread, new_minus_parent=diff,
                         within_parent_spread=bool(diff <= spread))
        print(f"sigma pass {name:38s} new {np.median(new):9.1f} us  parent {np.median(par):9.1f} us  ({diff:+.1f} us; parent's "
              f"round-to-round spread {spread:.1f} us: {'within' if diff <= spread else 'SLOWER THAN THE SPREAD ALLOWS'})", flush=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def make_frames(content, F, H, W, rng):
    if content == "noise":
        return rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    if content == "letterbox":
        frames = make_frames("textured", F, H, W, rng)
        bar = H // 64 * 8                                                   # whole tile rows
        frames[:, :bar] = 0; frames[:, H - bar:] = 0
        return frames
    # smooth field + sensor noise: every regime of the gain
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 70 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 40 * np.sin((xx + 2 * yy) / 91.0)
    std = np.kron(rng.choice([0.0, 1.0, 3.0, 10.0, 30.0], (H // 64 + 1, W // 64 + 1)), np.ones((64, 64)))[:H, :W]
    distinct = [np.clip(base + rng.normal(0, 1, (H, W)) * std, 0, 255).astype(np.uint8) for _ in range(min(F, 4))]
    return np.stack([distinct[i % len(distinct)] for i in range(F)])       # (a launch's time does not depend on the frames differing)


class Side:
    """one build's buffers and launches at one frame size"""

    def __init__(self, ctx, host, wys, alpha, masked):
        self.ctx, self.alpha = ctx, alpha
        F, H, W = self.dims = host.shape
        nt = (H // 8) * (W // 8)
        self.d_host = ctx.malloc(host.nbytes); ctx.h2d(self.d_host, host)
        self.d_stego = ctx.malloc(host.nbytes)
        self.d_wys = d_wys = ctx.malloc(wys.nbytes); ctx.h2d(d_wys, wys)
        self.d_U = ctx.malloc(nt * 256); self.d_V = ctx.malloc(nt * 256)
        self.d_S = ctx.malloc(nt * 32)
        self.d_sc = ctx.malloc(F * nt * 32)
        self.d_out = ctx.malloc(F * H * W * 4)
        self.d_scores = ctx.malloc(F * 8)
        gain_pass = masked or hasattr(ctx.lib, "wm_mask_sigma_w_tiles_u8_dev")       # (a parent build that has the pass)
        self.d_eff = ctx.malloc(F * nt * 32) if gain_pass else 0
        ctx.svd_tiles_f32_dev(d_wys, self.d_U, self.d_S, self.d_V, 1, H, W, W, H * W)
        ctx.tile_factors_to_pixel_dev(self.d_U, self.d_V, self.d_U, self.d_V, nt)
        self.plane = (F, H, W, W, H * W)
        self.variants = {"embed_uniform": self.embed_uniform, "extract_plain": self.extract_plain, "detect_plain": self.detect_plain}
        if gain_pass and not masked:
            self.variants.update(sigma_tiles=self.sigma_tiles, mask_sigma_w=self.mask_sigma_w)
        if masked:
            self.variants.update(sigma_tiles=self.sigma_tiles)
            self.variants.update(embed_masked=self.embed_masked, mask_sigma_w=self.mask_sigma_w,
                                 extract_masked=self.extract_masked, detect_masked=self.detect_masked,
                                 extract_plain_on_masked_stego=self.extract_plain_m, detect_plain_on_masked_stego=self.detect_plain_m)
        # the masked stego is what the masked extract / detect read; the plain ones read the uniform stego (left last)
        if masked:
            self.d_stego_m = ctx.malloc(host.nbytes); self.d_sc_m = ctx.malloc(F * nt * 32)
            ctx.embed_tiles_masked_u8_dev(self.d_host, self.d_S, self.d_stego_m, self.d_sc_m, None, *self.plane, 0, alpha, 8, *MASK[:2])
        self.embed_uniform()
        ctx.sync(); ctx.check_status()

    def embed_uniform(self):
        self.ctx.embed_tiles_u8_dev(self.d_host, self.d_S, self.d_stego, self.d_sc, None, *self.plane, 0, self.alpha, 8)

    def embed_masked(self):
        self.ctx.embed_tiles_masked_u8_dev(self.d_host, self.d_S, self.d_stego_m, self.d_sc_m, None, *self.plane, 0, self.alpha, 8,
                                           *MASK[:2])

    def sigma_tiles(self):          # (into d_eff: [plane][tile][8] as well)
        self.ctx.sigma_tiles_u8_dev(self.d_host, self.d_eff, *self.plane)

    def mask_sigma_w(self):
        self.ctx.mask_sigma_w_tiles_u8_dev(self.d_host, self.d_S, self.d_eff, None, *self.plane, 0, *MASK[:2])

    def extract_plain(self):
        self.ctx.extract_tiles_px_u8_dev(self.d_stego, self.d_sc, self.d_U, self.d_V, self.d_out, *self.plane, 0, self.alpha, 8)

    def extract_masked(self):
        self.ctx._call("wm_extract_tiles_px_masked_u8_dev", self.d_stego_m, self.d_sc_m, self.d_U, self.d_V, self.d_out, *self.plane,
                       0, self.alpha, 8, *MASK)

    # the plain rule on the MASKED stego: the sweeps a wave needs depend on its tiles, so the flag's own cost is
    # extract_masked against this, not against extract_plain on the uniform stego
    def extract_plain_m(self):
        self.ctx.extract_tiles_px_u8_dev(self.d_stego_m, self.d_sc_m, self.d_U, self.d_V, self.d_out, *self.plane, 0, self.alpha, 8)

    def detect_plain_m(self):
        self.ctx.detect_tiles_u8_dev(self.d_stego_m, self.d_sc_m, self.d_S, self.d_scores, *self.plane, 0, self.alpha)

    def detect_plain(self):
        self.ctx.detect_tiles_u8_dev(self.d_stego, self.d_sc, self.d_S, self.d_scores, *self.plane, 0, self.alpha)

    def detect_masked(self):
        self.ctx._call("wm_detect_tiles_masked_u8_dev", self.d_stego_m, self.d_sc_m, self.d_S, self.d_scores, *self.plane, 0,
                       self.alpha, *MASK)

    def time_us(self, fn, launches):
        self.ctx.sync()
        self.ctx.event_record(0)
        for _ in range(launches):
            fn()
        self.ctx.event_record(1)
        self.ctx.sync()
        return self.ctx.event_elapsed_ms(0, 1) * 1e3 / launches

    def free(self):
        for k, v in list(self.__dict__.items()):
            if k.startswith("d_") and v:
                self.ctx.free(v)


def bench_size(name, a, ctxs):
    H, W = SIZES[name]
    rng = np.random.default_rng(1234)
    host = np.ascontiguousarray(make_frames(a.content, a.frames, H, W, rng))
    wys = rng.integers(0, 256, (H, W)).astype(np.float32)
    sides = {k: Side(c, host, wys, a.alpha, masked=(k == "new" or hasattr(c.lib, "wm_embed_tiles_masked_u8_dev")))
             for k, c in ctxs.items()}
    runs = [(k, v) for k, s in sides.items() for v in s.variants]
    t = {kv: [] for kv in runs}
    for r in range(-a.warmup_rounds, a.rounds):
        for k, v in (runs if r % 2 == 0 else runs[::-1]):             # alternate the order round by round
            us = sides[k].time_us(sides[k].variants[v], a.launches)
            if r >= 0:
                t[k, v].append(us)
    for s in sides.values():
        s.ctx.check_status()
        s.free()
    out = {}
    for (k, v), xs in t.items():
        out[v if k == "new" else f"{k}.{v}"] = dict(median_us=float(np.median(xs)), min_us=float(np.min(xs)), max_us=float(np.max(xs)),
                                                    spread_us=float(np.ptp(xs)))
    m = {k: v["median_us"] for k, v in out.items()}
    out["derived"] = dict(masked_embed_minus_uniform_us=m["embed_masked"] - m["embed_uniform"], mask_sigma_w_us=m["mask_sigma_w"],
                          masked_embed_over_uniform=m["embed_masked"] / m["embed_uniform"],
                          masked_extract_over_plain=m["extract_masked"] / m["extract_plain"],
                          masked_detect_over_plain=m["detect_masked"] / m["detect_plain"],
                          masked_extract_over_plain_same_stego=m["extract_masked"] / m["extract_plain_on_masked_stego"],
                          masked_detect_over_plain_same_stego=m["detect_masked"] / m["detect_plain_on_masked_stego"])
    if "parent" in ctxs:
        out["derived"].update({f"{v}_new_over_parent": m[v] / m[f"parent.{v}"]
                               for v in ("embed_uniform", "extract_plain", "detect_plain", "embed_masked") if f"parent.{v}" in m})
        if a.sigma_pass_out:
            sigma_pass_record(a.sigma_pass_out, {f"mask_bench.{v}_{name}": (t["new", v], t["parent", v]) for v in ("sigma_tiles", "mask_sigma_w")
                                                 if ("parent", v) in t})
    print(name, json.dumps(out["derived"]), flush=True)
    return out


def parity_figures(ctx):
    """the figures tests/test_gpu_mask.py::test_masked_embed_against_the_oracle holds to its bars"""
    import mask_refs as mr
    out = {}
    for H, W in ((64, 64), (72, 100)):
        for case in ("one_plane", "three_shared", "three_per_plane"):
            planes = mr.planes_of(H, W, 1 if case == "one_plane" else 3)
            wms = [mr.watermark(H, W, 9 + p) for p in range(3)] if case == "three_per_plane" else mr.watermark(H, W)
            out[f"{case}_{H}x{W}"] = mr.embed_figures(ctx, planes, wms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libwmhip.so of the parent commit: its unmasked variants run in the same rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_bench.json"))
    ap.add_argument("--sigma-pass-out", help="with --parent-lib: add sigma_tiles / mask_sigma_w of both builds to this JSON (sigma_pass_record)")
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup-rounds", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=0.12)
    ap.add_argument("--content", default="textured", choices=["textured", "noise", "letterbox"])
    a = ap.parse_args()
    if api.device_count() < 1:
        sys.exit("mask_bench needs a GPU: there is no host fallback")
    ctxs = {"new": api.Context(0)}
    if a.parent_lib:
        ctxs["parent"] = LibContext(load_build(a.parent_lib))
    res = dict(frames=a.frames, rounds=a.rounds, launches=a.launches, warmup_rounds=a.warmup_rounds, alpha=a.alpha, mask=MASK,
               content=a.content, unit="us per launch of `frames` frames, HIP events, variants interleaved in one process",
               parent_lib=bool(a.parent_lib), sizes={})
    for name in a.sizes.split(","):
        res["sizes"][name] = bench_size(name, a, ctxs)
    res["embed_parity_on_test_hosts"] = parity_figures(ctxs["new"])
    for c in ctxs.values():
        c.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
