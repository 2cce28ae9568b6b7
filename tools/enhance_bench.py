"""Device-event timing of the extract post-processing chain (csrc/wm_enhance.hip) per 1080p and 4K plane:
NL-means (gray h=7, ab pair h=3), CLAHE, unsharp (gray, BGR) and the whole gray / colour chains.  Prints one JSON line
per (size, step) and writes them all to --out.  --oracle also times the NumPy specification (tests/enhance_oracle.py)
once at 1080p gray, for context: it is the NumPy oracle, not OpenCV.

    python tools/enhance_bench.py --out profiles/enhance_bench.json [--reps 20] [--oracle]

k_nlmeans does H*W*441 patch distances; the rate printed is pixel-offsets/s, and VALU lane-ops/s with the kernel's
VALU instructions per pixel and offset counted in its gfx950 ISA (NLM_VALU_PER_PX_OFFSET)."""
from __future__ import annotations

import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "digital-watermarking-for-image-video-using-dct-svd-singular-value-decomposition_amd"
SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}
# VALU instructions of one search offset's loop body (hipcc -O3 --save-temps) x 256 lanes / 64 x 26 outputs of a workgroup
NLM_VALU_PER_PX_OFFSET = {1: 107 * 256 / (64 * 26), 2: 122 * 256 / (64 * 26)}
VALU_PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9   # CUs x SIMDs x lanes per clock x clock: 157.3 TFLOPS FP32 vector / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--oracle", action="store_true")
    a = ap.parse_args()
    api = importlib.import_module(PKG + ".hostapi")
    assert api.device_count() >= 1, "enhance_bench needs a GPU"
    ctx = api.Context(0)
    vp = C.c_void_p
    rows = []
    for name in a.sizes.split(","):
        H, W = SIZES[name]
        n = H * W
        rng = np.random.default_rng(1)
        yy, xx = np.mgrid[:H, :W]
        base = 128 + 60 * np.sin(xx / 37.0) * np.cos(yy / 23.0)
        bgr = np.clip(base[..., None] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
        src, dst = ctx.malloc(3 * n + 4096), ctx.malloc(3 * n + 4096)
        ctx.h2d(src, bgr)
        steps = {
            "nlmeans_gray_h7": ("wm_nlmeans_u8_dev", (vp(src), vp(dst), H, W, 1, 7.0, 7, 21), 1),
            "nlmeans_ab_h3": ("wm_nlmeans_u8_dev", (vp(src), vp(dst), H, W, 2, 3.0, 7, 21), 2),
            "clahe": ("wm_clahe_u8_dev", (vp(src), vp(dst), H, W, 2.0, 8, 8), None),
            "unsharp_gray": ("wm_unsharp_u8_dev", (vp(src), vp(dst), H, W, 1, 0.25), None),
            "unsharp_bgr": ("wm_unsharp_u8_dev", (vp(src), vp(dst), H, W, 3, 0.15), None),
            "chain_gray": ("wm_enhance_extract_u8_dev", (vp(src), vp(dst), H, W, 1), None),
            "chain_color": ("wm_enhance_extract_u8_dev", (vp(src), vp(dst), H, W, 3), None),
        }
        for step, (fn, args, nlm_ch) in steps.items():
            for _ in range(a.warmup):
                ctx._call(fn, *args)
            ctx.sync()
            ctx.event_record(0)
            for _ in range(a.reps):
                ctx._call(fn, *args)
            ctx.event_record(1)
            ctx.sync()
            ms = ctx.event_elapsed_ms(0, 1) / a.reps
            row = dict(size=name, H=H, W=W, step=step, ms=round(ms, 4), reps=a.reps)
            if nlm_ch:
                row["pixel_offsets_per_s"] = n * 441 / (ms * 1e-3)
                row["valu_lane_ops_per_s"] = row["pixel_offsets_per_s"] * NLM_VALU_PER_PX_OFFSET[nlm_ch]
                row["share_of_valu_peak"] = row["valu_lane_ops_per_s"] / VALU_PEAK_LANE_OPS
            print(json.dumps(row), flush=True)
            rows.append(row)
        ctx.free(src); ctx.free(dst)
    if a.oracle:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        eo = importlib.import_module("enhance_oracle")
        img = np.random.default_rng(2).integers(0, 256, (1080, 1920), dtype=np.uint8)
        t = time.perf_counter()
        eo.enhance_gray(img)
        row = dict(size="1080p", step="numpy_oracle_chain_gray", ms=round((time.perf_counter() - t) * 1e3, 1), reps=1)
        print(json.dumps(row), flush=True)
        rows.append(row)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
