"""Device-event timing of the colour video frame codec (csrc/wm_pixel.hip k_frame_codec: stored Y, Cb, Cr frames with
subsampled chroma <-> planar B, G, R) at 1080p and 4K, 4:2:0 and 4:2:2, 8 frames per launch, alternated in the same run
with k_color<YCC_TO_BGR> / <BGR_TO_YCC> (the interleaved 4:4:4 conversion) on the same pixel counts; then the file-level
embed_watermark_video_color on a 16-frame 1080p clip, 4:2:0 with subsampling="box" against the clip's 4:4:4 form.

    python tools/chroma_codec_bench.py --out profiles/chroma_codec_bench.json [--rounds 15] [--inner 10] [--no-file]

Bytes moved are what the algorithm needs (every input byte read once, every output byte written once); the share is of
the 8 TB/s HBM roof.  A 1080p batch (75-100 MB) fits the 256 MB Infinity Cache, a 4K batch (300-400 MB) does not."""
from __future__ import annotations

import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "digital-watermarking-for-image-video-using-dct-svd-singular-value-decomposition_amd"
SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}
SUBS = {"420": (2, 2), "422": (2, 1)}
HBM_ROOF = 8e12
N_FRAMES = 8


def kernel_rows(ctx, api, rounds: int, inner: int):
    vp = C.c_void_p
    rows = []
    for size, (H, W) in SIZES.items():
        n_px = N_FRAMES * H * W
        d_a, d_b = ctx.malloc(3 * n_px), ctx.malloc(3 * n_px)
        ctx.h2d(d_a, np.random.default_rng(1).integers(0, 256, 3 * n_px, dtype=np.uint8))
        ctx.memset(d_b, 0, 3 * n_px)
        for fmt, sub in SUBS.items():
            fsz = api.Context.frame_bytes(H, W, sub)
            per_px = fsz / (H * W) + 3.0
            calls = {       # step -> (entry point, arguments, bytes moved per pixel)
                f"frames{fmt}_to_bgr_planes": ("wm_yuv_frames_to_bgr_planes_u8_dev",
                                               (vp(d_a), vp(d_b), N_FRAMES, H, W, sub[0], sub[1], fsz), per_px),
                "k_color_ycrcb2bgr": ("wm_ycrcb_to_bgr_u8_dev", (vp(d_a), vp(d_b), n_px), 6.0),
                f"bgr_planes_to_frames{fmt}": ("wm_bgr_planes_to_yuv_frames_u8_dev",
                                               (vp(d_a), vp(d_b), N_FRAMES, H, W, sub[0], sub[1], fsz), per_px),
                "k_color_bgr2ycrcb": ("wm_bgr_to_ycrcb_u8_dev", (vp(d_a), vp(d_b), n_px), 6.0),
            }
            for fn, args, _ in calls.values():
                for _ in range(3):
                    ctx._call(fn, *args)
            ctx.sync()
            ms = {k: [] for k in calls}
            for _ in range(rounds):                        # alternated: every round times each step once
                for step, (fn, args, _) in calls.items():
                    ctx.event_record(0)
                    for _ in range(inner):
                        ctx._call(fn, *args)
                    ctx.event_record(1)
                    ctx.sync()
                    ms[step].append(ctx.event_elapsed_ms(0, 1) / inner)
            for step, (fn, args, bpp) in calls.items():
                t = statistics.median(ms[step]) * 1e-3
                nbytes = bpp * n_px
                row = dict(kind="kernel", size=size, H=H, W=W, n_frames=N_FRAMES, alternated_with=fmt, step=step,
                           us_per_frame=round(t * 1e6 / N_FRAMES, 3), us_per_frame_min=round(min(ms[step]) * 1e3 / N_FRAMES, 3),
                           us_per_frame_max=round(max(ms[step]) * 1e3 / N_FRAMES, 3), bytes_per_px=round(bpp, 3),
                           bytes_moved=int(nbytes), gb_per_s=round(nbytes / t / 1e9, 1),
                           share_of_8tbs=round(nbytes / t / HBM_ROOF, 4), rounds=rounds, launches_per_timing=inner)
                print(json.dumps(row), flush=True)
                rows.append(row)
        ctx.sync()
        ctx.free(d_a); ctx.free(d_b)
    return rows


def file_rows(ctx, runs: int):
    """embed_watermark_video_color, tile=8, on one 16-frame 1080p clip stored as 4:2:0 (subsampling="box") and as 4:4:4"""
    v = importlib.import_module(PKG + ".video")
    hg = importlib.import_module(PKG + ".hostglue")
    H, W, n = 1080, 1920, 16
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[:H, :W]
    planes = np.empty((n, 3, H, W), np.uint8)
    for i in range(n):
        for c, (a, b) in enumerate(((11.0, 3), (7.0, -2), (13.0, 1))):
            planes[i, c] = np.clip(110 + 50 * np.sin((xx + b * i) / a) * np.cos(yy / (a + 4)) + rng.normal(0, 6, (H, W)), 0, 255)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        wp = os.path.join(d, "wm.png")
        assert hg.write_png(wp, rng.integers(0, 256, (64, 64, 3), dtype=np.uint8))
        clips = {}
        for tag, sub in (("420jpeg", (2, 2)), ("444", (1, 1))):
            frames = np.concatenate([ctx.bgr_planes_to_yuv_frames(planes[i:i + 4], sub) for i in range(0, n, 4)])
            clips[tag] = os.path.join(d, f"in{tag}.y4m")
            v.write_y4m(clips[tag], frames[:, :H * W].reshape(n, H, W), frames[:, H * W:], chroma_tag=tag)
        secs = {tag: [] for tag in clips}
        for r in range(runs + 1):                          # alternated; the first pass of each is the warm-up
            for tag, path in clips.items():
                t = time.perf_counter()
                v.embed_watermark_video_color(path, wp, os.path.join(d, "out.y4m"), os.path.join(d, "m.npz"), alpha=0.1,
                                              password="pw", nonce=bytes(8), tile=8, subsampling="box")
                if r:
                    secs[tag].append(time.perf_counter() - t)
        for tag, s in secs.items():
            row = dict(kind="file", step="embed_watermark_video_color", container="C" + tag, H=H, W=W, n_frames=n, tile=8,
                       batch=8, seconds_median=round(statistics.median(s), 4), seconds_all=[round(x, 4) for x in s],
                       ms_per_frame=round(statistics.median(s) * 1e3 / n, 2))
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--file-runs", type=int, default=3)
    ap.add_argument("--no-file", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    api = importlib.import_module(PKG + ".hostapi")
    assert api.device_count() >= 1, "chroma_codec_bench needs a GPU"
    with api.Context(0) as ctx:
        rows = kernel_rows(ctx, api, a.rounds, a.inner)
        if not a.no_file:
            rows += file_rows(ctx, a.file_runs)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
