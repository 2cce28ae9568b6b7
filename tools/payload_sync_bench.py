"""What crop resynchronisation of the blind payload costs on the device (no torch, no fallback without a GPU).

One resident plane at 1080p and at 4K, the variants timed interleaved in ONE process with HIP events on the context's stream,
after warm-up rounds that are left out, the order of the variants drawn afresh for every round (payload_bench.time_variants):

    phase_scan        wm_payload_phase_scan_u8_dev: the votes and sums of all 64 grid phases in one launch
    metric_64_calls   the yardstick: the same windows as 64 calls of wm_payload_metric_tiles_u8_dev on offset pointers - the
                      way to scan the phases without a new kernel (it leaves float metrics; the sums would be another pass)
    metric_1_call     one such call (phase 0): what one decode of an uncropped stego pays for its sigma pass
    offset_scan       wm_payload_offset_scores_dev for a half-size crop (ny = nby / 2, nx = nbx / 2) under a map of
                      n_bits = 1024: (nby - ny + 1) (nbx - nx + 1) placements, a workgroup each

Also records that the phase scan's votes equal rint(32768 m) of the 64-call form's metrics, window for window.

    python tools/payload_sync_bench.py [--out profiles/payload_sync_bench.json]

Development aid; bench.py is the contract benchmark."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mask_bench import api, make_frames                     # noqa: E402
from payload_bench import DELTA, SIZES, summary, time_variants   # noqa: E402

N_BITS = 1024


def bench_size(ctx, label, warmup, rounds, content):
    H, W = SIZES[label]
    rng = np.random.default_rng(23)
    nby, nbx = H // 8, W // 8
    pitch = nby * nbx
    plane = make_frames(content, 1, H, W, rng)[0]
    tile_bit = rng.integers(0, 2, pitch).astype(np.uint8)
    stego = ctx.embed_tiles_payload(plane, tile_bit, DELTA)[0]              # a marked plane: phase 0 is the embed's grid
    d_p = ctx.malloc(stego.nbytes); ctx.h2d(d_p, stego)
    d_votes, d_sums, d_metric = ctx.malloc(64 * pitch * 4), ctx.malloc(64 * 8), ctx.malloc(64 * pitch * 4)
    ny, nx = nby // 2, nbx // 2
    V = rng.integers(-32768, 32769, (ny, nx)).astype(np.int32)
    T = (rng.permutation(pitch) % N_BITS).astype(np.int32)
    scores = np.zeros((nby - ny + 1, nbx - nx + 1), np.int64)
    d_V, d_T, d_scores = ctx.malloc(V.nbytes), ctx.malloc(T.nbytes), ctx.malloc(scores.nbytes)
    ctx.h2d(d_V, V); ctx.h2d(d_T, T)
    vp = api._vp

    def phase_scan():
        ctx._call("wm_payload_phase_scan_u8_dev", vp(d_p), vp(d_votes), vp(d_sums), 1, H, W, W, H * W, DELTA)

    def metric_call(p):
        py, px = divmod(p, 8)
        ctx._call("wm_payload_metric_tiles_u8_dev", vp(d_p + py * W + px), vp(d_metric + p * pitch * 4), 1, H - py, W - px, W, H * W, DELTA)

    def metric_64_calls():
        for p in range(64):
            metric_call(p)

    def offset_scan():
        ctx._call("wm_payload_offset_scores_dev", vp(d_V), vp(d_T), vp(d_scores), ny, nx, nby, nbx, N_BITS)

    variants = {"phase_scan": ("this", phase_scan), "metric_64_calls": ("this", metric_64_calls),
                "metric_1_call": ("this", lambda: metric_call(0)), "offset_scan": ("this", offset_scan)}
    ms = time_variants({"this": ctx, "parent": ctx}, variants, warmup, rounds, shuffle_seed=31)
    ctx.sync(); ctx.check_status()
    votes = np.empty((64, pitch), np.int32); metric = np.empty((64, pitch), np.float32); sums = np.empty(64, np.int64)
    ctx.d2h(votes, d_votes); ctx.d2h(metric, d_metric); ctx.d2h(sums, d_sums); ctx.d2h(scores, d_scores); ctx.sync()
    equal, own_sums = True, True
    for p in range(64):
        n = ((H - p // 8) // 8) * ((W - p % 8) // 8)
        equal &= bool(np.array_equal(votes[p, :n], np.rint(metric[p, :n] * np.float32(32768)).astype(np.int32)))
        own_sums &= int(np.abs(votes[p, :n].astype(np.int64)).sum()) == int(sums[p])
    for d in (d_p, d_votes, d_sums, d_metric, d_V, d_T, d_scores):
        ctx.free(d)
    res = {k: summary(v) for k, v in ms.items()}
    a, b = res["phase_scan"], res["metric_64_calls"]
    mean = sums / (32768.0 * np.array([((H - p // 8) // 8) * ((W - p % 8) // 8) for p in range(64)]))
    return dict(H=H, W=W, windows=int(sum(((H - p // 8) // 8) * ((W - p % 8) // 8) for p in range(64))), content=content,
                order="a seeded permutation of the variants per round", variants=res,
                phase_scan_against_64_calls=dict(
                    median_ratio=a["median_ms"] / b["median_ms"], median_minus_its_median_ms=a["median_ms"] - b["median_ms"],
                    inside_its_spread=bool(b["min_ms"] <= a["median_ms"] <= b["max_ms"]),
                    outside_by_ms=float(max(a["median_ms"] - b["max_ms"], b["min_ms"] - a["median_ms"], 0.0))),
                offset_scan=dict(ny=ny, nx=nx, nby=nby, nbx=nbx, n_bits=N_BITS, placements=int(scores.size),
                                 windows_per_placement=ny * nx),
                votes_equal_rint_of_64_call_metrics=equal, sums_equal_sum_abs_votes=own_sums,
                mean_abs_m=dict(phase_0=float(mean[0]), best_other=float(np.delete(mean, 0).max()), median=float(np.median(mean))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "payload_sync_bench.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--content", default="natural")
    a = ap.parse_args()
    ctx = api.Context(0)
    res = dict(delta=DELTA, sizes={})
    for label in a.sizes.split(","):
        res["sizes"][label] = bench_size(ctx, label, a.warmup, a.rounds, a.content)
        print(label, {k: round(x["median_ms"], 3) for k, x in res["sizes"][label]["variants"].items()}, flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
