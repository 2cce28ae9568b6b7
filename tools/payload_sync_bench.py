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

--keyed: the keyed search of a dithered payload's crop instead (wmhip.h, "keyed crop resynchronisation"), to
profiles/payload_keyed_sync_bench.json.  One resident plane marked with dither at 1080p and at 4K; the crop is the half-size
window at an odd origin, read in place (the plane's row stride):

    sigma1_scan            wm_payload_sigma1_scan_u8_dev of the crop: sigma_1 of the windows of all 64 grid phases
    phase_scan             its yardstick: wm_payload_phase_scan_u8_dev of the same build on the same crop (the same kernel
                           with the dither-free epilogue)
    keyed_scan             wm_payload_keyed_scores_dev: every phase and placement; here a lane per placement
    keyed_scan_full_width  the same for the crop (H / 2) x W, which has one placement across at px = 0 and two at the other
                           phases: the entry point puts the lanes over a row's windows there, a wave per placement

with the evaluations (windows x placements over the phases), evaluations per second, and that rate against the FP32 vector
peak.  Also records that the winner of the scores is the crop's true origin.

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


# FP32 vector peak of one MI355X: 157.3 TFLOPS (spec), a fused multiply-add per lane and clock = 78.65e12 vector
# instructions x lanes a second.  An evaluation (dither word -> d -> metric -> |.| -> vote -> add) is EVAL_OPS such
# instructions in k_payload_keyed_scan's inner loop: 93 vector instructions for its 8 windows a pass in the compiler's
# assembly (tools/kregs.sh), loads and scalar loop control left out; the same count is used for the other kernel.
PEAK_FP32_FLOPS = 157.3e12
PEAK_LANE_OPS = PEAK_FP32_FLOPS / 2
EVAL_OPS = 93 / 8
LANE_MAPPINGS = {False: "k_payload_keyed_scan: a wave owns 64 consecutive tx of one (phase, ty), a lane one placement; the table through L1, no LDS",
                 True: "k_payload_keyed_scan_windows: a wave owns one placement, a lane every 64th window of a row"}


def lanes_over_windows(w, nbx):
    """the entry points' choice between their two kernels (csrc/wm_payload.hip, keyed_launch), restated for the record"""
    nx, n_tx = w // 8, nbx - w // 8 + 1
    return nx * ((n_tx + 63) // 64) >= 2 * n_tx * ((nx + 63) // 64)


def keyed_evaluations(h, w, nby, nbx):
    n = 0
    for p in range(64):
        ny, nx = (h - p // 8) // 8, (w - p % 8) // 8
        if ny > 0 and nx > 0:
            n += ny * nx * (nby - ny + 1) * (nbx - nx + 1)
    return n


def bench_keyed_size(ctx, label, warmup, rounds, content):
    P = api.P
    H, W = SIZES[label]
    rng = np.random.default_rng(37)
    nby, nbx = H // 8, W // 8
    plane = make_frames(content, 1, H, W, rng)[0]
    tile_bit = rng.integers(0, 2, nby * nbx).astype(np.uint8)
    U = rng.integers(0, 65536, nby * nbx, dtype=np.uint16)
    stego = ctx.embed_tiles_payload(plane, tile_bit, DELTA, dither=U)[0]      # one resident marked plane
    d_p = ctx.malloc(stego.nbytes); ctx.h2d(d_p, stego)
    d_u = ctx.malloc(U.nbytes); ctx.h2d(d_u, U)
    vp = api._vp
    crops = {"keyed_scan": (H // 4 + 3, W // 4 + 5, H // 2, W // 2), "keyed_scan_full_width": (H // 4 + 3, 0, H // 2, W)}
    bufs, calls = {}, {}
    for name, (y0, x0, h, w) in crops.items():
        pitch = (h // 8) * (w // 8)
        sp = P.keyed_score_pitch(h, w, nby, nbx)
        bufs[name] = (ctx.malloc(64 * pitch * 4), ctx.malloc(64 * sp * 8), pitch, sp)

        def scan(name=name, y0=y0, x0=x0, h=h, w=w):
            ctx._call("wm_payload_sigma1_scan_u8_dev", vp(d_p + y0 * W + x0), vp(bufs[name][0]), 1, h, w, W, H * W)

        def keyed(name=name, h=h, w=w):
            ctx._call("wm_payload_keyed_scores_dev", vp(bufs[name][0]), vp(d_u), vp(bufs[name][1]), h, w, nby, nbx, DELTA)
        scan()                                                               # the scans the keyed variants read
        calls[name] = (scan, keyed)
    y0, x0, h, w = crops["keyed_scan"]
    pitch = bufs["keyed_scan"][2]
    d_votes, d_sums = ctx.malloc(64 * pitch * 4), ctx.malloc(64 * 8)

    def phase_scan():
        ctx._call("wm_payload_phase_scan_u8_dev", vp(d_p + y0 * W + x0), vp(d_votes), vp(d_sums), 1, h, w, W, H * W, DELTA)

    variants = {"sigma1_scan": ("this", calls["keyed_scan"][0]), "phase_scan": ("this", phase_scan),
                "keyed_scan": ("this", calls["keyed_scan"][1]), "keyed_scan_full_width": ("this", calls["keyed_scan_full_width"][1])}
    ms = time_variants({"this": ctx, "parent": ctx}, variants, warmup, rounds, shuffle_seed=41)
    ctx.sync(); ctx.check_status()
    res = {k: summary(v) for k, v in ms.items()}
    out = dict(H=H, W=W, content=content, order="a seeded permutation of the variants per round", variants=res, crops={})
    for name, (cy, cx, ch, cw) in crops.items():
        d_s1, d_sc, pitch, sp = bufs[name]
        raw = np.empty((64, sp), np.int64)
        ctx.d2h(raw, d_sc); ctx.sync()
        win = P.pick_keyed(ctx._keyed_grids(raw, ch, cw, nby, nbx), P.phase_counts(ch, cw))
        (py, px), (ty, tx) = win
        evals = keyed_evaluations(ch, cw, nby, nbx)
        rate = evals / (res[name]["median_ms"] * 1e-3)
        out["crops"][name] = dict(origin=[cy, cx], h=ch, w=cw, lane_mapping=LANE_MAPPINGS[lanes_over_windows(cw, nbx)], evaluations=evals, evaluations_per_s=rate,
                                  lane_ops_per_s_against_fp32_peak=rate * EVAL_OPS / PEAK_LANE_OPS, ops_per_evaluation=EVAL_OPS,
                                  placements_across_at_phase_0=nbx - cw // 8 + 1,
                                  winner_is_the_true_origin=bool((8 * ty - py, 8 * tx - px) == (cy, cx)))
    a, b = res["sigma1_scan"], res["phase_scan"]
    out["sigma1_scan_against_phase_scan"] = dict(
        median_ratio=a["median_ms"] / b["median_ms"], inside_its_spread=bool(b["min_ms"] <= a["median_ms"] <= b["max_ms"]),
        outside_by_ms=float(max(a["median_ms"] - b["max_ms"], b["min_ms"] - a["median_ms"], 0.0)))
    for d in (d_p, d_u, d_votes, d_sums) + tuple(x for b4 in bufs.values() for x in b4[:2]):
        ctx.free(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyed", action="store_true", help="the keyed search of a dithered payload's crop")
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--content", default="natural")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "payload_keyed_sync_bench.json" if a.keyed else "payload_sync_bench.json")
    ctx = api.Context(0)
    res = dict(delta=DELTA, sizes={})
    if a.keyed:
        res.update(fp32_vector_peak_tflops=PEAK_FP32_FLOPS / 1e12)
    for label in a.sizes.split(","):
        res["sizes"][label] = (bench_keyed_size if a.keyed else bench_size)(ctx, label, a.warmup, a.rounds, a.content)
        print(label, {k: round(x["median_ms"], 3) for k, x in res["sizes"][label]["variants"].items()}, flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
