"""What the frame search of a dithered payload's video costs on the device (wmhip.h, "frame resynchronisation"; no torch, no
fallback without a GPU), to profiles/payload_frames_bench.json.

64 resident marked frames at 1080p and at 4K, frame interval 1, a dither table per frame: 64 clip frames against 64 tables,
uncropped and on a half-size crop at an odd origin, at the true grid phase and place.  The variants are timed interleaved in
ONE process with HIP events on the context's stream, after warm-up rounds that are left out, the order of the variants drawn
afresh for every round (payload_bench.time_variants):

    frame_scores[_crop]         wm_payload_frame_scores_dev alone on the resident sigma pass output (window stride 8)
    match_frames[_crop]         the sigma pass of the 64 views and the scores, as Context.payload_match_frames runs them
    keyed_best_calls[_crop]     the yardstick: the same 64 x 64 matrix from the same build without the new kernel - one call
                                of wm_payload_keyed_best_dev per clip frame with one anchor and 64 candidates, which searches
                                all 64 phases and every placement again for every frame.  Where --yard-calls-4k-crop is below
                                64 only that many frames' calls are timed at the 4K crop and the figure for 64 is their
                                median times 64 / calls, marked `extrapolated`.

Also records that the winner of every row of the matrix, and of every timed call of the yardstick, is the true table.

    python tools/payload_frames_bench.py [--out profiles/payload_frames_bench.json]

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
from payload_sync_bench import keyed_evaluations   # noqa: E402

FRAMES = TABLES = 64
EMBED_BATCH = 8
KEYED_SCAN_EVALUATIONS_PER_S = (3.4e12, 4.3e12)             # k_payload_keyed_scan, profiles/payload_keyed_sync_bench.json


def bench_size(ctx, label, warmup, rounds, content, yard_calls_4k_crop):
    P = api.P
    H, W = SIZES[label]
    rng = np.random.default_rng(53)
    nby, nbx = H // 8, W // 8
    tile_bit = rng.integers(0, 2, nby * nbx).astype(np.uint8)
    U = rng.integers(0, 65536, (TABLES, nby * nbx), dtype=np.uint16)        # a table per frame of the marked video
    stego = np.empty((FRAMES, H, W), np.uint8)
    for b0 in range(0, FRAMES, EMBED_BATCH):
        planes = make_frames(content, EMBED_BATCH, H, W, rng)
        stego[b0:b0 + EMBED_BATCH] = ctx.embed_tiles_payload(planes, tile_bit, DELTA, dither=U[b0:b0 + EMBED_BATCH])[0]
    every_table = np.arange(TABLES, dtype=np.int32)[:, None]
    d_p, d_u, d_of = ctx.malloc(stego.nbytes), ctx.malloc(U.nbytes), ctx.malloc(every_table.nbytes)
    ctx.h2d(d_p, stego); ctx.h2d(d_u, U); ctx.h2d(d_of, every_table)
    vp = api._vp
    crops = {"": (0, 0, H, W), "_crop": (H // 4 + 3, W // 4 + 5, H // 2, W // 2)}
    variants, bufs, rows = {}, [d_p, d_u, d_of], {}
    for tag, (y0, x0, h, w) in crops.items():
        py, px = (-y0) % 8, (-x0) % 8
        ny, nx = (h - py) // 8, (w - px) // 8
        ty, tx = (y0 + py) // 8, (x0 + px) // 8
        view = np.ascontiguousarray(stego[:, y0 + py:y0 + py + 8 * ny, x0 + px:x0 + px + 8 * nx])
        n_yard = yard_calls_4k_crop if (label == "4k" and tag) else FRAMES
        pitch = (h // 8) * (w // 8)
        d_view, d_sig, d_sc = ctx.malloc(view.nbytes), ctx.malloc(FRAMES * ny * nx * 32), ctx.malloc(FRAMES * TABLES * 8)
        d_s1, d_best = ctx.malloc(n_yard * 64 * pitch * 4), ctx.malloc(n_yard * TABLES * 64 * 16)
        bufs += [d_view, d_sig, d_sc, d_s1, d_best]
        ctx.h2d(d_view, view)
        ctx._call("wm_payload_sigma1_scan_u8_dev", vp(d_p + y0 * W + x0), vp(d_s1), n_yard, h, w, W, H * W)

        def sigma(d_view=d_view, d_sig=d_sig, ny=ny, nx=nx):
            ctx._call("wm_sigma_tiles_u8_dev", vp(d_view), vp(d_sig), FRAMES, 8 * ny, 8 * nx, 8 * nx, 64 * ny * nx)

        def scores(d_sig=d_sig, d_sc=d_sc, ny=ny, nx=nx, ty=ty, tx=tx):
            ctx._call("wm_payload_frame_scores_dev", vp(d_sig), 8, 8 * ny * nx, FRAMES, vp(d_u), TABLES, vp(d_sc), ny, nx, nby, nbx,
                      ty, tx, DELTA)

        def match(sigma=sigma, scores=scores):
            sigma(); scores()

        def calls(d_s1=d_s1, d_best=d_best, h=h, w=w, pitch=pitch, n_yard=n_yard):
            for f in range(n_yard):
                ctx._call("wm_payload_keyed_best_dev", vp(d_s1 + f * 64 * pitch * 4), 1, vp(d_u), TABLES, vp(d_of), TABLES,
                          vp(d_best + f * TABLES * 64 * 16), h, w, nby, nbx, DELTA)
        match(); calls()
        got = np.zeros((FRAMES, TABLES), np.int64)
        best = np.zeros((n_yard, TABLES, 64, 2), np.int64)
        ctx.d2h(got, d_sc); ctx.d2h(best, d_best); ctx.sync()
        counts = P.phase_counts(h, w)
        yard_true = all(P.pick_clip(best[f], counts, np.ones(TABLES))[:2] == (f, 8 * py + px) for f in range(n_yard))
        rows[tag] = dict(origin=[y0, x0], h=h, w=w, phase=[py, px], place=[ty, tx], windows=ny * nx,
                         evaluations=FRAMES * TABLES * ny * nx, yardstick_calls_timed=n_yard,
                         yardstick_evaluations_a_call=keyed_evaluations(h, w, nby, nbx) * TABLES,
                         winner_of_every_row_is_the_true_table=bool(np.array_equal(np.argmax(got, axis=1), np.arange(FRAMES))),
                         every_frame_names_its_table=bool(np.array_equal(P.pick_frames(got, ny * nx), np.arange(FRAMES))),
                         yardstick_winner_is_the_true_table_phase=bool(yard_true))
        variants["frame_scores" + tag] = ("this", scores)
        variants["match_frames" + tag] = ("this", match)
        variants["keyed_best_calls" + tag] = ("this", calls)
    ms = time_variants({"this": ctx, "parent": ctx}, variants, warmup, rounds, shuffle_seed=59)
    ctx.sync(); ctx.check_status()
    res = {k: summary(v) for k, v in ms.items()}
    for tag, row in rows.items():
        a, m, y = res["frame_scores" + tag], res["match_frames" + tag], res["keyed_best_calls" + tag]
        scale = FRAMES / row["yardstick_calls_timed"]
        row.update(evaluations_per_s=row["evaluations"] / (a["median_ms"] * 1e-3),
                   keyed_scan_evaluations_per_s_for_comparison=list(KEYED_SCAN_EVALUATIONS_PER_S),
                   yardstick_ms_for_64_frames=y["median_ms"] * scale, yardstick_extrapolated=bool(scale != 1.0),
                   yardstick_min_max_ms_for_64_frames=[y["min_ms"] * scale, y["max_ms"] * scale],
                   match_frames_ratio_to_the_yardstick=m["median_ms"] / (y["median_ms"] * scale),
                   beats_the_yardstick_outside_its_spread=bool(m["max_ms"] < y["min_ms"] * scale))
    for d in bufs:
        ctx.free(d)
    return dict(H=H, W=W, content=content, frames=FRAMES, tables=TABLES, order="a seeded permutation of the variants per round",
                variants=res, clips={"uncropped" if not t else "half_size_crop": r for t, r in rows.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "payload_frames_bench.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--content", default="natural")
    ap.add_argument("--yard-calls-4k-crop", type=int, default=FRAMES,
                    help="clip frames whose yardstick calls are timed at the 4K crop (each searches 64 tables over every phase and place)")
    a = ap.parse_args()
    ctx = api.Context(0)
    res = dict(delta=DELTA, library=os.path.basename(api.LIB_PATH), sizes={})
    for label in a.sizes.split(","):
        res["sizes"][label] = bench_size(ctx, label, a.warmup, a.rounds, a.content, max(1, min(FRAMES, a.yard_calls_4k_crop)))
        print(label, {k: round(x["median_ms"], 3) for k, x in res["sizes"][label]["variants"].items()},
              {k: (x["winner_of_every_row_is_the_true_table"], x["yardstick_winner_is_the_true_table_phase"])
               for k, x in res["sizes"][label]["clips"].items()}, flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
