"""What the clip search of a dithered payload's video costs on the device (wmhip.h, "clip resynchronisation"; no torch, no
fallback without a GPU), to profiles/payload_clip_bench.json.

One resident marked clip of 4 frames at 1080p and at 4K, frame interval 1, 4 anchors, 64 candidates for the clip's first frame
(a marked video of 67 frames, 67 dither tables), the true one among them.  The variants are timed interleaved in ONE process
with HIP events on the context's stream, after warm-up rounds that are left out, the order of the variants drawn afresh for
every round (payload_bench.time_variants):

    keyed_best                  wm_payload_keyed_best_dev on the half-size crop at an odd origin: the anchors' scores added in
                                registers, 64 x 64 (score, index) pairs out; here a lane per placement
    keyed_scores_256_calls      the yardstick: the same search without the new kernel - 64 x 4 calls of
                                wm_payload_keyed_scores_dev of the same build, each with the download of its scores (the
                                host would add and compare them; that is not timed)
    keyed_best_full_width       the same for the clip (H / 2) x W, cut in rows only: one placement across at px = 0 and two at
                                the other phases, so a wave per placement with the lanes over a row's windows
    keyed_scores_256_calls_full_width

Also records that the winner of ``best`` is the true (first frame, origin) in every row.

    python tools/payload_clip_bench.py [--out profiles/payload_clip_bench.json]

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
from payload_sync_bench import keyed_evaluations, lanes_over_windows   # noqa: E402

ANCHORS, CANDIDATES, T0 = 4, 64, 29


def bench_size(ctx, label, warmup, rounds, content):
    P = api.P
    H, W = SIZES[label]
    rng = np.random.default_rng(43)
    nby, nbx = H // 8, W // 8
    n_frames = CANDIDATES + ANCHORS - 1
    planes = make_frames(content, ANCHORS, H, W, rng)
    tile_bit = rng.integers(0, 2, nby * nbx).astype(np.uint8)
    U = rng.integers(0, 65536, (n_frames, nby * nbx), dtype=np.uint16)      # a table per frame of the marked video
    stego = ctx.embed_tiles_payload(planes, tile_bit, DELTA, dither=U[T0:T0 + ANCHORS])[0]
    table_of = P.clip_table_of(n_frames, 1, ANCHORS, ANCHORS)
    assert table_of.shape == (CANDIDATES, ANCHORS)
    d_p, d_u, d_of = ctx.malloc(stego.nbytes), ctx.malloc(U.nbytes), ctx.malloc(table_of.nbytes)
    ctx.h2d(d_p, stego); ctx.h2d(d_u, U); ctx.h2d(d_of, table_of)
    d_best = ctx.malloc(CANDIDATES * 64 * 16)
    vp = api._vp
    crops = {"": (H // 4 + 3, W // 4 + 5, H // 2, W // 2), "_full_width": (H // 4 + 3, 0, H // 2, W)}
    variants, bufs, best_of = {}, [d_p, d_u, d_of, d_best], {}
    for tag, (y0, x0, h, w) in crops.items():
        pitch = (h // 8) * (w // 8)
        sp = P.keyed_score_pitch(h, w, nby, nbx)
        d_s1, d_sc = ctx.malloc(ANCHORS * 64 * pitch * 4), ctx.malloc(64 * sp * 8)
        bufs += [d_s1, d_sc]
        scores = np.zeros((64, sp), np.int64)
        ctx._call("wm_payload_sigma1_scan_u8_dev", vp(d_p + y0 * W + x0), vp(d_s1), ANCHORS, h, w, W, H * W)

        def best(d_s1=d_s1, h=h, w=w):
            ctx._call("wm_payload_keyed_best_dev", vp(d_s1), ANCHORS, vp(d_u), n_frames, vp(d_of), CANDIDATES, vp(d_best), h, w, nby,
                      nbx, DELTA)

        def calls(d_s1=d_s1, d_sc=d_sc, h=h, w=w, pitch=pitch, scores=scores):
            for g in range(CANDIDATES):
                for a in range(ANCHORS):
                    ctx._call("wm_payload_keyed_scores_dev", vp(d_s1 + a * 64 * pitch * 4), vp(d_u + int(table_of[g, a]) * nby * nbx * 2),
                              vp(d_sc), h, w, nby, nbx, DELTA)
                    ctx.d2h(scores, d_sc)
        best()
        got = np.zeros((CANDIDATES, 64, 2), np.int64)
        ctx.d2h(got, d_best); ctx.sync()
        best_of[tag] = got
        variants["keyed_best" + tag] = ("this", best)
        variants["keyed_scores_256_calls" + tag] = ("this", calls)
    ms = time_variants({"this": ctx, "parent": ctx}, variants, warmup, rounds, shuffle_seed=47)
    ctx.sync(); ctx.check_status()
    res = {k: summary(v) for k, v in ms.items()}
    out = dict(H=H, W=W, content=content, anchors=ANCHORS, candidates=CANDIDATES, tables=n_frames, first_frame=T0,
               order="a seeded permutation of the variants per round", variants=res, clips={})
    for tag, (cy, cx, ch, cw) in crops.items():
        g, p, i = P.pick_clip(best_of[tag], P.phase_counts(ch, cw), np.full(CANDIDATES, ANCHORS))
        n_tx = nbx - (cw - p % 8) // 8 + 1
        origin = (8 * (i // n_tx) - p // 8, 8 * (i % n_tx) - p % 8)
        evals = keyed_evaluations(ch, cw, nby, nbx) * ANCHORS * CANDIDATES
        a, b = res["keyed_best" + tag], res["keyed_scores_256_calls" + tag]
        out["clips"]["keyed_best" + tag] = dict(
            origin=[cy, cx], h=ch, w=cw, lanes_over_windows=bool(lanes_over_windows(cw, nbx)), evaluations=evals,
            evaluations_per_s=evals / (a["median_ms"] * 1e-3), placements_across_at_phase_0=nbx - cw // 8 + 1,
            score_bytes_a_call_of_the_yardstick=int(64 * P.keyed_score_pitch(ch, cw, nby, nbx) * 8), bytes_out=CANDIDATES * 64 * 16,
            median_ratio_to_the_256_calls=a["median_ms"] / b["median_ms"],
            winner_is_the_true_first_frame_and_origin=bool((g, origin) == (T0, (cy, cx))))
    for d in bufs:
        ctx.free(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "payload_clip_bench.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--content", default="natural")
    a = ap.parse_args()
    ctx = api.Context(0)
    res = dict(delta=DELTA, sizes={})
    for label in a.sizes.split(","):
        res["sizes"][label] = bench_size(ctx, label, a.warmup, a.rounds, a.content)
        print(label, {k: round(x["median_ms"], 3) for k, x in res["sizes"][label]["variants"].items()},
              {k: x["winner_is_the_true_first_frame_and_origin"] for k, x in res["sizes"][label]["clips"].items()}, flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
