"""What rotation resynchronisation of the blind payload costs on the device (no torch, no fallback without a GPU).

A resident plane, the variants timed interleaved in ONE process with HIP events on the context's stream, after warm-up rounds
that are left out, the order of the variants drawn afresh for every round (payload_bench.time_variants), at 1080p and at 4K:

    rotate_<size>_<n>    wm_rotate_planes_u8_dev - k_rotate_planes - of n candidates of one plane, n = 1 and n = one chunk of the
                         search (the candidates whose restored planes fill Context.ROTATE_PLANE_BYTES), the destination's rows
                         16-byte multiples apart as the search has them
    metric_<size>_<n>    wm_payload_metric_tiles_dither_u8_dev on the same n restored planes under one shared table
    scores_<size>_<n>    wm_payload_angle_scores_dev on those metrics, n = 1 and n = one chunk, as the search calls it

and from them the cost per candidate and of the whole +-10 degree search (coarse + 17 fine candidates), beside the wall-clock time
of Context.payload_locate_angle itself (upload, both stages, the downloads; the median of 3 calls after one) on a marked frame
rotated by 3 degrees, with the angle it finds.  Also records that
candidate 0 of the chunk equals the NumPy restatement (tests/rotate_refs.py) byte for byte on a 256-row band.

    python tools/payload_rotate_bench.py [--out profiles/payload_rotate_bench.json]

Development aid; bench.py is the contract benchmark."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mask_bench import api, make_frames                     # noqa: E402  (puts tests/ on the path)
from payload_bench import SIZES, summary, time_variants     # noqa: E402
import rotate_refs as rf                                    # noqa: E402

P, R = api.P, api.R
DELTA = 32.0
MAX_ANGLE = 10.0
ATTACK_DEG = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "payload_rotate_bench.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--content", default="natural")
    a = ap.parse_args()
    ctx = api.Context(0)
    vp = api._vp
    rng = np.random.default_rng(53)
    K = np.ascontiguousarray(R.rotate_weights())
    d_K = ctx.malloc(K.nbytes); ctx.h2d(d_K, K)
    variants, cases, bufs, walls = {}, {}, [d_K], {}
    for label, (H, W) in SIZES.items():
        H, W = H // 8 * 8, W // 8 * 8                                       # (1080 rows: 135 tiles down)
        frame = make_frames(a.content, 1, H, W, rng)[0]
        pitch = (W + 15) // 16 * 16
        n_tiles = (H // 8) * (W // 8)
        coarse, den = P.angle_candidates(H, W, MAX_ANGLE)
        n_stage = len(coarse)
        chunk = max(1, min(ctx.ROTATE_PLANE_BYTES // (H * pitch), n_stage))
        cs = R.angle_candidates_cs(coarse / den)
        table = rng.integers(0, 65536, n_tiles, dtype=np.uint16)
        d_src, d_dst, d_cs, d_u = ctx.malloc(H * W), ctx.malloc(chunk * H * pitch), ctx.malloc(cs.nbytes), ctx.malloc(table.nbytes)
        d_m, d_s, d_n = ctx.malloc(chunk * n_tiles * 4), ctx.malloc(8 * n_stage), ctx.malloc(4 * n_stage)
        bufs += [d_src, d_dst, d_cs, d_u, d_m, d_s, d_n]
        ctx.h2d(d_src, frame); ctx.h2d(d_cs, cs); ctx.h2d(d_u, table)
        mid = n_stage // 2 - chunk // 2                                     # the chunk around the zero candidate

        def rotate(n, d_src=d_src, d_dst=d_dst, d_cs=d_cs, H=H, W=W, pitch=pitch, mid=mid):
            ctx._call("wm_rotate_planes_u8_dev", vp(d_src), vp(d_dst), 1, H, W, W, H * W, H, W, pitch, H * pitch, vp(d_cs + 8 * mid), n, vp(d_K))

        def metric(n, d_dst=d_dst, d_u=d_u, d_m=d_m, H=H, W=W, pitch=pitch):
            ctx._call("wm_payload_metric_tiles_dither_u8_dev", vp(d_dst), vp(d_u), vp(d_m), n, H, W, pitch, H * pitch, 0, DELTA)

        def scores(n, d_m=d_m, d_cs=d_cs, d_s=d_s, d_n=d_n, H=H, W=W, mid=mid):
            ctx._call("wm_payload_angle_scores_dev", vp(d_m), vp(d_cs + 8 * mid), n, vp(d_s), vp(d_n), None, H, W, H, W)
        rotate(chunk); metric(chunk); scores(chunk)                         # buffers grown, code loaded
        ctx.sync(); ctx.check_status()
        band = 256
        got = np.empty((band, pitch), np.uint8)
        ctx.d2h(got, d_dst); ctx.sync()
        C0, S0 = (int(x) for x in cs[mid])
        same = bool(np.array_equal(got[:, :W], _band_ref(frame, H, W, C0, S0, band)))
        cases[label] = dict(shape=[H, W], dst_row_stride=pitch, n_tiles=n_tiles, coarse_candidates=n_stage, fine_candidates=17,
                            chunk=chunk, chunk_starts_at_degrees=math.degrees(float(coarse[mid] / den)),
                            band_of_candidate_equals_the_restatement=same)
        for n in (1, chunk):
            variants[f"rotate_{label}_{n}"] = ("this", lambda n=n, f=rotate: f(n))
            variants[f"metric_{label}_{n}"] = ("this", lambda n=n, f=metric: f(n))
            variants[f"scores_{label}_{n}"] = ("this", lambda n=n, f=scores: f(n))
        # the search itself, wall clock, on a frame that carries a payload (random tile bits under the same table) and was
        # rotated on the device by the rule's own filter at -ATTACK_DEG (the restatement's float attacker would take minutes at
        # 4K on the host): the search should come back with +ATTACK_DEG
        stego = ctx.embed_tiles_payload(frame, rng.integers(0, 2, n_tiles, dtype=np.uint8), DELTA, dither=table)[0]
        att = ctx.rotate_planes(stego, H, W, R.angle_candidates_cs([math.radians(-ATTACK_DEG)]))[0]
        ts = []
        for i in range(4):
            t0 = time.perf_counter()
            found = ctx.payload_locate_angle(att, H, W, MAX_ANGLE, DELTA, dither=table)
            ts.append((time.perf_counter() - t0) * 1e3)
        walls[label] = dict(median_ms=float(np.median(ts[1:])), all_ms=ts, first_call_ms=ts[0],
                            attacked_by_degrees=ATTACK_DEG, found_degrees=None if found is None else math.degrees(found[0]),
                            fine_step_degrees=math.degrees(1.0 / (P.ANGLE_FINE * den)))
    ms = time_variants({"this": ctx, "parent": ctx}, variants, a.warmup, a.rounds, shuffle_seed=59)
    ctx.sync(); ctx.check_status()
    res = {k: summary(v) for k, v in ms.items()}
    derived = {}
    for label, c in cases.items():
        ch, n_stage = c["chunk"], c["coarse_candidates"]
        total = n_stage + c["fine_candidates"]
        per = {k: res[f"{k}_{label}_{ch}"]["median_ms"] * 1e3 / ch for k in ("rotate", "metric", "scores")}
        derived[label] = dict(us_per_candidate=per, us_single_call={k: res[f"{k}_{label}_1"]["median_ms"] * 1e3 for k in ("rotate", "metric", "scores")},
                              whole_search_ms={k: per[k] * total / 1e3 for k in per}, candidates=total,
                              whole_search_device_ms=sum(per.values()) * total / 1e3, locate_angle_wall=walls[label])
        print(label, json.dumps(derived[label]), flush=True)
    for b in bufs:
        ctx.free(b)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(dict(delta=DELTA, max_angle=MAX_ANGLE, content=a.content, order="a seeded permutation of the variants per round",
                       timed="each entry point between two events on the context's stream; medians of the rounds",
                       cases=cases, derived=derived, variants=res), f, indent=1)


def _band_ref(frame, H, W, C, S, band):
    """rows 0 .. band - 1 of tests/rotate_refs.rotate_ref, computed on those rows alone (bounded memory at 4K)"""
    x0, fx, y0, fy = rf.coords_ref(H, W, H, W, C, S, ys=np.arange(band))
    K = rf.weights_ref().astype(np.int64)
    px = frame.reshape(-1).astype(np.int64)
    acc = np.zeros((band, W), np.int64)
    for j in range(4):
        yj = np.clip(y0 - 1 + j, 0, H - 1) * W
        row = sum(K[fx, i] * np.take(px, yj + np.clip(x0 - 1 + i, 0, W - 1)) for i in range(4))
        acc += K[fy, j] * ((row + 128) >> 8)
    return np.clip((acc + (1 << 19)) >> 20, 0, 255).astype(np.uint8)


if __name__ == "__main__":
    main()
