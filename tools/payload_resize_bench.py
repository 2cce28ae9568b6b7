"""What resize resynchronisation of the blind payload costs on the device (no torch, no fallback without a GPU).

Resident planes, the variants timed interleaved in ONE process with HIP events on the context's stream, after warm-up
rounds that are left out, the order of the variants drawn afresh for every round (payload_bench.time_variants):

    resample_<dir>_<n>   wm_resample_planes_u8_dev - k_resample_h, then k_resample_v - of n planes, dir = up (1080p -> 4K) or
                         down (4K -> 1080p), the destination's rows 16-byte multiples apart as the extract has them
    soft_<dir>_<n>       the yardstick, what the decode behind it costs: wm_payload_soft_tiles_u8_dev (n_bits = 1024) on the
                         same restored planes

with the bytes the two passes have to move (source + intermediate written + intermediate read + destination), the
achieved bytes/s and that rate against the 8 TB/s HBM roof.  An event pair brackets the entry point, so a figure is both
kernels and the gap between them; for a kernel on its own run the tool under a kernel trace in a run of its own.  Also
records that plane 0 of every result equals the NumPy restatement (tests/resample_refs.py) byte for byte.

    python tools/payload_resize_bench.py [--out profiles/payload_resize_bench.json]

Development aid; bench.py is the contract benchmark."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mask_bench import api, make_frames                     # noqa: E402  (puts tests/ on the path)
from payload_bench import SIZES, csr, summary, time_variants   # noqa: E402
import resample_refs as rr                                  # noqa: E402

HBM_ROOF = 8.0e12
DELTA = 32.0
N_BITS = 1024
DIRECTIONS = {"up": ("1080p", "4k"), "down": ("4k", "1080p")}


def restated(plane, H, W, rows=128):
    """tests/resample_refs.resample_ref of one plane, a block of rows at a time (bounded memory at 4K)"""
    h, w = plane.shape
    fx, wx = rr.taps_ref(w, W)
    mid = np.concatenate([rr.round_acc(rr.pass_acc(plane[r:r + rows], fx, wx)) for r in range(0, h, rows)])
    fy, wy = rr.taps_ref(h, H)
    midT = np.ascontiguousarray(mid.T)
    return np.concatenate([rr.round_acc(rr.pass_acc(midT[c:c + rows], fy, wy)) for c in range(0, W, rows)]).T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "payload_resize_bench.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--planes", default="1,64")
    ap.add_argument("--content", default="natural")
    a = ap.parse_args()
    counts = [int(x) for x in a.planes.split(",")]
    n_max = max(counts)
    ctx = api.Context(0)
    vp = api._vp
    rng = np.random.default_rng(43)
    variants, cases, bufs = {}, {}, []
    for d, (src_label, dst_label) in DIRECTIONS.items():
        (h, w), (H, W) = SIZES[src_label], SIZES[dst_label]
        pitch = (W + 15) // 16 * 16
        frames = make_frames(a.content, min(n_max, 4), h, w, rng)
        d_src, d_dst = ctx.malloc(n_max * h * w), ctx.malloc(n_max * H * pitch)
        for p in range(n_max):
            ctx.h2d(d_src + p * h * w, frames[p % len(frames)])
        _, order, offs = csr((H // 8) * (W // 8), N_BITS, rng)
        d_order, d_offs, d_soft = ctx.malloc(order.nbytes), ctx.malloc(offs.nbytes), ctx.malloc(N_BITS * 8)
        ctx.h2d(d_order, order); ctx.h2d(d_offs, offs)
        bufs += [d_src, d_dst, d_order, d_offs, d_soft]
        ctx.resample_planes_dev(d_src, d_dst, n_max, h, w, w, h * w, H, W, pitch, H * pitch)    # tables cached, buffers grown
        ctx.sync()
        got = np.empty((H, pitch), np.uint8)
        ctx.d2h(got, d_dst); ctx.sync()
        cases[d] = dict(src=[h, w], dst=[H, W], dst_row_stride=pitch, taps=[int(rr.taps_ref(w, W)[1].shape[1]), int(rr.taps_ref(h, H)[1].shape[1])],
                        plane_0_equals_the_restatement=bool(np.array_equal(got[:, :W], restated(frames[0], H, W))))
        for n in counts:
            def resample(n=n, d_src=d_src, d_dst=d_dst, h=h, w=w, H=H, W=W, pitch=pitch):
                ctx.resample_planes_dev(d_src, d_dst, n, h, w, w, h * w, H, W, pitch, H * pitch)

            def soft(n=n, d_dst=d_dst, d_order=d_order, d_offs=d_offs, d_soft=d_soft, H=H, W=W, pitch=pitch):
                ctx._call("wm_payload_soft_tiles_u8_dev", vp(d_dst), vp(d_order), vp(d_offs), N_BITS, vp(d_soft), n, H, W, pitch,
                          H * pitch, DELTA)
            variants[f"resample_{d}_{n}"] = ("this", resample)
            variants[f"soft_{d}_{n}"] = ("this", soft)
    ms = time_variants({"this": ctx, "parent": ctx}, variants, a.warmup, a.rounds, shuffle_seed=47)
    ctx.sync(); ctx.check_status()
    res = {k: summary(v) for k, v in ms.items()}
    for d, c in cases.items():
        (h, w), (H, W) = c["src"], c["dst"]
        for n in counts:
            r = res[f"resample_{d}_{n}"]
            moved = n * (h * w + 2 * h * W + H * W)
            rate = moved / (r["median_ms"] * 1e-3)
            r.update(planes=n, bytes_moved=moved, bytes_per_s=rate, fraction_of_hbm_roof=rate / HBM_ROOF,
                     us_per_plane=r["median_ms"] * 1e3 / n,
                     against_the_decode_behind_it=r["median_ms"] / res[f"soft_{d}_{n}"]["median_ms"])
        print(d, {k: round(v["median_ms"], 4) for k, v in res.items() if f"_{d}_" in k}, flush=True)
    for b in bufs:
        ctx.free(b)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(dict(delta=DELTA, n_bits=N_BITS, hbm_roof_bytes_per_s=HBM_ROOF, content=a.content,
                       order="a seeded permutation of the variants per round",
                       timed="wm_resample_planes_u8_dev between two events: k_resample_h, k_resample_v and the gap between them",
                       bytes_model="planes x (source + intermediate written + intermediate read + destination)",
                       cases=cases, variants=res), f, indent=1)


if __name__ == "__main__":
    main()
