"""What the blind payload's channel code costs on the device (no torch, no fallback without a GPU).

wm_payload_decode_k7_dev on one codeword of n_info = 1 024, 16 384 and 64 794 frame bits (the last fills a 4K plane: 2 (n_info +
6) = 129 600 coded bits = its tiles), timed with HIP events on the context's stream: medians of 12 rounds after 3 warm-up
rounds, with min and max.  Beside each: the NumPy restatement (tests/payload_code_refs.py) on the host for the same vector,
and wm_payload_soft_tiles_u8_dev on ONE resident plane with at least as many tiles as coded bits, in the same build and the same
rounds - what a decode costs without the code.  One wave walks the steps one after another, so the time per step is the figure
that matters; it is recorded in ns.  Nothing in the parent commit decodes a code: no time here is a threshold.

    python tools/payload_code_bench.py [--out profiles/payload_code_bench.json]

Development aid; bench.py is the contract benchmark."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mask_bench import api, make_frames                  # noqa: E402
from payload_bench import csr, summary                   # noqa: E402

DELTA = 16.0
# n_info -> (H, W) of the plane beside it: the smallest near-square tile grid that holds the coded bits; 4K for the last
CASES = {1024: (368, 360), 16384: (1456, 1448), 64794: (2160, 3840)}


def vector(P, n_info, rng):
    """a noisy soft vector of a seeded frame, quantised: 4 tiles a coded bit, 6 % of the tiles voting wrong at full weight"""
    coded = P.encode_k7(rng.integers(0, 2, n_info).astype(np.uint8)).astype(np.int64)
    votes = np.where(rng.random((4, coded.size)) < 0.06, -1.0, 1.0) * rng.uniform(0.3, 1.0, (4, coded.size))
    return P.quantise_soft(((1 - 2 * coded) * votes).sum(0))


def bench_case(ctx, P, cr, n_info, warmup, rounds, host_rounds):
    rng = np.random.default_rng(n_info)
    n_steps = n_info + P.K7_TAIL
    L = vector(P, n_info, rng)
    H, W = CASES[n_info]
    nt = (H // 8) * (W // 8)
    assert nt >= L.size
    plane = make_frames("natural", 1, H, W, rng)
    _, order, offs = csr(nt, L.size, rng)
    d = dict(L=ctx.malloc(L.nbytes), info=ctx.malloc(n_info), fm=ctx.malloc(4), D=ctx.malloc(8 * n_steps), plane=ctx.malloc(plane.nbytes),
             order=ctx.malloc(order.nbytes), offs=ctx.malloc(offs.nbytes), soft=ctx.malloc(8 * L.size))
    for k, a in (("L", L), ("plane", plane), ("order", order), ("offs", offs)):
        ctx.h2d(d[k], a)
    vp = api._vp
    variants = {
        "decode_k7": lambda: ctx._call("wm_payload_decode_k7_dev", vp(d["L"]), n_info, 1, L.size, vp(d["info"]), vp(d["fm"]), vp(d["D"])),
        "decode_k7_own_words": lambda: ctx._call("wm_payload_decode_k7_dev", vp(d["L"]), n_info, 1, L.size, vp(d["info"]), None, None),
        "payload_soft_one_plane": lambda: ctx._call("wm_payload_soft_tiles_u8_dev", vp(d["plane"]), vp(d["order"]), vp(d["offs"]),
                                                    int(L.size), vp(d["soft"]), 1, H, W, W, H * W, DELTA),
    }
    ms = {k: [] for k in variants}
    for r in range(warmup + rounds):
        for slot, fn in enumerate(variants.values()):
            ctx.event_record(2 * slot); fn(); ctx.event_record(2 * slot + 1)
        ctx.sync()
        for slot, k in enumerate(variants):
            if r >= warmup:
                ms[k].append(ctx.event_elapsed_ms(2 * slot, 2 * slot + 1))
    ctx.check_status()
    info = np.empty(n_info, np.uint8); fm = np.empty(1, np.int32); D = np.empty(n_steps, np.uint64)
    ctx._call("wm_payload_decode_k7_dev", vp(d["L"]), n_info, 1, L.size, vp(d["info"]), vp(d["fm"]), vp(d["D"]))
    ctx.d2h(info, d["info"]); ctx.d2h(fm, d["fm"]); ctx.d2h(D, d["D"]); ctx.sync()
    host_s = []
    for _ in range(host_rounds):
        t = time.perf_counter()
        want = cr.viterbi_ref(L, n_info)
        host_s.append(time.perf_counter() - t)
    for p in d.values():
        ctx.free(p)
    res = {k: summary(v) for k, v in ms.items()}
    return dict(n_info=n_info, n_steps=n_steps, n_coded=int(L.size), plane=dict(H=H, W=W, n_tiles=nt), variants=res,
                decode_ns_per_step=1e6 * res["decode_k7"]["median_ms"] / n_steps,
                numpy_restatement=dict(median_ms=1e3 * float(np.median(host_s)), min_ms=1e3 * min(host_s), max_ms=1e3 * max(host_s),
                                       rounds=host_rounds),
                equal_to_restatement=bool(np.array_equal(info, want[0]) and int(fm[0]) == want[1] and np.array_equal(D, want[2])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "payload_code_bench.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=12)
    a = ap.parse_args()
    import payload_code_refs as cr
    P = cr.P
    ctx = api.Context(0)
    res = dict(delta=DELTA, timing="HIP events on the context's stream, the three variants one after another in every round",
               cases={})
    for n_info in CASES:
        r = bench_case(ctx, P, cr, n_info, a.warmup, a.rounds, host_rounds=1 if n_info > 20000 else 3)
        res["cases"][str(n_info)] = r
        print(n_info, {k: round(v["median_ms"], 4) for k, v in r["variants"].items()}, f"{r['decode_ns_per_step']:.1f} ns/step",
              f"numpy {r['numpy_restatement']['median_ms']:.0f} ms", "equal" if r["equal_to_restatement"] else "DIFFERS", flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    if not all(r["equal_to_restatement"] for r in res["cases"].values()):
        sys.exit("the device decode differs from the restatement")


if __name__ == "__main__":
    main()
