"""What the blind payload costs on the device (no torch, no fallback without a GPU).

64 resident 4K planes (and 1080p), the variants timed interleaved in ONE process, HIP events on the context's stream,
after warm-up rounds that are left out:

    sigma_tiles (K2, the yardstick)   payload_metric (K2 + m, 4 bytes a tile)   payload_soft (metric + per-bit sums)
    embed_masked (the yardstick)      payload_sigma_w (K2 + target)            embed_payload

With --parent-lib the two yardsticks run from ANOTHER build of libwmhip.so (the parent commit's) in the same rounds, and
so do its payload_sigma_w and payload_metric; --sigma-pass-out then records each sigma pass of this build against the
parent's own round-to-round spread.
The expectations to confirm or correct: payload_metric <= sigma_tiles, payload_soft - payload_metric = a few us,
embed_payload = embed_masked.  payload_soft is timed at n_bits = 16 (each wave sums n_planes * n_tiles / 16 values: the
reduce at its least parallel), at 1024 and at n_tiles.

With --dither the keyed-dither forms are timed beside them (payload_metric_dither, payload_sigma_w_dither,
payload_soft_dither_*, embed_payload_dither: a per-plane table, 2 more bytes a tile), the embeds write to a buffer of their
own so that every decode variant reads the same payload stego whatever ran before it, and the order of the variants is
drawn afresh for every round (a variant's place in the round moves its time by more than the variants differ).  Each
dithered row is then recorded against payload_metric_parent's own min-max spread; no threshold is set.

Also records the device figures at the test shapes (tests/payload_refs.py): worst |m| deficit against the restatement,
worst |soft - ref| / count, share of stego pixels differing from the restatement.

    python tools/payload_bench.py [--parent-lib /path/to/parent/libwmhip.so] [--out profiles/payload_bench.json]
    python tools/payload_bench.py --dither --parent-lib /path/to/parent/libwmhip.so --out profiles/payload_dither_bench.json

Development aid; bench.py is the contract benchmark."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mask_bench import LibContext, api, load_build, make_frames, sigma_pass_record   # noqa: E402

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}
MASK = (8.0, 64.0)
DELTA = 16.0


def csr(n_tiles, n_bits, rng):
    tbi = (rng.permutation(n_tiles) % n_bits).astype(np.int32)
    order = np.argsort(tbi, kind="stable").astype(np.int32)
    offs = np.concatenate([[0], np.cumsum(np.bincount(tbi, minlength=n_bits))]).astype(np.int32)
    return tbi, order, offs


def time_variants(ctxs, variants, warmup, rounds, shuffle_seed=None):
    """variants: name -> (ctx key, callable).  Returns name -> list of ms, one per round, interleaved.
    Two builds are two contexts with a stream each, and launches on two streams overlap on the device: with a parent build
    every variant starts on an idle device (both contexts synchronised first), so that no variant is timed against whatever
    the other build happens to run beside it, and a variant and its `_parent` twin, which stand next to each other, swap
    places every other round, so that neither always follows the same neighbour.  With shuffle_seed the order of all
    variants is a fresh seeded permutation every round instead."""
    out = {k: [] for k in variants}
    two_streams = ctxs["parent"] is not ctxs["this"]
    names = list(variants)
    shuffle = None if shuffle_seed is None else np.random.default_rng(shuffle_seed)
    for r in range(warmup + rounds):
        order = list(range(len(names)))
        if shuffle is not None:
            order = [int(i) for i in shuffle.permutation(len(names))]
        elif r % 2:
            for i in range(len(names) - 1):
                if names[i] + "_parent" == names[i + 1] or names[i] == names[i + 1] + "_parent":
                    order[i], order[i + 1] = order[i + 1], order[i]
        for slot in order:
            ck, fn = variants[names[slot]]
            c = ctxs[ck]
            if two_streams:
                ctxs["this"].sync(); ctxs["parent"].sync()
            c.event_record(2 * slot); fn(); c.event_record(2 * slot + 1)
        for slot, (name, (ck, fn)) in enumerate(variants.items()):
            ms = ctxs[ck].event_elapsed_ms(2 * slot, 2 * slot + 1)
            if r >= warmup:
                out[name].append(ms)
    return out


def summary(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), rounds=len(a))


def bench_size(ctx, parent, label, F, warmup, rounds, content, sigma_pass_out=None, dither=False):
    H, W = SIZES[label]
    rng = np.random.default_rng(17)
    nt = (H // 8) * (W // 8)
    host = make_frames(content, F, H, W, rng)
    plane = (F, H, W, W, H * W)
    ctxs = {"this": ctx, "parent": parent or ctx}
    bufs = {}
    for k, c in ctxs.items():
        if k == "parent" and parent is None:
            bufs[k] = bufs["this"]; continue
        b = dict(host=c.malloc(host.nbytes), stego=c.malloc(host.nbytes), sigma=c.malloc(F * nt * 32), sc=c.malloc(F * nt * 32),
                 sw=c.malloc(nt * 32))
        c.h2d(b["host"], host)
        c.h2d(b["sw"], rng.uniform(0, 2000, (nt, 8)).astype(np.float32))
        bufs[k] = b
    t = bufs["this"]
    tile_bit = rng.integers(0, 2, nt).astype(np.uint8)
    for k, c in ctxs.items():
        if k == "this" or parent is not None:
            b = bufs[k]
            b["metric"] = c.malloc(F * nt * 4); b["eff"] = c.malloc(F * nt * 32); b["bit"] = c.malloc(nt)
            c.h2d(b["bit"], tile_bit)
    maps = {}
    for nb in (16, 1024, nt):
        _, order, offs = csr(nt, nb, rng)
        d_o, d_f, d_s = ctx.malloc(order.nbytes), ctx.malloc(offs.nbytes), ctx.malloc(nb * 8)
        ctx.h2d(d_o, order); ctx.h2d(d_f, offs)
        maps[nb] = (d_o, d_f, d_s)
    # the stego the decode variants read: the payload embed of the frames
    ctx._call("wm_embed_tiles_payload_u8_dev", t["host"], t["bit"], t["stego"], t["sc"], None, *plane, DELTA)
    ctx.sync(); ctx.check_status()
    p = bufs["parent"]
    pc = ctxs["parent"]
    if parent is not None:                                  # the parent's K2 reads the same payload stego
        st = np.empty_like(host); ctx.d2h(st, t["stego"])
        p["pstego"] = pc.malloc(st.nbytes); pc.h2d(p["pstego"], st)
    else:
        p = dict(p, pstego=t["stego"])
    variants = {
        "sigma_tiles_parent": ("parent", lambda: pc.sigma_tiles_u8_dev(p["pstego"], p["sigma"], *plane)),
        "sigma_tiles": ("this", lambda: ctx.sigma_tiles_u8_dev(t["stego"], t["sigma"], *plane)),
        "payload_metric": ("this", lambda: ctx._call("wm_payload_metric_tiles_u8_dev", t["stego"], t["metric"], *plane, DELTA)),
        "payload_metric_parent": ("parent", lambda: pc._call("wm_payload_metric_tiles_u8_dev", p["pstego"], p["metric"], *plane, DELTA)),
        "embed_masked_parent": ("parent", lambda: pc.embed_tiles_masked_u8_dev(p["host"], p["sw"], p["stego"], p["sc"], None, *plane, 0, 0.12, 8, *MASK)),
        "embed_masked": ("this", lambda: ctx.embed_tiles_masked_u8_dev(t["host"], t["sw"], t["stego"], t["sc"], None, *plane, 0, 0.12, 8, *MASK)),
        "payload_sigma_w": ("this", lambda: ctx._call("wm_payload_sigma_w_tiles_u8_dev", t["host"], t["bit"], t["eff"], *plane, DELTA)),
        "payload_sigma_w_parent": ("parent", lambda: pc._call("wm_payload_sigma_w_tiles_u8_dev", p["host"], p["bit"], p["eff"], *plane, DELTA)),
        "embed_payload": ("this", lambda: ctx._call("wm_embed_tiles_payload_u8_dev", t["host"], t["bit"], t["stego"], t["sc"], None, *plane, DELTA)),
    }
    for nb, (d_o, d_f, d_s) in maps.items():
        variants[f"payload_soft_{'ntiles' if nb == nt else nb}_bits"] = (
            "this", lambda d_o=d_o, d_f=d_f, d_s=d_s, nb=nb: ctx._call("wm_payload_soft_tiles_u8_dev", t["stego"], d_o, d_f, nb, d_s, *plane, DELTA))
    if dither:
        # the embeds of every build write beside the stego the decode variants read; the dithered forms take a table row per plane
        t["out"] = ctx.malloc(host.nbytes)
        if parent is not None:
            p["out"] = pc.malloc(host.nbytes)
        words = rng.integers(0, 65536, (F, nt), dtype=np.uint16)
        t["words"] = ctx.malloc(words.nbytes); ctx.h2d(t["words"], words)
        po = p["out"] if parent is not None else t["out"]
        variants.update({
            "embed_masked_parent": ("parent", lambda: pc.embed_tiles_masked_u8_dev(p["host"], p["sw"], po, p["sc"], None, *plane, 0, 0.12, 8, *MASK)),
            "embed_masked": ("this", lambda: ctx.embed_tiles_masked_u8_dev(t["host"], t["sw"], t["out"], t["sc"], None, *plane, 0, 0.12, 8, *MASK)),
            "embed_payload": ("this", lambda: ctx._call("wm_embed_tiles_payload_u8_dev", t["host"], t["bit"], t["out"], t["sc"], None, *plane, DELTA)),
            "payload_metric_dither": ("this", lambda: ctx._call("wm_payload_metric_tiles_dither_u8_dev", t["stego"], t["words"], t["metric"], *plane, nt, DELTA)),
            "payload_sigma_w_dither": ("this", lambda: ctx._call("wm_payload_sigma_w_tiles_dither_u8_dev", t["host"], t["bit"], t["words"], t["eff"], *plane, nt, DELTA)),
            "embed_payload_dither": ("this", lambda: ctx._call("wm_embed_tiles_payload_dither_u8_dev", t["host"], t["bit"], t["words"], t["out"], t["sc"], None, *plane, nt, DELTA)),
        })
        for nb, (d_o, d_f, d_s) in maps.items():
            variants[f"payload_soft_dither_{'ntiles' if nb == nt else nb}_bits"] = (
                "this", lambda d_o=d_o, d_f=d_f, d_s=d_s, nb=nb: ctx._call("wm_payload_soft_tiles_dither_u8_dev", t["stego"], t["words"], d_o, d_f, nb, d_s, *plane, nt, DELTA))
    # without --dither the embeds rewrite stego: embed_payload stays last so that the decode variants of the next round read a payload stego
    ms = time_variants(ctxs, variants, warmup, rounds, shuffle_seed=29 if dither else None)
    ctx.sync(); ctx.check_status(); pc.sync(); pc.check_status()
    res = {k: summary(v) for k, v in ms.items()}
    if parent is not None and sigma_pass_out:
        sigma_pass_record(sigma_pass_out, {f"payload_bench.{v}_{label}": (1e3 * np.asarray(ms[v]), 1e3 * np.asarray(ms[v + "_parent"]))
                                           for v in ("sigma_tiles", "payload_sigma_w", "payload_metric")})
    for k, c in ctxs.items():
        if k == "parent" and parent is None:
            continue
        for d in (p if k == "parent" else bufs[k]).values():
            c.free(d)
    for d3 in maps.values():
        for d in d3:
            ctx.free(d)
    out = dict(frames=F, H=H, W=W, n_tiles=nt, content=content, variants=res)
    if dither:
        out["order"] = "a seeded permutation of the variants per round"
        yard = res["payload_metric_parent" if parent is not None else "payload_metric"]
        out["against_parent_metric"] = {
            k: dict(median_minus_parent_median_ms=v["median_ms"] - yard["median_ms"],
                    inside_parent_spread=bool(yard["min_ms"] <= v["median_ms"] <= yard["max_ms"]),
                    outside_by_ms=float(max(v["median_ms"] - yard["max_ms"], yard["min_ms"] - v["median_ms"], 0.0)))
            for k, v in res.items() if k in ("payload_metric", "payload_metric_dither")}
        for pair in (("payload_sigma_w_dither", "payload_sigma_w"), ("embed_payload_dither", "embed_payload")) + tuple(
                (k, k.replace("_dither", "")) for k in res if k.startswith("payload_soft_dither")):
            a, b = res[pair[0]], res[pair[1]]
            out["against_parent_metric"][pair[0]] = dict(
                against=pair[1], median_minus_its_median_ms=a["median_ms"] - b["median_ms"],
                inside_its_spread=bool(b["min_ms"] <= a["median_ms"] <= b["max_ms"]),
                outside_by_ms=float(max(a["median_ms"] - b["max_ms"], b["min_ms"] - a["median_ms"], 0.0)))
    return out


def device_figures(ctx):
    import payload_refs as pr
    out = {}
    for name, Y in pr.all_hosts():
        H, W = Y.shape
        nt = (H // 8) * (W // 8)
        for n_bits in (nt, 16):
            bits = pr.seeded_bits(n_bits, 0)
            tbi, order, offs = pr.simple_map(nt, n_bits, seed=7)
            tb = bits[tbi].reshape(H // 8, W // 8)
            st, sc, _ = ctx.embed_tiles_payload(Y, tb, DELTA)
            soft = ctx.payload_soft(st, order, offs, n_bits, DELTA)
            ref = pr.embed_ref(Y, tb, DELTA)
            sign = np.where(tb != 0, -1, 1)
            m_dev, m_ref = sign * ctx.payload_metric(st, DELTA), sign * pr.metric_ref(ref["stego"], DELTA)
            ref_soft = pr.soft_ref(pr.metric_ref(st, DELTA).reshape(1, -1), order, offs)
            d = st.astype(int) - ref["stego"].astype(int)
            out[f"{name}_{n_bits}_bits"] = dict(
                bit_errors=int(np.sum((soft < 0) != (bits != 0))), min_margin_device=float(m_dev.min()), min_margin_restatement=float(m_ref.min()),
                worst_margin_deficit=float(np.max(m_ref - m_dev)), worst_soft_err_per_count=float(np.max(np.abs(soft - ref_soft) / np.diff(offs))),
                soft_bar_per_count=2 * 1e-4 * 2040 / DELTA, share_pixels_differing=float(np.mean(d != 0)), max_lsb=int(np.abs(d).max()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "payload_bench.json"))
    ap.add_argument("--sigma-pass-out", help="with --parent-lib: add sigma_tiles / payload_sigma_w / payload_metric of both builds "
                    "to this JSON (mask_bench.sigma_pass_record)")
    ap.add_argument("--dither", action="store_true", help="add the keyed-dither rows; the order of the variants is drawn per round")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--sizes", default="4k,1080p")
    ap.add_argument("--content", default="natural")
    a = ap.parse_args()
    ctx = api.Context(0)
    parent = LibContext(load_build(a.parent_lib)) if a.parent_lib else None
    res = dict(parent_lib=bool(a.parent_lib), delta=DELTA, sizes={}, figures={} if a.dither else device_figures(ctx))
    for label in a.sizes.split(","):
        res["sizes"][label] = bench_size(ctx, parent, label, a.frames, a.warmup, a.rounds, a.content, a.sigma_pass_out, a.dither)
        v = res["sizes"][label]["variants"]
        print(label, {k: round(x["median_ms"], 3) for k, x in v.items()}, flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["figures"], indent=1))
    ctx.close()
    if parent is not None:
        parent.close()


if __name__ == "__main__":
    main()
