#!/usr/bin/env python3
"""Executed instructions per class of the V-free Jacobi stream (tools/gen_jacobi_asm.py, interpreted by
tools/emu_jacobi_asm.py) on the 40 noise waves tests/test_jacobi_lq_prelude.py counts on, priced with the instruction
costs measured on the part (profiles/r02_embed_variants.md section 2, middle of each range): the stream with the scaled
rotations against the one whose every pair takes the unscaled rotation (gen_jacobi_asm.build(scaled=False)).

    python tools/jacobi_stream_cost.py
    python tools/jacobi_stream_cost.py --swapfree     # the in-place norm update of the swap-free scaled rotation against
                                                      # the body that takes max / min of the two norms ahead of the branch
    python tools/jacobi_stream_cost.py --byte-norms        # the prelude's row norms from the raw bytes
    python tools/jacobi_stream_cost.py --rcp               # 1 / c^2 from one v_rcp_f32
    python tools/jacobi_stream_cost.py --sigma-only        # the sigma-only stream whose columns stay scaled to the end
(each against the stream with that keyword of gen_jacobi_asm.build off, everything else as in the stream that hands out
B; --rcp prices the piece on that stream, where it is not committed - it is part of the sigma-only stream)
"""
import sys

import numpy as np

import emu_jacobi_asm as emu

# cycles per wave-instruction: v_mul / v_fma and their like 2.1-2.6, v_pk_mul_f32 4.3, v_pk_fma_f32 4.8-5.9, v_rsq_f32 8
# v_dot4_u32_u8 and v_cvt_f32_u32 (one class, "dot4"): 1.77 / 1.73 ns per wave-instruction at three waves per SIMD
# against 1.19 for v_mul_f32 and 1.9-2.4 for the packed classes in the same run (profiles/r08_ubench_dot4.log) - 1.5 v_mul
PRICE = {"valu": 2.35, "v_pk_mul_f32": 4.3, "v_pk_fma_f32": 5.3, "trans": 8.0, "dot4": 3.5}
CONFIGS = {"embed": (1e-7, 1e-12, 4, 3), "sigma": (1e-2, 1e-8, 3, 2)}       # what csrc/wmhip.hip / wm_tile_pass.h pass to the stream


def noise_waves():
    return np.random.default_rng(2025).integers(0, 256, (40, 64, 8, 8), dtype=np.uint8)


def count(cfg, scaled, waves=None, swapfree=True, **kw):
    """-> (executed instructions per wave by class, mean sweeps per wave, {sweep: (rotations, of them in the swap branch)})"""
    waves = noise_waves() if waves is None else waves
    tot, sweeps = {}, []
    for t in waves:
        st = {}
        _, _, more, k = emu.run(t, *cfg, stats=st, scaled=scaled, swapfree=swapfree, **kw)
        assert not np.any(more)
        sweeps.append(k)
        for key, val in st.items():
            if not isinstance(val, list):
                tot[key] = tot.get(key, 0) + val
    n = len(waves)
    per_class = {k: tot.get(k, 0) / n for k in ("valu", "v_pk_mul_f32", "v_pk_fma_f32", "trans")}
    if tot.get("dot4"):
        per_class["dot4"] = tot["dot4"] / n
    per_sweep = {k[1]: (tot[k] / n, tot.get(("swap", k[1]), 0) / n) for k in sorted(x for x in tot if isinstance(x, tuple) and x[0] == "rot")}
    return per_class, float(np.mean(sweeps)), per_sweep


def cycles(per_class):
    return sum(PRICE[k] * v for k, v in per_class.items())


def swapfree_rotations(per_sweep, cfg):
    """scaled rotations per wave that took the swap-free path: those of the untested sweeps (the first min_sweeps - 1)
    that did not enter the swap branch"""
    return sum(r - s for k, (r, s) in per_sweep.items() if k < cfg[2] - 1)


def price_swapfree():
    for name, cfg in CONFIGS.items():
        old, _, _ = count(cfg, True, swapfree=False)
        new, sw, ps = count(cfg, True)
        n = swapfree_rotations(ps, cfg)
        print(f"{name:5s} sweeps per wave {sw:.3f}, swap-free scaled rotations per wave {n:.1f} of {sum(r for k, (r, s) in ps.items() if k < cfg[2] - 1):.0f}")
        for tag, pc in (("max/min ahead", old), ("in place     ", new)):
            print(f"      {tag}  " + "  ".join(f"{k} {v:.1f}" for k, v in pc.items()) + f"  priced {cycles(pc):.0f} cycles")
        print(f"{name:5s} scalar VALU {new['valu'] - old['valu']:+.1f} per wave, priced cycles {cycles(new) - cycles(old):+.0f} "
              f"({100 * (cycles(new) / cycles(old) - 1):+.2f} %)")


# piece -> (configurations it touches, keywords of the stream without it, keywords of the stream with it)
PIECES = {"--byte-norms": (("embed", "sigma"), dict(byte_norms=False), dict()),
          "--rcp": (("embed", "sigma"), dict(), dict(rcp=True)),
          "--sigma-only": (("sigma",), dict(), dict(sigma_only=True))}


def price_piece(flag):
    names, off, on = PIECES[flag]
    for name in names:
        old, sw0, _ = count(CONFIGS[name], True, **off)
        new, sw1, _ = count(CONFIGS[name], True, **on)
        print(f"{name:5s} {flag[2:]}: sweeps per wave {sw0:.3f} -> {sw1:.3f}")
        for tag, pc in (("off", old), ("on ", new)):
            print(f"      {tag}  " + "  ".join(f"{k} {v:.1f}" for k, v in pc.items()) + f"  priced {cycles(pc):.0f} cycles")
        print(f"{name:5s} VALU instructions {sum(new.values()) - sum(old.values()):+.1f} per wave, priced cycles "
              f"{cycles(new) - cycles(old):+.0f} ({100 * (cycles(new) / cycles(old) - 1):+.2f} %)")


if __name__ == "__main__":
    if "--swapfree" in sys.argv[1:]:
        price_swapfree()
        sys.exit(0)
    if any(f in PIECES for f in sys.argv[1:]):
        for f in sys.argv[1:]:
            price_piece(f)
        sys.exit(0)
    for name, cfg in CONFIGS.items():
        cyc = {}
        for scaled in (False, True):
            pc, sw, ps = count(cfg, scaled)
            cyc[scaled] = cycles(pc)
            print(f"{name:5s} {'scaled  ' if scaled else 'unscaled'}  sweeps per wave {sw:.3f}  per wave: "
                  + "  ".join(f"{k} {v:.0f}" for k, v in pc.items()) + f"  priced {cyc[scaled]:.0f} cycles")
            print("      rotations per sweep (of them in the swap branch): "
                  + "  ".join(f"{k + 1}: {r:.1f} ({s:.1f})" for k, (r, s) in ps.items()))
        print(f"{name:5s} priced cycles {100 * (cyc[True] / cyc[False] - 1):+.2f} %")
