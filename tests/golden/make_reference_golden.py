"""Generate the fixtures under tests/golden/reference/ by running the REFERENCE PROGRAM.

REFERENCE-GENERATED (unlike make_golden.py's): the reference's own embed -> extract -> detect, loaded from
oracle/_ref/ (oracle/ref_build.py) over the stand-in cv2 (tests/cv2_standin.py), and kept is what the program read and
wrote: cover.png, logo.png, the stego, meta.npz and the watermark image per case, and one results.json (psnr, ssim,
detect flag and score, nonce, password, arguments, returned file names, SHA-256 of the reference source).  Runs on
the CPU where oracle/_ref/ exists.  What this pins and what it does not: DESIGN.md section 2.

    python tests/golden/make_reference_golden.py                 # rewrite the fixtures
    python tests/golden/make_reference_golden.py --sensitivity   # measure the enhanced-image bar (tests/ref_program.py)
"""
import hashlib
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
import enhance_oracle as eo  # noqa: E402
import ref_program as rp  # noqa: E402

OUT = os.path.join(HERE, "reference")

# cover (H, W), logo (h, w); stego_arg / wm_arg: the out_path handed to embed / extract (the program renames a path
# that does not end in .png)
CASES = {
    # H < W: Uw is (H, L), Vwt (L, W); logo rows shrink 50 -> 40, columns enlarge 30 -> 56 (mixed: the linear variant)
    "gray_40x56_mixed": dict(cover=(40, 56), logo=(50, 30), color=False, alpha=0.1, kfrac=0.6),
    # H > W: Uw[:L,:L], Wm_full[:hh,:ww] placement; both axes shrink (box filter); the cover is a gray PNG
    "gray_56x40_shrink": dict(cover=(56, 40), logo=(80, 64), color=False, alpha=0.1, kfrac=0.6, gray_file=True),
    # per-channel flow, one shared permutation, 9-part HMAC; integer enlargement x2
    "color_32x48_x2": dict(cover=(32, 48), logo=(16, 24), color=True, alpha=0.1, kfrac=0.6),
    # L = 6 < 8: K = max(8, ...) exceeds L, the slices run past the end
    "gray_6x10_tiny": dict(cover=(6, 10), logo=(12, 20), color=False, alpha=0.1, kfrac=0.6),
    # int(kfrac * L) truncates: 0.33 * 40 = 13.2 -> 13
    "gray_40x56_k033": dict(cover=(40, 56), logo=(50, 30), color=False, alpha=0.03, kfrac=0.33),
    # ... and where rounding would differ from truncation: 0.34 * 40 = 13.6 -> 13
    "gray_40x56_k034": dict(cover=(40, 56), logo=(50, 30), color=False, alpha=0.03, kfrac=0.34),
    # K = L
    "gray_40x56_k100": dict(cover=(40, 56), logo=(50, 30), color=False, alpha=0.03, kfrac=1.0),
    # clip-only path; _stego.png / _wm.png renaming
    "gray_40x56_nonorm_rename": dict(cover=(40, 56), logo=(50, 30), color=False, alpha=0.1, kfrac=0.6, normalize=False,
                                     stego_arg="out.jpg", wm_arg="mark"),
}


def seed_of(name: str) -> int:
    return int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)


def make_cover(name: str, H: int, W: int) -> np.ndarray:
    """Smooth field + noise, full rank, RGB."""
    rng = np.random.default_rng(seed_of(name))
    yy, xx = np.mgrid[0:H, 0:W]
    chans = []
    for c in range(3):
        f = 120 + 55 * np.sin(xx / (5.0 + c) + c) * np.cos(yy / (4.0 + 2 * c)) + 20 * (yy / max(H - 1, 1)) - 15 * (xx / max(W - 1, 1))
        chans.append(f + rng.normal(0, 14, (H, W)))
    return np.clip(np.stack(chans, -1), 0, 255).astype(np.uint8)


def make_logo(name: str, h: int, w: int) -> np.ndarray:
    """A high-contrast synthetic logo, RGB: frame, bar, disc, rules."""
    rng = np.random.default_rng(seed_of(name) ^ 0x5A5A)
    img = np.full((h, w, 3), 235, np.uint8)
    img[:max(h // 10, 1)] = img[-max(h // 10, 1):] = (20, 20, 90)
    img[:, :max(w // 10, 1)] = img[:, -max(w // 10, 1):] = (20, 20, 90)
    img[h // 3:h // 3 + max(h // 6, 1), w // 5:4 * w // 5] = (200, 30, 30)
    yy, xx = np.mgrid[0:h, 0:w]
    img[(yy - 0.68 * h) ** 2 / (0.2 * h) ** 2 + (xx - 0.5 * w) ** 2 / (0.25 * w) ** 2 < 1] = (10, 140, 60)
    img[::5, ::3] = 0
    return np.clip(img.astype(int) + rng.integers(-6, 7, img.shape), 0, 255).astype(np.uint8)


def run_case(prog, name: str, c: dict, out_dir: str) -> dict:
    os.makedirs(out_dir, exist_ok=True)
    H, W = c["cover"]
    cover = make_cover(name, H, W)
    logo = make_logo(name, *c["logo"])
    if c.get("gray_file"):
        Image.fromarray(cover[..., 1]).save(os.path.join(out_dir, "cover.png"))
    else:
        Image.fromarray(cover).save(os.path.join(out_dir, "cover.png"))
    Image.fromarray(logo).save(os.path.join(out_dir, "logo.png"))
    password = "pw-" + name
    nonce = hashlib.sha256(("nonce-" + name).encode()).digest()[:8]
    normalize = c.get("normalize", True)
    p = lambda f: os.path.join(out_dir, f)
    prog.log.clear()
    stego_path, meta_path, ps, ss = prog.embed(p("cover.png"), p("logo.png"), p(c.get("stego_arg", "stego.png")), p("meta.npz"),
                                               alpha=c["alpha"], color=c["color"], password=password, kfrac=c["kfrac"],
                                               nonce=nonce)
    wm_path = prog.extract(stego_path, meta_path, p(c.get("wm_arg", "wm.png")), password, normalize)
    ok, score = prog.detect(stego_path, meta_path)
    assert not prog.log.errors, prog.log.errors
    return dict(cover=[H, W], logo=list(c["logo"]), color=c["color"], alpha=c["alpha"], kfrac=c["kfrac"], normalize=normalize,
                password=password, nonce=nonce.hex(), stego_arg=c.get("stego_arg", "stego.png"), wm_arg=c.get("wm_arg", "wm.png"),
                stego_file=os.path.basename(stego_path), meta_file=os.path.basename(meta_path), wm_file=os.path.basename(wm_path),
                psnr=float(ps), ssim=float(ss), detect=bool(ok), score=float(score))


def main():
    prog = rp.load()
    info = rp.build_info()
    res = dict(source_sha256=info["sha256"], cases={})
    for name, c in CASES.items():
        res["cases"][name] = run_case(prog, name, c, os.path.join(OUT, name))
        d = os.path.join(OUT, name)
        print(name, {f: os.path.getsize(os.path.join(d, f)) for f in sorted(os.listdir(d))}, res["cases"][name]["score"])
    with open(os.path.join(OUT, "results.json"), "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


def sensitivity(seeds: int = 8, share: float = 5e-2):
    """The oracle chain's own sensitivity: enhance(x) against enhance(x +- 1 LSB on `share` of the pixels), x the
    oracle's un-enhanced estimate on every committed fixture case.  Prints the worst values (tests/ref_program.py)."""
    from oracle import wm_oracle as o
    worst_mean, worst_share = 0.0, 0.0
    for name, c in rp.results()["cases"].items():
        meta = rp.load_meta(rp.case_path(name, c["meta_file"]))
        x = o.extract_arrays(rp.read_png(rp.case_path(name, c["stego_file"])), meta, c["password"], c["normalize"], None)
        base = eo.enhance(np.ascontiguousarray(x))
        for s in range(seeds):
            rng = np.random.default_rng(1000 * s + 7)
            hit = rng.random(x.shape) < share
            step = np.where(rng.random(x.shape) < 0.5, -1, 1)
            y = np.clip(x.astype(int) + hit * step, 0, 255).astype(np.uint8)
            m, sh = rp.enhanced_distance(base, eo.enhance(np.ascontiguousarray(y)))
            worst_mean, worst_share = max(worst_mean, m), max(worst_share, sh)
            print(f"{name} seed {s}: mean abs {m:.4f}, share off by > {rp.ENHANCED_OFF_BY}: {sh:.4f}")
    print(f"worst: mean abs {worst_mean:.4f}, share {worst_share:.4f}")


if __name__ == "__main__":
    sensitivity() if "--sensitivity" in sys.argv else main()
