"""bench.py's own options: what a plain run prints, what --dump-outputs writes, and what --full adds.  The CPU tests
hold the dump helper (seeded sample, float32, size cap); the GPU tests run the benchmark at a small shape as a child
process, the way it is run for a pull request."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EXTRA_SECTIONS = ("cpu_baseline", "parity", "cpu_baseline_pool", "cpu_baseline_reference_semantics", "fullframe",
                  "full_extract", "end_to_end")


@pytest.fixture(scope="module")
def bench():
    return importlib.import_module("bench")


def _run_bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup, a.mode) == (False, None, 7, 2, "tile")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_whole_and_sampled(bench, tmp_path):
    """Small arrays are written whole in their own shape; larger ones as DUMP_MAX_ELEMS elements at seeded, sorted,
    distinct flat positions - the same positions on every call - and everything in float32."""
    import torch
    n_big = 3 * (bench.DUMP_MAX_ELEMS // 3 + 4000)
    big = torch.arange(n_big, dtype=torch.int32).reshape(-1, 3)       # each element holds its own flat index
    small = torch.randint(0, 256, (3, 16, 24), dtype=torch.uint8, generator=torch.Generator().manual_seed(7))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (3, 16, 24) and np.array_equal(s, small.numpy().astype(np.float32))
    b = np.load(tmp_path / "a" / "big.npy")
    assert b.dtype == np.float32 and b.shape == (bench.DUMP_MAX_ELEMS,)
    pos = b.astype(np.int64)                       # exact: flat indices stay below 2**24
    assert np.all(np.diff(pos) > 0) and pos[0] >= 0 and pos[-1] < big.numel()
    assert np.array_equal(np.load(tmp_path / "b" / "big.npy"), b)


def test_dump_stays_under_64_mb_at_the_bench_shape(bench):
    """The three outputs of the 4K tile workload (64 frames: stego, sigma_c, watermark estimate) all exceed the
    per-array cap, so the dump is three capped float32 arrays plus their .npy headers."""
    assert 3 * (bench.DUMP_MAX_ELEMS * 4 + 128) <= 64 * 1024 * 1024
    assert 64 * (2160 // 8) * (3840 // 8) * 8 > bench.DUMP_MAX_ELEMS


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run prints the contract line only (no CPU baselines or extra sections), --steps sets the number of timed
    steps, and --dump-outputs holds the last step's outputs: stego bytes, descending per-tile sigma, and a watermark
    estimate that the oracle's extract of those very bytes reproduces."""
    from oracle import wm_oracle as o
    F, H, W, alpha = 4, 256, 384, 0.15
    out = tmp_path / "out"
    j = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", str(F), "--height", str(H), "--width", str(W),
                    "--dump-outputs", str(out)])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j, k
    assert j["steps"] == 3 and j["warmup"] == 1 and j["higher_is_better"] is True and j["unit"] == "frames/s"
    assert j["ms_per_step"] > 0 and abs(j["value"] - F * 1e3 / j["ms_per_step"]) <= 1e-6 * j["value"]
    assert not [k for k in EXTRA_SECTIONS if k in j]
    assert "measured in this run" not in str(j["roofline"].get("traffic_source"))
    assert sorted(os.listdir(out)) == ["sigma_c.npy", "stego.npy", "wm_scrambled.npy"]
    stego, sc, wm = (np.load(out / f"{n}.npy") for n in ("stego", "sigma_c", "wm_scrambled"))
    assert stego.dtype == sc.dtype == wm.dtype == np.float32
    assert stego.shape == (F, H, W) and sc.shape == (F, (H // 8) * (W // 8), 8) and wm.shape == (F, H, W)
    assert np.array_equal(stego, np.round(stego)) and stego.min() >= 0 and stego.max() <= 255
    assert np.all(sc >= 0) and np.all(np.diff(sc, axis=-1) <= 1e-3 * sc[..., :1])
    wys = np.random.default_rng(4321).integers(0, 256, (H, W)).astype(np.float32)      # bench.py's watermark
    Uw, _, Vwt = o.watermark_decompose(wys, 8)
    for f in (0, F - 1):
        ref = o.extract_plane(stego[f], sc[f].reshape(H // 8, W // 8, 8), Uw, Vwt, alpha, 0.6, H, W, 8)
        assert np.corrcoef(wm[f].ravel(), ref.ravel())[0, 1] > 0.999


@pytest.mark.gpu
def test_full_adds_the_cpu_baseline_and_parity():
    """--full (here with --quick: no pool, no live counters) brings back the CPU baseline and the parity object."""
    j = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "2", "--height", "64", "--width", "96",
                    "--cpu-frames", "2", "--full", "--quick"])
    assert j["steps"] == 2 and j["cpu_baseline"]["value"] > 0
    assert j["parity"]["stego_max_lsb"] <= 1 and j["parity"]["sigma_max_rel"] < 1e-4
