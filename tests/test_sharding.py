"""Frame sharding + the watermark broadcast, on CPU with gloo (world_size 2)."""
import importlib
import os
import socket
import sys

import numpy as np
import pytest

from conftest import PKG_NAME

sh = importlib.import_module(PKG_NAME + ".sharding")


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("n", [0, 1, 7, 256, 1000])
def test_frame_ranges_tile_the_batch(world, n):
    rs = sh.all_ranges(world, n)
    assert rs[0][0] == 0 and rs[-1][1] == n
    for (a0, a1), (b0, b1) in zip(rs, rs[1:]):
        assert a1 == b0 and a0 <= a1
    sizes = [b - a for a, b in rs]
    assert max(sizes) - min(sizes) <= 1
    if n == 256 and world == 8:
        assert sizes == [32] * 8                      # BASELINE config 4: 32 frames per rank


def test_frame_range_rejects_bad_rank():
    with pytest.raises(ValueError):
        sh.frame_range(2, 2, 10)
    with pytest.raises(ValueError):
        sh.frame_range(0, 0, 10)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, tmp):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    shm = importlib.import_module(PKG_NAME + ".sharding")
    from oracle import wm_oracle as o
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    H, W, N, alpha = 32, 48, 5, 0.15
    nt = (H // 8) * (W // 8)
    Sw = torch.zeros((nt, 8), dtype=torch.float32)
    U = torch.zeros((nt, 8, 8), dtype=torch.float32); Vt = torch.zeros_like(U)
    if rank == 0:                                          # rank 0 owns the watermark
        wys = np.random.default_rng(4321).integers(0, 256, (H, W)).astype(np.float32)
        u, s, vt = o.watermark_decompose(wys, 8)
        Sw.copy_(torch.from_numpy(s.reshape(nt, 8))); U.copy_(torch.from_numpy(u.reshape(nt, 8, 8)))
        Vt.copy_(torch.from_numpy(vt.reshape(nt, 8, 8)))
    shm.broadcast_watermark([Sw, U, Vt], src=0)
    lo, hi = shm.frame_range(rank, world, N)
    psnrs = []
    for f in range(lo, hi):                                # this rank's frames (CPU stand-in for the kernel)
        host = np.random.default_rng(1234 + f).integers(0, 256, (H, W), dtype=np.uint8)
        wm_svd = (U.numpy().reshape(H // 8, W // 8, 8, 8), Sw.numpy().reshape(H // 8, W // 8, 8),
                  Vt.numpy().reshape(H // 8, W // 8, 8, 8))
        e = o.embed_plane(host.astype(np.float32), None, alpha, 0.6, 8, wm_svd=wm_svd)
        psnrs.append(o.psnr(host, e["stego"]))
    mine = float(np.sum(psnrs))
    allv = shm.gather_scalars(mine)
    np.save(os.path.join(tmp, f"r{rank}.npy"), np.array([lo, hi, float(Sw.sum()), allv.sum()]))
    dist.destroy_process_group()


def test_gloo_world2_broadcast_and_ranges(tmp_path):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = np.load(tmp_path / "r0.npy"); r1 = np.load(tmp_path / "r1.npy")
    assert (r0[0], r0[1], r1[0], r1[1]) == (0, 2, 2, 5)
    assert r0[2] == r1[2] and r0[2] > 0                    # rank 1 received rank 0's singular values
    assert abs(r0[3] - r1[3]) < 1e-9 and r0[3] > 0         # all-gathered report agrees on both ranks


def test_bench_launcher_fails_loudly_without_gpus():
    """No GPU here: `bench.py --gpus 2` must still start its two ranks itself (each says it needs a GPU)
    and hand their failure back as a non-zero status - never a silent single-rank measurement."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--height", "64", "--width", "96",
                        "--frames", "2", "--steps", "1", "--warmup", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, env=env, timeout=300, cwd=root)
    assert r.returncode != 0
    assert r.stdout.strip() == ""
    # the launcher tears the second rank down as soon as the first one fails: one message is guaranteed
    assert r.stderr.count("bench.py needs a GPU") >= 1, r.stderr[-1500:]
    assert "--nproc-per-node=2" in r.stderr or "local_rank" in r.stderr or "ChildFailedError" in r.stderr


def test_live_pmc_section_returns_none_instead_of_raising(monkeypatch):
    """bench.py measures roofline.traffic / roofline.valu with child `rocprofv3 --pmc` passes; whatever goes wrong in a
    child (the child bench exits non-zero; no rocprofv3; a timeout) must come back as None so that the contract line is
    still printed, with the committed profile replayed and labelled."""
    import argparse
    import importlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    # the child's argument parser rejects this --alpha, so the child fails before it opens a device, GPU or not
    a = argparse.Namespace(alpha="not-a-number")
    assert bench.live_pmc_section(a, 2, 64, 96, timeout_s=120) is None
    monkeypatch.setattr(bench.os.path, "exists", lambda p: False if "rocprofv3" in str(p) else os.path.isfile(p) or os.path.isdir(p))
    monkeypatch.setattr("shutil.which", lambda name: None)
    assert bench.live_pmc_section(a, 2, 64, 96, timeout_s=5) is None
