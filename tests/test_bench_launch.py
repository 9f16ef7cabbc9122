"""bench.py's rank plumbing (CPU): ``--gpus N`` without a torchrun environment starts N ranks
itself and the line reports the ranks that ran; ``--gpus`` disagreeing with WORLD_SIZE is an
error; the row split of BASELINE.md §2's multi-GPU synthetic.  The GPU legs themselves run in
tests/test_bench_gpu.py (2 gloo ranks sharing the one card) and in the driver's N-GPU runs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    return env


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_n_spawns_n_ranks(n):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--launch-check"],
                       capture_output=True, text=True, timeout=240, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 alone prints
    line = lines[0]
    assert line["n_gpus"] == n and line["ranks_seen"] == n
    assert sorted(x["rank"] for x in line["ranks"]) == list(range(n))
    assert sorted(x["local_rank"] for x in line["ranks"]) == list(range(n))
    assert len({x["pid"] for x in line["ranks"]}) == n


def test_gpus_mismatch_with_world_size_fails():
    env = _env()
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True,
                       text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 2 and "WORLD_SIZE=1" in r.stderr
    assert not [x for x in r.stdout.splitlines() if x.startswith("{")]


def test_dump_outputs_is_exact_bounded_and_repeatable(tmp_path):
    """``--dump-outputs``: small tensors whole and exact in float32 / float64, large ones as the
    same seeded sample on every call, the whole dump within the byte budget."""
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(3)
    packed = torch.randint(-2 ** 31, 2 ** 31 - 1, (300, 40), generator=g, dtype=torch.int64).to(torch.int32)
    tensors = {"m.weight_packed": packed,
               "m.weight_scale": torch.rand(300, 7, generator=g).to(torch.bfloat16),
               "m.weight_shape": torch.tensor([300, 320]),
               "n.weight_packed": packed[:2]}
    budget = 40_000  # m.weight_packed (96 kB as float64) must be sampled, the others fit
    wrote = bench.dump_outputs(tensors, str(tmp_path / "a"), budget=budget)
    assert bench.dump_outputs(tensors, str(tmp_path / "b"), budget=budget) == wrote <= budget
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in tensors}
    assert sum(a.nbytes for a in got.values()) == wrote
    for n in tensors:
        assert np.array_equal(got[n], np.load(tmp_path / "b" / (n + ".npy"))), n
    assert got["m.weight_scale"].dtype == np.float32 and got["m.weight_scale"].shape == (300, 7)
    assert np.array_equal(got["m.weight_scale"], tensors["m.weight_scale"].float().numpy())
    assert got["m.weight_shape"].dtype == np.float64 and got["m.weight_shape"].tolist() == [300, 320]
    assert np.array_equal(got["n.weight_packed"], packed[:2].double().numpy())
    s = got["m.weight_packed"]
    assert s.dtype == np.float64 and s.ndim == 1 and 1000 < s.size < packed.numel()
    assert np.isin(s, packed.double().numpy()).all()
    other = dict(tensors, **{"m.weight_packed": packed.flip(0).contiguous()})
    bench.dump_outputs(other, str(tmp_path / "c"), budget=budget)  # same indices, other values
    assert not np.array_equal(s, np.load(tmp_path / "c" / "m.weight_packed.npy"))
    assert bench.DUMP_BUDGET <= 60_000_000


@pytest.mark.parametrize("world", [1, 2, 3, 4, 5, 7, 8, 16])
def test_row_blocks_cover_the_weight(world):
    import bench
    blocks, blk = bench.row_blocks(bench.ROWS, world)
    assert blk % 8 == 0 and len(blocks) == world
    assert blocks[0][0] == 0 and blocks[-1][1] == bench.ROWS
    for (a0, a1), (b0, _) in zip(blocks, blocks[1:]):
        assert a1 == b0
    for r0, r1 in blocks:
        assert 0 <= r1 - r0 <= blk and r0 % 8 == 0
