"""bench.py's multi-rank legs on the GPU: ``--gpus 2`` starts two ranks itself; on the one-GPU
box they share cuda:0 over gloo (QZ_BENCH_BACKEND=gloo -- RCCL refuses two ranks on one
device), which runs the same code as the driver's N-GPU RCCL runs: barriers, max-over-ranks
timing, the row-sharded synthetic with its all-gather (checked bit for bit against one
whole-weight quantize) and the sharded whole-model plan with gather_state."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


FULL_ONLY = ("per_launch", "steady_state", "cpu_baseline", "parity_check", "pcie_inclusive",
             "row_sharded_synthetic_11008x4096", "strong_scaling_qwen3_4b_sharded",
             "north_star_synthetic_11008x4096", "awq_kernels", "awq_oneshot_qwen3_4b", "other_configs")


@pytest.fixture(scope="module")
def plain_run(cuda, tmp_path_factory):
    """One plain ``--gpus 1 --dump-outputs`` run shared by the tests below: (process result, seconds
    from start to exit, dump directory)."""
    out = tmp_path_factory.mktemp("plain") / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    return r, time.perf_counter() - t0, out


@pytest.mark.gpu
def test_bench_plain_run_is_headline_only_and_dumps_outputs(plain_run):
    """A plain run: K timed steps, the result line without any ``--full`` leg, at most 30 s of the
    whole run (start to exit) outside its steps, and with ``--dump-outputs`` the last step's
    compressed tensors as float32 / float64 .npy files within 64 MB (three per targeted linear:
    packed codes, scales, shape)."""
    import numpy as np
    r, wall, out = plain_run
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = lines[0]
    assert line["unit"] == "params/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["metric"].startswith("params quantized/sec") and line["n_gpus"] == 1
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    assert wall - (line["steps"] + line["warmup"]) * line["ms_per_step"] * 1e-3 < 30.0, (wall, line["ms_per_step"])
    params = line["config"]["params_per_step"]
    assert line["value"] == pytest.approx(params / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]
    files = sorted(out.glob("*.npy"))
    assert len(files) == 3 * 252
    total = 0
    for f in files:
        a = np.load(f)
        total += a.nbytes
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f.name
        if f.name.endswith("weight_packed.npy"):
            assert a.dtype == np.float64 and (a == np.rint(a)).all() and -2.0 ** 31 <= a.min() <= a.max() < 2.0 ** 31, \
                f.name
            assert np.unique(a).size > 100, f.name  # packed codes of random weights, not a cleared buffer
        elif f.name.endswith("weight_scale.npy"):
            assert a.dtype == np.float32 and (a > 0).all(), f.name
    assert sum(f.stat().st_size for f in files) <= 64_000_000 and total > 32_000_000
    q = np.load(out / "model.layers.0.self_attn.q_proj.weight_shape.npy")
    assert q.tolist() == [4096, 2560]


@pytest.mark.gpu
def test_bench_two_ranks_gloo(cuda, plain_run, tmp_path):
    """Two ranks with ``--full`` and ``--dump-outputs``: rank 0 alone writes the dump and every
    rank keeps the same phase names (they are all-reduced); rank 0's weights are seeded as the
    one-rank run's, so its dump equals ``plain_run``'s file for file -- another process, another
    number of steps, the same inputs and outputs."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["QZ_BENCH_BACKEND"] = "gloo"
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
                        "--warmup", "1", "--full", "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = lines[0]
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2
    rs = line["row_sharded_synthetic_11008x4096"]
    assert rs["gathered_equals_single_gpu"] is True
    assert rs["kernel_only"]["params_per_s"] > 0 and rs["end_to_end"]["params_per_s"] > 0
    st = line["strong_scaling_qwen3_4b_sharded"]
    assert st["units_total"] == 252 and st["end_to_end"]["tensors_on_every_rank"] == 2 * 252
    assert "dump_outputs" in line["phase_seconds_max_rank"]
    ref = sorted(plain_run[2].glob("*.npy"))
    got = sorted(out.glob("*.npy"))
    assert [f.name for f in got] == [f.name for f in ref] and len(got) == 3 * 252
    differ = [f.name for f, g in zip(ref, got) if not np.array_equal(np.load(f), np.load(g))]
    assert not differ, differ[:5]
