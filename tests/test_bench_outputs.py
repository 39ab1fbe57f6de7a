"""bench.py's plain run and --dump-outputs: the arrays of the last timed step are written as float32
.npy files (whole, or a fixed seeded sample inside the byte budget), the same from run to run; a plain
run reports the headline figure only, --full is what adds the other objects."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import torch
    import bench
    a = torch.arange(6000, dtype=torch.float32).reshape(10, 20, 30) / 7
    W = types.SimpleNamespace(out=a)
    bench.dump_outputs(W, str(tmp_path / "whole"))
    got = np.load(tmp_path / "whole" / "out.npy")
    assert got.dtype == np.float32 and np.array_equal(got, a.numpy())
    # over the budget: a sample at fixed indices, in index order, identical from call to call
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 1000)
    bench.dump_outputs(W, str(tmp_path / "s1"))
    bench.dump_outputs(W, str(tmp_path / "s2"))
    s1, s2 = np.load(tmp_path / "s1" / "out.npy"), np.load(tmp_path / "s2" / "out.npy")
    assert s1.dtype == np.float32 and s1.shape == (1000,) and np.array_equal(s1, s2)
    flat = a.numpy().reshape(-1)
    assert np.all(np.diff(s1) >= 0) and np.all(np.isin(s1, flat))


def test_dump_outputs_u16_levels_share_the_budget(tmp_path, monkeypatch):
    import torch
    import bench
    # the u16 workloads hold their arrays as int16 on the device: values >= 32768 must come out positive
    lv = [torch.from_numpy((np.arange(n, dtype=np.uint16) * 13).view(np.int16)) for n in (9000, 500)]
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 2000)
    bench.dump_outputs(types.SimpleNamespace(outs=lv), str(tmp_path))
    l0, l1 = np.load(tmp_path / "level0.npy"), np.load(tmp_path / "level1.npy")
    assert l0.dtype == l1.dtype == np.float32
    assert l0.shape == (1000,) and l0.min() >= 0 and l0.max() > 32768
    assert np.array_equal(l1, (np.arange(500, dtype=np.uint16) * 13).astype(np.float32))
    assert l0.nbytes + l1.nbytes <= 4 * 2000


def test_budget_is_under_64_mb():
    import bench
    assert bench.DUMP_BUDGET_BYTES <= 60 * 10 ** 6  # room for the .npy headers under 64 MB


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """A plain run of the default workload on a 2x2x3 chunk grid: --steps sets the timed steps, the line
    holds the headline fields and none of --full's objects, and the dumped array is the decode of the
    seeded input (C2 encodes uniform values drawn with seed 1234, the same in every run)."""
    import torch
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--grid", "2", "2", "3"]
    line = _bench(args + ["--dump-outputs", str(tmp_path / "a")])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    nbytes = 2 * 2 * 3 * 64 ** 3 * 4
    assert line["value"] == pytest.approx(nbytes / (line["ms_per_step"] * 1e-3) / 2 ** 30, rel=1e-2)
    assert not {"roofline", "cpu_baseline", "host_leg", "secondary"} & set(line)
    got = np.load(tmp_path / "a" / "out.npy")
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    exp = (torch.rand([128, 128, 192], generator=g, device="cuda", dtype=torch.float32) * 2 - 1).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, exp)
