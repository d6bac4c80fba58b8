"""bench.py --gpus N without the torchrun environment launches the N ranks itself (a parent that never touches a GPU)
and relays rank 0's line: exercised here with --dry-launch over gloo (no GPU in this container)."""
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import ROOT


@pytest.mark.timeout(300)
def test_bench_launches_two_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-launch"], env=env, capture_output=True,
                       text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["dry_launch"] is True and d["backend"] == "gloo"


def test_bench_single_rank_dry_and_args():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = bench.parse_args([])
    assert a.gpus == 1 and a.steps % 9 == 0 and a.mode == "render"
    assert len(bench.GAZES) == 9 and bench.GAZES[4] == (0.5, 0.5) and (0.25, 0.75) in bench.GAZES
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-launch"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and json.loads(p.stdout.strip().splitlines()[-1])["n_gpus"] == 1


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_plain_and_full_args():
    """A plain run times exactly --steps frames once; --full keeps the five repeats and everything else the line carried."""
    bench = _bench_module()
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.repeats == 1 and a.dump_outputs is None
    f = bench.parse_args(["--full"])
    assert f.full is True and f.repeats == 5
    assert bench.parse_args(["--full", "--repeats", "3"]).repeats == 3
    assert bench.parse_args(["--dump-outputs", "x"]).dump_outputs == "x"
    with pytest.raises(SystemExit):
        bench.parse_args(["--mode", "train", "--dump-outputs", "x"])


@pytest.mark.parametrize("P,H,W", [(600_000, 1080, 1920), (1000, 2160, 3840)])
def test_bench_dump_outputs(tmp_path, P, H, W):
    """--dump-outputs writes float32 / float64 .npy files of the render() dict within the size budget: the per-Gaussian arrays at a
    fixed, seeded sample of rows (the same rows on every call), the image whole unless it alone would not fit."""
    import numpy as np
    import torch
    bench = _bench_module()
    g = torch.Generator().manual_seed(0)
    radii = torch.randint(0, 5, (P,), generator=g, dtype=torch.int32)
    out = {"render": torch.rand(3, H, W, generator=g), "viewspace_points": torch.rand(P, 3, generator=g),
           "visibility_filter": radii > 0, "radii": radii}
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert {"render.npy", "radii.npy", "visibility_filter.npy", "viewspace_points.npy", "gaussian_index.npy"} <= set(files)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BUDGET
    d = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert d[f[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(d[f[:-4]], np.load(tmp_path / "b" / f))
    rows = d["gaussian_index"].astype(np.int64)
    assert len(rows) == min(P, bench.DUMP_ROWS) and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(d["radii"], radii.numpy()[rows].astype(np.float32))
    np.testing.assert_array_equal(d["visibility_filter"], (radii.numpy()[rows] > 0).astype(np.float32))
    np.testing.assert_array_equal(d["viewspace_points"], out["viewspace_points"].numpy()[rows])
    img = out["render"].numpy()
    if "pixel_index" in d:
        np.testing.assert_array_equal(d["render"], img.reshape(3, -1)[:, d["pixel_index"].astype(np.int64)])
    else:
        np.testing.assert_array_equal(d["render"], img)
