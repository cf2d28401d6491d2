"""bench.py's plain line and --dump-outputs: a plain run times exactly --steps steps and prints the headline keys only; the dump holds the frames
of the last timed step, and two runs of the same command write the same arrays (so that two builds can be compared output for output)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _rig(n_out, step_no, shapes, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    outs = [tuple(torch.randint(0, 256, sh, generator=g, dtype=torch.uint8) for sh in shapes) for _ in range(n_out)]
    return types.SimpleNamespace(outs=outs, n_out=n_out, step_no=step_no, fmt="i420")


def test_dump_writes_the_last_step_in_push_order(tmp_path):
    b = _bench()
    rig = _rig(16, 37, [(6, 8), (3, 4), (3, 4)], seed=1)
    shapes = b.dump_outputs(rig, 16, str(tmp_path))
    assert shapes == {"y": [16, 48], "u": [16, 12], "v": [16, 12]}
    for k, name in enumerate(("y", "u", "v")):
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == np.float32
        for j, i in enumerate(range(37 - 16, 37)):                 # push i wrote outs[i % n_out]
            assert np.array_equal(a[j], rig.outs[i % 16][k].numpy().reshape(-1).astype(np.float32))


def test_dump_samples_within_its_budget_at_fixed_positions(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_BYTES", 4 * 4 * 300)
    rig = _rig(4, 4, [(40, 30), (20, 15), (20, 15)], seed=2)
    b.dump_outputs(rig, 4, str(tmp_path / "a"))
    b.dump_outputs(rig, 4, str(tmp_path / "b"))
    total = 0
    for name in ("y", "u", "v"):
        a, a2 = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert np.array_equal(a, a2)                               # the same positions from run to run
        total += a.nbytes
    assert 0 < total <= 4 * 4 * 300
    y = np.load(tmp_path / "a" / "y.npy")
    flat = [rig.outs[i][0].numpy().reshape(-1).astype(np.float32) for i in range(4)]
    assert y.shape[1] < flat[0].size
    # every row is the same selection of its own frame: one index set reproduces all four rows
    idx = np.sort(np.random.default_rng(b.DUMP_SEED).choice(flat[0].size, y.shape[1], replace=False))
    assert all(np.array_equal(y[j], flat[j][idx]) for j in range(4))


def _run(args, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--rows", "1080", "--cols", "1920", "--pool", "64"] + args
    return subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


@pytest.mark.gpu
def test_plain_line_and_dump_are_reproducible(tmp_path):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    lines = []
    for d in dirs:
        p = _run(["--dump-outputs", d])
        assert p.returncode == 0, p.stderr[-3000:]
        out = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, p.stdout[-2000:]
        lines.append(json.loads(out[0]))
    r = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    assert r["unit"] == "frames/s" and r["higher_is_better"] is True and r["steps"] == 3 and r["full"] is False
    rank = r["ranks"][0]
    assert rank["frames"] == 3 * 16 and abs(r["ms_per_step"] - rank["elapsed_s"] / 3 * 1e3) <= 1e-6 * r["ms_per_step"]
    assert abs(r["value"] - 3 * 16 / rank["elapsed_s"]) <= 1e-6 * r["value"]
    for k in ("sustained", "latency_ms", "roofline", "stage_us", "cpu_baseline", "configs", "multi_stream"):
        assert k not in r, k                                        # a plain run measures the timed steps only (--full: the rest)
    total = 0
    for name in ("y", "u", "v"):
        a, a2 = np.load(os.path.join(dirs[0], name + ".npy")), np.load(os.path.join(dirs[1], name + ".npy"))
        assert a.dtype == np.float32 and a.shape[0] == 16 and a.shape == a2.shape
        assert np.array_equal(a, a2), name                          # same arguments, same frames
        assert a.min() >= 0 and a.max() <= 255 and np.array_equal(a, np.round(a))
        total += a.nbytes
    assert total <= 64 << 20
    assert r["dump_outputs"]["arrays"]["y"] == list(np.load(os.path.join(dirs[0], "y.npy")).shape)
