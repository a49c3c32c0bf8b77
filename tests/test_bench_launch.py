"""bench.py's `--gpus N` contract: an unaided `--gpus N > 1`
starts N ranks itself, a launcher's WORLD_SIZE must agree with --gpus, and the
parent decides this before anything touches the GPU.  CPU only."""
import importlib.util
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_check_world_decisions():
    b = _bench()
    assert b.check_world(1, {}) == "run"
    assert b.check_world(8, {}) == "launch"
    assert b.check_world(2, {"WORLD_SIZE": "2"}) == "run"
    assert b.check_world(1, {"WORLD_SIZE": "1"}) == "run"
    with pytest.raises(SystemExit):
        b.check_world(8, {"WORLD_SIZE": "2"})
    with pytest.raises(SystemExit):
        b.check_world(1, {"WORLD_SIZE": "4"})
    with pytest.raises(SystemExit):
        b.check_world(0, {})


def test_launch_command_passes_every_flag():
    b = _bench()
    argv = ["--gpus", "4", "--steps", "20", "--warmup", "5", "--no-large"]
    cmd = b.launch_command(argv, 4, 29555)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert "--master-addr=127.0.0.1" in cmd and "--master-port=29555" in cmd
    k = cmd.index(os.path.join(REPO, "bench.py"))
    assert cmd[k + 1:] == argv


def test_plain_run_measures_the_headline_alone(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = b.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 20 and a.warmup == 5
    assert a.no_cpu_baseline and a.no_sharded and a.no_neumf and a.no_eval and a.no_large
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-large", "--dump-outputs", "d"])
    a = b.parse()
    assert a.full and a.dump_outputs == "d" and a.no_large
    assert not (a.no_cpu_baseline or a.no_sharded or a.no_neumf or a.no_eval)


def test_dump_outputs_writes_float32_tables(tmp_path, monkeypatch):
    import numpy as np
    import torch
    b = _bench()
    g = torch.Generator().manual_seed(0)
    tabs = [torch.randn(n, 8, generator=g) for n in (37, 23, 37, 23)]
    b.dump_outputs(str(tmp_path / "o"), tabs)
    for name, t in zip(("P", "Q", "accP", "accQ"), tabs):
        x = np.load(tmp_path / "o" / f"{name}.npy")
        assert x.dtype == np.float32 and np.array_equal(x, t.numpy())
    # beyond the size limit: the same seeded rows on every call, within the limit
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 2000)
    b.dump_outputs(str(tmp_path / "s1"), tabs)
    b.dump_outputs(str(tmp_path / "s2"), tabs, rank=1)
    total = 0
    for name, t in zip(("P", "Q", "accP", "accQ"), tabs):
        x, y = np.load(tmp_path / "s1" / f"{name}.npy"), np.load(tmp_path / "s2" / f"{name}_rank1.npy")
        assert np.array_equal(x, y) and 0 < x.shape[0] < t.shape[0]
        assert all((t.numpy() == r).all(1).any() for r in x)
        total += x.nbytes
    assert total <= 2000


def _run_bench(args, env_extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], env=env, cwd=REPO,
                          capture_output=True, text=True, timeout=300)


def test_mismatched_world_size_exits_nonzero():
    r = _run_bench(["--gpus", "8"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr and "--gpus 8" in r.stderr
    assert r.stdout == ""


@pytest.mark.skipif(__import__("torch").cuda.device_count() >= 2, reason="needs a host with fewer than 2 GPUs")
def test_unaided_multi_gpu_without_devices_refuses():
    r = _run_bench(["--gpus", "2"], {})
    assert r.returncode != 0
    assert "GPU(s) visible" in r.stderr
    assert r.stdout == ""
