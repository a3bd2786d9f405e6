"""`python bench.py --gpus N` without a launcher (the driver's command shape) must start the N ranks itself, before
any GPU call, relay rank 0's line and return the worst child code (reference layout: one process per GPU under DDP,
reflect_sampling_nerf_pipeline.py:72-77).  CPU only: the `selftest` workload runs the plumbing over gloo."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _run(extra_env=None, *argv, timeout=120):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(extra_env or {})
    return subprocess.run([sys.executable, BENCH, *argv], env=env, capture_output=True, text=True, timeout=timeout)


def test_gpus2_self_launches_two_gloo_ranks_and_prints_one_line():
    res = _run(None, "--gpus", "2", "--workload", "selftest")
    assert res.returncode == 0, res.stderr
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout  # exactly ONE JSON line on stdout (gloo's chatter goes to stderr)
    rec = json.loads(lines[0])
    assert rec == {"selftest": True, "n_gpus": 2, "rank_sum": 3.0}  # both ranks joined the all-reduce


def test_a_killed_rank_gives_a_nonzero_exit_code():
    # rank 1 dies by SIGKILL before the collective: rank 0's watchdog ends it with rc 3, the launcher reports the
    # worst code (128 + 9) and prints no result line
    res = _run({"RSN_BENCH_SELFTEST_FAIL_RANK": "1", "RSN_BENCH_WATCHDOG_S": "6"}, "--gpus", "2", "--workload", "selftest")
    assert res.returncode == 137, (res.returncode, res.stderr)
    assert not [ln for ln in res.stdout.splitlines() if ln.strip().startswith("{")]
    assert "child exit codes" in res.stderr


def test_too_few_gpus_is_refused_before_any_child_starts():
    res = _run({"HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""}, "--gpus", "2", "--steps", "1", "--warmup", "0")
    assert res.returncode == 2
    assert "GPU(s) visible" in res.stderr and not res.stdout.strip()


def test_self_launch_environment_and_worst_code(monkeypatch):
    """The spawn itself, mocked: N children of bench.py with the torchrun variables, same argv, rank 0 piped; the
    return value is the worst child code, a signal reads as 128 + k, survivors of a failed run are ended by PID."""
    sys.path.insert(0, REPO)
    import bench

    started = []

    class FakeProc:
        def __init__(self, cmd, env=None, stdout=None, stderr=None):
            self.cmd, self.env, self.rank = cmd, env, int(env["RANK"])
            self.stdout = iter([b'{"ok": 1}\n']) if stdout == subprocess.PIPE else None
            self.terminated = False
            started.append(self)

        def poll(self):
            if self.rank == 0:
                return 4  # the exception path of rank 0
            return -15 if self.terminated else None  # rank 1 hangs in the collective until terminated

        def terminate(self):
            self.terminated = True

        def kill(self):
            self.terminated = True

        def wait(self):
            return self.poll()

    monkeypatch.delenv("MASTER_PORT", raising=False)
    rc = bench.self_launch(2, ["--gpus", "2", "--steps", "3"], popen=FakeProc, grace=0.3, poll=0.05)
    assert rc in (5, 143)  # worst of [4 (rank 0), the survivor ended by the launcher]
    assert rc != 0 and len(started) == 2
    for r, p in enumerate(started):
        assert p.cmd[0] == sys.executable and p.cmd[1] == os.path.abspath(bench.__file__)
        assert p.cmd[2:] == ["--gpus", "2", "--steps", "3"]
        assert p.env["RANK"] == str(r) and p.env["LOCAL_RANK"] == str(r) and p.env["WORLD_SIZE"] == "2"
        assert p.env["MASTER_ADDR"] == "127.0.0.1" and int(p.env["MASTER_PORT"]) > 0
        assert p.env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert started[0].env["MASTER_PORT"] == started[1].env["MASTER_PORT"]
    assert started[1].terminated  # the hung survivor was ended


def test_main_takes_the_self_launch_branch_without_world_size(monkeypatch):
    sys.path.insert(0, REPO)
    import bench

    calls = []
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("RSN_BENCH_SHARE_GPU", "1")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "5", "--warmup", "2"])
    monkeypatch.setattr(bench, "self_launch", lambda n, argv: calls.append((n, argv)) or 0)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0 and calls == [(2, ["--gpus", "2", "--steps", "5", "--warmup", "2"])]
    # with WORLD_SIZE set (under torch.distributed.run) it is a rank and must NOT launch again
    calls.clear()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--workload", "selftest"])
    monkeypatch.setattr(bench, "run_selftest", lambda rank, world: calls.append(("rank", rank, world)))
    bench.main()
    assert calls == [("rank", 0, 2)]


def _load_bench():
    sys.path.insert(0, REPO)
    import bench

    return bench


def test_json_line_reports_rccl_ranks_for_the_nccl_backend():
    """The driver checks `config.rccl_ranks == N` on the N > 1 lines: it must be the process group's size whenever the
    backend is RCCL ("nccl" on ROCm), and 0 for the gloo rehearsal / a run without a collective."""
    bench = _load_bench()

    class FakeDist:
        def __init__(self, n):
            self.n = n

        def get_world_size(self):
            return self.n

    for n in (2, 4, 8):
        cfg = bench.collective_config(FakeDist(n), "nccl", n)
        assert cfg["rccl_ranks"] == n and cfg["parallelism"] == "dp%d" % n and cfg["backend"] == "nccl"
        assert "all-reduce" in cfg["collective"]
    assert bench.collective_config(FakeDist(2), "gloo", 2)["rccl_ranks"] == 0
    assert bench.collective_config(None, None, 1) == {"parallelism": "dp1", "collective": None, "rccl_ranks": 0, "backend": None}


def test_launcher_counts_gpus_without_initialising_hip(monkeypatch):
    """The self-launching parent must not touch HIP before it forks the ranks: the GPU count comes from the
    visible-devices environment or the KFD topology in sysfs, never from torch.cuda / hipGetDeviceCount."""
    bench = _load_bench()
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,1,2")
    assert bench.visible_gpu_count() == 3
    monkeypatch.delenv("HIP_VISIBLE_DEVICES")
    monkeypatch.delenv("CUDA_VISIBLE_DEVICES", raising=False)
    monkeypatch.delenv("ROCR_VISIBLE_DEVICES", raising=False)
    n = bench.visible_gpu_count()  # this container has no /dev/kfd: None (the ranks then report a shortfall themselves)
    assert n is None or n >= 0
    import inspect

    src = inspect.getsource(bench.main)
    assert "torch.cuda.device_count" not in src.split("self_launch(args.gpus")[0]


def test_dump_outputs_dtypes_and_seeded_sample(tmp_path, monkeypatch):
    """--dump-outputs: float64 stays float64, everything else is written as float32; over the byte budget every array is
    cut to its share by a sample whose positions are the same from run to run."""
    import numpy as np
    import torch

    bench = _load_bench()
    arrays = {"loss": torch.tensor(1.5), "w": torch.arange(12.0).reshape(3, 4), "f64": torch.ones(5, dtype=torch.float64),
              "mask": torch.tensor([True, False]), "bf": torch.ones(4, dtype=torch.bfloat16)}
    names = bench.dump_outputs(str(tmp_path / "a"), arrays)
    assert names == sorted(arrays)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert got["f64"].dtype == np.float64 and all(got[n].dtype == np.float32 for n in names if n != "f64")
    assert got["w"].shape == (3, 4) and np.array_equal(got["w"], np.arange(12.0, dtype=np.float32).reshape(3, 4))
    assert got["loss"].shape == () and float(got["loss"]) == 1.5 and got["mask"].tolist() == [1.0, 0.0]
    big = {"x": torch.randn(10000, generator=torch.Generator().manual_seed(0)), "y": torch.arange(3000.0)}
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 20000)
    for run in ("b", "c"):
        bench.dump_outputs(str(tmp_path / run), big)
    total = 0
    for n in big:
        b, c = np.load(tmp_path / "b" / (n + ".npy")), np.load(tmp_path / "c" / (n + ".npy"))
        assert np.array_equal(b, c) and 0 < b.size < big[n].numel()
        assert np.isin(b, big[n].numpy()).all()
        total += b.nbytes
    assert total <= 20000


def _fake_train_record(steps):
    kern = {q: 1.0 for q in ("achieved_tflops", "frac_of_fp32_mfma_peak", "avg_launch_ms", "launches_per_step",
                             "algorithmic_flop_per_step", "ms_per_step", "frac_of_bf16_mfma_peak",
                             "algorithmic_hbm_bytes_per_step", "achieved_hbm_tbps", "frac_of_hbm_peak")}
    kern["kernel"] = "k"
    return {"value": 1.0, "unit": "rays/s", "ms_per_step": 2.0, "steps": steps, "loss": 0.5, "reflect_ray_fraction": 0.5,
            "host_syncs_in_reducer": 0, "peak_device_memory_gb": 1.0, "ray_chunk": None, "launch_kinds": {},
            "kernels": {k: dict(kern) for k in ("forward", "backward", "wgrad")}, "algorithmic_flop_per_step": 1.0,
            "flop_formula": "", "end_to_end_tflops": 1.0, "end_to_end_frac_of_fp32_mfma_peak": 0.1, "other_ms_per_step": 0.0}


def test_plain_run_times_only_the_headline_and_full_adds_the_rest(monkeypatch, capsys):
    """A plain `bench.py --gpus 1 --steps N --warmup W` runs the headline training step once, with exactly N timed
    steps, and prints the line; the CPU baselines and the secondary legs run only under --full (GPU calls mocked)."""
    import json

    import torch

    import reflect_sampling_nerf_amd as pkg

    bench = _load_bench()
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RSN_BENCH_FORCE_COLLECTIVE", "RSN_BENCH_SHARE_GPU"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda i: None)
    monkeypatch.setattr(pkg, "load_library", lambda: None)
    calls = []

    def fake_train(pkg_, args, dev, rank, world, dist, share, samples, steps, warmup, dog, time_kernels=True, dump_dir=None):
        calls.append(("train", args.mma, steps, warmup, dump_dir))
        return _fake_train_record(steps)

    monkeypatch.setattr(bench, "run_train", fake_train)
    monkeypatch.setattr(bench, "run_level", lambda *a, **k: calls.append(("level",)) or {"value": 1.0})
    monkeypatch.setattr(bench, "run_eval_image", lambda *a, **k: calls.append(("eval_image",)) or {"value": 1.0})
    monkeypatch.setattr(bench, "cpu_baseline_train", lambda *a, **k: calls.append(("cpu_train",)) or {"value": 1.0})
    monkeypatch.setattr(bench, "cpu_baseline_level", lambda *a, **k: calls.append(("cpu_level",)) or {"value": 1.0})

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert calls == [("train", "f32", 7, 3, None)]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 7 and line["ms_per_step"] == 2.0 and line["dtype"] == "f32" and "cpu_baseline" not in line

    calls.clear()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3", "--full"])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    kinds = [c[0] for c in calls]
    assert calls[0] == ("train", "f32", 7, 3, None) and kinds.count("train") == 5
    assert {"level", "eval_image", "cpu_train", "cpu_level"} <= set(kinds)
    assert {"cpu_baseline", "eval_level", "eval_image", "train_step_configs2"} <= set(line)
