"""CPU tier: the parts of bench.py that do not need a GPU — the N > 1 self-launch command, the gating of
`roofline.traffic` on the library build and kernel symbol, the workload table."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_self_launch_spawns_torchrun_before_touching_the_gpu(monkeypatch, capsys):
    """`python bench.py --gpus 4 …` without a launcher: one `python -m torch.distributed.run` child with one rank per GPU on
    127.0.0.1, the original arguments passed through, rank 0's JSON line relayed on stdout, the child's exit code returned."""
    seen = {}

    class FakeProc:
        def __init__(self, cmd, env=None, stdout=None, stderr=None, text=None):
            seen["cmd"], seen["env"] = cmd, env
            self.stdout = iter(['[W] noise\n', '{"metric": "m", "value": 1.0}\n'])

        def wait(self):
            return 0
    monkeypatch.setattr(bench.subprocess, "Popen", FakeProc)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "20", "--warmup", "5"])

    class A:
        gpus = 4
    assert bench.self_launch(A()) == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-6:] == ["--gpus", "4", "--steps", "20", "--warmup", "5"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    out = capsys.readouterr()
    assert out.out.strip() == '{"metric": "m", "value": 1.0}' and "noise" in out.err


def test_self_launch_fails_loudly_without_a_result_line(monkeypatch):
    class FakeProc:
        def __init__(self, *a, **k):
            self.stdout = iter(["no json here\n"])

        def wait(self):
            return 0
    monkeypatch.setattr(bench.subprocess, "Popen", FakeProc)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])

    class A:
        gpus = 2
    assert bench.self_launch(A()) != 0


def test_traffic_is_only_carried_over_from_the_same_build_and_kernel(tmp_path, monkeypatch):
    """roofline.traffic comes from the newest profiles/r*_pmc_summary.json — but only if that summary was taken on the very
    library build that is running and holds the very kernel instantiation that dominated the run."""
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "r09_pmc_summary.json").write_text(json.dumps({
        "_meta": {"library_build_id": "abc", "git_head": "deadbeef"},
        "c5/accept_dir_trial": {"kernel_symbol": "k_cg<ObjQuadDiag, 7, 7, true>", "n_local": 100000000, "hbm_bytes_per_launch": 4.002e9},
        "shard/accept_dir_trial": {"kernel_symbol": "k_cg<ObjQuadDiag, 7, 7, false>", "n_local": 12500000, "hbm_bytes_per_launch": 5.0e8}}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    t, why = bench.pmc_traffic("abc", "k_cg<ObjQuadDiag, 7, 7, true>", 10**8)
    assert t == 4.002e9 and "same build" in why
    t, why = bench.pmc_traffic("abc", "k_cg<ObjQuadDiag, 7, 7, false>", 12500000)
    assert t == 5.0e8
    t, why = bench.pmc_traffic("other-build", "k_cg<ObjQuadDiag, 7, 7, true>", 10**8)
    assert t is None and "not carried over" in why
    t, why = bench.pmc_traffic("abc", "k_cg<ObjQuadDiag, 7, 3, true>", 10**8)
    assert t is None and "no entry" in why
    t, why = bench.pmc_traffic("abc", "k_cg<ObjQuadDiag, 7, 7, true>", 3 * 10**7)      # the same kernel at another size is another measurement
    assert t is None and "no entry" in why
    (prof / "r09_pmc_summary.json").unlink()
    assert bench.pmc_traffic("abc", "x", 1) == (None, "no PMC summary under profiles/")


def test_committed_pmc_summary_names_its_build():
    """The committed summary must say which build it was taken on (else bench.py can never use it)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_summary.json")))
    d = json.load(open(files[-1]))
    assert d["_meta"]["library_build_id"] and d["_meta"]["git_head"]
    syms = [v["kernel_symbol"] for k, v in d.items() if k != "_meta"]
    assert any(s.startswith("k_cg<ObjQuadDiag, 7, 7, true>") for s in syms)


def test_workload_table_covers_baseline_configs():
    assert {"c1", "c1c", "c2", "c3", "c4", "c5"} <= set(bench.WORKLOADS)
    assert bench.WORKLOADS["c5"][0] == 1e8 and bench.WORKLOADS["c2"][0] == 1e6 and bench.WORKLOADS["c3"][0] == 1e7
    assert bench.usable_cores() >= 1


@pytest.mark.parametrize("w", ["c1", "c1c", "c2", "c3", "c4", "c5"])
def test_cpu_baseline_runs_the_same_workload_for_every_config(w, monkeypatch):
    """`cpu_baseline` is printed beside EVERY workload line (VERDICT r02 missing #6): the oracle on the same objective,
    β flavour, line search and x0 as the GPU run, at the problem's FULL size, iterations w+1 … w+k of one run timed inside the
    oracle (no sample of the vector, nothing scaled by an n ratio) — here at a tiny n, to check the
    plumbing and the fields; the all-cores leg of a problem below the oracle's OpenMP threshold says it ran on one thread."""
    n = 1000 if w in ("c1", "c1c") else 4096
    monkeypatch.setitem(bench.CPU_SAMPLE, w, (2, 4, 1))
    r = bench.cpu_baseline(w, n)
    assert r["kind"] == "port" and r["cores"] == 1 and r["unit"] == "iterations/s" and r["value"] > 0
    assert f"({w})" in r["sample"] and "scaled" not in r["sample"] and "full size" in r["sample"] and "outer iterations 3..6" in r["sample"]
    a = bench.cpu_baseline(w, n, all_cores=True)
    assert a["cores"] == 1 and "below the OpenMP threshold" in a["sample"]


def test_a_hung_transport_is_reported_and_the_run_fails():
    """bench.py's N > 1 watchdog: the transport that hung is listed in transports_failed and the exit code is 5, not 0
     — checked on the source, the path needs N GPUs to execute."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    body = src[src.index("def give_up(kind):"):src.index("for kind in order:")]
    assert "results[kind] = None" in body and "os._exit(5)" in body and "os._exit(0)" not in body
    assert '"value_rccl"' in src and '"value_shm"' in src and "rccl_failed" in src


def test_dump_outputs_writes_float64_at_fixed_positions(tmp_path):
    """--dump-outputs: every array a caller of minimizeobjective receives, as float64; a vector longer than the sample is
    written at positions drawn from a fixed seed (the same in every run), and the default sample of n = 1e8 stays within
    64 MB in all."""
    import numpy as np
    from types import SimpleNamespace
    n, k = 5000, 4
    trace = SimpleNamespace(objective=np.linspace(3.0, 1.0, k), grad_norm=np.linspace(2.0, 0.5, k),
                            step_size=np.full(k, 0.25), objective_evals=np.arange(1, k + 1, dtype=np.int64))
    r = SimpleNamespace(minimizer=np.arange(n) * 0.5, gradient=np.arange(n) * -1.0, objective=1.0, iters_ran=k, trace=trace)
    bench.dump_outputs(str(tmp_path / "a"), r, sample=100)
    bench.dump_outputs(str(tmp_path / "b"), r, sample=100)
    names = {"minimizer", "gradient", "sample_index", "objective", "iters_ran", "trace_objective", "trace_grad_norm",
             "trace_step_size", "trace_objective_evals"}
    assert {p.stem for p in (tmp_path / "a").iterdir()} == names
    for name in names:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, b), name
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert 90 <= idx.size <= 100 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(np.load(tmp_path / "a" / "minimizer.npy"), 0.5 * idx)
    assert np.array_equal(np.load(tmp_path / "a" / "trace_objective_evals.npy"), [1.0, 2.0, 3.0, 4.0])
    bench.dump_outputs(str(tmp_path / "all"), r, sample=n)       # short vectors: every entry
    assert np.array_equal(np.load(tmp_path / "all" / "gradient.npy"), r.gradient)
    assert 3 * bench.DUMP_SAMPLE * 8 + 4 * 8 * 300 <= 64e6       # three sampled vectors + four traces of up to 300 iterations


def test_dump_outputs_is_refused_for_several_gpus():
    """Checked before anything starts ranks or touches a GPU."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dump-outputs", "x"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "single-GPU" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_exactly_the_steps_asked_for_and_dumps_its_outputs(tmp_path):
    """A plain run: one window of --steps steps, no CPU baseline; --dump-outputs writes the results of the last timed step
    (iteration warmup + steps), and --full keeps the extra windows and the CPU baselines."""
    import subprocess
    import numpy as np
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "2e5", "--steps", "7", "--warmup", "2"]
    r = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["windows"] == 1
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-9 * d["value"]
    assert "cpu_baseline" not in d and d["unit"] == "iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    out = tmp_path / "out"
    assert np.load(out / "iters_ran.npy")[0] == 9 and np.load(out / "trace_step_size.npy").size == 9
    x, idx = np.load(out / "minimizer.npy"), np.load(out / "sample_index.npy")
    assert x.dtype == np.float64 and x.size == idx.size == 200000 and np.all(np.isfinite(x))
    assert np.isclose(np.load(out / "objective.npy")[0], np.load(out / "trace_objective.npy")[-1], rtol=1e-12, atol=0)
    r = subprocess.run(cmd + ["--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["windows"] == 5
