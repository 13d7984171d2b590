"""bench.py contract on the GPU: one JSON line with the driver's fields; with --full also `roofline`, `extras` and `cpu_baseline`."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra", [[], ["--shapes-per-step", "1"], ["--workload", "nearest"]])
def test_bench_prints_one_json_line_with_the_contract_fields(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--ddnm-steps", "2", "--no-cpu-baseline", "--full"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["unit"] == "shapes/hour" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 3600e3 * d["config"]["shapes_per_step"] / d["ms_per_step"]) < 1e-6 * d["value"]
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    if "nearest" not in extra:
        assert r["bound"] == "mfma" and r["achieved"] > 100 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
        assert d["config"]["shapes_per_step"] == (1 if "--shapes-per-step" in extra else 4)
        # in-run calibration: the vendor GEMM on operands with the bench's statistics and on zeros, and a copy
        cal = r["calibration"]
        assert cal["gemm_f16_random_tflops"] > 300 and cal["gemm_f16_zeros_tflops"] >= 0.9 * cal["gemm_f16_random_tflops"] and cal["copy_gbs"] > 1000, cal
        assert abs(r["frac_of_calibrated"] - r["achieved"] / r["calibrated_peak"]) < 1e-9
        one = d["extras"]["ddnm_one_shape"]
        assert len(one["samples"]) == 3 and min(one["samples"]) <= one["seconds"] <= max(one["samples"])


def test_bench_two_ranks_rehearsal_carries_the_view_parallel_figure():
    """The N > 1 code path of bench.py on the one GPU there is (two ranks on cuda:0 over gloo): weak-scaling headline over both ranks'
    shapes, plus extras.view_parallel = one shape with its 8 views sharded 4 + 4 and gathered once, next to the same shape on rank 0
    alone -- the figure the driver's 8-GPU run needs for the >= 6x view-parallel claim (BASELINE.json north_star)."""
    import socket
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--ddnm-steps", "2", "--shapes-per-step", "1",
           "--backend", "gloo", "--one-device", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["shapes_per_step"] == 2 and d["cpu_baseline"] is None
    vp = d["extras"]["view_parallel"]
    assert "error" not in vp, vp
    assert vp["seconds_per_shape"] > 0 and vp["n1_one_shape_seconds"] > 0 and abs(vp["speedup_vs_n1_one_shape"] - vp["n1_one_shape_seconds"] / vp["seconds_per_shape"]) < 1e-9
    assert len(vp["samples"]) == 3


def test_bench_two_ranks_headline_survives_a_side_figure_that_does_not_come_back():
    """The view-parallel side figure is the only collective after the timed region and has never met N > 1 hardware: with a
    watchdog that fires at once (--extras-timeout 0.01) every rank leaves, rank 0 having printed the ONE headline line with
    extras.view_parallel = {error: ...} -- exit code 0, contract fields intact."""
    import socket
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--ddnm-steps", "2", "--shapes-per-step", "1",
           "--backend", "gloo", "--one-device", "--extras-timeout", "0.01", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["roofline"]["achieved"] > 0
    assert "error" in d["extras"]["view_parallel"]


def _run_plain(args, tmp):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(tmp)] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    """Without --full the line carries the headline only (no side measurements), --steps sets the timed steps, and --dump-outputs
    writes the atlases of the last step (four shapes per step by default) as float32 .npy files within the 64 MB budget."""
    import numpy as np
    d = _run_plain(["--steps", "2", "--warmup", "1", "--ddnm-steps", "2"], tmp_path / "dump")
    for k in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "dtype"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "shapes/hour" and d["higher_is_better"] is True
    assert abs(d["value"] - 3600e3 * d["config"]["shapes_per_step"] / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["roofline"] is None and d["extras"] is None and d["cpu_baseline"] is None
    files = sorted(os.listdir(tmp_path / "dump"))
    assert files == [f"shape{i}_atlas.npy" for i in range(4)], files
    assert sum(os.path.getsize(tmp_path / "dump" / f) for f in files) <= 64e6
    for f in files:
        a = np.load(tmp_path / "dump" / f)
        assert a.dtype == np.float32 and a.shape == (1024, 1024, 3) and np.isfinite(a).all() and a.std() > 0


def test_bench_dumped_outputs_repeat_run_to_run(tmp_path):
    """Same arguments, same inputs: two plain runs of the (deterministic) nearest workload dump identical arrays."""
    import numpy as np
    args = ["--workload", "nearest", "--steps", "2", "--warmup", "1"]
    _run_plain(args, tmp_path / "a")
    _run_plain(args, tmp_path / "b")
    files = sorted(os.listdir(tmp_path / "a"))
    assert files and files == sorted(os.listdir(tmp_path / "b"))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
