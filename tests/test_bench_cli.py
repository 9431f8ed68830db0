"""bench.py's command line: --steps sets the timed steps, a plain run reports the headline figures only (the
other measurements are --full's), and --dump-outputs writes the last timed step's arrays as float32 / float64
.npy files of at most 64 MB in all."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("env_kernel_ms", "env_reset", "learn_step_ms_eager", "data_parallel", "roofline", "roofline_env",
             "roofline_env_plateau", "iqn", "learn_b64", "fp32_learner", "dropin_single_env", "rainbow", "config5",
             "cpu_baseline")


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_and_dump_are_off_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 20, 5)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--steps", "15", "--unroll", "10")])
def test_steps_that_cannot_be_timed_as_asked_are_refused(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def test_dump_outputs_formats_and_size_cap(monkeypatch, tmp_path):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)   # 1024 bytes per array
    outs = {"f64": torch.arange(100, dtype=torch.float64), "u8": torch.ones(10, dtype=torch.uint8),
            "big32": torch.arange(5000, dtype=torch.float32).reshape(50, 100),
            "big64": torch.arange(5000, dtype=torch.float64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in outs}
    assert got["f64"].dtype == np.float64 and np.array_equal(got["f64"], np.arange(100.0))
    assert got["u8"].dtype == np.float32 and np.array_equal(got["u8"], np.ones(10, np.float32))
    assert got["big32"].dtype == np.float32 and got["big32"].shape == (256,)
    assert got["big64"].dtype == np.float64 and got["big64"].shape == (128,)
    assert sum(a.nbytes for a in got.values()) <= 4096
    for n in ("big32", "big64"):   # a sample of the array's own elements, in order, the same on every run
        assert np.all(np.diff(got[n]) > 0) and got[n][-1] < 5000
        assert np.array_equal(got[n], np.load(tmp_path / "b" / (n + ".npy")))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_its_outputs(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["full"] is False and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(4096 * 1e3 / d["ms_per_step"], rel=1e-9)
    assert all(d[k] is None for k in FULL_ONLY)
    files = sorted(os.listdir(tmp_path))
    assert files == ["actions.npy", "done.npy", "env_state.npy", "losses.npy", "obs.npy", "reward.npy",
                     "weights_actor.npy", "weights_critic.npy"]
    arrays = {f: np.load(tmp_path / f) for f in files}
    for f, a in arrays.items():
        assert a.dtype in (np.float32, np.float64) and a.size and np.isfinite(a).all(), f
    assert arrays["env_state.npy"].shape == (16, 4096 * 5)   # every state field but the COLREGs turn angle
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
