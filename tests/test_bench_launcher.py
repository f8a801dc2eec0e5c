"""bench.py's entry point: `python bench.py --gpus N` starts N ranks itself, an
outer launcher's WORLD_SIZE must agree with --gpus, and n_gpus is the process group's size.  Driven
with the GPU-free `dpcheck` workload over gloo."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, timeout=180):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout)


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [1, 2, 4])
def test_gpus_flag_starts_n_ranks(n):
    r = _run(["--gpus", str(n), "--workload", "dpcheck"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == n
    assert line["rank_sum"] == line["expected"] == n * (n + 1) / 2


def test_dump_outputs_files_budget_and_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs' writer: one float32 / float64 .npy per name, small arrays whole, an array over its
    share of the budget as the same sample of its elements on every call, all within the budget (64 MB
    in bench.py; a small one here)."""
    import numpy as np
    import torch

    import bench
    assert bench.DUMP_BUDGET_BYTES <= 64 * 10 ** 6
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 4 * 5000)
    g = torch.Generator().manual_seed(3)
    big = torch.randn(bench.DUMP_BUDGET_BYTES // 4 // 4 + 1001, generator=g)
    arrays = {"losses": torch.arange(9, dtype=torch.float64), "small": torch.randn(2, 3, 5, 7, generator=g).half(),
              "big": big, "big64": big.double()}
    total = bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), {k: v + 1 for k, v in arrays.items()})
    assert total <= bench.DUMP_BUDGET_BYTES
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "big64.npy", "losses.npy", "small.npy"]
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in arrays}
    b = {k: np.load(tmp_path / "b" / (k + ".npy")) for k in arrays}
    assert a["losses"].dtype == np.float64 and a["small"].dtype == np.float32 and a["big"].dtype == np.float32
    assert np.array_equal(a["losses"], np.arange(9.0))
    assert np.array_equal(a["small"], arrays["small"].float().numpy())
    cap = bench.DUMP_BUDGET_BYTES // 4 // 4
    assert a["big64"].dtype == np.float64 and a["big64"].shape == (cap // 2,)   # the share is in bytes
    assert a["big"].shape == (cap,) and len(np.unique(a["big"])) > cap // 2
    assert np.isin(a["big"], big.numpy()).all()
    assert np.array_equal(b["big"], (a["big"] + np.float32(1)).astype(np.float32))   # the same elements again


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    """One plain run, one timed step: the line has the headline keys and none of --full's legs, and
    --dump-outputs wrote, after the timed step, what a caller of optimize_parameters() has: the losses
    (float64, finite, the line's final_losses), the model's visuals and its networks' parameters."""
    import numpy as np
    d = tmp_path / "out"
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "1", "--dump-outputs", str(d)])
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "final_losses"):
        assert k in line, k
    assert line["steps"] == 1 and line["ms_per_step"] > 0 and line["unit"] == "frames/s"
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - 4.0) < 0.01   # B=4 frames in one timed step
    assert line["warp_backward"].startswith("ordered")
    for k in ("roofline", "roofline_convs", "inference", "mixed_policy", "extras", "cpu_baseline", "parity"):
        assert k not in line, k
    names = sorted(f[:-4] for f in os.listdir(d))
    visuals = ["real_A", "fake_B", "rec_A", "idt_B", "real_B", "fake_A", "rec_B", "idt_A"]
    assert names == sorted(["losses"] + ["visual_" + v for v in visuals] + ["params_" + n for n in
                                                                          ("G_A", "G_B", "D_A", "D_B")])
    arrays = {n: np.load(d / (n + ".npy")) for n in names}
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6
    assert arrays["losses"].dtype == np.float64
    assert np.allclose(arrays["losses"], list(line["final_losses"].values()), rtol=0, atol=1e-5)   # rounded to 5 places
    for n, a in arrays.items():
        assert np.isfinite(a).all(), n
        if n != "losses":
            assert a.dtype == np.float32, n
        if n.startswith("visual_"):
            assert a.shape == (4, 3, 256, 256) and np.abs(a).max() <= 1.0, n


def test_outer_world_size_must_match_gpus():
    r = _run(["--gpus", "2", "--workload", "dpcheck"], env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in (r.stderr + r.stdout)
