"""The driver keeps a bounded tail of bench.py's stdout (round 4: a 25.7 KB line came back unparsed, so the headline counted as
unmeasured).  The printed record must stay small, carry the contract's fields and round-trip; everything else lives in
bench_detail.json.  Input = the FULL records earlier rounds committed under profiles/ (the largest real ones there are)."""
import glob
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
            "roofline", "cpu_baseline")
FULL = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[2-9]_bench_*.json")))


@pytest.mark.parametrize("path", FULL, ids=[os.path.basename(p) for p in FULL])
def test_compact_line_is_small_complete_and_round_trips(path, tmp_path, capsys, monkeypatch):
    with open(path) as fh:
        full = json.load(fh)
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))               # the detail file goes to a scratch directory
    line = bench.emit(full)
    text = capsys.readouterr().out.strip()
    assert "\n" not in text and len(text) < bench.LINE_LIMIT == 4096
    back = json.loads(text)
    assert back == json.loads(json.dumps(line))
    for k in CONTRACT:
        assert k in back, k
    for k in ("metric", "value", "unit", "ms_per_step"):
        assert back[k] == full[k]
    assert "workload" in back["config"] and "model" not in back["config"]
    if full.get("roofline"):
        r = back["roofline"]
        for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
            assert k in r, k
        assert r["bound"] in ("hbm", "mfma") and 0 < r["frac"] <= 1.0
        assert "per_kernel" not in r and "conv_family" not in r and "whole_step" not in r      # tables and re-based figures: detail file only
    if full.get("cpu_baseline"):
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in back["cpu_baseline"], k
    with open(tmp_path / bench.DETAIL_FILE) as fh:                  # the full record is what the detail file holds
        assert json.load(fh) == full
    assert back["detail"] == bench.DETAIL_FILE


def test_line_survives_a_pathologically_long_record(tmp_path, capsys, monkeypatch):
    """Strings are bounded and optional parts are dropped before the limit is reached; an impossible record fails loudly HERE."""
    with open(FULL[-1]) as fh:
        full = json.load(fh)
    full["dtype"] = "x" * 5000
    full["config"]["workload"] = "NYU-v2 228x304 batch=16 " + "y" * 5000
    full["config"]["extra_configs"] = (full["config"].get("extra_configs") or [{"metric": "m", "value": 1.0}]) * 8
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    bench.emit(full)
    text = capsys.readouterr().out.strip()
    assert len(text) < bench.LINE_LIMIT
    assert json.loads(text)["config"]["workload"].startswith("NYU-v2 228x304 batch=16")


def test_dump_outputs_are_float_arrays_at_fixed_sample_positions(tmp_path, monkeypatch):
    """--dump-outputs: every array float32 or float64 (integers widened exactly), nested outputs named by position / key, a long
    output cut to the same seeded positions in every run, the whole set bounded by DUMP_LIMIT."""
    import numpy as np
    import torch
    parts = {"mse": torch.tensor(1.5), "labels": torch.arange(6, dtype=torch.int64).view(2, 3),
             "levels": [torch.ones(2, 2, dtype=torch.bfloat16), torch.zeros(3, dtype=torch.float64)]}
    arrays = bench.tensor_arrays("step", parts)
    assert sorted(arrays) == ["step_labels", "step_levels_0", "step_levels_1", "step_mse"]
    assert arrays["step_labels"].dtype == np.float64 and arrays["step_labels"].tolist() == [[0, 1, 2], [3, 4, 5]]
    assert arrays["step_levels_0"].dtype == np.float32 and arrays["step_levels_1"].dtype == np.float64
    monkeypatch.setattr(bench, "SAMPLE", 1000)
    ts = [torch.arange(3000, dtype=torch.float32), torch.arange(3000, 5000, dtype=torch.float32).view(40, 50)]
    a, b = bench.flat_sample(ts, seed=0), bench.flat_sample(ts, seed=0)
    assert a.shape == (1000,) and a.dtype == np.float32 and np.array_equal(a, b) and np.all(np.diff(a) >= 0) and a.max() < 5000
    assert not np.array_equal(a, bench.flat_sample(ts, seed=1))
    short = bench.flat_sample([torch.ones(3, dtype=torch.float32), torch.tensor([7], dtype=torch.int64)], seed=0)
    assert short.dtype == np.float64 and short.tolist() == [1, 1, 1, 7]
    arrays["sample"] = a
    total = bench.dump_outputs(str(tmp_path / "out"), arrays)
    for k, v in arrays.items():
        back = np.load(tmp_path / "out" / (k + ".npy"))
        assert back.dtype == v.dtype and np.array_equal(back, v)
    monkeypatch.setattr(bench, "DUMP_LIMIT", total - 1)
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "over"), arrays)


@pytest.mark.gpu
def test_plain_run_times_its_steps_only_and_dumps_the_last_one(tmp_path):
    """A plain `bench.py` run: the timed steps and the line (no roofline leg, CPU baseline or extra configuration - those are
    --full), `steps` timed steps behind `ms_per_step`, and --dump-outputs writes the last timed step's loss, components and
    seeded parameter / gradient / buffer samples, all finite at 50 steps (the repeated batch at the reference's lr of 1e-4
    reaches a NaN loss after ~43).  A second run with other step counts sees the same targets and the same (seeded) parameters."""
    import subprocess
    import numpy as np

    def run(out, steps, warmup):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == steps and d["warmup"] == warmup and d["ms_per_step"] > 0 and d["unit"] == "images/s" and d["higher_is_better"] is True
        return d
    out = tmp_path / "out"
    d = run(out, 50, 1)
    assert abs(d["value"] - 16 * 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and "extra_configs" not in d["config"]
    assert "per_stage_join_overhead_ms" not in d["config"]["comm"]
    files = {p.name[:-4]: np.load(p) for p in out.glob("*.npy")}
    assert {"loss", "step_final_depth", "step_ord_label_pred", "params", "grads", "buffers"} <= set(files)
    assert all(v.dtype in (np.float32, np.float64) for v in files.values()) and sum(v.nbytes for v in files.values()) <= bench.DUMP_LIMIT
    assert files["loss"].shape == (1,) and abs(float(files["loss"][0]) - d["config"]["loss"]) < 1e-3 * abs(d["config"]["loss"])
    assert files["params"].shape == files["grads"].shape == (bench.SAMPLE,)
    assert all(np.isfinite(v).all() for v in files.values())
    first = run(tmp_path / "first", 1, 0)
    for k in ("step_y", "step_ord_y", "params"):
        assert np.array_equal(np.load(tmp_path / "first" / (k + ".npy")), files[k]), k
    assert abs(first["config"]["loss"] - d["config"]["loss"]) < 1e-3 * abs(d["config"]["loss"])
