"""-m gpu: batched evaluation end to end - harness.evaluate (DepthEstimationNet.predict + MetricComputation.compute_rows per batch, one copy
at the end) and `python -m md_rdm_amd.evaluate` - against the batch-1 loop it replaces: harness.validation_step + MetricLogger.log_val and
MetricComputation.avg (the reference's validation with Lightning's epoch mean, module.py:99-117).

Inputs: md_rdm_amd.evaluate.synthetic_samples - the evaluation input of filler.MARGIN_SEEDS (every DORN decision on it carries a margin, so
the count map, and with it the predicted map, is the same at every batch size and in every run), each sample with its own hash-generated
depth.  The first test asserts that on the count maps; the averages are then held to rtol 1e-11, the project's bound for the metric sums in
another order (tests/test_gpu_ops.py).  Each comparison prints its observed figure before it asserts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from md_rdm_amd import filler

pytestmark = pytest.mark.gpu
METRICS = ["delta1", "delta2", "delta3", "mse", "mae", "log10", "absrel", "sqrel", "rmse"]
N, BS = 3, 2                                                          # the last batch holds one sample


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def make_model(dev, relative_decoders=()):
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet(relative_decoders=relative_decoders)
    filler.fill_state_dict(m.state_dict())
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def model(dev):
    return make_model(dev)


@pytest.fixture(scope="module")
def samples(dev):
    from md_rdm_amd import evaluate
    x, y = evaluate.synthetic_samples(N, 226, 226)
    return torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)


def batches_of(x, y, bs):
    return [(x[i:i + bs], y[i:i + bs]) for i in range(0, x.shape[0], bs)]


@pytest.fixture(scope="module")
def batch1_loop(model, samples):
    """The loop md_rdm_amd/train.py runs at --val_batch_size 1: validation_step + log_val per sample; computed once."""
    from md_rdm_amd import harness
    from md_rdm_amd.metrics import MetricLogger
    x, y = samples
    logger = MetricLogger(METRICS)
    per_sample = []
    with torch.no_grad():
        for i in range(N):
            y_hat, y_n = harness.validation_step(model, x[i:i + 1], y[i:i + 1])
            per_sample.append(logger.log_val(y_hat, y_n))
    return logger, per_sample


def test_batched_and_batch1_count_maps_are_equal(model, samples):
    x, _ = samples
    maps, counts = model.predict(x[:BS], return_counts=True)
    for i in range(BS):
        m1, c1 = model.predict(x[i:i + 1], return_counts=True)
        assert torch.equal(c1[0], counts[i]), i
        assert torch.equal(m1[0], maps[i]), i                         # the map is a function of the counts and the level weights only


def test_evaluate_matches_the_batch1_validation_loop(model, samples, batch1_loop):
    from md_rdm_amd import harness
    x, y = samples
    logger, per_sample = batch1_loop
    res = harness.evaluate(model, batches_of(x, y, BS), METRICS)
    assert res["n"] == N
    values = np.array([[s[m] for m in METRICS] for s in per_sample])
    assert np.abs(values[0] - values[1]).max() > 1e-3                 # the samples' targets differ: the mean is a mean of different rows
    for k, m in enumerate(METRICS):
        want = logger.computer.avg(m)
        print("%s: evaluate %.15g, batch-1 loop %.15g, rel %.3e" % (m, res[m], want, abs(res[m] / want - 1)))
        np.testing.assert_allclose(res[m], want, rtol=1e-11, atol=0)
        np.testing.assert_allclose(res[m], values[:, k].mean(), rtol=1e-11, atol=0)
    res1 = harness.evaluate(model, batches_of(x, y, 1), METRICS)     # independent of the batch size: the same rows, the same mean
    assert res1 == res


def test_return_maps_are_predicts_maps(model, samples):
    from md_rdm_amd import harness
    x, y = samples
    res, maps = harness.evaluate(model, batches_of(x, y, BS), METRICS, return_maps=True)
    assert maps.shape == (N, 1, 128, 128) and maps.dtype == torch.float64
    assert torch.equal(maps[:BS], model.predict(x[:BS])) and torch.equal(maps[BS:], model.predict(x[BS:]))
    res_exp = harness.evaluate(model, batches_of(x, y, BS), METRICS, exp_pred=True)
    assert res_exp["n"] == N and res_exp["mse"] != res["mse"]


def test_relative_decoder_goes_through_the_composed_predict_path(dev, samples):
    from md_rdm_amd import _lib, harness
    from md_rdm_amd.metrics import MetricComputation
    m = make_model(dev, relative_decoders=(10,))
    assert m._fused_tail_levels(8, 8) is None                          # predict composes the single operators for this model
    x, y = samples
    x, y = x[:2], y[:2]
    mc = MetricComputation(METRICS)
    res, maps = harness.evaluate(m, [(x, y)], mc, return_maps=True)    # ONE forward: the rows below are taken of the maps it scored
    assert maps.shape == (2, 1, 128, 128) and res["n"] == 2
    rows = mc.compute_rows(maps, y).cpu().numpy()
    tn = harness.normalize(harness.prepare_target(y))
    ref = torch.empty(2, 10, dtype=torch.float64, device=dev)
    for b in range(2):
        _lib.check(_lib.lib().rdm_depth_metrics_f64(_lib.ptr(maps[b].contiguous()), _lib.ptr(tn[b].contiguous()), 128 * 128, _lib.ptr(ref[b]), _lib.stream()))
    ref = ref.cpu().numpy()
    print("relative_decoders=(10,): rows vs rdm_depth_metrics_f64, max rel = %.3e" % np.abs(rows[:, 4:] / ref[:, 4:] - 1).max())
    np.testing.assert_array_equal(rows[:, :4], ref[:, :4])
    np.testing.assert_allclose(rows[:, 4:], ref[:, 4:], rtol=1e-11, atol=0)
    vals = mc.values_from_rows(rows)
    for k, name in enumerate(METRICS):
        np.testing.assert_allclose(res[name], (vals[0][k] + vals[1][k]) / 2, rtol=1e-11, atol=0)


def test_cli_writes_what_evaluate_gives(model, samples, tmp_path):
    from md_rdm_amd import harness
    out = tmp_path / "results.json"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "md_rdm_amd.evaluate", "--synthetic", str(N), "--batch_size", str(BS), "--metrics"] + METRICS
                       + ["--out", str(out)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "warning" in r.stdout
    rec = json.loads(out.read_text())
    x, y = samples
    res = harness.evaluate(model, batches_of(x, y, BS), METRICS)
    assert rec["n"] == res["n"] == N and rec["split"] == "synthetic" and rec["batch_size"] == BS and rec["exp_pred"] is False
    for m in METRICS:
        print("%s: CLI %.15g, in-process %.15g" % (m, rec["metrics"][m], res[m]))
        assert ("%s %.6f" % (m, res[m])) in r.stdout
        assert rec["metrics"][m] == res[m], m
