"""Batched evaluation without a GPU: the command's flags and argument errors, the no-GPU line, MetricComputation.values_from_rows on
hand-made rows, PrefetchLoader(indices=...) sharding and the mean over shards."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

ENV = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


def test_parser_defaults_and_flags():
    from md_rdm_amd import evaluate
    a = evaluate.build_parser().parse_args([])
    assert (a.checkpoint, a.nyu_path, a.split, a.synthetic, a.batch_size, a.precision, a.size, a.relative_decoders, a.exp_pred, a.out, a.worker) == \
        (None, None, "val", 0, 8, 32, [226, 226], [], False, None, 6)
    assert a.metrics == ["delta1", "delta2", "delta3", "mse", "mae", "log10", "rmse"]
    a = evaluate.build_parser().parse_args(["--nyu_path", "d", "--split", "test", "--batch_size", "16", "--precision", "16", "--size", "228", "304", "--relative_decoders",
                                            "6", "10", "--metrics", "mse", "--exp_pred", "--out", "r.json", "--worker", "2", "--checkpoint", "c.ckpt"])
    assert (a.nyu_path, a.split, a.batch_size, a.precision, a.size, a.relative_decoders, a.metrics, a.exp_pred, a.out, a.worker, a.checkpoint) == \
        ("d", "test", 16, 16, [228, 304], [6, 10], ["mse"], True, "r.json", 2, "c.ckpt")
    text = evaluate.build_parser().format_help()
    exp_help = " ".join(text[text.rindex("--exp_pred"):].split())   # the option's entry (the usage line names it first)
    assert "DEPARTS from the reference" in exp_help[:400]             # the flag's help says it is not what the reference computes
    with pytest.raises(SystemExit):
        evaluate.build_parser().parse_args(["--split", "train"])


@pytest.mark.parametrize("argv", [[], ["--nyu_path", "d", "--synthetic", "3"]])
def test_nyu_path_or_synthetic_not_both(argv):
    from md_rdm_amd import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(argv)
    assert "give --nyu_path DIR or --synthetic N (not both)" in str(e.value)


def test_no_visible_gpu_is_one_clear_line(tmp_path):
    from md_rdm_amd import evaluate
    env = dict(ENV, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = tmp_path / "r.json"
    r = subprocess.run([sys.executable, "-m", "md_rdm_amd.evaluate", "--synthetic", "1", "--out", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "Traceback" not in r.stderr
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert lines and lines[-1] == evaluate.NO_GPU and "no GPU is visible" in evaluate.NO_GPU
    assert not out.exists()


def test_values_from_rows_on_hand_made_rows():
    from md_rdm_amd.metrics import MetricComputation
    names = ["delta1", "delta2", "delta3", "mse", "mae", "log10", "absrel", "sqrel", "rmse"]
    mc = MetricComputation(names)
    rows = np.array([[16384, 5461, 10000, 16383, 100.0, 50.0, 25.0, 12.5, 6.25, 3.0],
                     [3, 1, 2, 3, 0.3, 0.6, 0.9, 1.2, 1.5, 1.8]])
    vals = mc.values_from_rows(rows)
    assert len(vals) == 2 and all(isinstance(v, float) for v in vals[0])
    for r, v in zip(rows, vals):
        for k in range(3):                                            # an integer count divided in float32
            assert v[k] == float(np.float32(r[1 + k]) / np.float32(r[0]))
        for k in range(6):                                            # float64 sums over the float64 count
            assert v[3 + k] == r[4 + k] / r[0]
    assert vals[1][0] != 1 / 3 and vals[1][1] != 2 / 3                 # float32, not float64, quotients
    assert mc.values_from_rows(torch.from_numpy(rows)) == vals
    # a subset, in the caller's order
    assert MetricComputation(["rmse", "delta2"]).values_from_rows(rows[1:]) == [[1.8 / 3, float(np.float32(2) / np.float32(3))]]
    with pytest.raises(AssertionError):
        mc.values_from_rows(np.zeros((1, 10)))                        # "invalid target!": no valid pixel


@pytest.mark.parametrize("tag,shape", [("a", (4, 1, 128, 128)), ("b", (1, 1, 8, 8))])
def test_values_from_rows_against_the_reference_metric_fixture(tag, shape):
    """tests/golden/metric_goldens.npz holds the reference's own MetricComputation values (metrics.py:48-128) on hash-generated maps (as
    tests/test_oracle_ops.py regenerates them).  A row of sums formed on the host from the same maps must come out as those values: the
    deltas EQUAL (a float32 division of an exact count, as the reference's `.float().mean()`), the others within 1e-12 (another summation order)."""
    from md_rdm_amd import filler
    from md_rdm_amd.metrics import MetricComputation
    G = np.load(os.path.join(GOLDEN, "metric_goldens.npz"), allow_pickle=False)
    names = [str(n) for n in G["names"]]
    pred = filler.uniform(f"met.p.{tag}", shape, -0.5, 3.0).astype(np.float64)
    tgt = filler.log_uniform(f"met.t.{tag}", shape, 0.2, 4.0).astype(np.float64)
    tgt.flat[::7] = 0.0
    m = tgt > 0
    p, t = np.maximum(pred, 1e-7)[m], tgt[m]
    r, d = np.maximum(p / t, t / p), p - t
    row = np.array([m.sum(), (r < 1.25).sum(), (r < 1.25 ** 2).sum(), (r < 1.25 ** 3).sum(), (d * d).sum(), np.abs(d).sum(),
                    np.abs(np.log10(p) - np.log10(t)).sum(), (np.abs(d) / t).sum(), (d * d / t).sum(), np.sqrt(d * d / t).sum()], dtype=np.float64)
    got = MetricComputation(names).values_from_rows(row[None])[0]
    want = G[f"metrics_{tag}_float64"]
    for k, name in enumerate(names):
        if name.startswith("delta"):
            assert got[k] == want[k], name
        else:
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, err_msg=name)


class StubDataset:
    """What PrefetchLoader reads of a dataset before the first batch: length, split, resize, output size."""
    split, resize, output_size = "val", 250, (226, 226)

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def get_raw(self, i):
        raise AssertionError("no sample is read before a batch is requested")


def test_prefetch_loader_indices_shard_without_dropping(monkeypatch):
    from md_rdm_amd.dataloaders import PrefetchLoader
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a CUDA stream before the first batch")))
    flat = lambda bs: [int(i) for b in bs for i in b]
    # indices=None: today's order - equal shards, the remainder dropped
    for world in (1, 2, 3):
        seen = []
        for r in range(world):
            ld = PrefetchLoader(StubDataset(11), 4, device="cpu", drop_last=False, rank=r, world=world)
            got = flat(ld.batch_indices())
            assert got == list(range(11))[:11 // world * world][r::world]
            assert len(ld) == len(ld.batch_indices())
            seen += got
        assert sorted(seen) == list(range(11 // world * world))
    ld = PrefetchLoader(StubDataset(11), 4, device="cpu", drop_last=True)
    assert [len(b) for b in ld.batch_indices()] == [4, 4] and len(ld) == 2
    # a shuffling loader: the same permutation on every rank, disjoint shards (unchanged)
    a = PrefetchLoader(StubDataset(12), 4, shuffle=True, seed=5, device="cpu", drop_last=False, rank=0, world=2).batch_indices()
    b = PrefetchLoader(StubDataset(12), 4, shuffle=True, seed=5, device="cpu", drop_last=False, rank=1, world=2).batch_indices()
    perm = np.random.default_rng(5).permutation(12)
    assert flat(a) == [int(i) for i in perm[0::2]] and flat(b) == [int(i) for i in perm[1::2]]
    # indices=[...]: r::world, nothing dropped, unequal shards, never shuffled
    idx = [9, 0, 3, 7, 1, 10, 4]
    for world in (1, 2, 3, 4):
        seen = []
        for r in range(world):
            ld = PrefetchLoader(StubDataset(11), 2, shuffle=True, device="cpu", drop_last=False, rank=r, world=world, indices=idx)
            got = flat(ld.batch_indices())
            assert got == idx[r::world]
            assert all(len(b) <= 2 for b in ld.batch_indices()) and len(ld) == len(ld.batch_indices()) == (len(got) + 1) // 2
            seen += got
        assert sorted(seen) == sorted(idx)
    from md_rdm_amd import evaluate
    assert [evaluate.shard(range(7), r, 3) for r in range(3)] == [[0, 3, 6], [1, 4], [2, 5]]


def test_mean_over_shards_is_the_global_mean():
    from md_rdm_amd.metrics import mean_over_shards
    vals = np.array([[0.5, 2.0], [0.25, 4.0], [1.0, 8.0], [0.75, 16.0], [0.125, 32.0]])       # five samples, two metrics
    for world in (1, 2, 3, 5):
        shards = [(vals[r::world].sum(axis=0), len(vals[r::world])) for r in range(world)]       # unequal shards at world 2, 3
        means, n = mean_over_shards(shards)
        assert n == 5
        np.testing.assert_allclose(means, vals.mean(axis=0), rtol=1e-15)
    # the mean of the per-rank means is NOT that when the shards differ in size
    per_rank = np.mean([vals[r::2].mean(axis=0) for r in range(2)], axis=0)
    assert abs(per_rank[1] - vals.mean(axis=0)[1]) > 1e-3
    with pytest.raises(ValueError):
        mean_over_shards([([0.0], 0)])
