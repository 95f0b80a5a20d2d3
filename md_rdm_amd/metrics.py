"""``metrics.py`` of the reference (MetricLogger / MetricComputation, :13-128) without Lightning: all
metrics of one prediction come out of ONE fused kernel (`rdm_depth_metrics_f64`); under data parallelism
the per-pixel sums and the valid-pixel count are all-reduced before the division, so every rank reports the
global value (the reference logs per-rank values, `self.log` without sync_dist - SURVEY.md 2.1-C).
Batched evaluation (harness.evaluate) goes through `compute_rows` / `values_from_rows`: one launch per batch from the raw depth and the
predicted map to one row of sums per sample (`rdm_eval_target_metrics_f64`), read on the host once."""
import torch
import torch.distributed as dist

from . import _lib

# name -> (index into the kernel's sums, post-processing)
_SLOTS = {"delta1": 1, "delta2": 2, "delta3": 3, "mse": 4, "mae": 5, "log10": 6, "absrel": 7, "sqrel": 8,
          "rmse": 9}          # NB 'rmse' is the reference's RelativeMeanSquareError: mean sqrt((p-t)^2/t) (metrics.py:107-110,128)


def mean_over_shards(shards):
    """[(per-metric sums of the per-sample values, sample count), ...], one entry per rank -> (means over ALL samples, total count).  What
    the single all-reduce of a sharded evaluation computes (harness.evaluate): shards of unequal size weigh by their counts."""
    shards = list(shards)
    n = sum(int(c) for _, c in shards)
    if n <= 0:
        raise ValueError("mean_over_shards: no samples")
    width = len(shards[0][0])
    return [sum(float(s[i]) for s, _ in shards) / n for i in range(width)], n


class MetricComputation:
    def __init__(self, metrics):
        for m in metrics:
            if m not in _SLOTS:
                raise KeyError(f"metric '{m}' is not built (available: {sorted(_SLOTS)})")
        self.names = list(metrics)
        self.reset()

    def reset(self):
        self.count = 0
        self.sum = [0.0 for _ in self.names]

    def compute(self, pred, target, sync=True):
        if not pred.is_cuda:
            raise _lib.RdmError("metrics run on the GPU only")
        p = pred.detach().double().contiguous()
        t = target.detach().double().contiguous()
        out = torch.empty(10, dtype=torch.float64, device=p.device)
        _lib.check(_lib.lib().rdm_depth_metrics_f64(_lib.ptr(p), _lib.ptr(t), p.numel(), _lib.ptr(out), _lib.stream()))
        if sync and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(out)
        out = out.cpu()
        assert out[0] > 0, "invalid target!"
        # delta1-3 are float32 in the reference: `(maxRatio < 1.25 ** k).float().mean()` (metrics.py:79-89) - an exact integer count
        # divided in float32; the other metrics stay in the dtype of the inputs (float64 from validation_step)
        n = float(out[0])
        values = [float(torch.tensor(float(out[_SLOTS[m]]), dtype=torch.float32) / n) if m.startswith("delta") else float(out[_SLOTS[m]]) / n
                  for m in self.names]
        self.count += 1
        for i, v in enumerate(values):
            self.sum[i] += v
        return values

    def compute_rows(self, pred, depth, exp_pred=False, target_out=None, gm_out=None):
        """Batched evaluation in ONE launch (`rdm_eval_target_metrics_f64`): the (B,1,128,128) float64 map ``predict`` returns and the loader's
        raw (B,1,H,W) float32 / float64 depth -> the (B,10) float64 DEVICE tensor of per-sample metric sums; target preparation
        (harness.prepare_target), normalisation (harness.normalize) and the sums of ``compute`` happen inside.  Nothing is copied to the host
        and nothing synchronises: ``values_from_rows`` reads the rows once they have been brought over.
        ``exp_pred``: compare ``exp(pred)`` instead of the log-domain map - NOT what the reference does (module.py:117).
        ``target_out`` (B,1,128,128) / ``gm_out`` (B) float64: optionally receive the normalised target and the geometric means."""
        if not pred.is_cuda or not depth.is_cuda:
            raise _lib.RdmError("metrics run on the GPU only")
        if pred.dim() != 4 or tuple(pred.shape[1:]) != (1, 128, 128) or pred.dtype != torch.float64:
            raise _lib.RdmError("compute_rows: pred must be the (B,1,128,128) float64 map of DepthEstimationNet.predict, got %s %s" % (pred.dtype, tuple(pred.shape)))
        if depth.dim() != 4 or depth.shape[0] != pred.shape[0] or depth.shape[1] != 1 or depth.dtype not in (torch.float32, torch.float64):
            raise _lib.RdmError("compute_rows: depth must be (B,1,H,W) float32 or float64 with pred's B, got %s %s" % (depth.dtype, tuple(depth.shape)))
        B, _, H, W = depth.shape
        p, d = pred.detach().contiguous(), depth.detach().contiguous()
        rows = torch.empty(B, 10, dtype=torch.float64, device=p.device)
        _lib.check(_lib.lib().rdm_eval_target_metrics_f64(_lib.ptr(p), _lib.ptr(d), int(d.dtype == torch.float64), B, H, W, _lib.ptr(rows), _lib.ptr(target_out),
                                                          _lib.ptr(gm_out), 1 if exp_pred else 0, _lib.stream()))
        return rows

    def values_from_rows(self, rows):
        """(N,10) rows of metric sums (``compute_rows``, on the host or not) -> N lists of this computer's metric values, with ``compute``'s
        conventions: delta1..3 are the integer count divided in float32, the others are float64 sums over the float64 count."""
        r = torch.as_tensor(rows).detach().to("cpu", torch.float64).reshape(-1, 10)
        assert bool((r[:, 0] > 0).all()), "invalid target!"
        cols = [(r[:, _SLOTS[m]].float() / r[:, 0].float()).double() if m.startswith("delta") else r[:, _SLOTS[m]] / r[:, 0] for m in self.names]
        return [[float(c[i]) for c in cols] for i in range(r.shape[0])]

    def avg(self, metric):
        if isinstance(metric, int):
            return self.sum[metric] / self.count
        return self.sum[self.names.index(metric)] / self.count


class MetricLogger:
    """log_train / log_val / log_test return the dicts the reference returns; `records` replaces self.log."""

    def __init__(self, metrics, module=None):
        self.context = module
        self.computer = MetricComputation(metrics)
        self.records = []

    def _log(self, prefix, pred, target, extra=None):
        values = self.computer.compute(pred, target)
        result = dict(extra or {})
        for name, value in zip(self.computer.names, values):
            result[name] = value
            self.records.append((f"{prefix}{name}", value))
        return result

    def log_train(self, pred, target, loss):
        return self._log("train_", pred, target, {"loss": loss})

    def log_val(self, pred, target):
        return self._log("val_", pred, target)

    def log_test(self, pred, target):
        return self._log("", pred, target)

    def reset(self):
        self.computer.reset()
