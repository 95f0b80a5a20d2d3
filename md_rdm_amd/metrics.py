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


# the standard protocol (include/rdm_eval.h): name -> how the value is formed from a row of rdm_eval_standard_f64
_STANDARD = ("delta1", "delta2", "delta3", "abs_rel", "sq_rel", "rmse", "rmse_log", "silog", "log10", "mae", "scale")
STANDARD_COLS = 16
EIGEN_CROP = (45, 41, 471, 601)                                       # NYU, of the 480x640 frame: rows [45, 471), columns [41, 601)
GARG_CROP = (0.40810811, 0.03594771, 0.99189189, 0.96405229)          # KITTI: y0, x0, y1, x1 as fractions of H, W, H, W
NAMED_CROPS = ("eigen", "garg")


def named_crop(name, H, W):
    """A crop of the published protocols as (y0, x0, y1, x1) of an (H, W) depth frame.  ``"eigen"``: the NYU crop of Eigen et al.,
    (45, 41, 471, 601), defined for the 480x640 frame only - any other size raises.  ``"garg"``: the KITTI crop of Garg et al., the fractions
    0.40810811 / 0.99189189 of H and 0.03594771 / 0.96405229 of W; each product is TRUNCATED to an integer (``int()``, as the usual evaluation
    scripts' ``astype(int32)`` does; the products are positive, so this is the floor): 352x1216 -> (143, 43, 349, 1172)."""
    if name == "eigen":
        if (H, W) != (480, 640):
            raise ValueError(f"crop 'eigen' is the NYU crop of the 480x640 frame; the depth is {H}x{W}")
        return EIGEN_CROP
    if name == "garg":
        f = GARG_CROP
        return (int(f[0] * H), int(f[1] * W), int(f[2] * H), int(f[3] * W))
    raise ValueError(f"crop '{name}' is not one of {NAMED_CROPS}")



class StandardMetrics:
    """The evaluation protocol of the published depth-estimation tables (Eigen et al.), beside the reference's (``MetricComputation``): linear
    depth ``exp(map)`` at the ground truth's OWN resolution, valid pixels only (finite, ``min_depth < d < max_depth``, inside ``crop`` =
    (y0, x0, y1, x1) when given), a per-image scale ``align``-ment (``"median"``: median(d) / median(p); ``"logmean"``: exp(mean ln d - mean ln p);
    ``"none"``), the aligned prediction clamped to [min_depth, max_depth], then per image

      delta1..3  share of pixels with max(q/d, d/q) < 1.25^k (a float64 quotient)     abs_rel  mean |q-d|/d          sq_rel  mean (q-d)^2/d
      rmse       sqrt(mean (q-d)^2)                                                  rmse_log sqrt(mean (ln q - ln d)^2)
      silog      100 sqrt(max(mean g^2 - (mean g)^2, 0)), g = ln q - ln d            log10    mean |log10 q - log10 d|   mae  mean |q-d|
      scale      the alignment scale s

    NB ``rmse`` here is the TRUE root mean square.  It is not the reference's metric of the same name (``MetricComputation``'s 'rmse' is the
    reference's mean sqrt((p-t)^2/t), metrics.py:107-110), and none of these figures is comparable with the reference protocol's.
    ``compute_rows`` is one launch per batch (``rdm_eval_standard_f64``); ``values_from_rows`` forms the values on the host.
    ``crop`` may also name a published crop, ``"eigen"`` (NYU) or ``"garg"`` (KITTI): it resolves when the depth's shape is known (``named_crop``).
    ``view`` = (vy0, vx0, vh, vw): the rectangle of the depth frame, in depth pixels, that the predicted map covers (include/rdm_eval_view.h;
    ``dataloaders.nyu.test_view`` for raw NYU depth); None: the map covers the whole frame.  Depth pixels outside the view are scored against
    the map's replicated edge.  The attribute may be set between batches."""

    available = _STANDARD

    def __init__(self, names=None, align="median", min_depth=1e-3, max_depth=10.0, crop=None, view=None):
        names = list(_STANDARD) if names is None else list(names)
        for m in names:
            if m not in _STANDARD:
                raise KeyError(f"metric '{m}' is not built in the standard protocol (available: {sorted(_STANDARD)})")
        if align not in _lib.EVAL_ALIGN:
            raise ValueError(f"align '{align}' is not one of {sorted(_lib.EVAL_ALIGN)}")
        if not (0 <= float(min_depth) < float(max_depth)):
            raise ValueError(f"need 0 <= min_depth < max_depth, got {min_depth}, {max_depth}")
        if isinstance(crop, str):
            if crop not in NAMED_CROPS:
                raise ValueError(f"crop '{crop}' is not one of {NAMED_CROPS}")
        elif crop is not None:
            crop = tuple(int(c) for c in crop)
            if len(crop) != 4 or not (0 <= crop[0] < crop[2] and 0 <= crop[1] < crop[3]):
                raise ValueError(f"crop must be (y0, x0, y1, x1) with 0 <= y0 < y1 and 0 <= x0 < x1, got {crop}")
        self.names, self.align, self.min_depth, self.max_depth, self.crop = names, align, float(min_depth), float(max_depth), crop
        self.view = view

    @property
    def view(self):
        return self._view

    @view.setter
    def view(self, view):
        import math
        if view is not None:
            view = tuple(float(v) for v in view)
            if len(view) != 4 or not all(math.isfinite(v) for v in view) or not (view[2] > 0 and view[3] > 0):
                raise ValueError(f"view must be (vy0, vx0, vh, vw), finite with vh > 0 and vw > 0, got {view}")
        self._view = view

    def resolve_crop(self, H, W):
        """the crop of an (H, W) depth frame as (y0, x0, y1, x1), or None: a named crop becomes its integers here"""
        return named_crop(self.crop, H, W) if isinstance(self.crop, str) else self.crop

    def compute_rows(self, pred, depth, pred_out=None):
        """The (B,1,128,128) float64 log map ``predict`` returns and the loader's raw (B,1,H,W) float32 / float64 depth -> the (B,16) float64
        DEVICE tensor of per-sample sums (columns: include/rdm_eval.h).  One launch, nothing is copied to the host and nothing synchronises.
        ``pred_out`` (B,1,H,W) float64: optionally receives the aligned, clamped prediction at every pixel.
        With a ``view`` the launch is ``rdm_eval_standard_view_f64``, without one ``rdm_eval_standard_f64``."""
        import ctypes as C
        if not pred.is_cuda or not depth.is_cuda:
            raise _lib.RdmError("metrics run on the GPU only")
        if pred.dim() != 4 or tuple(pred.shape[1:]) != (1, 128, 128) or pred.dtype != torch.float64:
            raise _lib.RdmError("compute_rows: pred must be the (B,1,128,128) float64 map of DepthEstimationNet.predict, got %s %s" % (pred.dtype, tuple(pred.shape)))
        if depth.dim() != 4 or depth.shape[0] != pred.shape[0] or depth.shape[1] != 1 or depth.dtype not in (torch.float32, torch.float64):
            raise _lib.RdmError("compute_rows: depth must be (B,1,H,W) float32 or float64 with pred's B, got %s %s" % (depth.dtype, tuple(depth.shape)))
        if pred_out is not None and (pred_out.dtype != torch.float64 or tuple(pred_out.shape) != tuple(depth.shape) or not pred_out.is_cuda):
            raise _lib.RdmError("compute_rows: pred_out must be a float64 device tensor of depth's shape, got %s %s" % (pred_out.dtype, tuple(pred_out.shape)))
        B, _, H, W = depth.shape
        p, d = pred.detach().contiguous(), depth.detach().contiguous()
        L = _lib.lib()
        need = L.rdm_eval_standard_workspace_bytes(B, H, W)
        ws = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=p.device)
        rows = torch.empty(B, STANDARD_COLS, dtype=torch.float64, device=p.device)
        crop = self.resolve_crop(H, W)
        crop = (C.c_int32 * 4)(*crop) if crop is not None else None
        if self.view is not None:
            _lib.check(L.rdm_eval_standard_view_f64(_lib.ptr(p), _lib.ptr(d), int(d.dtype == torch.float64), B, H, W, _lib.EVAL_ALIGN[self.align], self.min_depth,
                                                    self.max_depth, crop, (C.c_double * 4)(*self.view), _lib.ptr(rows), _lib.ptr(pred_out), _lib.ptr(ws),
                                                    ws.numel() * 8, _lib.stream()))
        else:
            _lib.check(L.rdm_eval_standard_f64(_lib.ptr(p), _lib.ptr(d), int(d.dtype == torch.float64), B, H, W, _lib.EVAL_ALIGN[self.align], self.min_depth,
                                               self.max_depth, crop, _lib.ptr(rows), _lib.ptr(pred_out), _lib.ptr(ws), ws.numel() * 8, _lib.stream()))
        return rows

    def values_from_rows(self, rows):
        """(N,16) rows (``compute_rows``, on the host or not) -> N entries: the list of this computer's metric values in float64, or None for a
        sample without a valid pixel (n = 0), which the caller leaves out of its means."""
        import math
        r = torch.as_tensor(rows).detach().to("cpu", torch.float64).reshape(-1, STANDARD_COLS).tolist()
        out = []
        for row in r:
            n = row[0]
            if not n > 0:
                out.append(None)
                continue
            g2, g1 = row[7] / n, row[8] / n
            var = g2 - g1 * g1
            v = {"delta1": row[1] / n, "delta2": row[2] / n, "delta3": row[3] / n, "abs_rel": row[4] / n, "sq_rel": row[5] / n,
                 "rmse": math.sqrt(row[6] / n) if row[6] == row[6] else float("nan"), "rmse_log": math.sqrt(g2) if g2 == g2 else float("nan"),
                 "silog": 100.0 * math.sqrt(max(var, 0.0)) if var == var else float("nan"), "log10": row[9] / n, "mae": row[10] / n, "scale": row[11]}
            out.append([v[m] for m in self.names])
        return out


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
