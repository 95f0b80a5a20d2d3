"""The training/validation step of the reference's Lightning module (network/module.py:49-149),
restated without Lightning so that it runs on this stack: same target preparation, same loss sum,
AdamW(lr) as in ``configure_optimizers`` (:38-47).  ``train.py``'s flags are mirrored in
md_rdm_amd/train.py."""
import ctypes as C

import torch

from . import loss as l
from . import utils as u
from .network import computations as cp
from .network.RDM_Net import DepthEstimationNet


def normalize(batch):
    """module.py:145-149: divide by the geometric mean, exponent 1/H**2 (quick_gm squares its arg)."""
    B, C, H, W = batch.size()
    return cp.gm_normalize(batch, 1.0 / (H * H))


def prepare_target(y):
    """module.py:68,75-78: bicubic to 128x128, invalid pixels -> 1e-4."""
    y = cp.resize(y, 128)
    mask1 = y > 0
    mask2 = (y <= 0) + 1e-4
    return (y * mask1) + mask2


def compute_final_depth(fine_detail_list, target, has_ordinal):
    """module.py:119-133."""
    component_target = cp.decompose_depth_map([], normalize(target), 7)[::-1]
    if has_ordinal:
        ord_components = cp.decompose_depth_map([], normalize(u.depth2label_sid(cp.resize(target, 8), cuda=True)), 3)[::-1]
        component_target[0] = ord_components[0]
    components, loss = cp.optimize_components(fine_detail_list, component_target, True)
    final = cp.recombination(components)
    return final, loss


def compute_ordinal_target(ord_pred, target):
    """module.py:135-143; for non-square head outputs (where the reference raises) the target is
    resized to the head's (h, w)."""
    h, w = ord_pred.shape[2], ord_pred.shape[3]
    target = cp.resize(target, h if h == w else (h, w))
    return u.depth2label_sid(target, cuda=True)


def training_step(model, x, y):
    """module.py:64-97 without logging.  Returns (loss_all, dict of components)."""
    y = prepare_target(y)
    fine_details, ord_depth_pred, ord_label_pred = model(x)
    has_ordinal = fine_details[0].shape[2] == 1
    y_hat = list(fine_details)                      # recombination pops from the list it is given (computations.py:405-407)
    final_depth, fine_detail_loss = compute_final_depth(fine_details, y, has_ordinal=has_ordinal)
    ord_y = compute_ordinal_target(ord_depth_pred, y)
    ord_loss = l.Ordinal_Loss().calc(ord_label_pred, ord_y, cuda=True)
    mse = torch.nn.functional.mse_loss(final_depth, y)
    loss_all = mse + fine_detail_loss + ord_loss
    return loss_all, dict(mse=mse, fine_detail_loss=fine_detail_loss, ord_loss=ord_loss, final_depth=final_depth, y=y, ord_y=ord_y,
                          fine_details=y_hat, ord_depth_pred=ord_depth_pred, ord_label_pred=ord_label_pred)


def validation_step(model, x, y):
    """module.py:99-117: returns (y_hat, normalized target)."""
    y = prepare_target(y)
    fine_details, _, _ = model(x)
    has_ordinal = fine_details[0].shape[2] == 1
    y_hat, _ = compute_final_depth(fine_details, y, has_ordinal=has_ordinal)
    return y_hat, normalize(y)


def evaluate(model, batches, metrics, exp_pred=False, return_maps=False, rows_out=None, rows_max=16, flip=False, scale=None, sid="nyu", sid_offset=0.0):
    """Score a model on an iterable of (x, raw depth) batches of ANY batch size: per batch ``model.predict(x)`` and ONE launch from the map and
    the raw depth to a row of metric sums per sample (``MetricComputation.compute_rows``); the rows stay on the device and come over in one
    copy after the last batch.  The result, {metric: mean over the samples of the per-sample value, "n": samples}, is what the reference's
    batch-1 validation with Lightning's epoch mean reports (module.py:99-117; ``validation_step`` + ``MetricLogger.log_val`` here), whatever
    the batch size: ``validation_step``'s prediction does not depend on the target (optimize_components returns its predictions unchanged),
    so it is ``predict``'s map.  ``metrics``: a MetricComputation or a list of metric names.  Under an initialised process group every rank
    passes its own shard (unequal shards are fine) and one all-reduce of the per-metric sums and the count makes the result global.
    ``exp_pred``: compare exp(map) - not what the reference does.  ``return_maps``: also return the (n,1,128,128) maps of this rank.
    ``rows_out``: a list that receives, for the first ``rows_max`` samples of this rank, the (H,3W,3) uint8 host image input | normalised target
    (``compute_rows``' target_out) | the map the metrics saw (exp of it under ``exp_pred``), rendered on the device in one launch per batch
    (viz.comparison_rows) and copied over once per batch.
    ``metrics`` may also be a ``metrics.StandardMetrics``: the standard protocol (linear depth at the depth's own resolution, valid pixels, scale
    alignment, the Eigen et al. error set; include/rdm_eval.h), again ``predict`` + ONE launch per batch with the rows kept on the device.  The
    result is the mean over the samples of the per-sample values (the per-image averaging of the NYU / KITTI protocols); samples without a
    valid pixel are left out of the means and counted in ``"skipped"``; if every sample is skipped it raises.  ``rows_out`` then shows
    input | raw depth | the aligned, clamped prediction over one colour range.  ``exp_pred`` does not apply.  A StandardMetrics with a ``view``
    scores depth of which the network saw a part (``PrefetchLoader(native_depth=True)``: the raw frame and ``loader.view``).
    ``flip``: every map is ``model.predict(x, flip=True)``, the mirror test-time augmentation of the published tables (two passes per batch).
    ``scale="sid"`` (standard protocol only; the reference protocol compares normalised maps): ``predict`` also hands over the DORN counts, and
    ``depth.sid_log_scale(counts, sid, sid_offset)`` is added to every log map before the metrics launch, so ``StandardMetrics(align="none")``
    scores metric predictions; ``return_maps`` then returns the shifted maps.  None leaves every path as it was."""
    import torch.distributed as dist
    from .metrics import MetricComputation, StandardMetrics, mean_over_shards
    standard = isinstance(metrics, StandardMetrics)
    if standard and exp_pred:
        raise ValueError("evaluate: exp_pred belongs to the reference protocol; the standard protocol always compares linear depth")
    if scale not in (None, "sid"):
        raise ValueError("evaluate: scale must be None or 'sid', got %r" % (scale,))
    if scale is not None and not standard:
        raise ValueError("evaluate: scale='sid' belongs to the standard protocol; the reference protocol compares maps normalised by their geometric mean")
    mc = metrics if isinstance(metrics, (MetricComputation, StandardMetrics)) else MetricComputation(list(metrics))
    rows, maps = [], []
    for x, y in batches:
        if scale is not None:
            from . import depth
            pred, counts = model.predict(x, return_counts=True, flip=flip)
            pred = pred + depth.sid_log_scale(counts, sid, sid_offset).reshape(-1, 1, 1, 1)
        else:
            pred = model.predict(x, flip=True) if flip else model.predict(x)
        want = rows_out is not None and len(rows_out) < rows_max
        if standard:
            tgt = torch.empty(y.shape, dtype=torch.float64, device=pred.device) if want else None      # q, at the depth's resolution
            rows.append(mc.compute_rows(pred, y, pred_out=tgt))
        else:
            tgt = torch.empty_like(pred) if want else None
            rows.append(mc.compute_rows(pred, y, exp_pred=exp_pred, target_out=tgt))
        if want:
            from . import viz
            k = min(x.shape[0], rows_max - len(rows_out))
            if standard:
                img = viz.comparison_rows(x[:k].float(), y[:k], tgt[:k])
            else:
                img = viz.comparison_rows(x[:k].float(), tgt[:k], (pred.exp() if exp_pred else pred)[:k])
            rows_out.extend(img.cpu().numpy())
        if return_maps:
            maps.append(pred)
    values = mc.values_from_rows(torch.cat(rows).cpu()) if rows else []          # the one device-to-host copy
    skipped = sum(1 for v in values if v is None)                                # standard protocol: samples without a valid pixel
    values = [v for v in values if v is not None]
    sums = [0.0] * len(mc.names)
    for v in values:                                                             # per-sample values summed in order, as MetricComputation.compute does
        for i, s in enumerate(v):
            sums[i] += s
    n = len(values)
    if dist.is_initialized() and dist.get_world_size() > 1:
        t = torch.tensor(sums + [float(n), float(skipped)], dtype=torch.float64, device=next(model.parameters()).device)
        dist.all_reduce(t)
        t = t.cpu()
        sums, n, skipped = [float(s) for s in t[:-2]], int(t[-2]), int(t[-1])
    if n == 0:
        raise ValueError("evaluate: no samples" if not skipped else "evaluate: none of the %d samples has a valid pixel" % skipped)
    means, n = mean_over_shards([(sums, n)])
    result = dict(zip(mc.names, means), n=n)
    if standard:
        result["skipped"] = skipped
    return (result, torch.cat(maps)) if return_maps else result


def ema_decay_at(decay, updates, warmup=True):
    """The decay of the weight average's next update after ``updates`` updates: ``decay``, or with ``warmup`` min(decay, (1 + u) / (10 + u))
    (0.1, 2/11, 3/12, ... until ``decay`` takes over), so that a young average follows the weights instead of its seed.  Formed in float64 and
    rounded once to float32, the value the kernel receives."""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + updates) / (10.0 + updates))
    return C.c_float(d).value


class FusedAdamW:
    """torch.optim.AdamW(lr) semantics (module.py:41) as one launch per contiguous TRAINABLE range of the model's flat parameter /
    gradient buffers (2 for the reference's live graph) + a tiny torch step for the 4 Weights scalars.

    Gradient accumulation (Lightning's ``accumulate_grad_batches``): a window of k micro-batches is k backward passes with
    ``accumulate_grad()`` after each but the last and ``step()`` after the last; ``zero_grad()`` opens the window.  The backward pass
    overwrites the flat gradient buffer, so the running sum lives in a buffer of its own (allocated on first use, like the moments):
    ``accumulate_grad()`` is acc = g after the first micro-batch and acc += g after the later ones, over the trainable ranges; the last
    micro-batch's gradient gets g += acc just before the update, so the step reads the gradient buffer as it always does.  ``step``
    applies 1/k for the k micro-batches actually seen (a partial window at the end of an epoch divides by what it holds).  The four
    ``weight_layer`` scalars accumulate in their ``.grad``, as torch does.  BatchNorm running statistics are updated by EVERY micro-batch's
    forward, as under Lightning: k micro-batches of B are k momentum updates with statistics over B samples, not one over k B.
    Data parallel: the backward of a non-final micro-batch runs inside ``no_sync()`` and issues no collective (DDP's ``no_sync``); the final
    one adds the accumulator per stage slice inside the stage hook, before that stage's reduction is issued (``attach_sync(sync)`` installs that
    hook and must be called before the window's first backward pass), and the scale is 1/(k world).

    ``clip`` (Lightning's ``gradient_clip_val``; None = off): clip by the global 2-norm of the scaled gradient, as
    ``torch.nn.utils.clip_grad_norm_`` on every trainable tensor would.  One sum of squares per trainable range (rdm_grad_sumsq_f64) into
    consecutive float64 slots, one more slot for the ``weight_layer`` gradients; the update is rdm_adamw_fused_clip, whose threads form the
    coefficient from the slots themselves, and the small gradients are multiplied by the coefficient that kernel wrote.  Nothing is read
    by the host: ``last_grad_norm`` (the norm before clipping) is a device scalar, and reading it is the caller's synchronisation.  Data
    parallel: the norm must be the reduced gradient's, so clipping waits for every stage (``finish()``) and updates after the last one;
    with the "reduce_scatter" exchange a rank holds only its shard of the sum, and ``step`` raises.

    ``ema_decay`` (None = off: the launches, the state and the buffers of before): an exponential moving average of the weights,
    ema += (1 - d)(w - ema) once per optimiser step (so once per accumulation window) with d = ``ema_decay_at(ema_decay, ema_updates,
    ema_warmup)``.  ``ema`` is a flat float32 buffer like the moments, seeded at the first ``step()`` with the weights of before that step's
    update (equal on every data-parallel rank) and advanced by the AdamW launch itself (rdm_adamw_fused_ema, clipped or not: the weight it
    has just formed is still in registers), so every path through ``_update`` carries it; parameter and moment bytes are those of the step
    without the average.  The four ``weight_layer`` scalars get float32 averages of their own (``ema_small``), updated in torch.  What this
    optimiser does not update is not averaged: the relative decoders d_6..d_10 and ``d_1.conv1.*`` are used as they are, and so are the
    BatchNorm running statistics - the averaged weights run with the LIVE statistics, the ``use_buffers=False`` behaviour of
    ``torch.optim.swa_utils.AveragedModel``.  ``swap_ema()`` exchanges weights and average in place (one rdm_ema_swap_f32 launch per trainable
    range, no third buffer); ``with opt.ema_weights():`` does it on entry and again on exit, and inside it ``model.state_dict()``,
    ``forward``, ``predict`` and ``evaluate`` see the averaged weights while ``step()`` and ``state_dict()`` raise.  With the "reduce_scatter"
    exchange a rank advances the average of the ranges it owns, and ``ema`` is all-gathered where the moments are: in ``state_dict()`` and
    before a swap - collectives, so every rank must get there."""

    def __init__(self, model: DepthEstimationNet, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, clip=None, ema_decay=None, ema_warmup=True):
        self.model, self.lr, self.betas, self.eps, self.wd = model, lr, betas, eps, weight_decay
        self.step_count = 0
        self.m = self.v = None
        self.sync, self.mode = None, "after the last stage"        # data parallel: set by step(sync=...)
        self.small = torch.optim.AdamW([p for p in model.weight_layer.parameters() if p.requires_grad], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        if clip is not None and not float(clip) >= 0.0:
            raise ValueError(f"FusedAdamW: clip must be None or a non-negative norm (got {clip!r})")
        self.clip = clip
        self.acc = None                                            # the running gradient sum of an accumulation window
        self.micro = 0                                             # micro-batches held by acc
        self.last_grad_norm = None                                 # device scalar (float64): the global norm the last clipped step saw
        self._folded = self._no_sync = False
        self._hooked = None
        self._slots = self._coef = self._sumsq_ws = None
        if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError(f"FusedAdamW: ema_decay must be None or lie in [0, 1] (got {ema_decay!r})")
        self.ema_decay, self.ema_warmup = None if ema_decay is None else float(ema_decay), bool(ema_warmup)
        self.ema = self.ema_small = None                           # the averages: allocated at the first step, only when ema_decay is set
        self.ema_updates = 0
        self._ema_d = 1.0                                          # this step's decay (ema_decay_at), set by step()
        self._ema_swapped = False

    def zero_grad(self):
        """Opens a window: clears the ``weight_layer`` gradients and forgets whatever the accumulator holds."""
        self.small.zero_grad(set_to_none=True)
        self.micro, self._folded = 0, False

    # ---- gradient accumulation ----
    def _accumulate(self, dst, src, a, b, mode):
        """dst = src (mode 0) / dst += src (mode 1) on the trainable parts of the flat element range [a, b)"""
        from . import _lib
        L, st = _lib.lib(), _lib.stream()
        for ta, tb in self.trainable_ranges():
            lo, hi = max(a, ta), min(b, tb)
            if lo < hi:
                _lib.check(L.rdm_grad_accumulate_f32(C.c_void_p(dst.data_ptr() + 4 * lo), C.c_void_p(src.data_ptr() + 4 * lo), hi - lo, mode, st))

    def accumulate_grad(self):
        """After the backward pass of a micro-batch that is NOT the last of its window: the flat gradient joins the accumulator."""
        from . import _lib
        flat, gflat, _ = self.model._flat
        if self.acc is None or self.acc.numel() != gflat.numel() or self.acc.device != gflat.device:
            self.acc = torch.zeros_like(gflat)
        self._accumulate(self.acc, gflat, 0, gflat.numel(), _lib.GRAD_ACC_COPY if self.micro == 0 else _lib.GRAD_ACC_ADD)
        self.micro += 1

    def no_sync(self):
        """Context for the backward pass of a non-final micro-batch under data parallelism: the stage hook issues no collective."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            prev, self._no_sync = self._no_sync, True
            try:
                yield self
            finally:
                self._no_sync = prev
        return scope()

    def attach_sync(self, sync):
        """Put this optimiser's stage hook in front of the exchange's (``parallel.attach`` installed ``sync.on_stage``): silent inside
        ``no_sync()``, and on the window's last micro-batch it adds the accumulator to the stage's slice before the reduction is issued."""
        if sync is None or sync.world <= 1 or self._hooked is sync:
            return
        self.sync, self._hooked = sync, sync

        def hook(stage):
            if self._no_sync:
                return
            if self.micro:
                a, b = sync.slices[stage]
                self._accumulate(self.model._flat[1], self.acc, a, b, 1)
                self._folded = True
            sync.on_stage(stage)
        self.model.grad_ready_hook = hook

    def trainable_ranges(self):
        """Maximal contiguous [start, stop) element ranges of the flat buffer that hold tensors which receive a gradient.
        torch.optim.AdamW (the reference's optimiser) skips every parameter whose ``.grad is None``: ``d_1.conv1.*`` (constructed
        for every decoder, used only for id > 5, RDM_Net.py:146,156-157) and whatever ``freeze_encoder()`` froze (:65-67) must
        stay bit-unchanged - no weight decay, no moments.  Alignment padding between two trainable tensors is swept along
        (parameter, gradient and moments are all zero there and stay zero)."""
        _, _, entries = self.model._flat
        key = tuple(p.requires_grad for _, p, _, _, _ in entries)
        if getattr(self, "_ranges_key", None) != key:
            ranges = []
            for k, p, o, n, _ in entries:
                if not p.requires_grad or k.startswith("d_1.conv1."):
                    continue
                if ranges and ranges[-1][2] == o:                 # previous trainable tensor (padded to its 64-float slot) ends here
                    ranges[-1][1], ranges[-1][2] = o + n, o + (n + 63) // 64 * 64
                else:
                    ranges.append([o, o + n, o + (n + 63) // 64 * 64])
            self._ranges, self._ranges_key = [(a, b) for a, b, _ in ranges], key
        return self._ranges

    def _update(self, a, b, grad_scale, clip=None, n_slots=0):
        """AdamW on the trainable parts of the flat element range [a, b) (one launch per contiguous trainable piece); with ``clip`` the
        clipped step, its coefficient formed in the kernel from the first ``n_slots`` slots."""
        from . import _lib
        flat, gflat, _ = self.model._flat
        L, st = _lib.lib(), _lib.stream()
        off = C.c_void_p
        for ta, tb in self.trainable_ranges():
            lo, hi = max(a, ta), min(b, tb)
            if lo < hi and self.ema_decay is not None:            # either step, and the average from the weight it forms
                _lib.check(L.rdm_adamw_fused_ema(off(flat.data_ptr() + 4 * lo), off(gflat.data_ptr() + 4 * lo), off(self.m.data_ptr() + 4 * lo),
                                                 off(self.v.data_ptr() + 4 * lo), off(self.ema.data_ptr() + 4 * lo), hi - lo, self.lr, self.betas[0],
                                                 self.betas[1], self.eps, self.wd, self.step_count, float(grad_scale),
                                                 None if clip is None else _lib.ptr(self._slots), n_slots if clip is not None else 0,
                                                 0.0 if clip is None else float(clip), None if clip is None else _lib.ptr(self._coef), self._ema_d, st))
            elif lo < hi and clip is None:
                _lib.check(L.rdm_adamw_fused(off(flat.data_ptr() + 4 * lo), off(gflat.data_ptr() + 4 * lo), off(self.m.data_ptr() + 4 * lo),
                                             off(self.v.data_ptr() + 4 * lo), hi - lo, self.lr, self.betas[0], self.betas[1], self.eps, self.wd,
                                             self.step_count, float(grad_scale), st))
            elif lo < hi:
                _lib.check(L.rdm_adamw_fused_clip(off(flat.data_ptr() + 4 * lo), off(gflat.data_ptr() + 4 * lo), off(self.m.data_ptr() + 4 * lo),
                                                  off(self.v.data_ptr() + 4 * lo), hi - lo, self.lr, self.betas[0], self.betas[1], self.eps, self.wd,
                                                  self.step_count, float(grad_scale), _lib.ptr(self._slots), n_slots, float(clip), _lib.ptr(self._coef), st))

    def _norm_slots(self, grad_scale, small_grads):
        """Sum of squares of the UNSCALED flat gradient per trainable range into consecutive slots, one more slot for the small gradients
        (already final, so divided by grad_scale^2 to stand beside the others); sets ``last_grad_norm``.  -> the number of slots."""
        from . import _lib
        gflat = self.model._flat[1]
        L, st = _lib.lib(), _lib.stream()
        ranges = self.trainable_ranges()
        if len(ranges) + 1 > _lib.CLIP_MAX_SLOTS:
            raise _lib.RdmError(f"FusedAdamW(clip=...): {len(ranges)} trainable ranges + 1 exceed the {_lib.CLIP_MAX_SLOTS} norm slots of rdm_adamw_fused_clip")
        need = max(int(L.rdm_grad_sumsq_workspace_bytes(b - a)) for a, b in ranges)
        if self._slots is None or self._slots.device != gflat.device or self._sumsq_ws.numel() * 8 < need:
            self._slots = torch.zeros(_lib.CLIP_MAX_SLOTS, dtype=torch.float64, device=gflat.device)
            self._coef = torch.ones(1, dtype=torch.float32, device=gflat.device)
            self._sumsq_ws = torch.empty(need // 8, dtype=torch.float64, device=gflat.device)
        for i, (a, b) in enumerate(ranges):                        # (the launches of one stream run in order: the ranges share the workspace)
            _lib.check(L.rdm_grad_sumsq_f64(C.c_void_p(gflat.data_ptr() + 4 * a), b - a, C.c_void_p(self._slots.data_ptr() + 8 * i), _lib.ptr(self._sumsq_ws),
                                            self._sumsq_ws.numel() * 8, st))
        n = len(ranges)
        if small_grads:
            self._slots[n] = torch.stack([g.detach().double().square().sum() for g in small_grads]).sum() / (float(grad_scale) ** 2)
            n += 1
        self.last_grad_norm = self._slots[:n].sum().sqrt() * abs(float(grad_scale))
        return n

    @staticmethod
    def _scale_small(grads, factor):
        for g in grads:                                            # the weight_layer scalars: a handful of one-element launches
            g.mul_(factor)

    def step(self, grad_scale=1.0, sync=None, clip=None):
        """``sync`` = the GradSync of a data-parallel run: the update then runs PER BUCKET as each stage's reduction lands
        (``GradSync.finish(on_reduced=...)``: stage k's wait is a stream dependency and its AdamW launch follows at once, under the
        reductions still in flight; with the "reduce_scatter" exchange on this rank's shard only, the updated parameters are
        all-gathered).  Without it: the monolithic update of the whole buffer with the given ``grad_scale`` (what one process runs:
        2 launches for the reference's live graph, around d_1.conv1).
        After k - 1 calls of ``accumulate_grad()`` the gradient is the window's sum and the scale ``grad_scale`` / k (/ world under data
        parallelism).  ``clip``: this step's clipping norm (None: the constructor's); see the class text.  With neither, the launches are
        exactly those of the plain step."""
        from . import _lib
        flat, gflat, _ = self.model._flat
        if self._ema_swapped:
            raise _lib.RdmError("FusedAdamW.step inside ema_weights(): the model holds the averaged weights - leave the context (or swap_ema() back) first")
        if self.m is None or self.m.data_ptr() == 0 or self.m.numel() != flat.numel():
            self.m = torch.zeros_like(flat)
            self.v = torch.zeros_like(flat)
        if self.ema_decay is not None:
            self._seed_ema()
            self._ema_d = ema_decay_at(self.ema_decay, self.ema_updates, self.ema_warmup)
        clip = self.clip if clip is None else clip
        if clip is not None and not float(clip) >= 0.0:
            raise ValueError(f"FusedAdamW.step: clip must be a non-negative norm (got {clip!r})")
        dp = sync is not None and sync.world > 1
        if dp and clip is not None and sync.exchange == "reduce_scatter":
            raise _lib.RdmError("FusedAdamW: gradient clipping with the 'reduce_scatter' exchange is not built - a rank holds one shard of the reduced "
                                "gradient, so its norm is not the global norm; use the 'all_reduce' exchange")
        k = self.micro + 1                                         # micro-batches in this window
        if dp and k > 1 and self._hooked is not sync:
            raise _lib.RdmError("FusedAdamW: gradient accumulation under data parallelism needs attach_sync(sync) before the window's first backward pass "
                                "(the stage hook must stay silent on the non-final micro-batches and add the accumulator before the last one's reductions)")
        if self.micro and not self._folded:                        # one process (or no stage hook): the window's sum, just before the update
            self._accumulate(gflat, self.acc, 0, gflat.numel(), _lib.GRAD_ACC_ADD)
        self.micro, self._folded = 0, False
        self.step_count += 1
        small_grads = [p.grad for g in self.small.param_groups for p in g["params"] if p.grad is not None]
        if dp:
            self.sync = sync
            scale = float(grad_scale) / (k * sync.world)
        else:
            scale = float(grad_scale) / k if k > 1 else grad_scale
        if dp and clip is None:
            self.mode = "per stage, as its reduction lands"
            covered = []

            def on_reduced(stage, ranges):
                for a, b in ranges:
                    self._update(a, b, scale)
                covered.append(sync.slices[stage])
            sync.finish(on_reduced=on_reduced)
            # parameters outside every stage bucket (none for the reference's graph: the stages tile the stack) would be stale replicas
            assert sum(b - a for a, b in covered) >= sum(b - a for a, b in self.trainable_ranges()), "backward stages do not cover the trainable parameters"
            if k > 1:
                self._scale_small(small_grads, 1.0 / k)          # finish() left the rank mean of the window's sum
        else:
            if dp:                                                 # the norm is the REDUCED gradient's: every stage first, one update after the last
                self.mode = "after the last stage"
                sync.finish()
            if k > 1:
                self._scale_small(small_grads, 1.0 / k)
            n_slots = self._norm_slots(scale, small_grads) if clip is not None else 0
            for a, b in self.trainable_ranges():                  # 2 launches for the reference's live graph (around d_1.conv1)
                self._update(a, b, scale, clip, n_slots)
            if clip is not None and small_grads:
                self._scale_small(small_grads, self._coef[0])    # the coefficient the kernel formed from the same slots
        self.model.mark_weights_changed(relative_decoders=False)  # derived bf16 copies are stale now (d_6..d_10 are not in the flat buffer: untouched)
        self.small.step()
        if self.ema_decay is not None:
            omd = C.c_float(1.0 - self._ema_d).value              # 1.f - d in float32, as the kernel's host side forms it
            if omd != 0.0:
                with torch.no_grad():
                    for e, p in zip(self.ema_small, self._small_params()):
                        e.add_((p.detach() - e) * omd)
            self.ema_updates += 1

    # ---- the weight average ----
    def _small_params(self):
        return [p for g in self.small.param_groups for p in g["params"]]

    def _seed_ema(self):
        """The averages start as copies of the current weights (first step, or a resumed state that held none)."""
        flat = self.model._flat[0]
        if self.ema is None or self.ema.numel() != flat.numel() or self.ema.device != flat.device:
            self.ema = flat.detach().clone()
            self.ema_small = [p.detach().clone() for p in self._small_params()]
            self.ema_updates = 0

    def swap_ema(self):
        """Exchange the live weights and their average in place: one rdm_ema_swap_f32 launch per trainable range between the flat parameters
        and ``ema``, the ``weight_layer`` scalars in torch, and the derived bf16 copies marked stale.  Twice is the identity, bit for bit.
        Under the "reduce_scatter" exchange it first all-gathers ``ema`` (a collective: every rank calls it)."""
        from . import _lib
        if self.ema_decay is None:
            raise _lib.RdmError("FusedAdamW.swap_ema: the weight average is off (ema_decay=None)")
        self._seed_ema()                                           # before any step the average IS the weights
        flat = self.model._flat[0]
        if self.sync is not None:
            self.sync.allgather_shards(self.ema)
        L, st = _lib.lib(), _lib.stream()
        for a, b in self.trainable_ranges():
            _lib.check(L.rdm_ema_swap_f32(C.c_void_p(flat.data_ptr() + 4 * a), C.c_void_p(self.ema.data_ptr() + 4 * a), b - a, st))
        with torch.no_grad():
            for e, p in zip(self.ema_small, self._small_params()):
                live = p.detach().clone()
                p.copy_(e)
                e.copy_(live)
        self._ema_swapped = not self._ema_swapped
        self.model.mark_weights_changed(relative_decoders=False)

    def ema_weights(self):
        """Context in which the model holds the averaged weights (validation, export): ``swap_ema()`` on entry and again on exit, also when
        the body raises.  Afterwards weights and average are bit for bit what they were."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            self.swap_ema()
            try:
                yield self
            finally:
                self.swap_ema()
        return scope()

    def state_dict(self):
        """Moments, step and lr (the ``optimizer_states`` entry of a checkpoint); with the weight average on also ``ema``, ``ema_small``,
        ``ema_updates`` and ``ema_decay``."""
        if self._ema_swapped:
            from . import _lib
            raise _lib.RdmError("FusedAdamW.state_dict inside ema_weights(): weights and average are exchanged - leave the context first")
        if self.sync is not None and self.m is not None:          # "reduce_scatter": each rank holds the moments of its shards only
            self.sync.allgather_shards(self.m)
            self.sync.allgather_shards(self.v)
        sd = {"step": self.step_count, "lr": self.lr, "exp_avg": None if self.m is None else self.m.detach().cpu().clone(),
              "exp_avg_sq": None if self.v is None else self.v.detach().cpu().clone(), "small": self.small.state_dict()}
        if self.ema_decay is not None:
            if self.sync is not None and self.ema is not None:
                self.sync.allgather_shards(self.ema)
            sd.update(ema=None if self.ema is None else self.ema.detach().cpu().clone(),
                      ema_small=None if self.ema_small is None else [e.detach().cpu().clone() for e in self.ema_small],
                      ema_updates=self.ema_updates, ema_decay=self.ema_decay)
        return sd

    def load_state_dict(self, sd):
        flat = self.model._flat[0]
        self.step_count, self.lr = int(sd["step"]), float(sd["lr"])
        if sd.get("exp_avg") is not None:
            if sd["exp_avg"].numel() != flat.numel():
                raise ValueError("optimizer state does not match the model's flat parameter buffer")
            self.m, self.v = sd["exp_avg"].to(flat.device).clone(), sd["exp_avg_sq"].to(flat.device).clone()
        self.small.load_state_dict(sd["small"])
        for g in self.small.param_groups:
            g["lr"] = self.lr
        if self.ema_decay is not None:
            if sd.get("ema") is not None:                          # (this optimiser's ema_decay holds; the saved one is a record)
                if sd["ema"].numel() != flat.numel() or len(sd["ema_small"]) != len(self._small_params()):
                    raise ValueError("optimizer state's weight average does not match the model's flat parameter buffer")
                self.ema = sd["ema"].to(flat.device).clone()
                self.ema_small = [e.to(flat.device).clone() for e in sd["ema_small"]]
                self.ema_updates = int(sd["ema_updates"])
            else:                                                  # a state from a run without the average: re-seeded at the next step
                self.ema = self.ema_small = None
                self.ema_updates = 0


def accumulation_windows(batches, k):
    """``batches`` cut into windows of ``k``: yields (batch, index in its window, last of its window).  One batch is held ahead, so the last
    batch of the iterable closes its window even when the window is not full (the epoch-end flush)."""
    if k < 1:
        raise ValueError(f"accumulation_windows: k = {k} must be at least 1")
    it = iter(batches)
    try:
        cur = next(it)
    except StopIteration:
        return
    i = 0
    while True:
        try:
            nxt, more = next(it), True
        except StopIteration:
            nxt, more = None, False
        last = i == k - 1 or not more
        yield cur, i, last
        if not more:
            return
        cur, i = nxt, 0 if last else i + 1


def train_epoch(model, opt, batches, accumulate=1, sync=None, on_step=None, step_fn=None):
    """One pass over ``batches`` with an optimiser step per window of ``accumulate`` batches (module.py:64-97 under Lightning's
    ``accumulate_grad_batches``): ``zero_grad`` opens a window, the backward pass of every batch but the window's last runs inside
    ``opt.no_sync()`` and is followed by ``opt.accumulate_grad()``, the last one by ``opt.step(sync=sync)``, which divides by the batches the
    window actually holds.  ``on_step(step index, batches in the window, loss, parts)`` is called after every optimiser step with the losses of
    the window's last batch.  ``accumulate=1`` is the plain loop: zero_grad, training_step, backward, step.  -> optimiser steps taken."""
    step_fn = step_fn or training_step
    steps = 0
    for (x, y), i, last in accumulation_windows(batches, accumulate):
        if i == 0:
            opt.zero_grad()
        if last:
            loss, parts = step_fn(model, x, y)
            loss.backward()
            opt.step(sync=sync)
            if on_step is not None:
                on_step(steps, i + 1, loss, parts)
            steps += 1
        else:
            with opt.no_sync():
                loss, parts = step_fn(model, x, y)
                loss.backward()
            opt.accumulate_grad()
    return steps


def find_learning_rate(model, opt, batches, min_lr=1e-8, max_lr=1.0, num_training=100, early_stop_threshold=4.0, beta=0.98, sync=None):
    """The learning-rate range test the reference runs for ``--find_learning_rate`` (train.py:74-80: ``trainer.tuner.lr_find(module)``
    + ``lr_finder.suggestion()``; pytorch_lightning 1.1.7 defaults, third party): ``num_training`` steps with the learning rate swept
    exponentially from ``min_lr`` to ``max_lr``, an exponentially smoothed (beta 0.98, bias-corrected) loss per step, early stop once
    it exceeds ``early_stop_threshold`` x the best; the suggestion is the rate at the steepest descent of the smoothed loss
    (``numpy.gradient(...).argmin()``, skipping the first 10 and the last point).  Weights, BatchNorm buffers and optimiser state are
    restored afterwards, as Lightning does.  Returns (suggested_lr or None, lrs, smoothed losses)."""
    import numpy as np
    flat = model._flat[0]
    saved = (flat.detach().clone(), {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith("weight_layer.") or "running_" in k or "num_batches" in k},
             opt.state_dict())
    lrs, losses, avg, best = [], [], 0.0, None
    seen, it = [], iter(batches)
    for i in range(num_training):
        try:
            x, y = next(it)
            if len(seen) < 64:
                seen.append((x, y))                                  # a one-shot generator is cycled from what it yielded
        except StopIteration:
            if not seen:
                raise ValueError("find_learning_rate: no batches")
            x, y = seen[i % len(seen)]
        lr = min_lr * (max_lr / min_lr) ** (i / max(num_training - 1, 1))
        opt.lr = lr
        for g in opt.small.param_groups:
            g["lr"] = lr
        opt.zero_grad()
        loss, _ = training_step(model, x, y)
        loss.backward()
        if sync is not None:
            opt.step(sync=sync)
        else:
            opt.step()
        cur = float(loss.item())
        if sync is not None:
            # data parallel: the early stop below must be a COLLECTIVE decision.  Each rank's shard loss diverges at a different
            # step near lr -> 1; a rank that left the sweep alone would leave the others blocked in the next stage all-reduce.
            # Every rank smooths the rank-mean loss, so all of them run the same number of steps and suggest the same rate.
            cur = sync.mean_scalar(cur)
        avg = beta * avg + (1 - beta) * cur
        smooth = avg / (1 - beta ** (i + 1))
        lrs.append(lr)
        losses.append(smooth)
        if not np.isfinite(smooth) or (i > 0 and best is not None and smooth > early_stop_threshold * best):
            break
        if best is None or smooth < best:
            best = smooth
    with torch.no_grad():                                           # restore: the sweep must not leave a trace
        flat.copy_(saved[0])
        sd = model.state_dict()
        for k, v in saved[1].items():
            sd[k].copy_(v)
    opt.load_state_dict(saved[2])
    if opt.m is not None and saved[2]["exp_avg"] is None:
        opt.m.zero_()
        opt.v.zero_()
    model.mark_weights_changed()
    skip_begin, skip_end = 10, 1
    suggestion = None
    if len(losses) > skip_begin + skip_end + 1:
        window = np.array(losses[skip_begin:-skip_end])
        suggestion = lrs[skip_begin + int(np.gradient(window).argmin())]
    return suggestion, lrs, losses
