"""MI355X-native ``DepthEstimationNet`` - same nn.Module surface as the reference
``network/RDM_Net.py`` (no-arg constructor :26, ``forward(x) -> (y_hat, x_d1, ord_labels)`` :70-135,
968-key ``state_dict``, module globals ``use_cuda`` / ``freeze_encoder`` :8-9), but every op of the
hot path is a hand-written gfx950 kernel reached through the C ABI in ``include/rdm_hip.h``:

  * the whole conv stack (encoder + decoder d_1 up to conv2) is ONE autograd node that runs the
    native plan ``rdm_net_forward`` / ``rdm_net_backward`` (md_rdm_amd/csrc/net.hip);
  * the DORN head, geometric-mean normalisation, decomposition and weighting are single launches.

The nn.Conv2d / nn.BatchNorm2d objects below are *parameter holders only* (names, shapes and
PyTorch's default initialisation, so checkpoints interchange); their ``forward`` is never called.
There is no PyTorch/CPU fallback: without librdm_hip.so or without a GPU, ``forward`` raises.
"""
import ctypes as C
import math
import os

import numpy as np
import scipy.io
import torch
import torch.nn as nn

from .. import _lib
from . import computations as cp

use_cuda = True
freeze_encoder = False

_DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")
GROWTH = 48


class BaseModel(nn.Module):
    def load(self, path):
        """Reference stub (RDM_Net.py:10-22): intentionally does nothing."""
        pass


# ------------------------------------------------------------------------------------------
# parameter holders with torchvision's naming (denselayer%d / norm1 relu1 conv1 norm2 relu2 conv2;
# norm relu conv pool), see tests/golden/state_dict_keys.txt
# ------------------------------------------------------------------------------------------
class _DenseLayerParams(nn.Module):
    def __init__(self, cin, bn_size):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(cin)
        self.conv1 = nn.Conv2d(cin, bn_size * GROWTH, kernel_size=1, stride=1, bias=False)
        self.norm2 = nn.BatchNorm2d(bn_size * GROWTH)
        self.conv2 = nn.Conv2d(bn_size * GROWTH, GROWTH, kernel_size=3, stride=1, padding=1, bias=False)


class _DenseBlockParams(nn.Module):
    """torchvision ``_DenseBlock(num_layers, num_input_features, bn_size, growth_rate=48, ...)``.
    The reference passes the spatial size as bn_size (57/29/15/8), SURVEY.md F8."""

    def __init__(self, num_layers, cin, bn_size):
        super().__init__()
        for i in range(num_layers):
            self.add_module("denselayer%d" % (i + 1), _DenseLayerParams(cin + i * GROWTH, bn_size))


class _TransitionParams(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm = nn.BatchNorm2d(cin)
        self.conv = nn.Conv2d(cin, cout, kernel_size=1, stride=1, bias=False)


def _make_encoder_():
    """RDM_Net.py:493-532."""
    encoder = nn.Module()
    encoder.conv_e1 = nn.Conv2d(in_channels=3, kernel_size=7, stride=2, out_channels=96, padding=3)
    encoder.dense_e2 = _DenseBlockParams(6, 96, 57)
    encoder.trans_e2 = _TransitionParams(384, 192)
    encoder.dense_e3 = _DenseBlockParams(12, 192, 29)
    encoder.trans_e3 = _TransitionParams(768, 384)
    encoder.dense_e4 = _DenseBlockParams(36, 384, 15)
    encoder.trans_e4 = _TransitionParams(2112, 1056)
    return encoder


def _wsm_output_planes(decoder_id):
    """RDM_Net.py:556-567."""
    return {1: 2208, 6: 2208, 7: 1664, 8: 832, 9: 416, 10: 208}.get(decoder_id, 1)


class Quantization:
    """Lloyd tables (RDM_Net.py:397-442), resolved relative to the package instead of the CWD.
    ``depth_ratio_008_008_quant`` is missing upstream and DERIVED as 016**2."""

    def __init__(self):
        for s in ("016", "032", "064", "128"):
            m = scipy.io.loadmat(os.path.join(_DATA, f"depth_ratio_{s}_{s}_quant.mat"))
            setattr(self, f"depth_ratio_{s}_{s}_quant", m[f"depth_ratio_{s}_{s}_quant"])
            setattr(self, f"depth_ratio_{s}_{s}_quant_inv", m[f"depth_ratio_{s}_{s}_quant_inv"])
        self.depth_ratio_008_008_quant = self.depth_ratio_016_016_quant ** 2          # derived, not upstream
        self.depth_ratio_008_008_quant_inv = self.depth_ratio_016_016_quant_inv ** 2
        self._dev = {}

    def get_with_id(self, id):
        s = {3: "008", 4: "016", 5: "032", 6: "064", 7: "128"}[id]
        return getattr(self, f"depth_ratio_{s}_{s}_quant"), getattr(self, f"depth_ratio_{s}_{s}_quant_inv")

    def get_size_id(self, id):
        return {3: 8, 4: 16, 5: 32, 6: 64, 7: 128}[id]

    def device_tables(self, id, device):
        key = (id, str(device))
        if key not in self._dev:
            q, inv = self.get_with_id(id)
            self._dev[key] = (torch.from_numpy(np.ascontiguousarray(q[:, 0])).to(device), torch.from_numpy(np.ascontiguousarray(inv[:, 0])).to(device))
        return self._dev[key]


class Ordinal_Layer(nn.Module):
    """RDM_Net.py:237-396.  DORN=True: ordinal regression head; DORN=False: the relative decoders
    (ratio grid -> Lloyd -> rank-1 ALS), dormant in the reference graph, live here as operators."""

    def __init__(self, decoder_id, DORN, quantizer):
        super().__init__()
        self.quant = quantizer
        self.id = decoder_id - 3
        self.dorn = DORN

    def DornOrdinalRegression(self, x):
        return cp.dorn_ordinal_regression(x)

    def sparse_comparison_v1(self, d_3):
        q, inv = self.quant.device_tables(3, d_3.device)
        return cp.ratio_grid_lloyd_dense(d_3, q, inv)

    def sparse_comparison_id(self, dn, dn_1):
        q, inv = self.quant.device_tables(self.id, dn.device)
        return cp.ratio_grid_lloyd_paged(dn, dn_1, q, inv)[0]

    def forward(self, x):
        if self.dorn:
            return self.DornOrdinalRegression(x)
        if self.id == 3:                                                     # d_6
            return cp.quadratic_als(self.sparse_comparison_v1(x), cuda=x.is_cuda, n=3)
        dn = x
        dn_1 = cp.resize(dn, self.quant.get_size_id(self.id - 1))
        q, inv = self.quant.device_tables(self.id, dn.device)
        pages = cp.als_pages_fused(dn, dn_1, q, inv, limit=100)              # (P,B,1,16,16) f32: grid + Lloyd formed inside the ALS load
        if self.id == 4:                                                     # d_7: single page
            return pages[0]
        return cp.reconstruct(list(pages))                                   # d_8..d_10


def _make_wsm_layers_(num_of_layers):
    """RDM_Net.py:533-554: WSM_1..WSM_k (1664@16, 832@32, 416@64, 208@128)."""
    from .wsm import WSMLayer
    block = nn.Sequential()
    for i, (c, k) in enumerate([(1664, 16), (832, 32), (416, 64), (208, 128)][:num_of_layers]):
        block.add_module("WSM_%d" % (i + 1), WSMLayer(c, k, k, i + 1))
    return block


def _bn_affine(bn, s, q, count, training):
    """BatchNorm as the per-channel (scale, shift) the conv prologue applies (rdm_bn_finalize): training mode uses the batch statistics
    (f64 sums from the producing kernel) and updates the running statistics like nn.BatchNorm2d."""
    L = _lib.lib()
    c = bn.weight.numel()
    out = torch.empty(4, c, dtype=torch.float32, device=bn.weight.device)        # scale | shift | mean | rstd
    _lib.check(L.rdm_bn_finalize(_lib.ptr(s) if training else None, _lib.ptr(q) if training else None, float(count), _lib.ptr(bn.weight.detach()),
                                 _lib.ptr(bn.bias.detach()), _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), _lib.ptr(bn.num_batches_tracked),
                                 _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(out[3]), c, int(training), _lib.stream()))
    return out[0], out[1]


def _dense_block_forward(block, x, training):
    """torchvision ``_DenseBlock`` forward (RDM_Net.py:144) for the relative decoders, inference through the C ABI:
    one NHWC buffer holds all channels (concat-free), every conv is ``rdm_conv2d_fwd`` with the consumer's BN-ReLU as
    prologue and the next BatchNorm's channel statistics as epilogue; layout change, input statistics and the BatchNorm
    bookkeeping are C-ABI calls too (rdm_layout_nchw_to_nhwc_f32, rdm_bn_stats, rdm_bn_finalize).  No autograd (the reference's
    Lloyd step severs the graph above these decoders anyway, RDM_Net.py:296-297).  x (B,C,H,W) -> (B,H,W,C + 48*layers) NHWC."""
    from . import wsm as _wsm
    L = _lib.lib()
    B, cin0, H, W = x.shape
    layers = list(block.children())
    cb = layers[0].conv1.out_channels
    ctot = cin0 + GROWTH * len(layers)
    M = B * H * W
    dev = x.device
    st = _lib.stream()
    blk = torch.zeros(B, H, W, ctot, dtype=torch.float32, device=dev)
    _lib.check(L.rdm_layout_nchw_to_nhwc_f32(_lib.ptr(x.contiguous()), _lib.ptr(blk), ctot, B, cin0, H * W, st))
    ssum = torch.zeros(ctot, dtype=torch.float64, device=dev)
    ssq = torch.zeros(ctot, dtype=torch.float64, device=dev)
    _lib.check(L.rdm_bn_stats(_lib.ptr(blk), ctot, M, cin0, _lib.ptr(ssum), _lib.ptr(ssq), st))
    Y = torch.empty(M, cb, dtype=torch.float32, device=dev)
    ysum = torch.zeros(cb, dtype=torch.float64, device=dev)
    ysq = torch.zeros(cb, dtype=torch.float64, device=dev)
    for i, lay in enumerate(layers):
        cin = cin0 + i * GROWTH
        sc1, sh1 = _bn_affine(lay.norm1, ssum[:cin], ssq[:cin], M, training)
        ysum.zero_()
        ysq.zero_()
        d1 = _lib.ConvDesc(B, H, W, cin, ctot, cb, cb, 1, 1, 1, 1, 0, 0)
        _lib.check(L.rdm_conv2d_fwd(C.byref(d1), _lib.ptr(blk), _lib.ptr(lay.conv1.weight.detach().contiguous()), None, _lib.ptr(sc1), _lib.ptr(sh1),
                                    _lib.ptr(Y), _lib.ptr(ysum), _lib.ptr(ysq), st))
        sc2, sh2 = _bn_affine(lay.norm2, ysum, ysq, M, training)
        wp, _, _ = _wsm._packed_cached(lay.conv2, ("dense3x3",), (lay.conv2.weight,), lambda lay=lay: (lay.conv2.weight.detach(), None, 3, 3))   # packed once, not per call
        d2 = _lib.ConvDesc(B, H, W, cb, cb, GROWTH, ctot, 3, 3, 1, 1, 1, 1)
        _lib.check(L.rdm_conv2d_fwd(C.byref(d2), _lib.ptr(Y), _lib.ptr(wp), None, _lib.ptr(sc2), _lib.ptr(sh2), C.c_void_p(blk.data_ptr() + 4 * cin),
                                    C.c_void_p(ssum.data_ptr() + 8 * cin), C.c_void_p(ssq.data_ptr() + 8 * cin), st))
    return blk


class Decoder(nn.Module):
    """RDM_Net.py:137-162.  id 1 (the only decoder the reference instantiates) runs inside the native plan; ids 6..9 are the
    relative decoders of SURVEY.md 8(f)4 (d_10, :61, included): dense block -> WSM chain -> conv1 -> ratio grid / Lloyd / ALS head,
    forward only, every derived (padded / packed) weight built once and reused until its parameter changes."""

    def __init__(self, in_channels, num_wsm_layers, DORN, id, quant):
        super().__init__()
        assert 0 <= num_wsm_layers < 5
        self.id = id
        self.dense_layer = _DenseBlockParams(24, 1056, 8)
        self.wsm_block = _make_wsm_layers_(num_wsm_layers)
        self.conv1 = nn.Conv2d(in_channels=_wsm_output_planes(id), out_channels=1, kernel_size=1)
        self.conv2 = nn.Conv2d(in_channels=_wsm_output_planes(id), out_channels=180, kernel_size=1)
        self.ord_layer = Ordinal_Layer(id, DORN, quant)

    # ---- bf16 inference (rdm_rel_forward_bf16, csrc/wsm_bf16.hip): prepared weights are derived data, rebuilt when stale ----
    def set_precision(self, precision):
        """"f32" (default) or "bf16": ``features`` of an eval-mode relative decoder on the bf16 path (training still runs in f32 only)."""
        if precision not in ("f32", "bf16"):
            raise ValueError("precision must be 'f32' or 'bf16'")
        self.precision = precision
        return self

    # Two staleness flags: _bf16_rel_stale (the eval path: weights or running statistics changed) and _bf16_rel_wstale (the training path
    # reads only the packed conv weights: weights changed).  A training forward moves the running statistics, so it sets the first only.
    def mark_weights_changed(self):
        self._bf16_rel_stale = True
        self._bf16_rel_wstale = True

    def load_state_dict(self, *a, **k):
        self.mark_weights_changed()
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self.mark_weights_changed()
        return super()._apply(fn, *a, **k)

    def _prepare_bf16(self, device, weights_only=False):
        L = _lib.lib()
        tensors = list(self.state_dict().values())
        if len(tensors) != L.rdm_rel_num_tensors(self.id):
            raise _lib.RdmError("decoder %d: %d state tensors, the library expects %d" % (self.id, len(tensors), L.rdm_rel_num_tensors(self.id)))
        nbytes = int(L.rdm_rel_bf16_weight_bytes(self.id))
        w = self.__dict__.get("_bf16_rel_w")
        if w is None or w.numel() < nbytes or w.device != device:
            w = self.__dict__["_bf16_rel_w"] = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self._bf16_rel_stale = True
            self._bf16_rel_wstale = True
        if self.__dict__.get("_bf16_rel_wstale" if weights_only else "_bf16_rel_stale", True):
            table = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
            _lib.check(L.rdm_rel_bf16_prepare(self.id, table, C.c_void_p(w.data_ptr()), nbytes, _lib.stream()))
            self._bf16_rel_stale = False
            self._bf16_rel_wstale = False
        return w

    def features_bf16_train(self, enc, ld_enc, batch, enc_stats=None):
        """The TRAINING-mode bf16 forward (rdm_rel_forward_bf16_train): enc as ``features_bf16``; BatchNorm from the batch statistics,
        running statistics updated in place like nn.BatchNorm2d; forward only.  ``enc_stats``: optional (2*1056,) float64 column sums and
        sums of squares of enc (rdm_colstats_bf16), shared by the decoders of one forward.  (B,1,S,S) f32."""
        L = _lib.lib()
        if not self.training:
            raise _lib.RdmError("features_bf16_train is the training-mode forward (batch-statistics BatchNorm): call train(), or features_bf16 for inference")
        w = self._prepare_bf16(enc.device, weights_only=True)
        tensors = list(self.state_dict().values())
        ws_bytes = int(L.rdm_rel_bf16_train_workspace_bytes(self.id, batch))
        ws = self.__dict__.get("_bf16_rel_tws")
        if ws is None or ws.numel() < ws_bytes or ws.device != enc.device:
            ws = self.__dict__["_bf16_rel_tws"] = torch.empty(ws_bytes, dtype=torch.uint8, device=enc.device)
        S = 2 ** (self.id - 3)
        out = torch.empty(batch, 1, S, S, dtype=torch.float32, device=enc.device)
        table = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        _lib.check(L.rdm_rel_forward_bf16_train(self.id, _lib.ptr(enc), ld_enc, _lib.ptr(enc_stats), batch, table, C.c_void_p(w.data_ptr()),
                                                C.c_void_p(ws.data_ptr()), ws_bytes, _lib.ptr(out), _lib.stream()))
        self._bf16_rel_stale = True                     # the running statistics moved: the eval-folded affines are stale (the packed weights are not)
        return out

    def features_bf16(self, enc, ld_enc, batch):
        """The bf16 forward from the encoder output as (batch*8*8, ld_enc) NHWC bf16 (any dtype holding those bytes): (B,1,S,S) f32."""
        L = _lib.lib()
        if self.training:
            raise _lib.RdmError("the bf16 path is inference only (eval-mode BatchNorm): call eval(), or use the f32 path to train")
        w = self._prepare_bf16(enc.device)
        ws_bytes = int(L.rdm_rel_bf16_workspace_bytes(self.id, batch))
        ws = self.__dict__.get("_bf16_rel_ws")
        if ws is None or ws.numel() < ws_bytes or ws.device != enc.device:
            ws = self.__dict__["_bf16_rel_ws"] = torch.empty(ws_bytes, dtype=torch.uint8, device=enc.device)
        S = 2 ** (self.id - 3)
        out = torch.empty(batch, 1, S, S, dtype=torch.float32, device=enc.device)
        _lib.check(L.rdm_rel_forward_bf16(self.id, _lib.ptr(enc), ld_enc, batch, C.c_void_p(w.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes, _lib.ptr(out),
                                          _lib.stream()))
        return out

    def features(self, x):
        """dense block -> WSM chain -> conv1 (:151-157): the one-channel map the relative head consumes, (B,1,S,S)."""
        from . import wsm
        if not x.is_cuda:
            raise _lib.RdmError("Decoder runs on the GPU only")
        if self.id <= 5:
            raise _lib.RdmError("decoder %d is part of the native plan (DepthEstimationNet.forward); only the relative decoders 6..10 run standalone" % self.id)
        if getattr(self, "precision", "f32") == "bf16":
            if self.training:
                raise _lib.RdmError("the bf16 path is inference only (eval-mode BatchNorm): call eval(), or set_precision('f32') to train")
            B = x.shape[0]
            if tuple(x.shape[1:]) != (1056, 8, 8):
                raise _lib.RdmError("the bf16 relative decoders take the (B,1056,8,8) encoder output, got %s" % (tuple(x.shape),))
            enc = torch.empty(B * 64, 1056, dtype=torch.bfloat16, device=x.device)
            _lib.check(_lib.lib().rdm_rel_bf16_input_nchw(_lib.ptr(x.contiguous().float()), B, _lib.ptr(enc), 1056, _lib.stream()))
            return self.features_bf16(enc, 1056, B)
        if self.training:
            self._bf16_rel_stale = True                 # the training forward updates the running statistics in place (a kernel: no _version bump)
        with torch.no_grad():
            h = _dense_block_forward(self.dense_layer, x.float(), self.training)
            if len(self.wsm_block):
                t = h.permute(0, 3, 1, 2)
                for m in self.wsm_block:
                    t = m(t)
                h = t.permute(0, 2, 3, 1).contiguous()
            return wsm.conv_nhwc(h, self.conv1)[..., :1].permute(0, 3, 1, 2).contiguous()

    def forward(self, x):
        with torch.no_grad():
            return self.ord_layer(self.features(x))


class Weights(nn.Module):
    """RDM_Net.py:443-491: one weight vector per pyramid level, |randn| initialised."""

    def __init__(self, vector_sizes, use_cuda, relative_only):
        super().__init__()
        self.use_cuda = use_cuda
        self.relative_only = relative_only
        for n, s in zip(["d0", "f1", "f2", "f3", "f4", "f5", "f6", "f7"], vector_sizes):
            setattr(self, n, nn.Parameter(torch.abs(torch.randn((s, 1)))))
        self.weight_list = [self.d0, self.f1, self.f2, self.f3, self.f4, self.f5, self.f6, self.f7]
        for w in self.weight_list:
            if w.shape[0] == 0:
                w.requires_grad = False

    def get(self, index):
        return self.weight_list[index]

    def forward(self, x):
        return cp.make_pred(self.weight_list, x, self.use_cuda, self.relative_only)


# ------------------------------------------------------------------------------------------
# the conv stack as one autograd node over the native plan
# ------------------------------------------------------------------------------------------
class _ConvStackFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, *params):
        logits = model._native_forward(x)
        ctx.model = model
        ctx.gen = model._ws_generation
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        model = ctx.model
        if ctx.gen != model._ws_generation:
            raise _lib.RdmError("the saved activations were overwritten by a later forward() of the same model "
                                "(one in-flight training step per model instance)")
        grads = model._native_backward(dlogits.contiguous())
        return (None, None) + tuple(grads)


def mirror_average(predict, x):
    """Mirror test-time augmentation of a map predictor: the mean of the map of ``x`` and the mirrored map of the mirrored ``x``, two calls of
    ``predict`` on batches of ``x``'s size, the unmirrored one first.  ``DepthEstimationNet.predict(x, flip=True)`` is this of its own maps."""
    return 0.5 * (predict(x) + predict(x.flip(-1)).flip(-1))


class DepthEstimationNet(BaseModel):
    """Drop-in for the reference class (RDM_Net.py:25-135)."""

    def __init__(self, relative_decoders=()):
        """``relative_decoders``: () = the reference's live graph (d_1 only).  A subset of (6, 7, 8, 9, 10) adds the relative
        decoders the reference keeps commented out (RDM_Net.py:57-61,106-125) with the reference's own
        module names, so a checkpoint of the uncommented model loads; they run forward-only (see ``Decoder``)."""
        super().__init__()
        self.quantizers = Quantization()
        self.encoder = _make_encoder_()
        if freeze_encoder:
            self.freeze_encoder()
        self.d_1 = Decoder(in_channels=1056, num_wsm_layers=0, DORN=True, id=1, quant=self.quantizers)
        self.relative_ids = tuple(sorted(set(int(d) for d in relative_decoders)))
        if not set(self.relative_ids) <= {6, 7, 8, 9, 10}:
            raise ValueError("relative_decoders must be a subset of (6, 7, 8, 9, 10), got %r" % (relative_decoders,))
        sizes = [1, 1, 1, 1, 0, 0, 0, 0]                       # candidates per pyramid level: d_1 gives levels 0..3,
        for did in self.relative_ids:                           # d_k (map side 2^(k-3)) gives F_1..F_(k-3) (relative_map drops d_0)
            setattr(self, "d_%d" % did, Decoder(in_channels=1056, num_wsm_layers=did - 6, DORN=False, id=did, quant=self.quantizers))
            for level in range(1, did - 2):
                sizes[level] += 1
        self.weight_layer = Weights(vector_sizes=sizes, use_cuda=use_cuda, relative_only=False)
        # native-plan state (not part of the state_dict)
        self._plans = {}
        self._ws = None
        self._ws_generation = 0
        self._flat = None          # (flat_params, flat_grads, [(name, tensor, offset, numel)])
        self._names = None
        self.direct_grads = False  # True: backward writes straight into the flat gradient buffer (fast path of our harness)
        self.grad_ready_hook = None  # callable(stage) fired after each backward stage has been enqueued (DP overlap)
        self.deterministic = False  # True (set before the first forward): RDM_NET_OPT_DETERMINISTIC - ordered reductions, bit-reproducible gradients (tests)
        self.precision = "f32"     # "bf16": eval-mode forward on the bf16 MFMA path (set_precision)
        self.forward_split = True    # conv1 of dense_e2 / dense_e3 on the three-way-split bf16x6 kernel (RDM_NET_OPT_SPLIT_FWD: float32-equivalent accuracy, measured
                                   # 3-9e-7 of the result's maximum against float64 - the f32 MFMA kernel's own level); False: exact-f32 MFMA
        self.prepack = True          # RDM_NET_OPT_PREPACK: the split kernels' weight images are formed for all layers once per step on the side stream (off the dependent chains)
        self.fuse_stats3 = True      # RDM_NET_OPT_FUSE_STATS3: the K-split 3x3 conv of the few-pixel blocks takes its output's channel statistics in the same launch (training forward)
        self.wino_x6 = False         # RDM_NET_OPT_WINO_X6: conv2 (3x3) of dense_e2 / dense_e3 forward as Winograd on three-way-split bf16 MFMAs (float32-equivalent; with forward_split).
                                     # Correct (2e-6 of the maximum vs float64) but NOT faster than the f32 MFMA kernel at these sizes (7.1 vs 6.7 ms per step): the kernel is bound by
                                     # its producers and the per-workgroup prologue / epilogue of the deep K split, not by the matrix pipe (profiles/r05_wino_x6_ablation.txt)
        self.split_rows = True       # RDM_NET_OPT_SPLIT_ROWS: dY and relu1(norm1(x)) reach the split conv1 gradient kernels as split rows written once by their producers (bit-identical gradients)
        self.defer_norm1 = True      # RDM_NET_OPT_DEFER_NORM1: the norm1 BatchNorm backward of the blocks on the split kernels without its O(layers^2) elementwise pass (same gradients to f32 rounding)
        self.gemm_bf16 = 0           # 1 (or True): forward and gradient GEMMs, 2: forward only, 3: gradient GEMMs only - MIXED-PRECISION arithmetic (the reference's default `--precision 16`, train.py:11,57-58): every GEMM the two options
                                   # around this line route to the split kernels rounds its operands to bf16 (one MFMA per product, float32 accumulation);
                                   # activations, weights, BatchNorm statistics, losses and AdamW stay float32.  Not the parity configuration.
        self.backward_precision = "bf16x3"   # "bf16x3" (default): the gradient GEMMs of dense_e2 / dense_e3 run the split-precision kernels
                                   # (RDM_NET_OPT_SPLIT_BWD, csrc/xsplit.hip: ~5e-6 of a gradient's maximum); "f32": exact-f32 MFMA everywhere
        self.relative_train_precision = "f32"   # "bf16": the training-mode forward of the relative decoders on the bf16 path (set_relative_train_precision)
        self._bf16_w = None        # prepared bf16 weights + folded BatchNorm affines (rdm_net_bf16_prepare)
        self._bf16_stale = True
        self._bf16_ws = None

    def freeze_encoder(self):
        for parameter in self.encoder.parameters():
            parameter.requires_grad = False

    # ---- plumbing ---------------------------------------------------------------------------
    def _tensor_table(self):
        """state_dict tensors in the registry order of the native plan (== reference order)."""
        L = _lib.lib()
        if self._names is None:
            n = L.rdm_net_num_tensors()
            self._names = [L.rdm_net_tensor_name(i).decode() for i in range(n)]
            self._is_param = [bool(L.rdm_net_tensor_is_param(i)) for i in range(n)]
        named = dict(self.named_parameters())
        named.update(dict(self.named_buffers()))
        return [named[k] for k in self._names]

    def stack_parameters(self):
        """Float parameters of the conv stack, in plan order (everything except weight_layer.*)."""
        tensors = self._tensor_table()
        return [(k, t) for k, t, p in zip(self._names, tensors, self._is_param) if p and not k.startswith("weight_layer.")]

    def flatten_parameters(self):
        """Re-home every conv-stack parameter into ONE contiguous buffer (and a twin gradient
        buffer) so the optimiser and the gradient all-reduce are single flat operations.
        Parameter objects keep their identity; only ``.data`` is re-pointed.
        The 78 dense-layer 3x3 weights live there PACKED [tap][out][in] - the layout the MFMA kernels read (forward rows, dgrad
        columns) and the weight-gradient kernel writes - and ``.data`` / ``.grad`` are OIHW-shaped strided VIEWS of it, so
        state_dict / checkpoints / tests see PyTorch's logical tensor while no pack / unpack pass ever runs (AdamW is elementwise:
        parameter, gradient and moments share the layout)."""
        ps = self.stack_parameters()
        dev = ps[0][1].device
        offs, off = [], 0
        for _, p in ps:
            offs.append(off)
            off += (p.numel() + 63) // 64 * 64          # 256-byte alignment of every tensor
        flat = torch.zeros(off, dtype=torch.float32, device=dev)
        gflat = torch.zeros(off, dtype=torch.float32, device=dev)

        def view_of(buf, k, p, o, n):
            if p.dim() == 4 and tuple(p.shape[2:]) == (3, 3) and ".denselayer" in k:
                O, I = p.shape[0], p.shape[1]
                return buf[o:o + n].view(9, O, I).permute(1, 2, 0).unflatten(2, (3, 3))      # (O, I, 3, 3), strides (I, 1, 3*O*I, O*I)
            return buf[o:o + n].view(p.shape)
        entries = []
        for (k, p), o in zip(ps, offs):
            n = p.numel()
            v = view_of(flat, k, p, o, n)
            v.copy_(p.data)
            p.data = v
            entries.append((k, p, o, n, view_of(gflat, k, p, o, n)))
        self._flat = (flat, gflat, entries)
        self._flatten_buffers()
        return flat, gflat

    def _flatten_buffers(self):
        """BatchNorm running statistics -> ONE float32 buffer, the batch counters -> ONE int64 buffer (the module's registered buffers
        become views): DDP's per-forward buffer broadcast (md_rdm_amd/parallel.py) is then two collectives and no copy at all,
        instead of a cat and ~640 scatter-back copies per step."""
        fl, it = [], []
        for mod in self.modules():
            for name, b in list(mod._buffers.items()):
                if b is None or not b.numel():
                    continue
                (fl if b.dtype == torch.float32 else it if b.dtype == torch.int64 else []).append((mod, name, b))
        self._flat_buffers = []
        for group, dtype in ((fl, torch.float32), (it, torch.int64)):
            if not group:
                continue
            total = sum(b.numel() for _, _, b in group)
            buf = torch.empty(total, dtype=dtype, device=group[0][2].device)
            o = 0
            for mod, name, b in group:
                v = buf[o:o + b.numel()].view(b.shape)
                v.copy_(b)
                mod._buffers[name] = v
                o += b.numel()
            self._flat_buffers.append(buf)

    def _ensure_flat(self, device):
        if self._flat is None or self._flat[0].device != device or self._flat[2][0][1].data_ptr() != self._flat[0].data_ptr():
            self.flatten_parameters()

    def _plan(self, B, H, W):
        key = (B, H, W, bool(self.deterministic), self.backward_precision, bool(self.forward_split), int(self.gemm_bf16), bool(self.defer_norm1), bool(self.prepack), bool(self.split_rows), bool(self.wino_x6), bool(self.fuse_stats3))
        if self.backward_precision not in ("f32", "bf16x3"):
            raise ValueError("backward_precision must be 'f32' or 'bf16x3'")
        if key not in self._plans:
            L = _lib.lib()
            h = C.c_void_p()
            _lib.check(L.rdm_net_create(B, H, W, C.byref(h)))
            opts = [(_lib.NET_OPT_PACKED_3X3, 1),                  # flatten_parameters keeps the 3x3 weights packed
                    (_lib.NET_OPT_GRADS_PREZEROED, 1),             # _native_backward fills the flat gradient buffer once
                    (_lib.NET_OPT_DETERMINISTIC, int(bool(self.deterministic))),
                    (_lib.NET_OPT_SPLIT_BWD, int(self.backward_precision == "bf16x3")),
                    (_lib.NET_OPT_SPLIT_FWD, int(bool(self.forward_split))),
                    (_lib.NET_OPT_PREPACK, int(bool(self.prepack))),
                    (_lib.NET_OPT_DEFER_NORM1, int(bool(self.defer_norm1))),
                    (_lib.NET_OPT_SPLIT_ROWS, int(bool(self.split_rows))),
                    (_lib.NET_OPT_WINO_X6, int(bool(self.wino_x6))),
                    (_lib.NET_OPT_FUSE_STATS3, int(bool(self.fuse_stats3))),
                    (_lib.NET_OPT_GEMM_BF16, int(self.gemm_bf16))]
            for opt, value in opts:
                _lib.check(L.rdm_net_set_option(h, opt, value))
            oh, ow = C.c_int32(), C.c_int32()
            _lib.check(L.rdm_net_output_hw(h, C.byref(oh), C.byref(ow)))
            self._plans[key] = (h, int(L.rdm_net_workspace_bytes(h)), oh.value, ow.value)
        return self._plans[key]

    def _native_forward(self, x):
        if not x.is_cuda:
            raise _lib.RdmError("DepthEstimationNet runs on the MI355X only (input is on %s); there is no CPU fallback" % x.device)
        L = _lib.lib()
        x = x.contiguous().float()
        B, Cin, H, W = x.shape
        assert Cin == 3
        self._ensure_flat(x.device)
        h, ws_bytes, oh, ow = self._plan(B, H, W)
        if self._ws is None or self._ws.numel() < ws_bytes or self._ws.device != x.device:
            # zeroed once, when it is allocated: the plan never writes the padding columns of its buffers (logits: 180 of 192), and whoever reads a
            # whole buffer (debug_buffer) must not see what an earlier owner of the block left there
            self._ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=x.device)
        tensors = self._tensor_table()
        table = (C.c_void_p * len(tensors))(*[t.data_ptr() if t.numel() else None for t in tensors])
        logits = torch.empty(B, 180, oh, ow, dtype=torch.float32, device=x.device)
        self._ws_generation += 1
        if self.training:
            self._bf16_stale = True                     # a training forward updates the running statistics the bf16 affines were folded from
        _lib.check(L.rdm_net_forward(h, _lib.ptr(x), table, C.c_void_p(self._ws.data_ptr()), ws_bytes, _lib.ptr(logits), int(self.training), _lib.stream()))
        self._last = (h, ws_bytes, table, tensors)
        self._last_batch = B
        return logits

    def _native_backward(self, dlogits):
        L = _lib.lib()
        h, ws_bytes, table, tensors = self._last
        flat, gflat, entries = self._flat
        gview = {k: g for k, p, o, n, g in entries}
        want = {k: p.requires_grad for k, p, o, n, g in entries}
        gt = []
        for k, t, is_p in zip(self._names, tensors, self._is_param):
            g = gview.get(k) if (is_p and want.get(k, False)) else None
            gt.append(g.data_ptr() if g is not None else None)
        gtable = (C.c_void_p * len(gt))(*gt)
        st = _lib.stream()
        # without a per-stage consumer (the data-parallel exchange) the side stream joins once per segment, not after each of the 13 stages
        _lib.check(L.rdm_net_set_option(h, _lib.NET_OPT_JOIN_PER_SEGMENT, 0 if self.grad_ready_hook is not None else 1))
        gflat.zero_()                                                # ONE fill instead of ~160 per-tensor fills inside the plan
        for stage in range(L.rdm_net_num_backward_stages()):        # ~25 MB of gradients per stage: the DP exchange starts every few layers
            _lib.check(L.rdm_net_backward_stage(h, _lib.ptr(dlogits), table, gtable, C.c_void_p(self._ws.data_ptr()), ws_bytes, stage, st))
            if self.grad_ready_hook is not None:
                self.grad_ready_hook(stage)
        out = []
        for k, p, o, n, g in entries:
            if not p.requires_grad or k.startswith("d_1.conv1."):
                out.append(None)                      # d_1.conv1 is unused for id 1 (RDM_Net.py:156-157)
            elif self.direct_grads:
                p.grad = g
                out.append(None)
            else:
                out.append(g)
        return out

    # ---- reduced-precision inference (BASELINE config 2; the reference's default is mixed precision, train.py:11,57-58) ----
    def set_precision(self, precision):
        """"f32" (default: exact-f32 MFMA, training and inference) or "bf16" (inference only: ``model.eval()`` forward runs with bf16
        weights / activations, f32 accumulation and f32 BatchNorm affines; the DORN tail stays f64).  bf16 does not meet the 1e-4
        parity bar of the f32 path; its tolerance is stated in tests/test_gpu_bf16.py.  The relative decoders (``relative_decoders``) run on the
        bf16 path too (rdm_rel_forward_bf16: dense block, WSM chain and conv1 in bf16; the heads unchanged), tolerance in
        tests/test_gpu_relative_bf16.py."""
        if precision not in ("f32", "bf16"):
            raise ValueError("precision must be 'f32' or 'bf16'")
        self.precision = precision
        return self

    def set_relative_train_precision(self, precision):
        """"f32" (default) or "bf16": the TRAINING-mode forward of the relative decoders (``relative_decoders``).  "bf16" runs their dense
        blocks, WSM chains and conv1 on the bf16 MFMA kernels (rdm_rel_forward_bf16_train: bf16 conv operands, f32 accumulation, float32
        BatchNorm from the batch statistics, running statistics updated like nn.BatchNorm2d) - the reference's `--precision 16` treatment of
        these forward-only decoders.  No effect in eval mode (``set_precision`` decides there); tolerance in tests/test_gpu_relative_bf16_train.py."""
        if precision not in ("f32", "bf16"):
            raise ValueError("relative train precision must be 'f32' or 'bf16'")
        self.relative_train_precision = precision
        return self

    def mark_weights_changed(self, relative_decoders=True):
        """The bf16 copies are derived data: call after any in-place weight update that bypasses this class (the fused AdamW
        does it itself; load_state_dict / .to() are caught below).  The relative decoders' packed weights (the bf16 training forward reads
        them without passing through prepare_bf16) are marked too, unless the caller knows it changed none of d_6..d_10
        (``relative_decoders=False``: the fused AdamW, whose update covers the flat buffer and weight_layer only)."""
        self._bf16_stale = True
        if relative_decoders:
            for did in self.relative_ids:
                getattr(self, "d_%d" % did).mark_weights_changed()

    def load_state_dict(self, *a, **k):
        self._bf16_stale = True
        for did in self.relative_ids:                       # (the decoders' own load_state_dict is not called on this path)
            getattr(self, "d_%d" % did).mark_weights_changed()
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._bf16_stale = True
        return super()._apply(fn, *a, **k)

    def prepare_bf16(self, B, H, W):
        """bf16 weight copies (+ eval-mode BatchNorm folded to scale / shift) in one caller-owned buffer; redone when stale."""
        L = _lib.lib()
        h = self._plan(B, H, W)[0]
        tensors = self._tensor_table()
        dev = tensors[0].device
        nbytes = int(L.rdm_net_bf16_weight_bytes(h))
        if self._bf16_w is None or self._bf16_w.numel() < nbytes or self._bf16_w.device != dev:
            self._bf16_w = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self._bf16_stale = True
        table = (C.c_void_p * len(tensors))(*[t.data_ptr() if t.numel() else None for t in tensors])
        if self._bf16_stale:
            _lib.check(L.rdm_net_bf16_prepare(h, table, C.c_void_p(self._bf16_w.data_ptr()), nbytes, _lib.stream()))
            for did in self.relative_ids:                   # the relative decoders' prepared weights follow the same staleness rule
                getattr(self, "d_%d" % did).mark_weights_changed()
            self._bf16_stale = False
        return h, table, nbytes

    def _native_forward_bf16(self, x):
        if not x.is_cuda:
            raise _lib.RdmError("DepthEstimationNet runs on the MI355X only (input is on %s); there is no CPU fallback" % x.device)
        if self.training:
            raise _lib.RdmError("the bf16 path is inference only (eval-mode BatchNorm, no saved activations): call model.eval(), or set_precision('f32') to train")
        L = _lib.lib()
        x = x.contiguous().float()
        B, Cin, H, W = x.shape
        assert Cin == 3
        self._ensure_flat(x.device)
        h, table, wbytes = self.prepare_bf16(B, H, W)
        ws_bytes = int(L.rdm_net_bf16_workspace_bytes(h))
        if self._bf16_ws is None or self._bf16_ws.numel() < ws_bytes or self._bf16_ws.device != x.device:
            self._bf16_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        _, _, oh, ow = self._plan(B, H, W)
        logits = torch.empty(B, 180, oh, ow, dtype=torch.float32, device=x.device)
        _lib.check(L.rdm_net_forward_bf16(h, _lib.ptr(x), table, C.c_void_p(self._bf16_w.data_ptr()), wbytes, C.c_void_p(self._bf16_ws.data_ptr()),
                                          ws_bytes, _lib.ptr(logits), _lib.stream()))
        self._last_bf16 = (h, ws_bytes, B)
        return logits

    def encoder_output_bf16(self):
        """(B*h*w, 1056) bf16 NHWC: the encoder output (trans_e4, RDM_Net.py:94) of the last bf16 forward - the relative decoders' input."""
        h, ws_bytes, B = self._last_bf16
        _, _, oh, ow = next(v for k, v in self._plans.items() if v[0] is h)
        out = torch.empty(B * oh * ow, 1056, dtype=torch.bfloat16, device=self._bf16_ws.device)
        _lib.check(_lib.lib().rdm_net_encoder_output_bf16(h, C.c_void_p(self._bf16_ws.data_ptr()), ws_bytes, _lib.ptr(out), 1056, _lib.stream()))
        return out

    def encoder_output(self):
        """(B,1056,h,w) float32: the encoder output (trans_e4, RDM_Net.py:94) of the last f32 forward - what every decoder consumes."""
        h, ws_bytes, _, _ = self._last
        B = self._last_batch
        _, _, oh, ow = next(v for k, v in self._plans.items() if v[0] is h)
        out = torch.empty(B, 1056, oh, ow, dtype=torch.float32, device=self._ws.device)
        _lib.check(_lib.lib().rdm_net_encoder_output(h, C.c_void_p(self._ws.data_ptr()), ws_bytes, _lib.ptr(out), _lib.stream()))
        return out

    def debug_buffer(self, name):
        """Float view of a named internal buffer of the last forward's plan (tests / debugging)."""
        h = self._last[0]
        off, n = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().rdm_net_buffer(h, name.encode(), C.byref(off), C.byref(n)))
        return self._ws[off.value:off.value + 4 * n.value].view(torch.float32)

    def stage_slices(self):
        """[(start, stop)] element ranges of the flat gradient buffer completed by backward stages 0 .. n-1 (~25 MB each, last
        registered tensors first: the buckets of the data-parallel gradient exchange)."""
        L = _lib.lib()
        flat, gflat, entries = self._flat
        pos = {k: (o, o + n) for k, p, o, n, g in entries}
        res = []
        for stage in range(L.rdm_net_num_backward_stages()):
            a, b = C.c_int32(), C.c_int32()
            _lib.check(L.rdm_net_backward_stage_range(stage, C.byref(a), C.byref(b)))
            ks = [self._names[i] for i in range(a.value, b.value + 1) if self._names[i] in pos]
            res.append((min(pos[k][0] for k in ks), max(pos[k][1] for k in ks)))
        return res

    segment_slices = stage_slices          # former name (4 coarse segments)

    # ---- image -> depth map (no target): recombination(model(x)[0]), computations.py:394-421 on RDM_Net.py:70-135 --------
    def _fused_tail_levels(self, oh, ow):
        """log2 of the head side when rdm_predict_tail_f32 covers this model and head (ordinal-only, square power-of-two side <= 16, one
        weight per level), else None."""
        if self.relative_ids or oh != ow or oh & (oh - 1) or oh > 16:
            return None
        n = oh.bit_length() - 1
        if any(self.weight_layer.get(k).numel() != 1 for k in range(n + 1)):
            return None
        return n

    def predict(self, x, linear=False, size=None, return_counts=False, flip=False):
        """The (B,1,128,128) float64 map of log relative depth for a batch of images - what the reference computes for an image,
        ``recombination(model(x)[0])`` (optimize_components returns its predictions unchanged, computations.py:499-510) - without a target.
        Eval mode only; the forward runs at the model's ``precision``.  The ordinal-only model with a square power-of-two head (226/228-pixel
        inputs) takes the d_1 logits to the map in ONE launch (rdm_predict_tail_f32); models with relative decoders and rectangular heads
        compose the single operators exactly as ``forward`` + ``recombination`` do.
        ``linear``: return float32 ``exp`` of the map instead.  ``size=(H, W)``: bicubic ``resize`` of the log map first.
        ``return_counts``: also return the (B,1,h,w) int64 DORN count map (``forward``'s second result).
        ``flip``: mirror test-time augmentation, by definition ``0.5 * (predict(x) + predict(x.flip(-1)).flip(-1))`` of the log-domain maps:
        two passes at the caller's batch size, averaged before ``size`` and ``linear`` apply.  The counts are the unmirrored pass's."""
        if self.training:
            raise _lib.RdmError("predict is inference only (eval-mode BatchNorm): call model.eval() first")
        if not x.is_cuda:
            raise _lib.RdmError("DepthEstimationNet runs on the MI355X only (input is on %s); there is no CPU fallback" % x.device)
        if flip:
            with torch.no_grad():
                passes = []

                def plain(v):
                    passes.append(self.predict(v, return_counts=return_counts))
                    return passes[-1][0] if return_counts else passes[-1]
                out = mirror_average(plain, x)
                counts = passes[0][1] if return_counts else None
                if size is not None:
                    out = cp.resize(out, tuple(size))
                if linear:
                    out = torch.exp(out).float()
                return (out, counts) if return_counts else out
        with torch.no_grad():
            B, _, H, W = x.shape
            _, _, oh, ow = self._plan(B, H, W)
            n = self._fused_tail_levels(oh, ow)
            lin = None
            if n is not None:
                logits = self._native_forward_bf16(x) if self.precision == "bf16" else self._native_forward(x)
                wv = torch.cat([self.weight_layer.get(k).reshape(-1)[:1].float() for k in range(n + 1)]).contiguous()
                out = torch.empty(B, 1, 128, 128, dtype=torch.float64, device=x.device)
                counts = torch.empty(B, 1, oh, ow, dtype=torch.int64, device=x.device) if return_counts else None
                if linear and size is None:
                    lin = torch.empty(B, 1, 128, 128, dtype=torch.float32, device=x.device)
                _lib.check(_lib.lib().rdm_predict_tail_f32(_lib.ptr(logits), _lib.ptr(wv), _lib.ptr(out), _lib.ptr(counts), _lib.ptr(lin), B, logits.shape[1] // 2,
                                                           oh, ow, 7, 0, _lib.stream()))
            else:
                y_hat, counts, _ = self.forward(x)
                out = cp.recombination(list(y_hat))
            if size is not None:
                out = cp.resize(out, tuple(size))
            if linear:
                out = lin if lin is not None else torch.exp(out).float()
            return (out, counts) if return_counts else out

    def predict_metric(self, x, frame_hw, view=None, flip=False, refine=None, guide=None, anchors=None, anchor=None, **kwargs):
        """Metric depth frames for a batch of images: ``predict(x, return_counts=True, flip=flip)`` followed by ``depth.metric_frames`` of the
        map and the DORN counts (under ``flip`` the unmirrored pass's) over the (h, w) frame, of which the network saw ``view``.  ``kwargs`` are
        ``metric_frames``' (log_scale, sid, offset, unit, outside, want); the result is its dict.
        ``refine``: a dict of ``refine.joint_bilateral``'s keywords (radius, step, sigma_space, sigma_color, fill), or True for its defaults:
        the float32 plane of ``metric_frames`` is filtered under ``guide``, the (B,h,w,3) uint8 colour frame of the (h, w) frame, and the
        returned f32 / u16 planes are the refined ones (``unit`` is the metric one).
        ``anchors``: a (B,h,w) float32 frame of metric measurements of the (h, w) frame, 0 where there is none (md_rdm_amd.anchor).  The SID
        scale of the counts (plus ``log_scale``) becomes the prior of ``anchor.fit``, whose keywords ``anchor`` holds (fit, cell, sigma, lam,
        reject, min_depth, max_depth, field); the frames are ``anchor.metric_frames`` of the fitted scale and field, "log_scale" the fitted one,
        and ``refine`` filters the anchored plane.  Without ``anchors`` nothing changes."""
        from .. import depth
        if anchors is None:
            if anchor is not None:
                raise _lib.RdmError("predict_metric: the anchor options need anchors, the frame of measurements")

            def frames(log_map, counts, **kw):
                return depth.metric_frames(log_map, frame_hw, view=view, counts=counts, **kw)
        else:
            from .. import anchor as an
            aopts = {} if anchor is None else dict(anchor) if isinstance(anchor, dict) else None
            if aopts is None or any(k not in an.DEFAULTS for k in aopts):
                raise _lib.RdmError("anchor must be a dict of %s, got %r" % (", ".join(an.DEFAULTS), anchor))

            def frames(log_map, counts, log_scale=None, sid="nyu", offset=0.0, **kw):
                prior = depth.sid_log_scale(counts, sid=sid, offset=offset)
                if log_scale is not None:
                    prior = prior + log_scale.reshape(-1)
                return an.metric_frames(log_map, frame_hw, an.fit(log_map, anchors, view=view, prior=prior, **aopts), view=view, **kw)
        if refine is None or refine is False:
            log_map, counts = self.predict(x, return_counts=True, flip=flip)
            return frames(log_map, counts, **kwargs)
        from .. import refine as rf
        opts = {} if refine is True else dict(refine) if isinstance(refine, dict) else None
        if opts is None or any(k not in rf.DEFAULTS for k in opts):
            raise _lib.RdmError("refine must be True or a dict of %s, got %r" % (", ".join(rf.DEFAULTS), refine))
        h, w = int(frame_hw[0]), int(frame_hw[1])
        if guide is None:
            raise _lib.RdmError("refine needs guide, the (B,h,w,3) uint8 colour frame of the output's geometry")
        if not isinstance(guide, torch.Tensor) or not guide.is_cuda or guide.dtype != torch.uint8 or tuple(guide.shape) != (x.shape[0], h, w, 3):
            raise _lib.RdmError("guide must be (%d,%d,%d,3) uint8 on the device, got %s %s" % (
                x.shape[0], h, w, getattr(guide, "dtype", type(guide)), tuple(getattr(guide, "shape", ()))))
        want = kwargs.pop("want", ("f32",))
        want = (want,) if isinstance(want, str) else tuple(want)
        planes = [k for k in want if k in ("f32", "u16")]
        log_map, counts = self.predict(x, return_counts=True, flip=flip)
        out = frames(log_map, counts, want=("f32",) + tuple(k for k in want if k not in ("f32", "u16")), **kwargs)
        refined = rf.joint_bilateral(out.pop("f32"), guide, unit=kwargs.get("unit", 1e-3), want=planes or ("f32",), **opts)
        out.update((k, refined[k]) for k in planes)
        return out

    def predict_cloud(self, x, frame_hw, intrinsics, view=None, rgb=None, normals=False, min_depth=0.0, max_depth=math.inf, step=1, flip=False, refine=None,
                      **kwargs):
        """Point clouds for a batch of images: ``predict_metric`` (its float32 plane; ``kwargs`` are its log_scale, sid, offset, outside, anchors, anchor) followed by
        ``cloud.point_cloud`` with ``intrinsics`` = (fx, fy, cx, cy) of the (h, w) frame; ``rgb`` (B,h,w,3) uint8 colours the points.  The
        result is ``point_cloud``'s (records, counts).  ``refine`` is ``predict_metric``'s, with ``rgb`` (required then) as the guide."""
        from .. import cloud
        on = not (refine is None or refine is False)
        if on and rgb is None:
            raise _lib.RdmError("predict_cloud: refine needs rgb, the guide of the filter")
        planes = self.predict_metric(x, frame_hw, view=view, flip=flip, want=("f32",), refine=refine, guide=rgb if on else None, **kwargs)
        return cloud.point_cloud(planes["f32"], intrinsics, rgb=rgb, normals=normals, min_depth=min_depth, max_depth=max_depth, step=step)

    def predict_mesh(self, x, frame_hw, intrinsics, view=None, rgb=None, normals=False, min_depth=0.0, max_depth=math.inf, step=1, edge_ratio=None, flip=False,
                     refine=None, **kwargs):
        """Triangle meshes for a batch of images: ONE ``predict_metric`` call (its float32 plane; ``kwargs`` and ``refine`` as for ``predict_cloud``)
        followed by ``mesh.depth_mesh`` of that plane: the cloud's records are the vertices, and the faces are the cells of the sampled pixel grid
        whose depths stay within ``edge_ratio`` of each other (default ``mesh.EDGE_RATIO``, a starting point whose effect has not been measured).
        The result is ``depth_mesh``'s (records, vertex_counts, faces, face_counts), the payloads of ``mesh.write_ply``."""
        from .. import mesh
        on = not (refine is None or refine is False)
        if on and rgb is None:
            raise _lib.RdmError("predict_mesh: refine needs rgb, the guide of the filter")
        planes = self.predict_metric(x, frame_hw, view=view, flip=flip, want=("f32",), refine=refine, guide=rgb if on else None, **kwargs)
        return mesh.depth_mesh(planes["f32"], intrinsics, rgb=rgb, normals=normals, min_depth=min_depth, max_depth=max_depth, step=step,
                               edge_ratio=mesh.EDGE_RATIO if edge_ratio is None else edge_ratio)

    def predict_view(self, x, frame_hw, intrinsics, pose, view=None, rgb=None, flip=False, refine=None, out_hw=None, intrinsics_out=None, min_depth=0.0,
                     max_depth=math.inf, splat=1, fill=0, want=("depth", "rgb", "index", "mask"), **kwargs):
        """The predicted frame seen from another camera: ONE ``predict_metric`` call (its float32 plane; ``kwargs`` and ``refine`` as for
        ``predict_cloud``) followed by ``warp.render`` of that plane under ``pose`` (source camera -> target camera), with ``intrinsics`` =
        (fx, fy, cx, cy) of the (h, w) frame and ``rgb`` (B,h,w,3) uint8 as its colours.  The result is ``render``'s dict of planes."""
        from .. import warp
        on = not (refine is None or refine is False)
        if on and rgb is None:
            raise _lib.RdmError("predict_view: refine needs rgb, the guide of the filter")
        planes = self.predict_metric(x, frame_hw, view=view, flip=flip, want=("f32",), refine=refine, guide=rgb if on else None, **kwargs)
        return warp.render(planes["f32"], intrinsics, pose, rgb=rgb, out_hw=out_hw, intrinsics_out=intrinsics_out, min_depth=min_depth, max_depth=max_depth,
                           splat=splat, fill=fill, want=want)

    def predict_fused(self, x, frame_hw, intrinsics, poses, volume, view=None, rgb=None, flip=False, refine=None, min_depth=0.0, max_depth=math.inf,
                      weight=1.0, **kwargs):
        """The predicted frames integrated into a ``fuse.Volume``: ONE ``predict_metric`` call (its float32 plane; ``kwargs`` and ``refine`` as for
        ``predict_cloud``, so ``anchors`` / ``anchor`` tie the frames to measurements first) followed by ``volume.integrate`` of that plane under
        ``poses`` (WORLD -> camera, one or one per sample), with ``intrinsics`` = (fx, fy, cx, cy) of the (h, w) frame and ``rgb`` (B,h,w,3) uint8
        as its colours.  The result is the float32 plane that went into the volume."""
        on = not (refine is None or refine is False)
        if on and rgb is None:
            raise _lib.RdmError("predict_fused: refine needs rgb, the guide of the filter")
        planes = self.predict_metric(x, frame_hw, view=view, flip=flip, want=("f32",), refine=refine, guide=rgb if on else None, **kwargs)
        volume.integrate(planes["f32"], intrinsics, poses, rgb=rgb, min_depth=min_depth, max_depth=max_depth, weight=weight)
        return planes["f32"]

    # ---- the reference forward (RDM_Net.py:70-135) -----------------------------------------
    def forward(self, x):
        bf16 = self.precision == "bf16"
        if bf16:
            logits = self._native_forward_bf16(x)                               # inference only; no autograd node
        else:
            params = [p for _, p in self.stack_parameters()] if self._flat is None else [p for _, p, _, _, _ in self._flat[2]]
            logits = _ConvStackFunction.apply(self, x, *params)                # encoder + d_1 up to conv2
        x_d1, ord_labels = self.d_1.ord_layer(logits)                           # DORN head, :347-357
        B, _, H, W = x_d1.size()
        # geometric-mean normalisation of the count map (:117); documented generalisation for
        # non-square encoder outputs (the reference raises there): exponent 1/(H*W) and a bicubic
        # resize to the largest power-of-two square before decomposition
        norm = cp.gm_normalize(x_d1, 1.0 / (H * W)).float()
        side = 2 ** int(math.floor(math.log2(min(H, W))))
        if (H, W) != (side, side):
            norm = cp.resize(norm, side)
        f_d1 = cp.decompose_depth_map([], norm, int(math.log2(side)))[::-1]     # :117
        rows = [f_d1]
        if self.relative_ids:                                                   # :106-125 as the paper intends (8(f)4)
            if (H, W) != (8, 8):
                raise _lib.RdmError("the relative decoders need the square 8x8 encoder output (226/228-pixel inputs), got %dx%d" % (H, W))
            with torch.no_grad():
                train_bf16 = not bf16 and self.training and self.relative_train_precision == "bf16"
                if bf16:                                                         # trans_e4 output as (B*64, 1056) bf16 NHWC, no layout pass
                    enc = self.encoder_output_bf16()
                else:
                    enc = self.encoder_output()                                  # trans_e4 output (B,1056,8,8) of the forward above
                if train_bf16:                                                   # converted once, its column statistics taken once: every decoder reads it
                    L = _lib.lib()
                    enc16 = torch.empty(B * 64, 1056, dtype=torch.bfloat16, device=enc.device)
                    _lib.check(L.rdm_rel_bf16_input_nchw(_lib.ptr(enc), B, _lib.ptr(enc16), 1056, _lib.stream()))
                    enc_stats = torch.empty(2 * 1056, dtype=torch.float64, device=enc.device)
                    _lib.check(L.rdm_colstats_bf16(_lib.ptr(enc16), 1056, B * 64, 1056, _lib.ptr(enc_stats[:1056]), _lib.ptr(enc_stats[1056:]), _lib.stream()))
                for did in self.relative_ids:
                    dec = getattr(self, "d_%d" % did)
                    if bf16:
                        x_dk = dec.ord_layer(dec.features_bf16(enc, 1056, B))    # (B,1,S,S) relative map, S = 2^(did-3)
                    elif train_bf16:
                        x_dk = dec.ord_layer(dec.features_bf16_train(enc16, 1056, B, enc_stats))
                    else:
                        x_dk = dec(enc)
                    rows.append(cp.decompose_depth_map([], x_dk, did - 3, relative_map=True)[::-1])
        y_hat = cp.relative_fine_detail_matrix(rows, use_cuda)                  # :126
        y_hat = self.weight_layer(y_hat)                                        # :133
        return y_hat, x_d1, ord_labels
