"""The reference's ``utils.py`` on this stack: ``depth2label_sid``, the one function on the hot path, and the SID tables ``get_depth_sid`` /
``get_labels_sid`` in the reference's float32 torch arithmetic (the metric-frame kernel uses the float64 formula of include/rdm_depth.h, not these)."""
import torch

from . import _lib


def _sid_tensors(name, cuda):
    from .depth import SID
    if name not in SID:
        raise _lib.RdmError("No Dataset named as %r (one of %s)" % (name, ", ".join(SID)))
    alpha, beta, K = (torch.tensor(v) for v in SID[name])                  # float32 scalars, as the reference builds them
    return (alpha.cuda(), beta.cuda(), K.cuda()) if cuda else (alpha, beta, K)


def get_depth_sid(args, labels, cuda=False):
    """utils.py:120-156: metres of SID label(s) under the parameter set named ``args`` ("nyu", "kitti", "floorplan3d", "Structured3D"),
    alpha * (beta / alpha) ** (label / K) through exp and log in float32; returns float32."""
    alpha, beta, K = _sid_tensors(args, cuda)
    return torch.exp(torch.log(alpha) + torch.log(beta / alpha) * labels / K).float()


def get_labels_sid(args, depth, cuda=False):
    """utils.py:159-193: the SID label of metric depth, K * log(depth / alpha) / log(beta / alpha) truncated by ``.int()``; returns int32."""
    alpha, beta, K = _sid_tensors(args, cuda)
    labels = K * torch.log(depth / alpha) / torch.log(beta / alpha)
    return (labels.cuda() if cuda else labels).int()


# Label of a NON-POSITIVE depth (log -> NaN -> `.int()`), which the reference leaves to the device it runs on: "cpu" = 0x80000000 (x86; what the
# parity fixtures - generated on the CPU - pin; the default), "cuda" = 0 (what the reference's own GPU training computes, utils.py:205-211 with
# cuda=True).  Either way such a pixel poisons compute_final_depth's geometric mean for its sample, exactly as in the reference (log of a
# negative label or of 0); harness.prepare_target's 1e-4 floor is applied BEFORE the resize to 8x8 and does not prevent the overshoot.
NAN_LABEL = "cpu"


def depth2label_sid(depth, K=90.0, alpha=0.02, beta=10.0, cuda=False):
    """utils.py:195-211 with K=90, alpha=0.02, beta=10 (the only values the path uses): SID label
    int(max(K*log(d/alpha)/log(beta/alpha), 0)), with the reference's float32 constants, one launch."""
    if NAN_LABEL not in ("cpu", "cuda"):
        raise _lib.RdmError("utils.NAN_LABEL must be 'cpu' or 'cuda'")
    if (K, alpha, beta) != (90.0, 0.02, 10.0):
        raise _lib.RdmError("depth2label_sid: only the reference defaults K=90, alpha=0.02, beta=10 are built")
    if not depth.is_cuda:
        raise _lib.RdmError("depth2label_sid runs on the GPU only")
    d = depth.double().contiguous()
    out = torch.empty(d.shape, dtype=torch.int32, device=d.device)
    _lib.check(_lib.lib().rdm_depth2label_sid_ex(_lib.ptr(d), _lib.ptr(out), d.numel(), 0 if NAN_LABEL == "cpu" else 1, _lib.stream()))
    return out
