"""Which kernels does the native plan launch?  One training step per configuration with the launch census on (rdm_census_*): the
{kernel variant: launches} dict and the rdm_launch_count() delta of the step, and for the deterministic configuration the SHA-256 of the
flat gradient buffer and of the logits.  Kernel selection and launch count are host logic and repeat exactly, so a recording made before a
change of the routing code says whether the change selected another kernel anywhere (tests/test_gpu_routes.py holds every step against
tests/golden/plan_census.json).  The shapes put dense blocks on both sides of every pixel threshold of the plan (1 024: split gradient
kernels, 8 192: split conv1 forward / Winograd forward / split 3x3 weight gradient, 12 288: Winograd weight gradient).

    python tools/plan_census.py                  print the recording as JSON
    python tools/plan_census.py --write          write tests/golden/plan_census.json
    python tools/plan_census.py --out FILE       write FILE
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_census.json")

DEFAULTS = dict(deterministic=False, backward_precision="bf16x3", forward_split=True, gemm_bf16=0, split_rows=True, defer_norm1=True, prepack=True)
# name: (batch, height, width, model attributes that differ from DEFAULTS, encoder frozen)
CONFIGS = {
    # dense blocks of 12 996 / 3 306 / 855 / 240 pixels
    "b3_defaults": (3, 228, 304, {}, False),
    "b3_f32": (3, 228, 304, dict(backward_precision="f32", forward_split=False), False),
    "b3_deterministic": (3, 228, 304, dict(deterministic=True), False),
    "b3_gemm_bf16_1": (3, 228, 304, dict(gemm_bf16=1), False),
    "b3_gemm_bf16_2": (3, 228, 304, dict(gemm_bf16=2), False),
    "b3_gemm_bf16_3": (3, 228, 304, dict(gemm_bf16=3), False),
    "b3_no_split_rows": (3, 228, 304, dict(split_rows=False), False),
    "b3_no_defer_norm1": (3, 228, 304, dict(defer_norm1=False), False),
    "b3_no_prepack": (3, 228, 304, dict(prepack=False), False),
    "b3_frozen_encoder": (3, 228, 304, {}, True),       # conv1 of the encoder's layers has no gradient slot
    "b2_defaults": (2, 228, 304, {}, False),            # dense_e2 at 8 664 pixels
    "b4_defaults": (4, 228, 304, {}, False),            # dense_e4 at 1 140 pixels
}


def new_model(dev):
    from md_rdm_amd import filler
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet()
    filler.fill_state_dict(m.state_dict())
    return m.to(dev).train()


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def record(model, name):
    """One training step + backward of configuration `name` on `model` (weights are not updated; the model's options and requires_grad
    flags are restored).  The census is switched on for the step only."""
    import torch
    from md_rdm_amd import _lib, filler, harness, utils
    B, H, W, attrs, frozen = CONFIGS[name]
    L = _lib.lib()
    dev = next(model.parameters()).device
    x, y = filler.synthetic_batch(B, H, W, seed=1234)
    xg, yg = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    for k, v in {**DEFAULTS, **attrs}.items():
        setattr(model, k, v)
    enc = [(p, p.requires_grad) for p in model.encoder.parameters()]
    if frozen:
        model.freeze_encoder()
    nan_label, utils.NAN_LABEL = utils.NAN_LABEL, "cpu"      # process-wide (md_rdm_amd.train sets "cuda"): it decides the ordinal target of invalid pixels, hence the gradients
    torch.cuda.synchronize()
    L.rdm_census_reset()
    L.rdm_census_enable(1)
    try:
        n0 = L.rdm_launch_count()
        loss, _ = harness.training_step(model, xg, yg)
        loss.backward()
        torch.cuda.synchronize()
        out = {"census": dict(sorted(_lib.census().items())), "launches": int(L.rdm_launch_count() - n0)}
    finally:
        L.rdm_census_enable(0)
        utils.NAN_LABEL = nan_label
        for p, rg in enc:
            p.requires_grad = rg
        for k, v in DEFAULTS.items():
            setattr(model, k, v)
    if attrs.get("deterministic"):
        out["grad_sha256"] = _sha(model._flat[1])
        out["logits_sha256"] = _sha(model.debug_buffer("logits").view(-1, 192)[:, :180])     # NHWC rows padded to 192: the pad is never written
    for p in model.parameters():
        p.grad = None
    return out


def main(argv):
    import torch
    model = new_model(torch.device("cuda:0"))
    rec = {name: record(model, name) for name in CONFIGS}
    text = json.dumps(rec, indent=1, sort_keys=True) + "\n"
    path = FIXTURE if "--write" in argv else argv[argv.index("--out") + 1] if "--out" in argv else None
    if path is None:
        sys.stdout.write(text)
    else:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(text)
        print(f"{len(rec)} configurations -> {path}")


if __name__ == "__main__":
    main(sys.argv[1:])
