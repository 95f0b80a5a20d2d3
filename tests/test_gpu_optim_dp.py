"""-m gpu: gradient accumulation under data parallelism as a SYSTEM, with the launch conventions of tests/test_gpu_dp.py: two fresh child ranks
(tests/optim_dp_child.py, started before they touch the GPU, each under its own time limit) run ONE accumulation window of two micro-batches each
through harness.train_epoch; this process accumulates the same four batches in one window.  Checked:
  * no_sync: the first micro-batch's thirteen stage hooks fire and issue NO reduction; the second's issue thirteen;
  * replicas: both ranks leave the step with bit-identical gradients, parameters and weight_layer scalars;
  * exchange: the reduced window sum equals the single process's window sum per stage slice, at the 2e-2 of tests/test_gpu_dp.py (the weight-gradient
    kernels add with atomics: two evaluations of one gradient differ by rounding, so that tolerance governs, not bit equality);
  * update: on both sides the post-step weights are torch.optim.AdamW fed (that side's own sum) / 4 - 1 / (k world) for the ranks, 1 / k for the single
    process - at test_gpu_dp.py's 2e-8 + 1e-6 max|w|, d_1.conv1.* untouched.
The box has ONE GPU: the ranks exchange over gloo (RCCL refuses two ranks on one device); with >= 2 GPUs the same test uses nccl."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from md_rdm_amd import filler

pytestmark = pytest.mark.gpu
CHILD_LIMIT_S = 300


@pytest.fixture(scope="module")
def single_process():
    """the four batches in ONE process and ONE window of four"""
    from md_rdm_amd import harness
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    dev = torch.device("cuda:0")
    m = DepthEstimationNet()
    filler.fill_state_dict(m.state_dict())
    m = m.to(dev).train()
    m.flatten_parameters()
    m.direct_grads = True
    flat, gflat, entries = m._flat
    init = flat.cpu().numpy().copy()
    opt = harness.FusedAdamW(m, lr=1e-4)

    def batches():
        for seed in (7, 14, 14, 7):                            # rank 0's two shards, then rank 1's
            x, y = filler.synthetic_batch(2, 228, 228, seed=seed)
            yield torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    seen = []
    steps = harness.train_epoch(m, opt, batches(), accumulate=4, on_step=lambda it, n, loss, parts: seen.append((it, n, float(loss.detach()))))
    assert steps == 1 and seen[0][:2] == (0, 4) and np.isfinite(seen[0][2])
    return dict(init=init, gsum=gflat.detach().cpu().numpy(), post=flat.detach().cpu().numpy(), slices=m.stage_slices(), entries=[(k, o, n) for k, p, o, n, g in entries],
                wlg={n: p.grad.detach().cpu().numpy() for n, p in m.weight_layer.named_parameters() if p.grad is not None})


def check_update(init, gsum, post, entries, scale):
    """post == torch.optim.AdamW(lr 1e-4) fed gsum * scale from init (tests/test_gpu_dp.py's update check)"""
    ref_p = [torch.nn.Parameter(torch.from_numpy(init[o:o + n].copy())) for k, o, n in entries]
    for rp, (k, o, n) in zip(ref_p, entries):
        rp.grad = None if k.startswith("d_1.conv1.") else torch.from_numpy(gsum[o:o + n] * np.float32(scale))
    torch.optim.AdamW(ref_p, lr=1e-4).step()
    for rp, (k, o, n) in zip(ref_p, entries):
        got, want = post[o:o + n], rp.detach().numpy()
        if k.startswith("d_1.conv1."):
            np.testing.assert_array_equal(got, init[o:o + n])
        else:
            assert np.abs(got - want).max() <= 2e-8 + 1e-6 * np.abs(want).max(), k


def test_two_ranks_accumulating_match_one_process_accumulating(tmp_path, single_process):
    assert torch.cuda.is_available()
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    port = str(32800 + os.getpid() % 1500)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")      # the child ranks share the card: dmabuf IPC, as bench.py / train.py set for themselves
    procs = [subprocess.Popen(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(ROOT, "tests", "optim_dp_child.py"), str(r), "2", port, str(tmp_path), backend],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=CHILD_LIMIT_S + 30)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append(p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-2000:] for o in outs)
    print("\n".join(o[-600:] for o in outs))
    r0, r1 = ({k: v for k, v in np.load(tmp_path / f"rank{r}.npz").items()} for r in range(2))
    sp = single_process
    # ---- no_sync: reductions only behind the window's last micro-batch ----
    for r in (r0, r1):
        assert int(r["n_slices"]) == 13 and int(r["steps"]) == 1 and int(r["step_count"]) == 1
        assert r["hook_calls"].tolist() == [13, 13] and r["exchange_calls"].tolist() == [0, 13], (r["hook_calls"], r["exchange_calls"])
        assert np.isfinite(r["losses"]).all() and len(r["losses"]) == 2
    assert not np.array_equal(r0["losses"], r1["losses"])          # the ranks saw different shards at each micro-batch
    # ---- replicas stay identical ----
    for k in r0:
        if k in ("init", "gsum", "post") or k.startswith("wlg_") or k.startswith("wlp_"):
            np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)
    np.testing.assert_array_equal(sp["init"], r0["init"])
    # ---- the exchange: the reduced window sum against the single process's window sum ----
    for a, b in sp["slices"]:
        num, den = np.linalg.norm(r0["gsum"][a:b] - sp["gsum"][a:b]), np.linalg.norm(sp["gsum"][a:b])
        assert den > 0 and num <= 2e-2 * den, (a, b, num / den)
    for n, g in sp["wlg"].items():                                  # both hold the MEAN over the four batches when the step ends
        np.testing.assert_allclose(r0["wlg_" + n], g, rtol=2e-3, atol=1e-7)
    # ---- the update, on each side from its own sum: 1 / (k world) and 1 / k are both 1 / 4 ----
    check_update(r0["init"], r0["gsum"], r0["post"], sp["entries"], 0.25)
    check_update(sp["init"], sp["gsum"], sp["post"], sp["entries"], 0.25)
    assert np.abs(r0["post"] - r0["init"]).max() > 5e-5
