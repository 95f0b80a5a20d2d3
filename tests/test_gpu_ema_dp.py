"""-m gpu: the weight average under data parallelism, with the launch conventions of tests/test_gpu_dp.py: two fresh child ranks (tests/ema_dp_child.py,
started before they touch the GPU, each under its own time limit; the parent checks the exit statuses and goes no further after a failure) take TWO
real training steps with FusedAdamW(ema_decay=0.9) through the per-stage update, over the "all_reduce" exchange and over "reduce_scatter" (where a
rank advances the average of the ranges it owns and state_dict() all-gathers it).  Checked per exchange:
  * replicas: after state_dict() the two ranks' averages (flat and the four scalars) are bit-identical, and so are their weights;
  * the average: on each rank it equals the float64 replay (tests/ema_ref.py) of that rank's own recorded post-step weights within 5 T 2^-24 M, T = 2;
    d_1.conv1.* and alignment padding hold the initial copy;
  * the swap: inside ema_weights() the model held the average, and afterwards weights and average were back bit for bit (compared in the child).
The box has ONE GPU: the ranks exchange over gloo (RCCL refuses two ranks on one device); with >= 2 GPUs the same test uses nccl."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ema_ref as er
from conftest import ROOT

pytestmark = pytest.mark.gpu
CHILD_LIMIT_S = 300


@pytest.mark.parametrize("exchange", ["all_reduce", "reduce_scatter"])
def test_two_ranks_keep_one_average(tmp_path, exchange):
    assert torch.cuda.is_available()
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    port = str(34400 + os.getpid() % 1500 + (0 if exchange == "all_reduce" else 1500))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")      # the child ranks share the card: dmabuf IPC, as bench.py / train.py set for themselves
    procs = [subprocess.Popen(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(ROOT, "tests", "ema_dp_child.py"), str(r), "2", port, str(tmp_path), backend,
                               exchange], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
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
    dev = torch.device("cuda:0")
    for r in (r0, r1):
        assert str(r["exchange"]) == exchange and str(r["mode"]).startswith("per stage") and int(r["updates"]) == 2
        assert bool(r["inside_ok"]) and bool(r["after_ok"])
        assert r["decays"].tolist() == [er.decay_at(0.9, 0), er.decay_at(0.9, 1)]
    # ---- replicas: one average, bit for bit ----
    for k in ("init", "post0", "post1", "ema", "ema_small", "small_post1", "mask"):
        assert np.array_equal(r0[k].view(np.int32) if r0[k].dtype == np.float32 else r0[k], r1[k].view(np.int32) if r1[k].dtype == np.float32 else r1[k]), k
    # ---- each rank's average against the float64 replay of its own weights (on the device: 90 M elements) ----
    for tag, r in (("rank 0", r0), ("rank 1", r1)):
        mask = torch.from_numpy(r["mask"]).to(dev)
        t = {k: torch.from_numpy(r[k]).to(dev) for k in ("init", "post0", "post1", "ema")}
        e = t["init"][mask].double()
        M = float(e.abs().max())
        for w, d in zip((t["post0"][mask], t["post1"][mask]), r["decays"]):
            e = e + float(er.one_minus(d)) * (w.double() - e)                                  # ema_ref.ema_step, in torch float64
            M = max(M, float(w.abs().max()), float(e.abs().max()))
        head, _ = er.ema_replay(r["init"][r["mask"]][:4099], [r["post0"][r["mask"]][:4099], r["post1"][r["mask"]][:4099]], r["decays"])
        assert np.array_equal(e[:4099].cpu().numpy(), head)                                    # the device replay IS the host restatement
        err = float((t["ema"][mask].double() - e).abs().max())
        print(f"BOUND {exchange} {tag}: flat average max error {err:.3g} of {er.bound(2, M):.3g} (M = {M:.3g})")
        assert err <= er.bound(2, M), (tag, err, er.bound(2, M))
        assert torch.equal(t["ema"][~mask].view(torch.int32), t["init"][~mask].view(torch.int32))
        assert not torch.equal(t["ema"], t["init"]) and not torch.equal(t["ema"], t["post1"])
        want, Ms = er.ema_replay(r["small_init"], [r["small_post0"], r["small_post1"]], r["decays"])
        assert np.abs(r["ema_small"].astype(np.float64) - want).max() <= er.bound(2, Ms)
        del t, e
