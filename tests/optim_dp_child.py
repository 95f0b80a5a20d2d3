"""Helper of tests/test_gpu_optim_dp.py (not a test module): ONE data-parallel rank in a fresh process, in the manner of tests/dp_child.py.
    python tests/optim_dp_child.py RANK WORLD PORT OUTDIR BACKEND
attach() + one accumulation window of TWO micro-batches through harness.train_epoch (the loop train.py runs), the exchange's stage hook wrapped so
that the parent can see which micro-batch issued reductions.  Rank r sees the shards (7, 14)[r] then (14, 7)[r]: at each micro-batch the ranks hold
different data, and the window's four batches are the ones the parent accumulates in one process."""
import os
import sys

rank, world, port, outdir, backend = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
import numpy as np
import torch
import torch.distributed as dist

ndev = torch.cuda.device_count()
dev = torch.device("cuda", rank % max(ndev, 1))
if backend == "nccl":
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
else:
    dist.init_process_group(backend, rank=rank, world_size=world)
torch.cuda.set_device(dev)

from md_rdm_amd import filler, harness, parallel
from md_rdm_amd.network.RDM_Net import DepthEstimationNet

model = DepthEstimationNet()
filler.fill_state_dict(model.state_dict())
model = model.to(dev).train()
model.flatten_parameters()
sync = parallel.attach(model)
opt = harness.FusedAdamW(model, lr=1e-4)
opt.attach_sync(sync)
flat, gflat, _ = model._flat
init = flat.detach().clone()

micro = [0]
hook_calls, exchange_calls = [0, 0], [0, 0]                 # per micro-batch: stage hooks fired / reductions issued
issue = sync.on_stage


def counted_exchange(stage):
    exchange_calls[micro[0]] += 1
    return issue(stage)


sync.on_stage = counted_exchange                            # the optimiser's hook looks the exchange up when it fires
inner = model.grad_ready_hook


def counted_hook(stage):
    hook_calls[micro[0]] += 1
    return inner(stage)


model.grad_ready_hook = counted_hook
losses = []


def batches():
    for seed in ((7, 14), (14, 7))[rank]:
        x, y = filler.synthetic_batch(2, 228, 228, seed=seed)
        yield torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)


def step_fn(m, x, y):
    micro[0] = len(losses)                                  # (the loop holds one batch ahead: the index is taken here, not where the batch is made)
    loss, parts = harness.training_step(m, x, y)
    losses.append(loss.detach())
    return loss, parts


steps = harness.train_epoch(model, opt, batches(), accumulate=2, sync=sync, step_fn=step_fn)
torch.cuda.synchronize()
print(f"rank {rank}: {steps} optimiser step(s), mode {opt.mode!r}, hooks {hook_calls}, reductions {exchange_calls}", flush=True)
np.savez(os.path.join(outdir, f"rank{rank}.npz"), init=init.cpu().numpy(), gsum=gflat.detach().cpu().numpy(), post=flat.detach().cpu().numpy(),
         losses=np.array([float(v) for v in losses]), steps=np.array(steps), hook_calls=np.array(hook_calls), exchange_calls=np.array(exchange_calls),
         step_count=np.array(opt.step_count), n_slices=np.array(len(sync.slices)),
         **{"wlg_" + n: p.grad.detach().cpu().numpy() for n, p in model.weight_layer.named_parameters() if p.grad is not None},
         **{"wlp_" + n: p.detach().cpu().numpy() for n, p in model.weight_layer.named_parameters() if p.numel()})
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "done", flush=True)
