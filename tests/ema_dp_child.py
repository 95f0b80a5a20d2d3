"""Helper of tests/test_gpu_ema_dp.py (not a test module): ONE data-parallel rank in a fresh process, in the manner of tests/optim_dp_child.py.
    python tests/ema_dp_child.py RANK WORLD PORT OUTDIR BACKEND EXCHANGE
attach(exchange=EXCHANGE) + TWO real training steps with FusedAdamW(ema_decay=0.9) through the per-stage update (opt.step(sync=sync)), the weights
recorded after each; then state_dict() (which completes the average on every rank under "reduce_scatter") and one pass through ema_weights(), whose
two comparisons (the model holds the average inside, everything is back afterwards) are made here, bit for bit, and handed over as flags.  The parent
compares the ranks and replays the average in float64."""
import os
import sys

rank, world, port, outdir, backend, exchange = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6]
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
sync = parallel.attach(model, exchange=exchange)
opt = harness.FusedAdamW(model, lr=1e-3, ema_decay=0.9)
opt.attach_sync(sync)
flat, gflat, entries = model._flat
smalls = [p for p in model.weight_layer.parameters() if p.requires_grad]
init, small_init = flat.detach().clone(), torch.stack([p.detach().reshape(()) for p in smalls]).clone()
posts, small_posts, decays = [], [], []
for step, seeds in enumerate(((7, 14), (14, 7))):                # the ranks hold different data at every step
    x, y = filler.synthetic_batch(2, 228, 228, seed=seeds[rank])
    opt.zero_grad()
    loss, _ = harness.training_step(model, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    loss.backward()
    decays.append(harness.ema_decay_at(0.9, opt.ema_updates, True))
    opt.step(sync=sync)
    torch.cuda.synchronize()
    posts.append(flat.detach().clone())
    small_posts.append(torch.stack([p.detach().reshape(()) for p in smalls]).clone())
print(f"rank {rank}: {opt.step_count} steps over {sync.exchange}, mode {opt.mode!r}, {opt.ema_updates} updates of the average", flush=True)
sd = opt.state_dict()                                            # all-gathers the moments and the average where the ranks hold shards
mask = torch.zeros(flat.numel(), dtype=torch.bool, device=dev)
for k, p, o, n, _ in entries:
    if p.requires_grad and not k.startswith("d_1.conv1."):
        mask[o:o + n] = True
ema_before = sd["ema"].to(dev)
eq = lambda a, b: bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))
with opt.ema_weights():
    torch.cuda.synchronize()
    inside_ok = eq(flat[mask], ema_before[mask]) and eq(opt.ema[mask], posts[1][mask])
torch.cuda.synchronize()
after_ok = eq(flat, posts[1]) and eq(opt.ema, ema_before)
np.savez(os.path.join(outdir, f"rank{rank}.npz"), init=init.cpu().numpy(), post0=posts[0].cpu().numpy(), post1=posts[1].cpu().numpy(), ema=sd["ema"].numpy(),
         ema_small=torch.stack([e.reshape(()) for e in sd["ema_small"]]).numpy(), small_init=small_init.cpu().numpy(), small_post0=small_posts[0].cpu().numpy(),
         small_post1=small_posts[1].cpu().numpy(), decays=np.array(decays), mask=mask.cpu().numpy(), updates=np.array(opt.ema_updates), mode=np.array(opt.mode),
         exchange=np.array(sync.exchange), inside_ok=np.array(inside_ok), after_ok=np.array(after_ok))
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "done", flush=True)
