"""Worker of test_rmsprop_gpu.py: one data-parallel rank stepping with RMSprop.

``same <out_dir> <steps>``: every rank feeds the SAME batch through the bucketed reducer, so the averaged gradient (sum of
two equal gradients times grad_scale 1/2) equals the single-process gradient bit for bit, and so do the parameters and the
RMSprop state after ``steps`` fused RMSprop launches.  ``run(..., with_reducer=False)`` is that single-process run.

``cli <out_dir> <train.py arguments...>``: ``iif_amd.train.main`` as ``python -m iif_amd.train`` runs it, keeping the model
so that each rank can save its parameters and RMSprop state (the checkpoint holds rank 0's only)."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _state(net):
    return {"params": net.param_arena.detach().cpu(), "sq": net._sq_arena.detach().cpu(),
            "mom": net._mom_arena.detach().cpu()}


def run(out_path, steps, with_reducer):
    import ddp_gpu_worker as W
    from iif_amd.ddp import broadcast_parameters
    dev = W._device()
    net, crit = W._setup(dev)
    reducer = None
    if with_reducer:
        broadcast_parameters(net)
        reducer = net.make_reducer(bucket_bytes=256 << 10)
    x, y = W._batch(dev, 0)
    scale = reducer.grad_scale if reducer is not None else 1.0
    losses = []
    for _ in range(steps):
        loss, _ = net.loss_and_backward(x, y, crit, reducer=reducer)
        net.rmsprop_step(1e-3, 0.9, 0.0316, 1e-4, 0.9, grad_scale=scale)
        losses.append(float(loss.item()))
    torch.cuda.synchronize()
    out = _state(net)
    out["losses"] = losses
    torch.save(out, out_path)


def cli(out_dir, argv):
    from iif_amd import train
    seen = {}
    inner = train.train_one_epoch

    def keep(model, *a, **k):
        seen["model"] = model
        return inner(model, *a, **k)
    train.train_one_epoch = keep
    train.main(train.get_args_parser().parse_args(argv))
    torch.cuda.synchronize()
    rank = dist.get_rank() if dist.is_initialized() else 0
    torch.save(_state(seen["model"]), os.path.join(out_dir, "rank%d.pt" % rank))
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    mode, out_dir = sys.argv[1], sys.argv[2]
    if mode == "cli":
        cli(out_dir, sys.argv[3:])
    else:
        dist.init_process_group("gloo")
        run(os.path.join(out_dir, "rank%d.pt" % dist.get_rank()), int(sys.argv[3]), True)
        dist.barrier()
        dist.destroy_process_group()
