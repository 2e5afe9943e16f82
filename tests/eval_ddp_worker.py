"""Worker of test_eval_stats_gpu.py: one of two ranks (gloo, both on GPU 0) accumulating its shard of a fixed set of
logits, then ``synchronize_between_processes``.  ``run_single`` is the one-process accumulator of both shards.

    python -m torch.distributed.run --nproc-per-node 2 tests/eval_ddp_worker.py <out_dir>
"""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, C = 300, 1000


def data():
    g = torch.Generator().manual_seed(20)
    x = (torch.randn(B, C, generator=g) * 4).cuda()
    t = torch.randint(0, C, (B,), generator=g).cuda()
    tab = (torch.rand(C, generator=g) + 0.5).cuda()
    return x, t, tab


def shard(rank):
    return slice(0, 113) if rank == 0 else slice(113, B)


def accumulator(tab):
    from iif_amd.eval_stats import EvalAccumulator
    return EvalAccumulator(C, topk=(1, 5), num_bins=15, table=tab, device="cuda:0")


def run_single():
    x, t, tab = data()
    a = accumulator(tab)
    for r in (0, 1):
        a.update(x[shard(r)], t[shard(r)])
    return a.acc.cpu()


if __name__ == "__main__":
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    x, t, tab = data()
    a = accumulator(tab)
    a.update(x[shard(rank)], t[shard(rank)])
    a.synchronize_between_processes()
    torch.save(a.acc.cpu(), os.path.join(sys.argv[1], "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()
