"""Worker of test_lt_gpu.py: one of two ranks (gloo, both on GPU 0) drawing one training epoch of DeviceLTLoader over the
same .npy list-file tree.

    python -m torch.distributed.run --nproc-per-node 2 tests/lt_ddp_worker.py <root> <train list> <out_dir>
"""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


if __name__ == "__main__":
    from iif_amd.imbalanced_dataset import LT_Dataset
    from iif_amd.lt_device import DeviceLTLoader
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    root, train_txt, out_dir = sys.argv[1:4]
    ds = LT_Dataset(root, train_txt, 5)
    loader = DeviceLTLoader(ds, 4, train=True, size=32, seed=3, distributed=True, workers=0, device="cuda:0")
    loader.set_epoch(1)
    out = {"targets_all": ds.targets, "index": torch.from_numpy(loader.indices())}
    batches = [(x.cpu(), t.cpu()) for x, t in loader]
    out["targets"] = torch.cat([t for _, t in batches])
    out["images"] = batches[0][0]
    torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()
