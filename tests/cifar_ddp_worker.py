"""Worker of test_cifar_gpu.py: one of two ranks (gloo, both on GPU 0) drawing two training epochs and the evaluation
shard of DeviceCIFARLoader over the same fake CIFAR set.

    python -m torch.distributed.run --nproc-per-node 2 tests/cifar_ddp_worker.py <out_dir>
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dataset(n):
    from iif_amd.cifar import CIFARData
    rows = np.random.RandomState(n).randint(0, 256, size=(n, 3072)).astype(np.uint8)
    return CIFARData(rows, np.arange(n) % 10, 10)


if __name__ == "__main__":
    from iif_amd.cifar import DeviceCIFARLoader
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    ds = dataset(370)
    loader = DeviceCIFARLoader(ds, 32, train=True, flags=7, seed=3, distributed=True, device="cuda:0")
    out = {"targets_all": ds.targets}
    for e in (0, 1):
        loader.set_epoch(e)
        out["index%d" % e] = torch.from_numpy(loader.indices())
        batches = list(loader)
        out["targets%d" % e] = torch.cat([t for _, t in batches]).cpu()
        out["images%d" % e] = batches[0][0].cpu()
    ev = DeviceCIFARLoader(dataset(100), 32, train=False, flags=0, distributed=True, device="cuda:0")
    out["eval"] = ev.indices().tolist()
    torch.save(out, os.path.join(sys.argv[1], "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()
