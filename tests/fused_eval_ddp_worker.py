"""Worker of test_fused_eval_gpu.py: train.evaluate() on the synthetic CIFAR-100-LT test set with
``--shot-acc --calibration-bins 10``, once without and once with ``--fused-eval``, on the same seeded model.  ``run`` is the
one-process form; as a script it is one of two ranks (gloo, both on GPU 0):

    IIF_REHEARSE_ONE_GPU=1 python -m torch.distributed.run --nproc-per-node 2 tests/fused_eval_ddp_worker.py <out_dir>
"""
import contextlib
import io
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARGV = ["--model", "resnet32", "--dset_name", "cifar100", "--classif", "iif", "--iif", "raw", "-b", "128", "-j", "0",
        "--shot-acc", "--calibration-bins", "10"]


def seeded_model(args, num_classes):
    """The same model on every rank and in every run: seeded weights, running statistics and BN affine."""
    from iif_amd import train
    from iif_amd.resnet_engine import BNParam
    torch.manual_seed(4321)
    model = train.build_model(args, num_classes)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, BNParam):
                c = m.num_features
                m.running_mean.copy_((torch.randn(c, generator=g) * 0.2).cuda())
                m.running_var.copy_((torch.rand(c, generator=g) * 1.5 + 0.25).cuda())
                m.weight.copy_((torch.rand(c, generator=g) * 0.8 + 0.4).cuda())
                m.bias.copy_((torch.randn(c, generator=g) * 0.1).cuda())
    return model


def run(fused, group=None):
    """The three report lines of evaluate() (accuracy, shot split, calibration), as printed on the main process.
    ``group``: the parsed arguments utils.init_distributed_mode filled in (this process is one rank of it)."""
    from iif_amd import initialisers, train
    args = train.get_args_parser().parse_args(ARGV + (["--fused-eval"] if fused else []))
    args.distributed = group is not None
    if group is not None:
        args.rank, args.world_size, args.gpu, args.dist_backend = group.rank, group.world_size, group.gpu, group.dist_backend
    dataset, num_classes, _, loader_test, _ = initialisers.get_data(args)
    model = seeded_model(args, num_classes)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.enable_fused_eval(model, args)
        criterion = initialisers.get_criterion(args, dataset, model, num_classes)
        stats = train.make_eval_stats(args, num_classes)
        train.evaluate(model, criterion, loader_test, device=torch.device("cuda"), stats=stats, train_targets=dataset.targets)
    text = buf.getvalue()
    lines = [l.strip() for l in text.splitlines() if re.match(r"\s*(\* Acc@1|Many shot Acc is|ECE is)", l)]
    return {"lines": lines, "fused": model.fused_eval, "summary": "fused eval: fused" in text}


if __name__ == "__main__":
    import torch.distributed as dist
    from iif_amd import train, utils
    group = train.get_args_parser().parse_args(ARGV)
    utils.init_distributed_mode(group)
    plain, fused = run(False, group), run(True, group)
    torch.save({"plain": plain, "fused": fused, "world": dist.get_world_size()},
               os.path.join(sys.argv[1], "rank%d.pt" % dist.get_rank()))
    dist.barrier()
    dist.destroy_process_group()
