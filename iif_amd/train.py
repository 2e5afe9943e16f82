"""Training entry point with the command line of the reference's
``classification/train.py`` (flags :288-392, loop :39-92, evaluate :95-119,
main :168-285), running on the native MI355X engine.

    python -m iif_amd.train --model resnet32 --dset_name cifar100 --classif iif --iif raw -b 128 --epochs 2
    python -m torch.distributed.run --nproc-per-node 8 -m iif_amd.train --model resnet50 --dset_name imagenet_lt ...

Differences, all forced by the environment or by the MI355X-first design:
  * without ``--data-path`` the datasets are synthetic long-tailed sets (no torchvision / network); CIFAR-10 / -100
    with ``--data-path`` are read from their files and augmented on the device (iif_amd/cifar.py); the list datasets
    are too with ``--device-augment`` (iif_amd/lt_device.py), their auto-augment policies with ``--device-policy``;
  * the step is the fused native one — forward, fused IIF loss (+mixup), backward,
    bucketed RCCL all-reduce overlapped with backward, ONE fused SGD or RMSprop launch — instead of
    autograd + torch.optim + DistributedDataParallel; schedules are evaluated on the host
    and passed to the kernel, optimizer state lives in the model's arenas;
  * metrics are read back every ``--print-freq`` iterations (the reference syncs the host
    three times per iteration, train.py:87-92);
  * new flags: ``--compute-dtype {bf16,f32}``, ``--max-iters``.
"""
import argparse
import datetime
import math
import os
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")     # distinct hardware queues for the main / wgrad / RCCL streams

import torch   # noqa: E402

from . import custom, initialisers, resnet_cifar, resnet_pytorch, utils
from .ddp import broadcast_parameters, sync_buffers

OPTIMIZERS = ("sgd", "nesterov", "rmsprop")
RMSPROP_ALPHA, RMSPROP_EPS = 0.9, 0.0316            # the reference's RMSprop constants (train.py:205-207)


def lr_at(args, epoch, it, iters_per_epoch):
    """Learning rate of iteration ``it`` of ``epoch``: MultiStep / cosine per epoch
    (train.py:223-228) times the linear warm-up of the first epoch (train.py:52-56)."""
    if args.cosine_scheduler:
        base = args.lr * (1 + math.cos(math.pi * epoch / args.epochs)) / 2
    else:
        base = args.lr * (args.lr_gamma ** sum(1 for m in args.milestones if epoch >= m))
    if epoch < 1:
        warm_iters = min(1000, iters_per_epoch - 1)
        base *= utils.warmup_factor(it, warm_iters, 1.0 / 1000) if warm_iters > 0 else 1.0
    return base


def scheduler_state_dict(args, last_epoch):
    """State of the reference's per-epoch scheduler (train.py:223-228) after ``last_epoch`` steps."""
    lr = lr_at(args, last_epoch, 10 ** 9, 10 ** 9)
    sd = {"last_epoch": last_epoch, "_step_count": last_epoch + 1, "base_lrs": [args.lr], "_last_lr": [lr],
          "_get_lr_called_within_step": False, "verbose": False}
    if args.cosine_scheduler:
        sd.update({"T_max": args.epochs, "eta_min": 0})
    else:
        from collections import Counter
        sd.update({"milestones": Counter(args.milestones), "gamma": args.lr_gamma})
    return sd


def train_one_epoch(model, criterion, data_loader, device, epoch, args, reducer=None):
    model.train()
    logger = utils.MetricLogger(delimiter="  ")
    logger.add_meter("lr", utils.SmoothedValue(window_size=1, fmt="{value}"))
    logger.add_meter("img/s", utils.SmoothedValue(window_size=10, fmt="{value}"))
    header = "Epoch: [{}]".format(epoch)
    n_iters = len(data_loader)
    nesterov = args.opt.lower() == "nesterov"
    rmsprop = args.opt.lower() == "rmsprop"
    scale = reducer.grad_scale if reducer is not None else 1.0
    mix = custom.Mixup(criterion, alpha=args.mixup) if args.mixup is not None else None
    it = 0
    t_last, imgs_since = time.time(), 0
    for image, target in logger.log_every(data_loader, args.print_freq, header):
        image = image.to(device, non_blocking=True)
        target = target.to(device, non_blocking=True)
        lr = lr_at(args, epoch, it, n_iters)
        probe = reducer is not None and args.bf16_buckets and not getattr(reducer, "probed", False)
        red = None if probe else reducer
        if mix is not None:
            image, ta, tb, lam = mix(image, target)
            loss, output = model.loss_and_backward(image, ta, criterion, targets_b=tb, lam=lam, reducer=red)
        else:
            loss, output = model.loss_and_backward(image, target, criterion, reducer=red)
        if probe:
            # first step: gradients are still local; measure what bf16 buckets would do to their average, switch
            # only if that stays within one bf16 rounding, then reduce this step (un-overlapped)
            worst = reducer.probe_bf16()
            reducer.probed = True
            try:
                reducer.set_bucket_dtype(torch.bfloat16)
                print("bf16 gradient buckets enabled (probe: %.2e relative L2)" % worst)
            except RuntimeError:
                print("bf16 gradient buckets REFUSED (probe: %.2e relative L2 > tolerance); staying with fp32" % worst)
            reducer.begin()
            reducer.finish()
        if rmsprop:
            model.rmsprop_step(lr, RMSPROP_ALPHA, RMSPROP_EPS, args.weight_decay, args.momentum, grad_scale=scale)
        else:
            model.sgd_step(lr, args.momentum, args.weight_decay, nesterov, grad_scale=scale)
        imgs_since += image.shape[0]
        if it % args.print_freq == 0 or it == n_iters - 1:
            acc1, acc5 = utils.accuracy(output, target, topk=(1, min(5, output.shape[1])))
            now = time.time()                                   # .item() below is the only host sync
            logger.update(loss=loss.item(), lr=lr)
            model.check_labels()                                # out-of-range targets raise here (device assert in the reference)
            logger.meters["acc1"].update(acc1.item(), n=image.shape[0])
            logger.meters["acc5"].update(acc5.item(), n=image.shape[0])
            logger.meters["img/s"].update(imgs_since / max(now - t_last, 1e-9))
            t_last, imgs_since = time.time(), 0
        it += 1
        if args.max_iters and it >= args.max_iters:
            break


def evaluate(model, criterion, data_loader, device, print_freq=100, stats=None, train_targets=None):
    """``stats`` (an eval_stats.EvalAccumulator, --shot-acc / --calibration-bins): also fed every batch, then reduced over
    the ranks and reported after the accuracy line (the shot split when ``train_targets`` is given)."""
    model.eval()
    logger = utils.MetricLogger(delimiter="  ")
    with torch.no_grad():
        for image, target in logger.log_every(data_loader, print_freq, "Test:"):
            image = image.to(device, non_blocking=True)
            target = target.to(device, non_blocking=True)
            output = model(image)
            if hasattr(criterion, "iif"):
                output = criterion(output, infer=True)
            acc1, acc5 = utils.accuracy(output, target, topk=(1, min(5, output.shape[1])))
            if stats is not None:
                stats.update(output, target)
            n = image.shape[0]
            logger.meters["acc1"].update(acc1.item(), n=n)
            logger.meters["acc5"].update(acc5.item(), n=n)
    logger.synchronize_between_processes()
    print(" * Acc@1 {top1.global_avg:.3f} Acc@5 {top5.global_avg:.3f}".format(top1=logger.acc1, top5=logger.acc5))
    if stats is not None:
        report_eval_stats(stats, train_targets)
    return logger.acc1.global_avg


def make_eval_stats(args, num_classes):
    """The accumulator of --shot-acc / --calibration-bins, or None when neither is set (the evaluation of the reference)."""
    if not (getattr(args, "shot_acc", False) or getattr(args, "calibration_bins", 0)):
        return None
    from .eval_stats import EvalAccumulator
    return EvalAccumulator(num_classes, topk=(1, min(5, num_classes)), num_bins=args.calibration_bins, device=args.device)


def report_eval_stats(stats, train_targets):
    stats.synchronize_between_processes()
    r = stats.result(train_targets=train_targets)
    stats.reset()
    if r["shot"] is not None:
        many, median, low = r["shot"]
        print(f"Many shot Acc is: {many}, median shot Acc is: {median}, low shot Acc is: {low}")
    if r["calibration"] is not None:
        cal = r["calibration"]
        print("ECE is: {}, MCE is: {} ({} bins)".format(cal["expected_calibration_error"], cal["max_calibration_error"],
                                                        stats.num_bins))


def build_model(args, num_classes):
    """train.py:184-187: look the constructor up in resnet_pytorch, then resnet_cifar."""
    cdt = torch.bfloat16 if args.compute_dtype == "bf16" else torch.float32
    kw = dict(num_classes=num_classes, use_norm=str(args.classif_norm), device=args.device, compute_dtype=cdt)
    if hasattr(resnet_pytorch, args.model):
        return getattr(resnet_pytorch, args.model)(pretrained=str(args.pretrained), **kw)
    if hasattr(resnet_cifar, args.model):
        return getattr(resnet_cifar, args.model)(**kw)
    raise AttributeError("unknown model %r" % (args.model,))


def enable_fused_eval(model, args):
    """--fused-eval: evaluation forwards with eval-mode BN folded into the convolution epilogues (NativeResNet.set_fused_eval);
    prints the route summary once."""
    if not getattr(args, "fused_eval", False):
        return model
    model.set_fused_eval(True)
    size = 32 if args.dset_name.lower().startswith("cifar") else getattr(args, "image_size", 224)
    route = model.eval_route(args.batch_size, size, size)
    unfused = [name for (name, r) in route if r.startswith("unfused")]
    print("fused eval: fused %d of %d units (%d shortcut convolutions stored raw; unfused: %s)"
          % (sum(r == "fused" for (_, r) in route), len(route), sum(r == "raw" for (_, r) in route), ", ".join(unfused) or "none"))
    return model


HOST_POLICIES = ("imagenet", "randaugment", "cifar", "cifar10")
DEVICE_POLICIES = HOST_POLICIES                        # lt_device.POLICIES: what --device-policy runs


def check_device_augment(args):
    """--device-augment builds the list datasets' batches on the device: it needs --data-path and refuses the auto-augment
    policies unless --device-policy runs them on the device too.  CIFAR is built on the device already (the flag changes
    nothing there)."""
    device_policy = getattr(args, "device_policy", False)
    augment_on_device = getattr(args, "device_augment", False)
    if device_policy and not augment_on_device:
        raise SystemExit("--device-policy needs --device-augment: the policy runs in the device pipeline that flag builds")
    if getattr(args, "device_decode", False) and not augment_on_device:
        raise SystemExit("--device-decode needs --device-augment: the decoded regions feed the device pipeline that flag builds")
    if not augment_on_device:
        return
    if not getattr(args, "data_path", ""):
        raise SystemExit("--device-augment needs --data-path: it builds batches from the dataset's files, and the synthetic "
                         "sets have none")
    name = args.dset_name.lower()
    if getattr(args, "device_decode", False) and name.startswith("cifar"):
        raise SystemExit("--device-decode decodes the list datasets' JPEG files; CIFAR reads pickled arrays")
    policy = getattr(args, "auto_augment", None)
    if device_policy:
        if policy in (None, "", "None"):
            raise SystemExit("--device-policy needs --auto-augment %s" % " | ".join(DEVICE_POLICIES))
        if policy not in DEVICE_POLICIES:
            raise SystemExit("--device-policy does not know --auto-augment %r (%s)" % (policy, ", ".join(DEVICE_POLICIES)))
        return
    if not name.startswith("cifar") and policy in HOST_POLICIES:
        raise SystemExit("--device-augment does not run --auto-augment %s: that policy stays on the host; drop one of the two "
                         "flags; add --device-policy to run it on the device" % (policy,))


def report_decode_failures(epoch, train_loader, eval_loader):
    """--device-decode: the images of this epoch (training and evaluation loaders, this rank) whose scan the device could
    not decode; both counts restart.  Printed by the main process."""
    n_train, n_eval = train_loader.decode_failures(reset=True), eval_loader.decode_failures(reset=True)
    if utils.is_main_process():
        print("epoch %d: device JPEG decode failures: train %d, eval %d" % (epoch, n_train, n_eval))


def main(args):
    check_device_augment(args)
    if args.output_dir:
        utils.mkdir(args.output_dir)
    utils.init_distributed_mode(args)
    if not torch.cuda.is_available():
        raise SystemExit("iif_amd.train needs an MI355X: the native engine has no CPU path")
    device = torch.device(args.device)
    print(args)
    if getattr(args, "auto_augment", None) and not getattr(args, "data_path", None):
        import warnings
        warnings.warn("--auto-augment %r applies to the list datasets (--data-path); the synthetic long-tailed data of this run "
                      "is not augmented" % (args.auto_augment,))
    dataset, num_classes, data_loader, data_loader_test, train_sampler = initialisers.get_data(args)
    print("Creating model")
    model = build_model(args, num_classes)
    enable_fused_eval(model, args)
    criterion = initialisers.get_criterion(args, dataset, model, num_classes)
    if args.sync_bn and args.distributed:
        model.enable_sync_bn()                # train.py:190-191: batch statistics over all ranks
    if args.opt.lower() not in OPTIMIZERS:
        raise RuntimeError("Invalid optimizer {}. Only SGD and RMSprop are supported.".format(args.opt))
    if args.decoup:
        model.select_training_param()       # train.py:123-145: classifier-only stage
    reducer = None
    if args.distributed:
        broadcast_parameters(model)
        reducer = model.make_reducer(mode=args.reduce_mode)
    if args.resume:
        # the reference's checkpoint dict (train.py:265-271): model / optimizer / lr_scheduler / epoch / args
        ckpt = torch.load(args.resume, map_location="cpu", weights_only=False)
        model.load_state_dict(ckpt["model"])
        if "optimizer" in ckpt:
            model.load_optimizer_state_dict(ckpt["optimizer"], optimizer=args.opt)
        args.start_epoch = ckpt["epoch"] + 1
    if args.load_from:
        model.load_state_dict(torch.load(args.load_from, map_location="cpu", weights_only=False)["model"])
    stats = make_eval_stats(args, num_classes)
    shot_targets = dataset.targets if getattr(args, "shot_acc", False) else None
    if args.test_only:
        evaluate(model, criterion, data_loader_test, device=device, stats=stats, train_targets=shot_targets)
        return
    print("Start training")
    start_time = time.time()
    best_acc = 0
    for epoch in range(args.start_epoch, args.epochs):
        if args.distributed or hasattr(train_sampler, "set_epoch"):     # the device CIFAR loader re-draws per epoch
            train_sampler.set_epoch(epoch)
        train_one_epoch(model, criterion, data_loader, device, epoch, args, reducer)
        if args.distributed:
            sync_buffers(model)               # rank 0's BN statistics everywhere, as DDP's broadcast_buffers
        acc = evaluate(model, criterion, data_loader_test, device=device, stats=stats, train_targets=shot_targets)
        if getattr(data_loader, "decode", "host") == "device":
            report_decode_failures(epoch, data_loader, data_loader_test)
        best_acc = max(best_acc, acc)
        if args.output_dir:
            nxt = lr_at(args, epoch + 1, 10 ** 9, 10 ** 9)
            if args.opt.lower() == "rmsprop":
                opt_sd = model.rmsprop_state_dict(nxt, RMSPROP_ALPHA, RMSPROP_EPS, args.weight_decay, args.momentum, False,
                                                  initial_lr=args.lr)
            else:
                opt_sd = model.optimizer_state_dict(nxt, args.momentum, args.weight_decay, args.opt.lower() == "nesterov",
                                                    initial_lr=args.lr)
            ckpt = {"model": model.state_dict(),
                    "optimizer": opt_sd,
                    "lr_scheduler": scheduler_state_dict(args, epoch + 1),
                    "epoch": epoch, "args": args}
            utils.save_on_master(ckpt, os.path.join(args.output_dir, "model_{}.pth".format(epoch)))
            utils.save_on_master(ckpt, os.path.join(args.output_dir, "checkpoint.pth"))
    print("Training time {}".format(datetime.timedelta(seconds=int(time.time() - start_time))))
    print("best acc is:", best_acc)


def get_args_parser(add_help=True):
    p = argparse.ArgumentParser(description="IIF classification training on MI355X", add_help=add_help)
    p.add_argument("--data-path", default="", help="dataset root of the list files or of the CIFAR python folders; "
                   "empty = synthetic long-tailed sets")
    p.add_argument("--train-txt", dest="train_txt", default=None, help="training list (default: the reference's path for --dset_name)")
    p.add_argument("--eval-txt", dest="eval_txt", default=None, help="evaluation list (default: the reference's path)")
    p.add_argument("--image-size", dest="image_size", default=224, type=int)
    p.add_argument("--dset_name", default="cifar100", help="cifar10|cifar100|imagenet_lt|places_lt|inat18 (synthetic)")
    p.add_argument("--rand_number", default=0, type=int)
    p.add_argument("--imb_type", default="exp", type=str)
    p.add_argument("--imb_factor", default=0.01, type=float)
    p.add_argument("--model", default="resnet32")
    p.add_argument("--device", default="cuda")
    p.add_argument("-b", "--batch-size", default=32, type=int)
    p.add_argument("--epochs", default=400, type=int, metavar="N")
    p.add_argument("-j", "--workers", default=4, type=int, metavar="N")
    p.add_argument("--opt", default="sgd", type=str)
    p.add_argument("--lr", default=0.1, type=float)
    p.add_argument("--cosine_scheduler", action="store_true")
    p.add_argument("--momentum", default=0.9, type=float, metavar="M")
    p.add_argument("--wd", "--weight-decay", default=1e-4, type=float, metavar="W", dest="weight_decay")
    p.add_argument("--milestones", nargs="+", default=[360, 380], type=int)
    p.add_argument("--lr-gamma", default=0.1, type=float)
    p.add_argument("--print-freq", default=100, type=int)
    p.add_argument("--output-dir", default="", help="path where to save")
    p.add_argument("--resume", default="")
    p.add_argument("--load_from", default="")
    p.add_argument("--classif", default="ce", type=str)
    p.add_argument("--classif_norm", default=None, type=str)
    p.add_argument("--gamma", default=0.0, type=float)
    p.add_argument("--alpha", default=None, type=float)
    p.add_argument("--iif", default="raw", type=str)
    p.add_argument("--iif_norm", default=0, type=int)
    p.add_argument("--decoup", action="store_true")
    p.add_argument("--mixup", default=None, type=float)
    p.add_argument("--sampler", default="random", type=str)
    p.add_argument("--reduction", default="mean", type=str)
    p.add_argument("--start-epoch", default=0, type=int, metavar="N")
    p.add_argument("--cache-dataset", dest="cache_dataset", action="store_true")
    p.add_argument("--sync-bn", dest="sync_bn", action="store_true",
                   help="cross-replica BN statistics (reference train.py:190); rehearsed over gloo and one RCCL rank only")
    p.add_argument("--test-only", dest="test_only", action="store_true")
    p.add_argument("--pretrained", dest="pretrained", default=None, type=str)
    p.add_argument("--deffered", action="store_true")
    p.add_argument("--auto-augment", default=None)
    p.add_argument("--device-augment", dest="device_augment", action="store_true",
                   help="list datasets with --data-path: resize, flip, ColorJitter and Normalize each batch on the device "
                   "(iif_amd/lt_device.py) instead of in the DataLoader workers")
    p.add_argument("--device-policy", dest="device_policy", action="store_true",
                   help="with --device-augment: run the --auto-augment policy (imagenet, randaugment, cifar) on the device "
                   "too, in place of ColorJitter (iif_lt_augment_policy)")
    p.add_argument("--device-decode", dest="device_decode", action="store_true",
                   help="with --device-augment: decode the baseline JPEG files on the device (iif_amd/jpeg.py); the workers "
                   "only read and parse them, and decode every other file as before")
    p.add_argument("--random-erase", default=0.0, type=float)
    p.add_argument("--apex", action="store_true")
    p.add_argument("--apex-opt-level", default="O2", type=str)
    p.add_argument("--world-size", default=1, type=int)
    p.add_argument("--dist-url", default="env://")
    p.add_argument("--record-result", dest="record_result", action="store_true")
    # MI355X-native additions
    p.add_argument("--compute-dtype", default="bf16", choices=["bf16", "f32"])
    p.add_argument("--reduce-mode", dest="reduce_mode", default="allreduce", choices=["allreduce", "rs_ag"],
                   help="gradient buckets: one all_reduce each, or reduce_scatter + all_gather")
    p.add_argument("--bf16-buckets", dest="bf16_buckets", action="store_true",
                   help="reduce bf16 copies of the gradient buckets (refused unless the first step's probe stays in tolerance)")
    p.add_argument("--max-iters", default=0, type=int, help="stop each epoch after this many iterations (0 = all)")
    p.add_argument("--synthetic-scale", dest="synthetic_scale", default=1.0, type=float)
    p.add_argument("--fused-eval", dest="fused_eval", action="store_true",
                   help="evaluate with eval-mode BN folded into the convolution epilogues (one launch per conv + BN + ReLU unit, "
                        "bit-identical logits; bf16 compute only)")
    p.add_argument("--shot-acc", dest="shot_acc", action="store_true",
                   help="after each evaluation also print the many / median / low-shot accuracy (per_shot_acc.shot_acc)")
    p.add_argument("--calibration-bins", dest="calibration_bins", default=0, type=int,
                   help="after each evaluation also print ECE / MCE over this many reliability bins (0 = off)")
    return p


if __name__ == "__main__":
    main(get_args_parser().parse_args())
