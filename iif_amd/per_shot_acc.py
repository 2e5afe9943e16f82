"""Many / median / low-shot accuracy report (what classification/per_shot_acc.py:62-106 returns), as three
``np.bincount`` passes over the label space instead of a per-class scan: host-side integer counting.

    python -m iif_amd.per_shot_acc --dset_name imagenet_lt --model resnet50 --load_from checkpoint.pth --classif iif

runs the reference script's evaluation (``main``) on the native engine with the counts accumulated on the device
(``eval_stats.EvalAccumulator``)."""
import numpy as np
import torch


def _as_int_array(v, what):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    elif not isinstance(v, (np.ndarray, list, tuple)):
        raise TypeError("Type ({}) of {} not supported".format(type(v), what))
    return np.asarray(v).astype(np.int64).reshape(-1)


def shot_acc(preds, labels, train_targets, many_shot_thr=100, low_shot_thr=20, acc_per_cls=False):
    """Mean per-class accuracy over the classes PRESENT in ``labels``, split by how often the class occurs in the
    training set: many (> many_shot_thr), low (< low_shot_thr), median (the rest).  An empty split reports 0.
    With ``acc_per_cls`` the per-class accuracies (ascending class id, present classes only) are appended."""
    if not isinstance(preds, (torch.Tensor, np.ndarray)):
        raise TypeError("Type ({}) of preds not supported".format(type(preds)))
    pred, gt, seen = _as_int_array(preds, "preds"), _as_int_array(labels, "labels"), _as_int_array(train_targets, "train_targets")
    width = int(max(gt.max(initial=-1), seen.max(initial=-1))) + 1
    n_test = np.bincount(gt, minlength=width)
    n_hit = np.bincount(gt[pred == gt], minlength=width)
    n_train = np.bincount(seen, minlength=width)
    present = n_test > 0
    acc = n_hit[present] / n_test[present]
    freq = n_train[present]
    splits = (freq > many_shot_thr, (freq <= many_shot_thr) & (freq >= low_shot_thr), freq < low_shot_thr)
    many, median, low = (acc[sel].mean() if sel.any() else np.float64(0) for sel in splits)
    if acc_per_cls:
        return many, median, low, list(acc)
    return many, median, low


def main(args):
    """classification/per_shot_acc.py:main on the native engine: evaluate ``--load_from`` on the test set, with the IIF
    table applied under ``--classif iif``, and print the top-1 accuracy and the many / median / low-shot split (plus ECE /
    MCE with ``--calibration-bins``).  Every batch is one iif_eval_accumulate launch on the engine's logits; the host
    reads the counts once, at the end."""
    from . import custom, initialisers, train
    from .eval_stats import EvalAccumulator
    if not torch.cuda.is_available():
        raise SystemExit("iif_amd.per_shot_acc needs an MI355X: the native engine has no CPU path")
    device = torch.device(args.device)
    dataset, num_classes, _, data_loader_test, _ = initialisers.get_data(args)
    model = train.build_model(args, num_classes)
    train.enable_fused_eval(model, args)
    table = None
    if args.classif == "iif":
        crit = custom.IIFLoss(dataset, variant=args.iif, iif_norm=0, reduction="mean", device=args.device)
        table = crit.iif[args.iif]
    if args.load_from:
        model.load_state_dict(torch.load(args.load_from, map_location="cpu", weights_only=False)["model"])
    else:
        print("no --load_from: evaluating the initial weights")
    model.eval()
    stats = EvalAccumulator(num_classes, topk=(1, min(5, num_classes)), num_bins=args.calibration_bins, table=table,
                            device=device)
    with torch.no_grad():
        for image, target in data_loader_test:
            image = image.to(device, non_blocking=True)
            target = target.to(device, non_blocking=True)
            stats.update(model.run_forward(image, False), target)       # the engine's padded logits, no copy
    r = stats.result(train_targets=dataset.targets)
    top1, top5 = (r["topk"][k] for k in stats.topk)
    print(" * Acc@1 {:.3f} Acc@5 {:.3f}".format(top1, top5))
    print(f"Avg Acc is: {top1}")
    many, median, low = r["shot"]
    print(f"Many shot Acc is: {many}, median shot Acc is: {median}, low shot Acc is: {low}")
    if r["calibration"] is not None:
        cal = r["calibration"]
        print("ECE is: {}, MCE is: {} ({} bins)".format(cal["expected_calibration_error"], cal["max_calibration_error"],
                                                        args.calibration_bins))
    return 0


def get_args_parser(add_help=True):
    """The reference script's flags (per_shot_acc.py:147-172) and the data / engine flags of iif_amd.train it needs."""
    import argparse
    p = argparse.ArgumentParser(description="Many / median / low-shot accuracy of a checkpoint on MI355X", add_help=add_help)
    p.add_argument("--distributed", default=False)
    p.add_argument("--dset_name", default="imagenet_lt", type=str, help="imagenet_lt|places_lt|inat18|cifar10|cifar100")
    p.add_argument("--data-path", default="", help="dataset root of the list files or of the CIFAR python folders; "
                   "empty = synthetic long-tailed sets")
    p.add_argument("--auto-augment", default=None)
    p.add_argument("--sampler", default="random", type=str)
    p.add_argument("--iif", default="raw", type=str)
    p.add_argument("--classif", default="ce", type=str)
    p.add_argument("--classif_norm", default=None, type=str)
    p.add_argument("--load_from", default="")
    p.add_argument("-j", "--workers", default=4, type=int, metavar="N")
    p.add_argument("-b", "--batch-size", default=256, type=int)
    p.add_argument("--model", default="resnet50")
    p.add_argument("--apex", action="store_true", help="accepted and ignored (no apex on the native engine)")
    p.add_argument("--apex-opt-level", default="O2", type=str)
    # MI355X-native additions (same meaning as in iif_amd.train)
    p.add_argument("--calibration-bins", dest="calibration_bins", default=0, type=int,
                   help="also print ECE / MCE over this many reliability bins (0 = off)")
    p.add_argument("--fused-eval", dest="fused_eval", action="store_true",
                   help="eval-mode BN folded into the convolution epilogues (bit-identical logits; bf16 compute only)")
    p.add_argument("--train-txt", dest="train_txt", default=None)
    p.add_argument("--eval-txt", dest="eval_txt", default=None)
    p.add_argument("--image-size", dest="image_size", default=224, type=int)
    p.add_argument("--rand_number", default=0, type=int)
    p.add_argument("--imb_type", default="exp", type=str)
    p.add_argument("--imb_factor", default=0.01, type=float)
    p.add_argument("--synthetic-scale", dest="synthetic_scale", default=1.0, type=float)
    p.add_argument("--pretrained", dest="pretrained", default=None, type=str)
    p.add_argument("--device", default="cuda")
    p.add_argument("--compute-dtype", default="bf16", choices=["bf16", "f32"])
    return p


if __name__ == "__main__":
    main(get_args_parser().parse_args())
