"""Criterion / data factories with the surface of classification/initialisers.py.
Only the IIF and plain cross-entropy criteria are on the hot path; the datasets
are the synthetic long-tailed sets of ``iif_amd.imbalanced_dataset`` (no
torchvision / network here)."""
import torch

from . import custom, imbalanced_dataset


def get_weights(dataset, device="cuda"):
    """Deferred re-weighting class weights ``sum/count`` (initialisers.py:16-19)."""
    c = torch.tensor(dataset.get_cls_num_list(), device=device)
    return c.sum() / c


class _UniformTable(object):
    def __init__(self, n):
        self.n = n

    def get_cls_num_list(self):
        return [1] * self.n


def get_criterion(args, dataset, model, num_classes):
    """initialisers.py:22-48.  'iif' -> fused IIFLoss; 'ce' -> the same fused kernel
    with an all-ones table built by hand (plain softmax cross-entropy); 'bce' ->
    FocalLoss(gamma=0) (sigmoid BCE with logits); 'focal_loss' ->
    FocalLoss(gamma=args.gamma, alpha=args.alpha).  In every branch the class weights
    are get_weights(dataset) under --deffered and None otherwise.

    The reference's 'focal_loss' branch also passes ``feat_select=args.feat_select``,
    which neither its parser nor its FocalLoss defines, so it crashes there; this
    builds the evident intent instead."""
    device = getattr(args, "device", "cuda")
    weight = get_weights(dataset, device) if getattr(args, "deffered", False) else None
    if args.classif == "iif":
        return custom.IIFLoss(dataset, variant=args.iif, iif_norm=args.iif_norm, reduction=args.reduction,
                              device=device, weight=weight)
    if args.classif == "ce":
        crit = custom.IIFLoss(dataset, variant="raw", reduction=args.reduction, device=device, weight=weight)
        ones = torch.ones(1, num_classes, device=device)
        crit.iif = {k: ones for k in crit.iif}
        crit.is_plain_ce = True
        # nn.CrossEntropyLoss(weight=w, reduction='mean') divides by the sum of the targets' weights
        # (initialisers.py:43-46), unlike IIFLoss whose .mean() divides by the batch size (custom.py:32-33)
        crit.weighted_mean = weight is not None and args.reduction == "mean"
        return crit
    if args.classif == "bce":
        return custom.FocalLoss(gamma=0, reduction=args.reduction, device=device, weights=weight)
    if args.classif == "focal_loss":
        return custom.FocalLoss(gamma=args.gamma, alpha=args.alpha, reduction=args.reduction, device=device,
                                weights=weight)
    raise NotImplementedError("unknown criterion %r (iif, ce, bce, focal_loss)" % (args.classif,))


def get_data(args):
    """initialisers.py:51-112: returns (dataset, num_classes, train_loader, test_loader, train_sampler).
    With ``--data-path`` the long-tailed sets are read from the reference's list files (``--train-txt`` /
    ``--eval-txt`` default to the paths hard-coded at initialisers.py:83-100) through ``LT_Dataset`` /
    ``LT_Dataset_Eval`` (with ``--device-augment``: batches built on the device, get_lt_device), and CIFAR-10 / CIFAR-100
    from their files through get_cifar_device; without it they are synthetic sets of the same shape (no dataset ships with
    the image)."""
    name = args.dset_name.lower()
    if name in ("cifar10", "cifar100") and getattr(args, "data_path", ""):
        return get_cifar_device(args, name)
    key = {"imagenet": "imagenet_lt", "imagenet_lt": "imagenet_lt", "places_lt": "places_lt", "inat18": "inat18"}.get(name)
    if key is not None and getattr(args, "data_path", "") and getattr(args, "device_augment", False):
        return get_lt_device(args, key)
    if key is not None and getattr(args, "data_path", ""):
        C, train_txt, eval_txt = imbalanced_dataset.LT_LISTS[key]
        ds, ds_test = imbalanced_dataset.get_dataset_lt(args, C, getattr(args, "train_txt", None) or train_txt,
                                                        getattr(args, "eval_txt", None) or eval_txt)
        ds.num_classes = len(ds.cls_num_list)
    elif name.startswith("cifar"):
        C = 100 if "100" in name else 10
        ds = imbalanced_dataset.synthetic_cifar_lt(C, args.imb_type, args.imb_factor, args.rand_number, True)
        ds_test = imbalanced_dataset.synthetic_cifar_lt(C, args.imb_type, args.imb_factor, args.rand_number, False)
    else:
        if key is None:
            raise KeyError("unknown dataset %r" % (args.dset_name,))
        ds = imbalanced_dataset.synthetic_lt(key, args.rand_number, True, getattr(args, "synthetic_scale", 1.0))
        ds_test = imbalanced_dataset.synthetic_lt(key, args.rand_number, False)
    sampler = test_sampler = None
    mode = getattr(args, "sampler", "random")
    if mode != "random":                     # initialisers.py:154-171: class-balanced index stream
        from .samplers import BalanceClassSampler, DistributedSamplerWrapper
        sampler = BalanceClassSampler(ds.targets, mode=mode)
        if getattr(args, "distributed", False):
            sampler = DistributedSamplerWrapper(sampler)
            test_sampler = torch.utils.data.distributed.DistributedSampler(ds_test, shuffle=False)
    elif getattr(args, "distributed", False):
        sampler = torch.utils.data.distributed.DistributedSampler(ds)
        test_sampler = torch.utils.data.distributed.DistributedSampler(ds_test, shuffle=False)
    pin = torch.cuda.is_available()
    loader = torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=sampler is None, sampler=sampler,
                                         num_workers=args.workers, pin_memory=pin, drop_last=True)
    loader_test = torch.utils.data.DataLoader(ds_test, batch_size=args.batch_size, shuffle=False, sampler=test_sampler,
                                              num_workers=args.workers, pin_memory=pin)
    return ds, ds.num_classes, loader, loader_test, sampler


def get_cifar_device(args, name):
    """load_cifar (initialisers.py:116-171) with the whole input pipeline on the device: IMBALANCECIFAR10/100 read from
    ``--data-path``, the full test file for evaluation, and DeviceCIFARLoader batches built by one kernel launch each -
    RandomCrop(32, 4) + flip, plus CIFAR10Policy and Cutout(1, 16) under ``--auto-augment cifar``, then Normalize.
    The loader stands in for the train sampler too (``set_epoch``)."""
    from . import cifar
    policy = getattr(args, "auto_augment", None)
    flags = cifar.CROP_FLIP
    if policy == "cifar":
        flags |= cifar.POLICY | cifar.CUTOUT
    elif policy:
        import warnings
        warnings.warn("--auto-augment %r has no CIFAR transform (only 'cifar' does); training with crop and flip, as the "
                      "reference does" % (policy,))
    ds = cifar.cifar_lt(args.data_path, name, args.imb_type, args.imb_factor, args.rand_number)
    ds_test = cifar.cifar_test(args.data_path, name)
    mode = getattr(args, "sampler", "random")
    dist = getattr(args, "distributed", False)
    device = getattr(args, "device", "cuda")
    loader = cifar.DeviceCIFARLoader(ds, args.batch_size, train=True, flags=flags, mode=mode, distributed=dist, device=device)
    loader_test = cifar.DeviceCIFARLoader(ds_test, args.batch_size, train=False, flags=0, distributed=dist, device=device)
    return ds, ds.num_classes, loader, loader_test, loader


def get_lt_device(args, key, loader=None):
    """The list datasets of ``--data-path`` with the input pipeline on the device (``--device-augment``): LT_Dataset /
    LT_Dataset_Eval only decode, DeviceLTLoader cuts the RandomResizedCrop box on the host and resizes, flips, jitters and
    normalises each batch in one launch (TensorTransform's pipeline; imbalanced_dataset.py:189-233); with ``--device-policy``
    the training loader runs the ``--auto-augment`` policy there in place of ColorJitter; with ``--device-decode`` the
    baseline JPEG files are decoded on the device too (iif_amd/jpeg.py), which replaces the default loader only: a custom
    ``loader`` is refused before any device is touched.  The loader stands in for the train sampler too (``set_epoch``)."""
    from . import lt_device
    decode = "device" if getattr(args, "device_decode", False) else "host"
    if decode == "device" and loader is not None:
        raise SystemExit("--device-decode replaces the default image loader; this dataset has a custom loader")
    C, train_txt, eval_txt = imbalanced_dataset.LT_LISTS[key]
    ds = imbalanced_dataset.LT_Dataset(args.data_path, getattr(args, "train_txt", None) or train_txt, C, loader=loader)
    ds_test = imbalanced_dataset.LT_Dataset_Eval(args.data_path, getattr(args, "eval_txt", None) or eval_txt, ds.class_map, C,
                                                 loader=loader)
    ds.num_classes = len(ds.cls_num_list)
    size = getattr(args, "image_size", 224)
    mode = getattr(args, "sampler", "random")
    dist = getattr(args, "distributed", False)
    device = getattr(args, "device", "cuda")
    workers = getattr(args, "workers", 4)
    policy = getattr(args, "auto_augment", None) if getattr(args, "device_policy", False) else None
    loader = lt_device.DeviceLTLoader(ds, args.batch_size, train=True, size=size, dset_name=key, seed=args.rand_number,
                                      mode=mode, distributed=dist, workers=workers, device=device, policy=policy,
                                      decode=decode)
    loader_test = lt_device.DeviceLTLoader(ds_test, args.batch_size, train=False, size=size, dset_name=key,
                                           distributed=dist, workers=workers, device=device, decode=decode)
    return ds, ds.num_classes, loader, loader_test, loader
