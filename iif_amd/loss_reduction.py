"""The glue every fused loss head repeats around its launch: mmdet's ``reduction`` / ``avg_factor`` convention
(losses/utils.py:29-55), the upstream-scalar scaling of a saved gradient, the ``LOSSES`` registration and the size of the
workspace of the in-kernel loss reduction (csrc/loss_reduce.h).  No device work at import; nothing here synchronises."""
import torch

from . import _lib

# IIF_CE_WORKSPACE_BYTES (include/iif_amd.h) in int32 words: the ticket, then one partial slot per block
CE_WORKSPACE_WORDS = 1 + 2048


def check_avg_factor(reduction, avg_factor):
    if avg_factor is not None and reduction == "sum":
        raise ValueError('avg_factor can not be used with reduction="sum"')


def check_reduction(reduction, avg_factor):
    if reduction not in ("none", "mean", "sum"):
        raise ValueError("unknown reduction %r" % (reduction,))
    check_avg_factor(reduction, avg_factor)


def reduction_scale(reduction, avg_factor, n, loss_weight=1.0):
    """The factor a kernel multiplies its sum over ``n`` rows / elements by: ``loss_weight`` for 'sum', else (the mean)
    ``loss_weight / avg_factor`` or, without one, ``loss_weight / max(n, 1)``."""
    if reduction == "sum":
        return loss_weight
    return loss_weight / (float(avg_factor) if avg_factor is not None else float(max(n, 1)))


def scale_by_device_scalar(grad, g, dtype=None):
    """``grad * g`` for a device scalar ``g`` into a fresh tensor (the saved gradient stays intact: backward may run
    twice), cast to ``dtype`` if one is given."""
    g = g.to(torch.float32).contiguous()
    out = torch.empty_like(grad)
    rc = _lib.lib().iif_scale_by_device_scalar(_lib.ptr(grad), _lib.dtype_code(grad), grad.numel(), _lib.ptr(g), _lib.ptr(out),
                                               _lib.stream_ptr())
    _lib.check(rc, "iif_scale_by_device_scalar")
    return out if dtype is None or dtype == out.dtype else out.to(dtype)


def register_losses(classes):
    """Register ``{name: class}`` in mmdet's ``LOSSES`` (``force=True`` replaces the stock ones) if mmdet is importable."""
    try:
        from mmdet.models.builder import LOSSES
    except Exception:
        return False
    for name, cls in classes.items():
        LOSSES.register_module(name=name, force=True, module=cls)
    return True
