"""iif_amd/loss_reduction.py without a GPU: the reduction / avg_factor checks raise the texts every loss module raised, the
scale mapping returns mmdet's values (losses/utils.py:29-55), and the workspace constant is the header's."""
import os
import re

import pytest

from iif_amd import loss_reduction as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVG_TEXT = 'avg_factor can not be used with reduction="sum"'


def test_checks_raise_the_same_texts():
    for red in ("none", "mean", "sum"):
        R.check_reduction(red, None)
        R.check_avg_factor(red, None)
    R.check_reduction("mean", 12.5)
    R.check_reduction("none", 12.5)                     # 'none' ignores avg_factor
    with pytest.raises(ValueError) as e:
        R.check_reduction("sum", 12.5)
    assert str(e.value) == AVG_TEXT
    with pytest.raises(ValueError) as e:
        R.check_avg_factor("sum", 0)                    # any avg_factor that is not None
    assert str(e.value) == AVG_TEXT
    with pytest.raises(ValueError) as e:
        R.check_reduction("bogus", 3.0)                 # the unknown reduction is reported first
    assert str(e.value) == "unknown reduction 'bogus'"
    R.check_avg_factor("bogus", 3.0)                    # the narrow check leaves the reduction's name to its caller


def test_the_modules_raise_through_the_shared_check():
    """Before any tensor is looked at (CPU tensors here): the order of the checks a caller can observe."""
    import torch
    from iif_amd import custom, mmdet_bbox_loss, mmdet_ce_loss
    x, t = torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)
    calls = [lambda red, avg: custom.fused_iif_cross_entropy(x, torch.ones(3), t, reduction=red, avg_factor=avg),
             lambda red, avg: mmdet_ce_loss.cross_entropy(x, t, reduction=red, avg_factor=avg),
             lambda red, avg: mmdet_ce_loss.binary_cross_entropy(x, t, reduction=red, avg_factor=avg),
             lambda red, avg: mmdet_bbox_loss.l1_loss(x, x, reduction=red, avg_factor=avg)]
    for call in calls:
        with pytest.raises(ValueError) as e:
            call("sum", 2.0)
        assert str(e.value) == AVG_TEXT
        with pytest.raises(ValueError) as e:
            call("bogus", None)
        assert str(e.value) == "unknown reduction 'bogus'"


def test_scale_mapping():
    assert R.reduction_scale("sum", None, 7) == 1.0
    assert R.reduction_scale("sum", None, 7, 0.3) == 0.3
    assert R.reduction_scale("mean", 12.5, 7) == 1.0 / 12.5
    assert R.reduction_scale("mean", 12.5, 7, 0.3) == 0.3 / 12.5
    assert R.reduction_scale("mean", None, 7) == 1.0 / 7.0
    assert R.reduction_scale("mean", None, 7, 0.3) == 0.3 / 7.0
    assert R.reduction_scale("mean", None, 0) == 1.0                     # n == 0: divided by max(n, 1)
    assert R.reduction_scale("mean", None, 0, 0.3) == 0.3
    assert R.reduction_scale("mean", 4, 0, 0.3) == 0.3 / 4.0             # an avg_factor wins over n, an int one included
    assert isinstance(R.reduction_scale("mean", 4, 3), float)


def test_registration_reports_a_missing_mmdet():
    try:
        import mmdet  # noqa: F401
    except Exception:
        assert R.register_losses({"NoSuchLoss": object}) is False


def test_workspace_words_are_the_headers():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    m = re.search(r"#define\s+IIF_CE_WORKSPACE_BYTES\s+\(4 \* \((\d+) \+ (\d+)\)\)", text)
    assert m, "IIF_CE_WORKSPACE_BYTES is no longer written as 4 * (ticket + slots)"
    assert R.CE_WORKSPACE_WORDS == int(m.group(1)) + int(m.group(2))
