"""Evaluation statistics without a device: the restated compute_calibration and shot_acc against the reference's outputs
(tests/golden/g20_eval.npz), the counts-to-result step of EvalAccumulator against both, and the argument checks of
EvalAccumulator and iif_eval_accumulate (which return before any HIP call)."""
import ctypes

import numpy as np
import pytest

from iif_amd import _lib, calibration
from iif_amd.eval_stats import EvalAccumulator, counts_to_result
from iif_amd.per_shot_acc import get_args_parser, shot_acc

from .eval_cases import CALIB, SHOT_REPS, calib_inputs, shot_inputs

KEYS = ("accuracies", "confidences", "counts", "bins", "avg_accuracy", "avg_confidence", "expected_calibration_error",
        "max_calibration_error")
EINVAL = -1


@pytest.mark.parametrize("case", CALIB, ids=[c[0] for c in CALIB])
def test_compute_calibration_equals_reference(golden, case):
    g = golden("g20_eval")
    name, B, C, nb = case
    t, p, conf = calib_inputs(name)
    assert np.array_equal(g[name + "_targets"], t)
    r = calibration.compute_calibration(t, p, conf, num_bins=nb)
    assert sorted(r) == sorted(KEYS)
    for k in KEYS:
        assert np.array_equal(np.asarray(r[k]), g["%s_%s" % (name, k)]), k
    # the edge rows: 0.5 and 1.0 sit on an upper edge, 0 and 1 + 2^-52 are in no bin
    assert r["counts"].sum() < B


@pytest.mark.parametrize("reps", SHOT_REPS)
def test_shot_acc_equals_reference(golden, reps):
    g = golden("g20_eval")
    preds, labels, train = shot_inputs(reps)
    for k, v in (("labels", labels), ("preds", preds), ("train", train)):
        assert np.array_equal(g["shot%d_%s" % (reps, k)], v)
    many, median, low, per_cls = shot_acc(preds, labels, train, acc_per_cls=True)
    assert np.array_equal(np.array([many, median, low]), g["shot%d_triple" % reps])
    assert np.array_equal(np.array(per_cls), g["shot%d_per_cls" % reps])


def host_counts(t, p, conf, C, topk, nb, ranks=None):
    """The iif_eval_accumulate buffer, built on the host from per-row (target, prediction, confidence[, rank])."""
    acc = np.zeros(EvalAccumulator.size(C, len(topk), nb), np.int64)
    ok = (t >= 0) & (t < C)
    acc[0], acc[1] = len(t), int((~ok).sum())
    if ranks is not None:
        for j, k in enumerate(topk):
            acc[2 + j] = int((ok & (ranks < k)).sum())
    o = 2 + len(topk)
    acc[o:o + C] = np.bincount(t[ok], minlength=C)
    acc[o + C:o + 2 * C] = np.bincount(t[ok & (p == t)], minlength=C)
    slot = np.digitize(conf.astype(np.float64), np.linspace(0, 1, nb + 1), right=True) - 1
    inb = (slot >= 0) & (slot < nb)
    b = o + 2 * C
    acc[b:b + nb] = np.bincount(slot[inb], minlength=nb)
    acc[b + nb:b + 2 * nb] = np.bincount(slot[inb & ok & (p == t)], minlength=nb)
    fixed = np.rint(conf.astype(np.float64) * 2.0 ** 32).astype(np.int64)
    np.add.at(acc[b + 2 * nb:], slot[inb], fixed[inb])
    return acc


@pytest.mark.parametrize("reps", SHOT_REPS)
def test_counts_to_result_shot_split_is_bit_equal(reps):
    preds, labels, train = shot_inputs(reps)
    C = len(np.bincount(train))
    conf = np.full(len(labels), 0.5, np.float32)
    r = counts_to_result(host_counts(labels, preds, conf, C, (1,), 10), C, (1,), 10, train_targets=train)
    ref = shot_acc(preds, labels, train)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(map(np.float64, r["shot"]), map(np.float64, ref)))
    # thresholds are forwarded
    r2 = counts_to_result(host_counts(labels, preds, conf, C, (1,), 10), C, (1,), 10, train_targets=train,
                          many_shot_thr=50, low_shot_thr=5)
    assert np.array_equal(np.array(r2["shot"]), np.array(shot_acc(preds, labels, train, 50, 5)))


@pytest.mark.parametrize("case", CALIB, ids=[c[0] for c in CALIB])
def test_counts_to_result_calibration_matches(golden, case):
    """Confidences on a 2^-32 grid (float32 values >= 2^-8 are): the fixed-point sums are exact, so the dictionary agrees
    with compute_calibration to rounding."""
    name, B, C, nb = case
    t, p, conf = calib_inputs(name)
    conf = conf.astype(np.float32)                      # what conf_out holds
    r = counts_to_result(host_counts(t, p, conf, C, (1, 5), nb), C, (1, 5), nb)
    ref = calibration.compute_calibration(t, p, conf.astype(np.float64), num_bins=nb)
    cal = r["calibration"]
    assert np.array_equal(cal["counts"], ref["counts"]) and np.array_equal(cal["bins"], ref["bins"])
    for k in ("accuracies", "confidences", "avg_accuracy", "avg_confidence", "expected_calibration_error",
              "max_calibration_error"):
        assert np.allclose(cal[k], ref[k], rtol=0, atol=1e-12), k
    assert r["shot"] is None and r["rows"] == B


def test_counts_to_result_topk_and_out_of_range():
    t = np.array([0, 1, 2, 7, -1, 3], np.int64)
    p = np.array([0, 2, 2, 0, 0, 3], np.int64)
    ranks = np.array([0, 1, 0, 0, 0, 4])
    conf = np.full(6, 0.75, np.float32)
    acc = host_counts(t, p, conf, 4, (1, 5), 4, ranks)
    r = counts_to_result(acc, 4, (1, 5), 4)
    assert r["rows"] == 6 and r["out_of_range"] == 2
    assert r["topk"] == {1: 100.0 * 2 / 6, 5: 100.0 * 4 / 6}
    assert r["calibration"]["counts"].tolist() == [0, 0, 6, 0]
    assert r["calibration"]["accuracies"][2] == 3 / 6             # the out-of-range rows are misses
    with pytest.raises(ValueError, match="outside"):
        counts_to_result(acc, 4, (1, 5), 4, train_targets=[0, 1, 2, 3])


def test_accumulator_argument_checks():
    with pytest.raises(ValueError):
        EvalAccumulator(10, num_bins=257, device="cpu")
    with pytest.raises(ValueError):
        EvalAccumulator(10, num_bins=-1, device="cpu")
    with pytest.raises(ValueError):
        EvalAccumulator(10, topk=(1, 2, 3, 4, 5), device="cpu")
    with pytest.raises(ValueError):
        EvalAccumulator(10, topk=(0,), device="cpu")
    with pytest.raises(ValueError, match="table"):
        EvalAccumulator(10, table=np.ones(9, np.float32), device="cpu")
    a = EvalAccumulator(3, topk=(1, 5), num_bins=256, device="cpu")       # top-5 of 3 classes is top-3
    assert a.topk == (1, 3) and a.acc.numel() == 2 + 2 + 6 + 3 * 256
    with pytest.raises(_lib.IIFNativeError):                              # no CPU emulation
        import torch
        a.update(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))


def _entry(B=4, C=10, nk=2, ks=(1, 5), nb=10, dtype=0, ld=None, logits=8, targets=8, edges=8, acc=8):
    k = (ctypes.c_int32 * 5)(*(list(ks) + [1] * (5 - len(ks))))
    return _lib.lib().iif_eval_accumulate(logits, dtype, C if ld is None else ld, 0, targets, B, C, k, nk, edges, nb, acc, 0, 0, 0)


@pytest.mark.parametrize("kw", [dict(nb=0), dict(nb=257), dict(nk=5, ks=(1, 2, 3, 4, 5)), dict(nk=0), dict(ks=(0, 5)),
                                dict(C=0), dict(B=-1), dict(dtype=2), dict(ld=9), dict(logits=0), dict(targets=0),
                                dict(edges=0), dict(acc=0)])
def test_entry_rejects_bad_arguments(kw):
    assert _entry(**kw) == EINVAL


def test_entry_empty_batch_is_a_no_op():
    assert _entry(B=0, logits=0, targets=0, acc=0) == 0


def test_per_shot_acc_parser_takes_the_reference_flags():
    a = get_args_parser().parse_args(["--dset_name", "places_lt", "--data-path", "x", "--iif", "rel", "--classif", "iif",
                                      "--classif_norm", "norm", "--load_from", "c.pth", "-b", "64", "--model", "resnet152",
                                      "-j", "2", "--sampler", "random", "--auto-augment", "rand", "--apex",
                                      "--calibration-bins", "15"])
    assert (a.dset_name, a.iif, a.classif, a.classif_norm, a.batch_size, a.workers, a.calibration_bins) == \
        ("places_lt", "rel", "iif", "norm", 64, 2, 15)
    assert get_args_parser().parse_args([]).calibration_bins == 0


def test_train_flags_default_off():
    from iif_amd import train
    a = train.get_args_parser().parse_args([])
    assert a.shot_acc is False and a.calibration_bins == 0
    a = train.get_args_parser().parse_args(["--shot-acc", "--calibration-bins", "10"])
    assert a.shot_acc is True and a.calibration_bins == 10
