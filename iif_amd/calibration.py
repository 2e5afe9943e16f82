"""Reliability statistics of a classifier (the numbers behind a reliability diagram): per-bin accuracy and
confidence, ECE and MCE, with the inputs, bins and dictionary of the reference's
``classification/reliability_diagrams.py::compute_calibration``.  Host-side numpy; the device path is
``eval_stats.EvalAccumulator``, whose ``keep_rows`` output can be fed here.  Plotting is not provided."""
import numpy as np


def summarise(accuracies, confidences, counts, bins):
    """The dictionary of ``compute_calibration`` from per-bin mean accuracy, mean confidence and count.  With no
    row in any bin the averages are NaN, as in the reference."""
    counts = np.asarray(counts)
    total = np.sum(counts)
    gaps = np.abs(accuracies - confidences)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg_acc = np.sum(accuracies * counts) / total
        avg_conf = np.sum(confidences * counts) / total
        ece = np.sum(gaps * counts) / total
    return {"accuracies": accuracies, "confidences": confidences, "counts": counts, "bins": bins,
            "avg_accuracy": avg_acc, "avg_confidence": avg_conf,
            "expected_calibration_error": ece, "max_calibration_error": np.max(gaps)}


def compute_calibration(true_labels, pred_labels, confidences, num_bins=10):
    """Bins the rows by confidence over ``np.linspace(0, 1, num_bins + 1)``: bin b holds
    ``bins[b] < confidence <= bins[b + 1]`` (``np.digitize(..., right=True)``); a confidence outside (0, 1]
    is in no bin.  Per bin: the fraction of rows whose prediction equals the label, the mean confidence and
    the count; then the count-weighted averages, ECE (count-weighted mean |accuracy - confidence|) and MCE
    (the largest gap over all bins, empty bins included)."""
    true_labels, pred_labels, confidences = np.asarray(true_labels), np.asarray(pred_labels), np.asarray(confidences)
    if not (len(confidences) == len(pred_labels) == len(true_labels)):
        raise ValueError("labels, predictions and confidences differ in length")
    if num_bins <= 0:
        raise ValueError("num_bins must be positive")
    bins = np.linspace(0.0, 1.0, num_bins + 1)
    slot = np.digitize(confidences, bins, right=True) - 1
    correct = true_labels == pred_labels
    accuracies = np.zeros(num_bins, dtype=np.float64)
    means = np.zeros(num_bins, dtype=np.float64)
    counts = np.zeros(num_bins, dtype=np.int64)
    for b in range(num_bins):
        rows = np.flatnonzero(slot == b)
        if rows.size:
            accuracies[b] = correct[rows].mean()
            means[b] = confidences[rows].mean()
            counts[b] = rows.size
    return summarise(accuracies, means, counts, bins)
