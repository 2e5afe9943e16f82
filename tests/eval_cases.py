"""Inputs of the evaluation-statistics fixture (tests/golden/g20_eval.npz) and tests: fixed integer-hash data, regenerated
wherever it is needed, so the fixture stores only targets, train targets and the reference's outputs."""
import numpy as np

# (name, rows, classes, bins) of the calibration cases
CALIB = (("c64x10_b10", 64, 10, 10), ("c500x100_b15", 500, 100, 15), ("c300x37_b1", 300, 37, 1), ("c900x1000_b256", 900, 1000, 256))
# confidences that sit on or just beside the bin edges of np.linspace(0, 1, nb + 1)
EDGE_CONF = (0.5, 1.0, 0.0, 0.1, 0.2, 0.3, 0.30000000000000004, 0.7, 0.9, 1.0 + 2 ** -52, 2 ** -60, 0.25, 0.75)

# training-set counts per class of the shot cases: the thresholds 20 and 100 and their neighbours, an unseen class
SHOT_TRAIN_COUNTS = (500, 101, 100, 99, 50, 21, 20, 19, 5, 1, 150, 0, 3, 100, 19, 20)


def ihash(*ints):
    """splitmix64-style mix of integer arrays (elementwise), as uint64."""
    h = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        for v in ints:
            h = (h ^ np.asarray(v, dtype=np.uint64)) * np.uint64(0xBF58476D1CE4E5B9)
            h ^= h >> np.uint64(31)
            h = h * np.uint64(0x94D049BB133111EB)
            h ^= h >> np.uint64(29)
    return h


def hash_logits(salt, B, C, scale=1.0 / 64, span=1024):
    """[B, C] float32 logits, multiples of ``scale`` in [-span/2, span/2) * scale."""
    i, j = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(C, dtype=np.uint64), indexing="ij")
    v = (ihash(salt, i, j) % np.uint64(span)).astype(np.int64) - span // 2
    return (v * scale).astype(np.float32)


def hash_targets(salt, B, C):
    return (ihash(salt + 1000, np.arange(B, dtype=np.uint64)) % np.uint64(C)).astype(np.int64)


def calib_inputs(name):
    """(true_labels, pred_labels, confidences float64) of a calibration case; the edge confidences come first."""
    k = [c[0] for c in CALIB].index(name)
    _, B, C, _ = CALIB[k]
    t = hash_targets(10 + k, B, C)
    # predictions: the target on about 60 % of the rows, else a hashed class
    r = ihash(20 + k, np.arange(B, dtype=np.uint64))
    p = np.where(r % np.uint64(5) < np.uint64(3), t, (r >> np.uint64(8)) % np.uint64(C)).astype(np.int64)
    conf = ((ihash(30 + k, np.arange(B, dtype=np.uint64)) >> np.uint64(11)).astype(np.float64) + 1.0) / 2.0 ** 53
    conf = np.maximum(conf, 1.0 / C)
    n = min(len(EDGE_CONF), B)
    conf[:n] = EDGE_CONF[:n]
    return t, p, conf


def shot_inputs(reps):
    """(preds, labels, train_targets) with SHOT_TRAIN_COUNTS; test labels over every class but one, ``reps`` per class
    on average, predictions right on a hashed subset."""
    C = len(SHOT_TRAIN_COUNTS)
    train = np.repeat(np.arange(C, dtype=np.int64), SHOT_TRAIN_COUNTS)
    n = reps * C
    labels = hash_targets(40 + reps, n, C)
    labels[labels == 4] = 5                               # class 4 (50 train rows) never occurs in the test set
    r = ihash(50 + reps, np.arange(n, dtype=np.uint64))
    preds = np.where(r % np.uint64(7) < np.uint64(4), labels, (r >> np.uint64(8)) % np.uint64(C)).astype(np.int64)
    return preds, labels, train


SHOT_REPS = (3, 40)
