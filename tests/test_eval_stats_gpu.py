"""iif_eval_accumulate / EvalAccumulator on the MI355X: predictions against torch.argmax, top-k hits against
iif_topk_hits, per-class counts against bincount, confidences against the float64 softmax, the reliability bins against
calibration.compute_calibration on the kernel's own confidences, order independence, out-of-range targets, the two CLIs
(train --shot-acc --calibration-bins, python -m iif_amd.per_shot_acc) and the all-reduce over two ranks."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from iif_amd import calibration, utils
from iif_amd.eval_stats import EvalAccumulator, split_counts
from iif_amd.per_shot_acc import shot_acc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = "cuda:0"


def logits(B, C, dtype, pad, seed, scale=3.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(B, C + pad, device=DEV, generator=g) * scale).to(dtype)
    return x[:, :C]


def check(x, t, tab, topk=(1, 5), nb=10):
    B, C = x.shape
    a = EvalAccumulator(C, topk=topk, num_bins=nb, table=tab, device=DEV, keep_rows=True)
    a.update(x, t)
    pred, conf, _ = a.rows()
    p = split_counts(a.counts(), C, len(a.topk), nb)
    z = x.float() * (tab.reshape(1, -1) if tab is not None else 1.0)
    assert np.array_equal(pred, torch.argmax(z, 1).cpu().numpy())
    hits = utils.topk_hit_counts(x, t, a.topk, table=tab).cpu().numpy()
    assert np.array_equal(p["hits"], hits)
    tn = t.cpu().numpy()
    assert p["rows"] == B and p["out_of_range"] == 0
    assert np.array_equal(p["n_test"], np.bincount(tn, minlength=C))
    assert np.array_equal(p["n_hit"], np.bincount(tn[pred == tn], minlength=C))
    ref_conf = torch.softmax(z.double(), 1).max(1).values.cpu().numpy()
    assert np.abs(conf - ref_conf).max() <= 4e-6
    cal = calibration.compute_calibration(tn, pred, conf.astype(np.float64), num_bins=nb)
    assert np.array_equal(p["bin_count"], cal["counts"])
    assert np.array_equal(p["bin_hit"], np.rint(cal["accuracies"] * cal["counts"]).astype(np.int64))
    got = a.result()["calibration"]
    for k in ("confidences", "accuracies", "expected_calibration_error", "max_calibration_error", "avg_confidence"):
        assert np.allclose(got[k], cal[k], rtol=0, atol=1e-9), k
    return a


@pytest.mark.parametrize("layout", ["contiguous", "ld+4", "ld+1"])
@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("B", [1, 7, 256])
@pytest.mark.parametrize("C", [10, 100, 1000, 1204, 8142])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_matches_torch_and_topk_hits(dtype, C, B, with_table, layout):
    pad = {"contiguous": 0, "ld+4": 4, "ld+1": 1}[layout]
    x = logits(B, C, dtype, pad, seed=C * 31 + B)
    g = torch.Generator(device=DEV).manual_seed(C + B)
    t = torch.randint(0, C, (B,), device=DEV, generator=g)
    tab = (torch.rand(C, device=DEV, generator=g) * 2.5 + 0.5) if with_table else None
    check(x, t, tab, nb=15 if C == 1000 else 10)


@pytest.mark.parametrize("C", [10, 100, 1000, 1204, 8142])
def test_heavy_ties_pick_the_first_maximum(C):
    """bf16 logits on a grid of five values: many equal maxima per row, and all-equal rows (prediction 0, confidence 1/C)."""
    B = 64
    g = torch.Generator(device=DEV).manual_seed(C)
    x = torch.randint(-2, 3, (B, C), device=DEV, generator=g).to(torch.bfloat16)
    x[::5] = 1.0
    t = torch.randint(0, C, (B,), device=DEV, generator=g)
    t[::5] = torch.arange(0, B, 5, device=DEV) % C
    for tab in (None, torch.ones(C, device=DEV)):
        a = check(x, t, tab)
        pred, conf, _ = a.rows()
        assert (pred[::5] == 0).all()
        assert np.all(conf[::5] == np.float32(1.0) / np.float32(C))        # C ones summed exactly


def test_edge_confidences_0_5_and_1_land_in_the_upper_bins():
    """Two equal maxima far above the rest: confidence exactly 0.5 (bin 4 of 10: 0.4 < 0.5 <= 0.5); one: exactly 1.0."""
    C = 100
    x = torch.full((4, C), -200.0, device=DEV)
    x[0, 3] = x[0, 7] = 5.0
    x[1, 9] = 5.0
    x[2, 0] = x[2, 99] = 0.0
    x[3] = 0.0
    t = torch.tensor([3, 9, 99, 0], device=DEV)
    a = check(x, t, None)
    _, conf, _ = a.rows()
    assert conf[0] == 0.5 and conf[1] == 1.0 and conf[2] == 0.5
    p = split_counts(a.counts(), C, 2, 10)
    assert p["bin_count"][4] == 2 and p["bin_count"][9] == 1 and p["bin_count"][0] == 1
    assert p["bin_hit"][4] == 1 and p["bin_hit"][9] == 1


def test_batch_split_and_order_do_not_change_the_counts():
    C, B = 1000, 517
    x = logits(B, C, torch.float32, 0, seed=7)
    t = torch.randint(0, C, (B,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    tab = torch.rand(C, device=DEV) + 0.5
    cuts = [0, 3, 100, 101, 400, B]
    runs = []
    for order in ("one", "split", "reversed"):
        a = EvalAccumulator(C, num_bins=20, table=tab, device=DEV)
        if order == "one":
            a.update(x, t)
        else:
            parts = list(zip(cuts[:-1], cuts[1:]))
            for lo, hi in (parts if order == "split" else parts[::-1]):
                a.update(x[lo:hi], t[lo:hi])
        runs.append(a.acc.cpu())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_out_of_range_targets(dtype):
    C, B = 100, 90
    x = logits(B, C, dtype, 0, seed=3)
    t = torch.randint(0, C, (B,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    z = x.float()
    t[::3] = torch.argmax(z[::3], 1)                      # rows that would be hits with a valid target...
    bad = torch.zeros(B, dtype=torch.bool, device=DEV)
    bad[::6] = True
    t[bad] = torch.where(torch.arange(B, device=DEV)[bad] % 12 == 0, -1, C + 5)
    a = EvalAccumulator(C, num_bins=10, device=DEV, keep_rows=True)
    a.update(x, t)
    p = split_counts(a.counts(), C, 2, 10)
    tn, pred = t.cpu().numpy(), a.rows()[0]
    ok = (tn >= 0) & (tn < C)
    assert p["rows"] == B and p["out_of_range"] == int((~ok).sum()) == 15
    assert p["n_test"].sum() == ok.sum()
    assert np.array_equal(p["hits"], utils.topk_hit_counts(x, t, (1, 5)).cpu().numpy())
    assert p["bin_count"].sum() == B and p["bin_hit"].sum() == int((ok & (pred == tn)).sum())   # ...now misses
    with pytest.raises(ValueError, match="outside"):
        a.result(train_targets=np.arange(C))
    assert a.result()["topk"][1] == 100.0 * p["hits"][0] / B


def _run(cmd, env=None):
    r = subprocess.run(cmd, env=env or dict(os.environ), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    return r.stdout


def _shot_line(out):
    m = re.findall(r"Many shot Acc is: (\S+), median shot Acc is: (\S+), low shot Acc is: (\S+)", out)
    assert m, out[-2000:]
    return tuple(float(v) for v in m[-1])


def test_train_and_per_shot_acc_cli(tmp_path):
    """train --shot-acc --calibration-bins prints the extra lines; per_shot_acc on its checkpoint prints the shot split
    that shot_acc gives on predictions collected through train.evaluate's path (model(x), IIF scaling, argmax)."""
    out = tmp_path / "out"
    tr = _run([sys.executable, "-m", "iif_amd.train", "--model", "resnet32", "--dset_name", "cifar100", "--classif", "iif",
               "--iif", "raw", "-b", "64", "-j", "0", "--epochs", "1", "--max-iters", "2", "--output-dir", str(out),
               "--shot-acc", "--calibration-bins", "10"])
    assert "Acc@1" in tr and "ECE is: " in tr and "(10 bins)" in tr
    _shot_line(tr)
    ckpt = str(out / "checkpoint.pth")
    ps = _run([sys.executable, "-m", "iif_amd.per_shot_acc", "--dset_name", "cifar100", "--model", "resnet32", "--load_from",
               ckpt, "--classif", "iif", "--iif", "raw", "-b", "64", "-j", "0", "--apex", "--calibration-bins", "10"])
    got = _shot_line(ps)
    avg = float(re.findall(r"Avg Acc is: (\S+)", ps)[-1])
    # the same evaluation through today's path, predictions collected on the host
    from iif_amd import custom, initialisers, per_shot_acc, train
    args = per_shot_acc.get_args_parser().parse_args(["--dset_name", "cifar100", "--model", "resnet32", "-b", "64", "-j", "0",
                                                      "--classif", "iif", "--iif", "raw"])
    ds, C, _, loader, _ = initialisers.get_data(args)
    model = train.build_model(args, C)
    model.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=False)["model"])
    crit = custom.IIFLoss(ds, variant="raw", device=DEV)
    model.eval()
    preds, labels = [], []
    with torch.no_grad():
        for image, target in loader:
            o = crit(model(image.to(DEV)), infer=True)
            preds.append(o.argmax(1).cpu())
            labels.append(target)
    preds, labels = torch.cat(preds).numpy(), torch.cat(labels).numpy()
    assert got == tuple(float(v) for v in shot_acc(preds, labels, ds.targets))
    assert abs(avg - 100.0 * (preds == labels).mean()) <= 1e-9


def test_two_ranks_sum_to_the_single_process_counts(tmp_path):
    sys.path.insert(0, HERE)
    import eval_ddp_worker
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
          "--master-port", "29581", os.path.join(HERE, "eval_ddp_worker.py"), str(tmp_path)], env=env)
    single = eval_ddp_worker.run_single()
    for r in (0, 1):
        assert torch.equal(torch.load(tmp_path / ("rank%d.pt" % r)), single)
