"""iif_cifar_augment and the device CIFAR pipeline on the MI355X: the dumped draws against the numpy hash, their
frequencies, every stage against the host oracle (tests/cifar_cases.py) built from those draws, out-of-range indices,
determinism per (seed, epoch, rank), the loader, the training CLI end to end on fake CIFAR trees, and two ranks."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from iif_amd import augment, cifar
from iif_amd.cifar import CROP_FLIP, CUTOUT, POLICY

from .cifar_cases import case_images, one_sub_policy, oracle, write_fake_cifar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STD = torch.tensor(cifar.STD)[None, :, None, None]
TOL01 = 2e-6           # on the [0, 1] scale, for the ops whose reductions sum in another order


def _dataset(n=64):
    rows = case_images(n)
    labels = np.arange(n, dtype=np.int64) % 10
    return rows, torch.from_numpy(rows).to(DEV), torch.from_numpy(labels).to(DEV)


def _run_kernel(data, labels, idx, flags, subs=None, seed=1, epoch=0, rank=0, pos0=0):
    pol = cifar.device_policy(subs, DEV) if flags & POLICY else None
    x, t, p = cifar.augment_batch(data, labels, torch.as_tensor(idx, dtype=torch.int64).to(DEV), flags, seed, epoch, rank,
                                  pos0, pol, params=True)
    torch.cuda.synchronize()
    return x.cpu(), t.cpu(), p.cpu().numpy()


def _close(a, b):
    """Per image: |a - b| within TOL01 on the [0, 1] scale (a, b normalised; 5e-7 for the two roundings of Normalize)."""
    return ((a - b).abs() <= TOL01 / STD + 5e-7).flatten(1).all(1)


# ------------------------------------------------------------------------------------------------------------ draws
def test_params_equal_numpy_hash():
    rows, data, labels = _dataset()
    B = 4096
    idx = np.arange(B) % len(rows)
    for flags, seed, epoch, rank, pos0 in ((7, 11, 0, 0, 0), (7, 2 ** 63 + 5, 3, 1, 100), (CROP_FLIP, 11, 2, 0, 9)):
        _, _, p = _run_kernel(data, labels, idx, flags, seed=seed, epoch=epoch, rank=rank, pos0=pos0)
        want = cifar.draw_params(seed, epoch, rank, pos0 + np.arange(B), cifar.policy_table() if flags & POLICY else None)
        assert np.array_equal(p, want)


def test_param_frequencies_within_5_sigma():
    """2^16 draws against the reference's distributions; the hash is deterministic, so this cannot flake."""
    rows, data, labels = _dataset()
    B, reps = 8192, 8
    p = np.concatenate([_run_kernel(data, labels, np.arange(B) % len(rows), 7, seed=99, pos0=r * B)[2] for r in range(reps)])
    n = len(p)

    def within(count, total, prob, what):
        sd = np.sqrt(total * prob * (1 - prob))
        assert abs(count - total * prob) <= 5 * sd + 1e-9, (what, count, total * prob, sd)
    for col, k in ((0, 9), (1, 9), (2, 2), (3, 25), (8, 32), (9, 32)):
        c = np.bincount(p[:, col], minlength=k)
        assert len(c) == k
        for v in range(k):
            within(c[v], n, 1.0 / k, (cifar.PARAMS[col], v))
    for j in range(2):
        within(p[:, 5 + 2 * j].sum(), n, 0.5, "sign%d" % j)
        for s, sub in enumerate(augment._P["cifar10"]):
            m = p[:, 3] == s
            within(p[m, 4 + 2 * j].sum(), m.sum(), sub[3 * j + 1], ("apply", s, j))


# ------------------------------------------------------------------------------------------------ stages vs oracle
@pytest.mark.parametrize("flags", [0, CROP_FLIP, CUTOUT, CROP_FLIP | CUTOUT])
def test_crop_flip_cutout_normalise_bit_exact(flags):
    rows, data, labels = _dataset()
    B = 8192
    idx = np.random.RandomState(1).randint(0, len(rows), size=B)
    x, t, p = _run_kernel(data, labels, idx, flags, seed=5)
    assert torch.equal(t, torch.from_numpy(idx % 10))
    assert torch.equal(x, oracle(rows[idx], p, flags))
    # coverage: every crop offset with both flips, cutout boxes clipped at all four corners
    assert len({(a, b, c) for a, b, c in p[:, :3].tolist()}) == 81 * 2
    cut = {(a, b) for a, b in p[:, 8:10].tolist()}
    assert {(0, 0), (0, 31), (31, 0), (31, 31)} <= cut


@pytest.mark.parametrize("name", cifar.OPS)
def test_each_op_at_every_magnitude_and_sign(name):
    """Exact for the integer and geometric ops on uint8-valued images; TOL01 for the blend ops (Color, Contrast,
    Brightness, Sharpness, AutoContrast)."""
    rows, data, labels = _dataset(48)
    idx = np.arange(len(rows))
    for mag in range(10):
        subs = one_sub_policy(name, mag)
        x, _, p = _run_kernel(data, labels, idx, POLICY, subs=subs, seed=mag)
        assert p[:, 4].all() and not p[:, 6].any()
        assert 0 < p[:, 5].sum() < len(idx)                     # both signs
        want = oracle(rows[idx], p, POLICY, subs)
        if name in cifar.BLEND or name == "AutoContrast":
            assert _close(x, want).all(), (name, mag)
        else:
            assert torch.equal(x, want), (name, mag, (x - want).abs().max().item())


def test_whole_sub_policies_with_crop_flip_cutout():
    """All stages, every sub-policy.  A blend op feeding a quantising op (Posterize, Solarize, Equalize) can turn a
    last-bit difference of the blend into a one-level flip of the quantiser (and Equalize's table shifts by that pixel), so
    here an image matches when it is within TOL01, at least 99 % must, and the others may differ by one level (1 / 255)."""
    rows, data, labels = _dataset()
    B = 4096
    idx = np.random.RandomState(2).randint(0, len(rows), size=B)
    x, _, p = _run_kernel(data, labels, idx, CROP_FLIP | POLICY | CUTOUT, seed=17, epoch=1)
    assert len(set(p[:, 3].tolist())) == 25
    want = oracle(rows[idx], p, CROP_FLIP | POLICY | CUTOUT)
    ok = _close(x, want)
    assert ok.float().mean().item() >= 0.99
    if not ok.all():
        diff = ((x[~ok] - want[~ok]).abs() * STD).max().item()
        assert diff <= 1.0 / 255 + TOL01, diff


# ------------------------------------------------------------------------------------------------ out of range
def test_out_of_range_index_gives_label_minus_one_and_the_trainer_raises():
    from iif_amd import resnet_cifar
    from iif_amd.custom import IIFLoss
    rows, data, labels = _dataset()
    idx = np.arange(32) + 3
    idx[[1, 2, 4]] = -1, len(rows), 2 ** 40
    x, t, _ = _run_kernel(data, labels, idx, 7)
    bad = np.zeros(32, bool)
    bad[[1, 2, 4]] = True
    assert t.tolist() == np.where(bad, -1, idx % 10).tolist()
    assert not x[bad].any() and x[~bad].abs().sum((1, 2, 3)).min() > 0

    class DS:
        def get_cls_num_list(self):
            return [50, 20, 10, 8, 6, 5, 4, 3, 2, 2]
    net = resnet_cifar.resnet32(num_classes=10, use_norm="None", compute_dtype=torch.float32)
    net.train()
    xi, ti = cifar.augment_batch(data, labels, torch.tensor(idx, device=DEV), 7, 1, 0, 0, 0, cifar.device_policy(None, DEV))
    net.loss_and_backward(xi, ti, IIFLoss(DS(), variant="raw"))
    with pytest.raises(IndexError):
        net.check_labels()


# ------------------------------------------------------------------------------------------------ loader
def _fake_ds(n_per_class=37, C=10):
    rows = case_images(n_per_class * C, seed=3)
    targets = np.repeat(np.arange(C), n_per_class)
    return cifar.CIFARData(rows, targets, C)


def _collect(loader):
    return [(x.cpu(), t.cpu()) for x, t in loader]


def test_same_seed_and_epoch_give_the_same_batches():
    ds = _fake_ds()
    mk = lambda **kw: cifar.DeviceCIFARLoader(ds, 32, train=True, flags=7, seed=4, device=DEV, **kw)   # noqa: E731
    a = mk()
    e0 = _collect(a)
    e1 = _collect(a)                                          # the next pass is epoch 1
    b = mk()
    b.set_epoch(0)
    again = _collect(b)
    assert len(e0) == len(a) == len(ds) // 32
    assert all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(e0, again))
    assert not torch.equal(e0[0][0], e1[0][0])
    # targets follow the epoch's list, the images its draws
    idx = cifar.epoch_indices(len(ds), 0, seed=4)
    assert torch.equal(torch.cat([t for _, t in e0]), torch.tensor(ds.targets)[idx[:len(e0) * 32]])
    data = torch.from_numpy(ds.data).to(DEV)
    lab = torch.tensor(ds.targets, device=DEV)
    pol = cifar.device_policy(None, DEV)
    ix = torch.from_numpy(idx[32:64]).to(DEV)
    x1, _ = cifar.augment_batch(data, lab, ix, 7, 4, 0, 0, 32, pol)
    assert torch.equal(x1.cpu(), e0[1][0])
    x2, _ = cifar.augment_batch(data, lab, ix, 7, 4, 0, 1, 32, pol)        # another rank draws other parameters
    assert not torch.equal(x2.cpu(), e0[1][0])


def test_eval_loader_covers_everything_in_order():
    ds = _fake_ds()
    ld = cifar.DeviceCIFARLoader(ds, 64, train=False, flags=0, device=DEV)
    got = _collect(ld)
    assert len(got) == len(ld) == -(-len(ds) // 64) and got[-1][0].shape[0] == len(ds) % 64
    assert torch.cat([t for _, t in got]).tolist() == ds.targets
    assert torch.equal(torch.cat([x for x, _ in got]), oracle(ds.data, np.zeros((len(ds), 10), np.int32), 0))
    assert ld.dataset.get_cls_num_list() == [37] * 10


@pytest.mark.parametrize("mode", ["upsampling", "downsampling"])
def test_balanced_loader(mode):
    ds = cifar.CIFARData(case_images(100, seed=4), np.repeat(np.arange(4), [60, 25, 10, 5]), 4)
    ld = cifar.DeviceCIFARLoader(ds, 10, train=True, flags=1, mode=mode, seed=2, device=DEV)
    t = torch.cat([t for _, t in _collect(ld)])
    per = 60 if mode == "upsampling" else 5
    assert len(ld) == 4 * per // 10 and np.bincount(t.numpy(), minlength=4).tolist() == [per] * 4


# ------------------------------------------------------------------------------------------------ CLI end to end
def _run(cmd, env=None):
    r = subprocess.run(cmd, env=env or dict(os.environ), capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


@pytest.fixture(scope="module")
def cifar100_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("cifar")
    write_fake_cifar(str(root), "cifar100", 100, 3, seed=5)
    return str(root)


def test_train_cli_on_cifar100_files(cifar100_tree, tmp_path):
    """The published two-stage recipe on a fake cifar-100-python tree: representation stage with --auto-augment cifar,
    mixup and the cosine classifier, then the --decoup --classif iif stage from its checkpoint."""
    common = [sys.executable, "-m", "iif_amd.train", "--dset_name", "cifar100", "--data-path", cifar100_tree, "--model",
              "resnet32", "--imb_factor", "0.1", "-b", "32", "-j", "0", "--epochs", "1", "--max-iters", "3",
              "--classif_norm", "cosine", "--auto-augment", "cifar"]
    s1 = tmp_path / "s1"
    out = _run(common + ["--mixup", "0.2", "--output-dir", str(s1)])
    assert re.search(r"\* Acc@1 \S+ Acc@5", out) and "Test:" in out
    ck = torch.load(s1 / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert ck["epoch"] == 0 and ck["args"].data_path == cifar100_tree
    s2 = tmp_path / "s2"
    out = _run(common + ["--load_from", str(s1 / "checkpoint.pth"), "--lr", "0.0001", "--classif", "iif", "--iif", "smooth",
                         "--decoup", "--output-dir", str(s2), "--shot-acc"])
    assert "Many shot Acc is:" in out and (s2 / "checkpoint.pth").exists()


def test_train_cli_upsampling_and_per_shot_acc(cifar100_tree, tmp_path):
    out = _run([sys.executable, "-m", "iif_amd.train", "--dset_name", "cifar100", "--data-path", cifar100_tree, "--model",
                "resnet32", "--imb_factor", "0.1", "-b", "32", "-j", "0", "--epochs", "1", "--max-iters", "2",
                "--sampler", "upsampling", "--output-dir", str(tmp_path)])
    assert "Acc@1" in out
    out = _run([sys.executable, "-m", "iif_amd.per_shot_acc", "--dset_name", "cifar100", "--data-path", cifar100_tree,
                "--model", "resnet32", "--imb_factor", "0.1", "--load_from", str(tmp_path / "checkpoint.pth"), "-b", "64",
                "-j", "0", "--classif", "iif"])
    assert "Many shot Acc is:" in out


# ------------------------------------------------------------------------------------------------ two ranks
def test_two_ranks_see_disjoint_shards(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
          "--master-port", "29583", os.path.join(HERE, "cifar_ddp_worker.py"), str(tmp_path)], env=env)
    r = [torch.load(tmp_path / ("rank%d.pt" % k)) for k in (0, 1)]
    for e in (0, 1):
        a, b = r[0]["index%d" % e], r[1]["index%d" % e]
        assert len(a) == len(b) and not set(a.tolist()) & set(b.tolist())
        assert sorted(a.tolist() + b.tolist()) == list(range(len(a) + len(b)))
        targets = torch.tensor(r[0]["targets_all"])
        assert torch.equal(r[0]["targets%d" % e], targets[a[:len(r[0]["targets%d" % e])]])
        assert torch.equal(r[1]["targets%d" % e], targets[b[:len(r[1]["targets%d" % e])]])
    assert not torch.equal(r[0]["index0"], r[0]["index1"])
    assert sorted(r[0]["eval"] + r[1]["eval"]) == list(range(2 * len(r[0]["eval"])))
    assert not torch.equal(r[0]["images0"], r[1]["images0"])
