"""CIFAR input without a device: the long-tailed subset against the reference's IMBALANCECIFAR10/100 (golden G21), the
file reader on fake trees, the per-epoch / per-rank index lists against torch's samplers and BalanceClassSampler, the
policy constants against augment.py's tables, the numpy hash, and the argument checks of iif_cifar_augment (which
return before any HIP call)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
from torch.utils.data.distributed import DistributedSampler

from iif_amd import _lib, augment, cifar, initialisers, train
from iif_amd.imbalanced_dataset import img_num_per_cls
from iif_amd.samplers import BalanceClassSampler

from .cifar_cases import write_fake_cifar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
G21 = [(C, t, f, r) for C in (10, 100) for t, f in (("exp", 0.01), ("exp", 0.02), ("exp", 0.1), ("step", 0.1)) for r in (0, 1)]


# -------------------------------------------------------------------------------------------------- G21: the subset
@pytest.mark.parametrize("case", G21, ids=["c%d_%s_%g_r%d" % c for c in G21])
def test_imbalanced_subset_equals_reference(golden, case):
    C, imb_type, imb, r = case
    g = golden("g21_cifar_imb")
    k = "c%d_%s_%g_r%d" % case
    labels = g["c%d_labels" % C].astype(np.int64)
    state = np.random.get_state()
    counts = img_num_per_cls(C, len(labels), imb_type, imb)
    sel, num_per_cls = cifar.gen_imbalanced_indices(labels, counts, r)
    assert np.array_equal(sel, g[k + "_index"].astype(np.int64))
    assert np.array_equal(labels[sel], g[k + "_targets"].astype(np.int64))
    assert [num_per_cls[i] for i in range(C)] == g[k + "_cls_num_list"].tolist()
    after = np.random.get_state()                       # numpy's global generator is left alone
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]


def test_cifar_lt_reads_and_selects(tmp_path):
    data, labels, test_data, test_labels = write_fake_cifar(str(tmp_path), "cifar10", 40, 7, seed=3)
    ds = cifar.cifar_lt(str(tmp_path), "cifar10", "exp", 0.1, 1)
    sel, _ = cifar.gen_imbalanced_indices(labels, img_num_per_cls(10, 400, "exp", 0.1), 1)
    assert np.array_equal(ds.source_index, sel)
    assert np.array_equal(ds.data, data[sel]) and ds.targets == labels[sel].tolist()
    assert ds.get_cls_num_list() == img_num_per_cls(10, 400, "exp", 0.1)
    assert ds.targets == sorted(ds.targets)                 # class-sorted, as the reference's vstack
    t = cifar.cifar_test(str(tmp_path), "cifar10")
    assert np.array_equal(t.data, test_data) and t.targets == test_labels.tolist()
    assert t.get_cls_num_list() == [7] * 10


# ---------------------------------------------------------------------------------------------------------- reader
@pytest.mark.parametrize("name", ["cifar10", "cifar100"])
def test_reader_layouts_and_row_order(tmp_path, name):
    data, labels, test_data, test_labels = write_fake_cifar(str(tmp_path), name, 6, 2, seed=11)
    d, t = cifar.read_cifar(str(tmp_path), name, train=True)
    assert d.dtype == np.uint8 and d.shape == (len(labels), 3072) and d.flags.c_contiguous
    assert np.array_equal(d, data) and np.array_equal(t, labels)       # CIFAR-10: five batches in file order
    d, t = cifar.read_cifar(str(tmp_path), name, train=False)
    assert np.array_equal(d, test_data) and np.array_equal(t, test_labels)


def test_reader_names_missing_files(tmp_path):
    write_fake_cifar(str(tmp_path), "cifar10", 2, 1)
    os.remove(os.path.join(str(tmp_path), "cifar-10-batches-py", "data_batch_4"))
    with pytest.raises(FileNotFoundError, match="data_batch_4"):
        cifar.read_cifar(str(tmp_path), "cifar10")
    with pytest.raises(FileNotFoundError, match=re.escape(os.path.join("cifar-100-python", "train"))):
        cifar.read_cifar(str(tmp_path), "cifar100")


def test_get_data_reads_cifar_from_data_path(tmp_path):
    """--data-path is no longer ignored for CIFAR: it is read (here: missing files raise); without it the synthetic set stays."""
    args = train.get_args_parser().parse_args(["--dset_name", "cifar100", "--data-path", str(tmp_path), "-j", "0"])
    with pytest.raises(FileNotFoundError, match="cifar-100-python"):
        initialisers.get_data(args)
    args = train.get_args_parser().parse_args(["--dset_name", "cifar100", "-j", "0"])
    ds, C, loader, _, sampler = initialisers.get_data(args)
    assert C == 100 and type(ds).__name__ == "SyntheticLT" and isinstance(loader, torch.utils.data.DataLoader)


# ----------------------------------------------------------------------------------------------------- index lists
@pytest.mark.parametrize("epoch", [0, 1, 5])
def test_random_list_is_random_sampler(epoch):
    g = torch.Generator().manual_seed(3 + epoch)
    ref = list(torch.utils.data.RandomSampler(range(1000), generator=g))
    assert cifar.epoch_indices(1000, epoch, seed=3).tolist() == ref
    assert cifar.epoch_indices(1000, epoch, seed=3, train=False).tolist() == list(range(1000))


@pytest.mark.parametrize("world", [2, 3, 8])
def test_distributed_lists_are_distributed_sampler(world):
    n = 1001
    for epoch in (0, 2):
        shards = []
        for rank in range(world):
            s = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=True, seed=4)
            s.set_epoch(epoch)
            got = cifar.epoch_indices(n, epoch, seed=4, rank=rank, world=world)
            assert got.tolist() == list(s)
            shards.append(got)
            e = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=False)
            assert cifar.epoch_indices(n, epoch, train=False, rank=rank, world=world).tolist() == list(e)
        assert set(np.concatenate(shards).tolist()) == set(range(n))
    assert not np.array_equal(cifar.epoch_indices(n, 0, rank=0, world=2), cifar.epoch_indices(n, 1, rank=0, world=2))


@pytest.mark.parametrize("mode", ["upsampling", "downsampling"])
def test_balanced_lists_are_balance_class_sampler(mode):
    labels = np.repeat(np.arange(6), [50, 31, 17, 9, 4, 2]).tolist()
    for epoch in (0, 1):
        np.random.seed(9 + epoch)
        ref = list(BalanceClassSampler(labels, mode=mode))
        got = cifar.epoch_indices(len(labels), epoch, seed=9, mode=mode, labels=labels)
        assert got.tolist() == ref
        # DDP: DistributedSamplerWrapper's shards of the same inner list (every rank draws the same list)
        world = 3
        shards = []
        for rank in range(world):
            w = DistributedSampler(range(len(ref)), num_replicas=world, rank=rank, shuffle=True, seed=9)
            w.set_epoch(epoch)
            got = cifar.epoch_indices(len(labels), epoch, seed=9, mode=mode, labels=labels, rank=rank, world=world)
            assert got.tolist() == [ref[i] for i in w]
            shards.append(list(w))
        assert set(sum(shards, [])) == set(range(len(ref)))


# ----------------------------------------------------------------------------------------------- policy constants
def test_policy_table_is_built_from_augment_tables():
    tab = cifar.policy_table()
    ranges = augment._ranges()
    assert tab.shape == (25, 2, 2, 8) and tab.dtype == np.uint32
    f32 = lambda v: np.float32(v).view(np.uint32)      # noqa: E731
    for s, sub in enumerate(augment._P["cifar10"]):
        for j in range(2):
            name, prob, mag = sub[3 * j:3 * j + 3]
            m = ranges[name][mag]
            for k, sign in enumerate((-1.0, 1.0)):
                w = tab[s, j, k]
                assert cifar.OPS[w[0]] == name and w[1] == round(prob * 2 ** 24)
                if name in augment.GEOMETRIC:
                    assert w[2:8].tolist() == [f32(v) for v in augment.affine_coefficients(name, m, sign, 32, 32)]
                elif name in cifar.BLEND:
                    assert w[2] == f32(1.0 + m * sign) and w[3] == f32(1.0 - (1.0 + m * sign))
                elif name == "Posterize":
                    assert w[2] == (0xFF << (8 - m)) & 0xFF
                elif name == "Solarize":
                    assert w[2] == math.ceil(m)
                else:
                    assert not w[2:].any()
    # the table follows augment.py: an edit there reaches the kernel's constants
    subs = list(augment._P["cifar10"])
    subs[3] = ("Rotate", 0.25, 9, "Posterize", 1.0, 9)
    t2 = cifar.policy_table(subs)
    assert cifar.OPS[t2[3, 0, 0, 0]] == "Rotate" and t2[3, 0, 0, 1] == 2 ** 22 and t2[3, 1, 1, 2] == 0xF0
    assert np.array_equal(np.delete(t2, 3, 0), np.delete(tab, 3, 0))
    with pytest.raises(ValueError):
        cifar.policy_table(subs[:24])


def test_apply_op_is_apply_op_signed_with_its_drawn_sign():
    img = torch.rand(3, 32, 32, generator=torch.Generator().manual_seed(0))
    for name in cifar.OPS:
        g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
        a = augment.apply_op(img, name, 6, g1)
        sign = 1.0 if torch.rand((), generator=g2).item() < 0.5 else -1.0
        assert torch.equal(a, augment.apply_op_signed(img, name, 6, sign)), name
        assert torch.equal(torch.rand(4, generator=g1), torch.rand(4, generator=g2))     # same RNG consumption


# ------------------------------------------------------------------------------------------------------------ hash
def _splitmix(z):
    M = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def test_hash_is_the_documented_splitmix_chain():
    tab = cifar.policy_table()
    seed, epoch, rank = 123456789012345, 7, 3
    pos = [0, 1, 1000, 2 ** 40]
    got = cifar.draw_params(seed, epoch, rank, pos, tab)
    for i, q in enumerate(pos):
        key = _splitmix(_splitmix(_splitmix(_splitmix(seed) ^ epoch) ^ rank) ^ q)
        u = [_splitmix(key ^ s) >> 32 for s in range(10)]
        sub = (u[3] * 25) >> 32
        want = [(u[0] * 9) >> 32, (u[1] * 9) >> 32, u[2] >> 31, sub,
                int((u[4] >> 8) < tab[sub, 0, 0, 1]), 1 - (u[5] >> 31), int((u[6] >> 8) < tab[sub, 1, 0, 1]), 1 - (u[7] >> 31),
                (u[8] * 32) >> 32, (u[9] * 32) >> 32]
        assert got[i].tolist() == want
    assert not cifar.draw_params(seed, epoch, rank, pos)[:, [4, 6]].any()      # without POLICY nothing is applied


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbol_in_header_and_ctypes_table():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    assert re.search(r"int iif_cifar_augment\(", text)
    for flag, v in (("IIF_CIFAR_CROP_FLIP", cifar.CROP_FLIP), ("IIF_CIFAR_POLICY", cifar.POLICY), ("IIF_CIFAR_CUTOUT", cifar.CUTOUT)):
        assert re.search(r"#define %s %du" % (flag, v), text)
    assert len(_lib.SIGNATURES["iif_cifar_augment"]) == 15
    assert hasattr(_lib.lib(), "iif_cifar_augment")


def test_argument_checks_return_einval_without_a_device():
    f = _lib.lib().iif_cifar_augment
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                       # never dereferenced: every call below returns before any HIP call

    def call(data=p, n=10, labels=p, index=p, batch=4, pos0=0, flags=1, policy=0, out=p, targets=p, params=0):
        return f(data, n, labels, index, batch, pos0, 1, 0, 0, flags, policy, out, targets, params, None)
    for kw in ({"data": 0}, {"labels": 0}, {"index": 0}, {"out": 0}, {"targets": 0}, {"n": 0}, {"n": -5}, {"batch": -1},
               {"pos0": -1}, {"flags": 8}, {"flags": 0x10 | 1}, {"flags": 2}, {"flags": 7}):
        assert call(**kw) == EINVAL, kw
    assert call(batch=0) == 0 and call(batch=0, flags=7, policy=p) == 0           # nothing to do, no launch
