"""The auto-augment policy of the list-dataset device input without a device: its draws (slots 48..55 of the per-sample
key) and their frequencies, the op records against cifar.policy_table, the packed policy section, the C ABI's argument
checks (which return before any HIP call), the --device-policy CLI checks and get_data's choice of loader."""
import ctypes
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from iif_amd import _lib, augment, cifar, initialisers, lt_device, train
from iif_amd.cifar import _mix64, sample_keys

from .lt_cases import smooth_image, write_npy_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
N = 1 << 16


def _uniforms_many(seed, epoch, rank, n):
    """policy_uniforms for positions 0 .. n - 1 at once, float64 [n, 8]."""
    key = sample_keys(seed, epoch, rank, np.arange(n))
    slots = np.arange(lt_device.POLICY_SLOT, lt_device.POLICY_SLOT + lt_device.N_POLICY_SLOTS, dtype=np.uint64)
    return (_mix64(key[:, None] ^ slots[None, :]) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def _within_5_sigma(count, n, p):
    return abs(count - n * p) <= 5 * math.sqrt(n * p * (1 - p)) + 1


# ---------------------------------------------------------------------------------------------------------- draws
def test_policy_draws_are_deterministic_and_differ_across_epochs_and_ranks():
    def d(seed, epoch, rank, pos, policy="imagenet"):
        return tuple(map(tuple, lt_device.policy_record(lt_device.draw_policy(policy, lt_device.policy_uniforms(
            seed, epoch, rank, pos)), 224).tolist()))
    for policy in ("imagenet", "randaugment"):
        a = [d(3, 2, 1, p, policy) for p in range(64)]
        assert a == [d(3, 2, 1, p, policy) for p in range(64)]
        assert len(set(a)) > 20
        for other in ([d(3, 3, 1, p, policy) for p in range(64)], [d(3, 2, 0, p, policy) for p in range(64)]):
            assert sum(x == y for x, y in zip(a, other)) < 16
    u = lt_device.policy_uniforms(3, 2, 1, 5)
    assert u.shape == (8,) and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(_uniforms_many(3, 2, 1, 6)[5], u)
    # slots 0..47 stay as they are
    assert lt_device.N_SLOTS == 48 and lt_device.uniforms(3, 2, 1, 5).shape == (48,)


def test_imagenet_draw_frequencies():
    u = _uniforms_many(11, 0, 0, N)
    subs = augment._P["imagenet"]
    sub = (u[:, 0] * 25).astype(int)
    for k in range(25):
        assert _within_5_sigma(int((sub == k).sum()), N, 1 / 25), k
    draws = [lt_device.draw_policy("imagenet", row) for row in u]
    for j in range(2):
        for k in range(25):
            rows = np.flatnonzero(sub == k)
            applied = sum(draws[i][j] is not None for i in rows)
            assert _within_5_sigma(applied, len(rows), subs[k][3 * j + 1]), (k, j)
        for i in range(4):                                 # the draw restates the rule
            assert (draws[i][j] is not None) == (u[i, 1 + 2 * j] < subs[sub[i]][3 * j + 1])
        signs = [draws[i][j][2] for i in range(N) if draws[i][j] is not None]
        assert _within_5_sigma(sum(s > 0 for s in signs), len(signs), 0.5)
        assert all(draws[i][j] is None or draws[i][j][:2] == (subs[sub[i]][3 * j], subs[sub[i]][3 * j + 2]) for i in range(N))


def test_randaugment_draw_frequencies():
    u = _uniforms_many(12, 1, 0, N)
    draws = [lt_device.draw_policy("randaugment", row) for row in u]
    ops = augment.RandAugment.OPS
    for j in range(2):
        assert all(d[j] is not None and d[j][1] == 9 for d in draws)
        names = [d[j][0] for d in draws]
        for name in ops:
            assert _within_5_sigma(names.count(name), N, 1 / 14), (j, name)
        assert _within_5_sigma(sum(d[j][2] > 0 for d in draws), N, 0.5)
        assert draws[0][j][0] == ops[int(u[0, 2 * j] * 14)]


def test_cifar_policy_uses_the_cifar10_table():
    u = lt_device.policy_uniforms(0, 0, 0, 0).copy()
    u[1:] = 0.0                                            # every op applied, signs +1
    for k in range(25):
        u[0] = (k + 0.5) / 25
        sub = augment._P["cifar10"][k]
        want = [(sub[3 * j], sub[3 * j + 2], 1.0) if sub[3 * j + 1] > 0 else None for j in range(2)]   # probability 0: never
        assert lt_device.draw_policy("cifar", u) == lt_device.draw_policy("cifar10", u) == want
    with pytest.raises(ValueError):
        lt_device.draw_policy("autoaugment", u)


# ---------------------------------------------------------------------------------------------------------- records
@pytest.mark.parametrize("policy,table", [("imagenet", "imagenet"), ("cifar", "cifar10")])
def test_records_equal_the_policy_table_words(policy, table):
    tab = cifar.policy_table(augment._P[table], 32, 32)
    for s, sub in enumerate(augment._P[table]):
        for k, sign in enumerate((-1.0, 1.0)):
            rec = lt_device.policy_record([(sub[0], sub[2], sign), (sub[3], sub[5], sign)], 32)
            for j in range(2):
                assert rec[j, 0] == tab[s, j, k, 0] and np.array_equal(rec[j, 1:7], tab[s, j, k, 2:8]) and rec[j, 7] == 0
    rec = lt_device.policy_record([None, ("Rotate", 4, 1.0)], 224)
    assert rec.dtype == np.uint32 and rec.shape == (2, 8)
    assert rec[0, 0] == lt_device.OP_NONE == 0xFF and not rec[0, 1:].any()
    want = np.asarray(augment.affine_coefficients("Rotate", augment._ranges()["Rotate"][4], 1.0, 224, 224), np.float32)
    assert rec[1, 0] == cifar.OPS.index("Rotate") and np.array_equal(rec[1, 1:7].view(np.float32), want)


def test_policy_table_is_unchanged_by_the_factoring():
    tab = cifar.policy_table()
    for s, sub in enumerate(augment._P["cifar10"]):
        for j in range(2):
            for k, sign in enumerate((-1.0, 1.0)):
                assert np.array_equal(tab[s, j, k, 2:], cifar.op_constants(sub[3 * j], sub[3 * j + 2], sign))
    assert cifar.op_constants("Posterize", 9, 1.0)[0] == 0xF0 and cifar.op_constants("Solarize", 0, 1.0)[0] == 256


# ---------------------------------------------------------------------------------------------------------- packing
def test_pack_round_trip_with_the_policy_section():
    imgs = [smooth_image(30, 41, 1), smooth_image(17, 5, 2), smooth_image(60, 61, 5)]
    plain, pol = [], []
    for i, im in enumerate(imgs):
        region, words, _ = lt_device.train_sample(im, 16, lt_device.uniforms(0, 0, 0, i))
        rec = lt_device.policy_record(lt_device.draw_policy("randaugment", lt_device.policy_uniforms(0, 0, 0, i)), 16)
        plain.append((region, words, None, 7 + i))
        pol.append((region, words, None, 7 + i, rec))
    a, b = lt_device.pack(plain), lt_device.pack(pol)
    pa, da, ja, ta = lt_device.unpack(a, 3)
    pb, db, jb, tb, ob = lt_device.unpack(b, 3, policy=True)
    assert torch.equal(pa, pb) and torch.equal(da, db) and torch.equal(ja, jb) and torch.equal(ta, tb)
    assert ob.shape == (3, 2, 8) and ob.dtype == torch.int32
    for i, s in enumerate(pol):
        assert np.array_equal(ob[i].numpy().view(np.uint32), s[4])
    assert b.numel() == a.numel() + 3 * 64
    with pytest.raises(ValueError):
        lt_device.pack([plain[0], pol[1]])


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbol_in_header_ctypes_table_and_library():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    assert re.search(r"int iif_lt_augment_policy\(", text) and re.search(r"#define IIF_LT_OP_NONE 0xFFu", text)
    assert len(_lib.SIGNATURES["iif_lt_augment_policy"]) == 10
    assert hasattr(_lib.lib(), "iif_lt_augment_policy")


def test_argument_checks_return_einval_without_a_device():
    f = _lib.lib().iif_lt_augment_policy
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)                       # never dereferenced as device memory: every call returns before any launch

    def call(pool=p, nbytes=64, desc=p, ops=p, batch=2, size=8, ms=p, work=p, out=p):
        return f(pool, nbytes, desc, ops, batch, size, ms, work, out, None)
    for kw in ({"pool": 0}, {"desc": 0}, {"ops": 0}, {"ms": 0}, {"work": 0}, {"out": 0}, {"nbytes": -1}, {"batch": -1},
               {"size": 0}, {"size": -3}, {"size": 16385}):
        assert call(**kw) == EINVAL, kw
    assert call(batch=0) == 0                       # nothing to do, no launch


def test_wrapper_refuses_cpu_tensors():
    x = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(_lib.IIFNativeError):
        lt_device.lt_augment_policy(x, torch.zeros(1, 8, dtype=torch.int64), torch.zeros(1, 2, 8, dtype=torch.int32), 8,
                                    (0.5,) * 3, (0.2,) * 3)


# ------------------------------------------------------------------------------------------------------------ CLI
NS = dict(device_augment=True, device_policy=True, data_path="/data", dset_name="places_lt", auto_augment="imagenet")


def test_cli_accepts_device_policy():
    for policy in ("imagenet", "randaugment", "cifar"):
        train.check_device_augment(types.SimpleNamespace(**dict(NS, auto_augment=policy)))
    args = train.get_args_parser().parse_args(["--dset_name", "imagenet_lt", "--device-augment", "--device-policy",
                                               "--auto-augment", "randaugment"])
    assert args.device_policy is True and args.device_augment is True
    assert train.get_args_parser().parse_args([]).device_policy is False


@pytest.mark.parametrize("kw,msg", [({"device_augment": False}, "needs --device-augment"),
                                    ({"auto_augment": None}, "needs --auto-augment"),
                                    ({"auto_augment": "autoaugment"}, "does not know")])
def test_cli_refuses_device_policy(kw, msg):
    with pytest.raises(SystemExit, match=msg):
        train.check_device_augment(types.SimpleNamespace(**dict(NS, **kw)))


def test_cli_refusal_without_the_flag_keeps_its_message_and_hints():
    with pytest.raises(SystemExit, match="stays on the host.*add --device-policy"):
        train.check_device_augment(types.SimpleNamespace(**dict(NS, device_policy=False)))


@pytest.mark.parametrize("extra,msg", [(["--device-policy", "--data-path", "/x", "--auto-augment", "imagenet"],
                                        "needs --device-augment"),
                                       (["--device-augment", "--device-policy", "--data-path", "/x"], "needs --auto-augment")])
def test_cli_refuses_before_touching_a_device(extra, msg):
    r = subprocess.run([sys.executable, "-m", "iif_amd.train", "--dset_name", "places_lt"] + extra,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and msg in r.stderr, r.stderr[-2000:]


def _args(tmp_path, **kw):
    train_txt, eval_txt = write_npy_tree(str(tmp_path), [(40 + i, 50, 3) for i in range(13)],
                                         [0] * 2 + [1] * 7 + [2] * 4, eval_count=5)
    a = dict(dset_name="places_lt", data_path=str(tmp_path), train_txt=train_txt, eval_txt=eval_txt, image_size=32,
             rand_number=0, sampler="random", distributed=False, batch_size=4, workers=0, device="cpu",
             device_augment=True)
    a.update(kw)
    return types.SimpleNamespace(**a)


@pytest.mark.parametrize("policy", ["imagenet", "randaugment"])
def test_get_data_passes_the_policy_to_the_training_loader(tmp_path, policy):
    ds, C, loader, loader_test, sampler = initialisers.get_data(_args(tmp_path, device_policy=True, auto_augment=policy))
    assert isinstance(loader, lt_device.DeviceLTLoader) and ds.transform is None and sampler is loader
    assert loader.policy == policy and loader.jitter is None and loader.flags == 0
    assert loader_test.policy is None and not loader_test.train
    # without --device-policy the policy stays out of the device loader (check_device_augment refuses such a run)
    _, _, plain, _, _ = initialisers.get_data(_args(tmp_path, auto_augment=policy))
    assert plain.policy is None and plain.flags == lt_device.JITTER


def test_policy_loader_crops_and_flips_as_the_jitter_loader(tmp_path):
    ds, _, jit, _, _ = initialisers.get_data(_args(tmp_path))
    _, _, pol, _, _ = initialisers.get_data(_args(tmp_path, device_policy=True, auto_augment="imagenet"))
    first = None
    for (a, Ba), (b, Bb) in zip(jit.batches(1), pol.batches(1)):
        pa, da, _, ta = lt_device.unpack(a, Ba)
        pb, db, _, tb, ob = lt_device.unpack(b, Bb, policy=True)
        assert torch.equal(da, db) and torch.equal(ta, tb) and torch.equal(pa, pb) and ob.shape == (Bb, 2, 8)
        first = ob if first is None else first
    for p in range(4):                                     # the workers' records of positions 0 .. 3
        want = lt_device.policy_record(lt_device.draw_policy("imagenet", lt_device.policy_uniforms(0, 1, 0, p)), 32)
        assert np.array_equal(first[p].numpy().view(np.uint32), want)
    with pytest.raises(ValueError):
        lt_device.DeviceLTLoader(ds, 4, device="cpu", policy="autoaugment")
