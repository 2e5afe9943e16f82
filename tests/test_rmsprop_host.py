"""RMSprop without a device: the C entry iif_rmsprop_step is declared, exported and bound, its argument checks return
before any HIP call, and the engine's RMSprop state round-trips through torch.optim.RMSprop (classification/train.py:205-207)
on a CPU-built engine."""
import argparse
import ctypes
import os
import re

import pytest
import torch

from iif_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
ALPHA, EPS = 0.9, 0.0316


def test_entry_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    assert re.search(r"\bint\s+iif_rmsprop_step\s*\(", hdr)
    assert "iif_rmsprop_step" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["iif_rmsprop_step"]) == 15
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "iif_rmsprop_step")


def _call(params=0x1000, grads=0x2000, sq=0x3000, buf=0x4000, gavg=0, n=16, lr=0.01, alpha=ALPHA, eps=EPS, wd=1e-4,
          momentum=0.9, centered=0):
    return _lib.lib().iif_rmsprop_step(params, grads, sq, buf, gavg, n, lr, 0, alpha, eps, wd, momentum, centered, 1.0, 0)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("kw", [
    dict(n=-1), dict(params=0), dict(grads=0), dict(sq=0), dict(buf=0), dict(centered=1),
    dict(lr=-0.1), dict(lr=NAN), dict(lr=INF), dict(eps=-1e-8), dict(eps=NAN), dict(alpha=-0.5), dict(alpha=INF),
    dict(momentum=-0.9), dict(momentum=NAN), dict(wd=-1e-4), dict(wd=INF), dict(n=0, lr=-1.0)])
def test_entry_rejects_bad_arguments(kw):
    assert _call(**kw) == EINVAL


@pytest.mark.parametrize("kw", [dict(params=0x1004), dict(grads=0x2008), dict(sq=0x300c), dict(buf=0x4004),
                                dict(gavg=0x5004, centered=1)])
def test_entry_refuses_misaligned_arena(kw):
    assert _call(**kw) == EUNSUPPORTED


def test_entry_optional_buffers_and_empty_arena():
    assert _call(n=0) == OK
    assert _call(n=0, params=0, grads=0, sq=0, buf=0) == OK
    # momentum 0 never reads the momentum buffer, no centering never reads grad_avg: neither is checked
    assert _call(buf=0x4004, momentum=0.0, sq=0x3001) == EUNSUPPORTED       # (the square_avg pointer still is)
    assert _call(buf=0, momentum=0.0, n=0) == OK


# ----------------------------------------------------------------- state interop on a CPU-built engine
def _net(head_only=False):
    from iif_amd import resnet_cifar
    net = resnet_cifar.resnet20(num_classes=10, device="cpu", compute_dtype=torch.float32)
    if head_only:
        net.select_training_param()
    return net


def _fill(net, momentum, centered, seed=0, steps=(7, 0)):
    """Random RMSprop state in the engine's arenas, as if it had stepped ``steps`` = (whole arena, head only) times.  Padding
    lanes stay 0 (the views cover the real elements only)."""
    g = torch.Generator().manual_seed(seed)
    net._alloc_rmsprop_state(centered)
    arenas = [net._sq_arena] + ([net._mom_arena] if momentum > 0 else []) + ([net._gavg_arena] if centered else [])
    for a in arenas:                                                   # square_avg > grad_avg^2, as a real run keeps it
        for v in net._arena_views(a):
            r = torch.rand(v.shape, generator=g)
            v.copy_(1.0 + r if a is net._sq_arena else r - 0.5)
    net._rms_steps = list(steps)
    net._optimizer_kind = "rmsprop"


def _torch_rmsprop(net, momentum, centered):
    params = [torch.nn.Parameter(torch.zeros_like(p)) for p in net.parameters()]
    return params, torch.optim.RMSprop(params, lr=0.1, alpha=ALPHA, eps=EPS, weight_decay=1e-4, momentum=momentum,
                                       centered=centered)


@pytest.mark.parametrize("momentum,centered", [(0.0, False), (0.9, False), (0.0, True), (0.9, True)])
def test_state_dict_loads_into_torch_rmsprop_and_back(momentum, centered):
    net = _net()
    _fill(net, momentum, centered)
    sd = net.rmsprop_state_dict(0.05, ALPHA, EPS, 1e-4, momentum, centered, initial_lr=0.1)
    g = sd["param_groups"][0]
    assert set(g) == {"lr", "momentum", "alpha", "eps", "centered", "weight_decay", "capturable", "foreach", "maximize",
                      "differentiable", "params", "initial_lr"}
    params, opt = _torch_rmsprop(net, momentum, centered)
    ref = opt.state_dict()["param_groups"][0]
    assert set(ref) | {"initial_lr"} == set(g)                        # exactly torch's keys, plus the scheduler's
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 0.05 and opt.param_groups[0]["initial_lr"] == 0.1
    views = {"square_avg": net._arena_views(net._sq_arena), "momentum_buffer": net._arena_views(net._mom_arena),
             "grad_avg": net._arena_views(net._gavg_arena) if centered else None}
    for i, p in enumerate(params):
        st = opt.state[p]
        want = {"step", "square_avg"} | ({"momentum_buffer"} if momentum > 0 else set()) | ({"grad_avg"} if centered else set())
        assert set(st) == want, i
        assert st["step"].dim() == 0 and st["step"].is_floating_point() and float(st["step"]) == 7.0
        for k in want - {"step"}:
            assert st[k].shape == p.shape and torch.equal(st[k], views[k][i]), (i, k)
    # torch steps once on these buffers without complaint (the structure is what its _init_group expects)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()
    # ... and a torch RMSprop state dict comes back into the arenas bit for bit
    net2 = _net()
    assert net2.load_optimizer_state_dict(opt.state_dict(), optimizer="rmsprop") == []
    assert net2._rms_steps == [8, 0]
    back = net2.rmsprop_state_dict(0.1, ALPHA, EPS, 1e-4, momentum, centered)
    for i, p in enumerate(params):
        for k, v in opt.state[p].items():
            assert torch.equal(back["state"][i][k], v), (i, k)
    for a in (net2._sq_arena, net2._mom_arena) + ((net2._gavg_arena,) if centered else ()):
        real = torch.zeros_like(a, dtype=torch.bool)
        for v in net2._arena_views(real):
            v.fill_(True)
        assert not a[~real].any()                                     # padding lanes hold 0


def test_head_only_engine_has_no_backbone_state():
    net = _net(head_only=True)
    _fill(net, 0.9, False, steps=(0, 3))
    sd = net.rmsprop_state_dict(0.01, ALPHA, EPS, 1e-4, 0.9, False)
    n = len(list(net.parameters()))
    head = [i for i, p in enumerate(net.parameters()) if p.requires_grad]
    assert head == [n - 2, n - 1] and sorted(sd["state"]) == head
    assert all(float(sd["state"][i]["step"]) == 3.0 for i in head)
    params, opt = _torch_rmsprop(net, 0.9, False)
    opt.load_state_dict(sd)
    assert all(len(opt.state[params[i]]) == 0 for i in range(n) if i not in head)
    # torch's own state after stepping only the head: the backbone has no entry, and comes back as reported missing
    for i in head:
        params[i].grad = torch.randn_like(params[i])
    opt.step()
    net2 = _net(head_only=True)
    missing = net2.load_optimizer_state_dict(opt.state_dict())
    assert missing == [i for i in range(n) if i not in head]
    assert net2._rms_steps == [0, 4]
    for v in net2._arena_views(net2._sq_arena)[:head[0]]:
        assert not v.any()
    # a run stepped on the whole arena first, then head-only: the head has taken both kinds of step
    net3 = _net()
    _fill(net3, 0.9, False, steps=(5, 2))
    sd3 = net3.rmsprop_state_dict(0.01, ALPHA, EPS, 1e-4, 0.9, False)
    assert [float(sd3["state"][i]["step"]) for i in (0, head[0])] == [5.0, 7.0]
    net4 = _net()
    net4.load_optimizer_state_dict(sd3)
    assert net4._rms_steps == [5, 2]


def test_unstepped_engine_has_empty_state_and_sgd_run_allocates_nothing():
    net = _net()
    assert net._sq_arena is None and net._gavg_arena is None
    sd = net.rmsprop_state_dict(0.1, ALPHA, EPS, 1e-4, 0.9, False)
    assert sd["state"] == {} and len(sd["param_groups"][0]["params"]) == len(list(net.parameters()))
    net.optimizer_state_dict(0.1)                                     # an SGD checkpoint: no RMSprop buffer appears
    assert net._sq_arena is None


def _sgd_state(net):
    params = [torch.nn.Parameter(torch.zeros_like(p)) for p in net.parameters()]
    opt = torch.optim.SGD(params, lr=0.1, momentum=0.9, weight_decay=1e-4)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()
    return opt.state_dict()


def test_sgd_state_with_rmsprop_expected_raises():
    net = _net()
    sd = _sgd_state(net)
    before = net._mom_arena.clone()
    with pytest.raises(ValueError, match="SGD state.*RMSprop"):
        net.load_optimizer_state_dict(sd, optimizer="RMSprop")
    assert torch.equal(net._mom_arena, before) and net._sq_arena is None
    # the other way round too; and without an expectation an SGD dict loads as before
    _fill(net, 0.9, False)
    with pytest.raises(ValueError, match="RMSprop state.*SGD"):
        _net().load_optimizer_state_dict(net.rmsprop_state_dict(0.1), optimizer="sgd")
    assert _net().load_optimizer_state_dict(sd) == []
    assert _net().load_optimizer_state_dict(sd, optimizer="nesterov") == []


def test_one_engine_serves_one_optimizer():
    net = _net()
    net.load_optimizer_state_dict(_sgd_state(net))
    with pytest.raises(RuntimeError, match="one optimizer"):
        net.load_optimizer_state_dict(_rms_dict(), optimizer="rmsprop")
    with pytest.raises(RuntimeError, match="stepped with SGD"):
        net.rmsprop_state_dict(0.1)
    net2 = _net()
    _fill(net2, 0.9, False)
    with pytest.raises(RuntimeError, match="stepped with RMSprop"):
        net2.optimizer_state_dict(0.1)


def _rms_dict():
    net = _net()
    _fill(net, 0.9, False)
    return net.rmsprop_state_dict(0.1)


def test_trainer_accepts_rmsprop_in_any_case_and_rejects_others(monkeypatch):
    from iif_amd import train
    assert "rmsprop" in train.OPTIMIZERS and (train.RMSPROP_ALPHA, train.RMSPROP_EPS) == (0.9, 0.0316)
    args = train.get_args_parser().parse_args(["--opt", "RMSprop"])
    assert args.opt.lower() in train.OPTIMIZERS
    # an unknown optimizer still fails with the reference's message, before any data or model is built
    monkeypatch.setattr(train.torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(train.initialisers, "get_data", lambda a: (None, 10, None, None, None))
    monkeypatch.setattr(train, "build_model", lambda a, n: argparse.Namespace())
    monkeypatch.setattr(train.initialisers, "get_criterion", lambda *a: None)
    bad = train.get_args_parser().parse_args(["--opt", "adam", "--device", "cpu"])
    with pytest.raises(RuntimeError, match="Invalid optimizer adam. Only SGD and RMSprop are supported."):
        train.main(bad)
