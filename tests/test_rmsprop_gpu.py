"""The fused RMSprop step (iif_rmsprop_step; classification/train.py:205-207 torch.optim.RMSprop) on the GPU: the kernel
against torch's RMSprop in fp64, the engine against torch on the engine's own gradients, the loss curve against the CPU
oracle, the frozen backbone, one optimizer per engine, and ``--opt rmsprop`` through the trainer on one and two ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import iif_oracle as O
from oracle import resnet_oracle as R

from .test_resnet_gpu import DS, _build, _data, damp_residual_branches, gpu_relu_masks, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ALPHA, EPS = 0.9, 0.0316


def f32(v):
    """The fp32 value the kernel receives, as a Python float (so the fp64 reference uses the same coefficients)."""
    return float(np.float32(v))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-30)


def _torch_ref(p, momentum, centered, wd, lr):
    return torch.optim.RMSprop([p], lr=lr, alpha=f32(ALPHA), eps=f32(EPS), weight_decay=f32(wd), momentum=f32(momentum),
                               centered=centered, foreach=False)


@pytest.mark.parametrize("n", [1, 3, 4099, (1 << 20) + 5])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_kernel_matches_torch_rmsprop_fp64(n, wd, centered, momentum):
    """20 steps on the same gradients, grad_scale 0.5, the learning rate from a device scalar that changes every step (the
    host lr passed is a decoy): parameters and every state buffer within 1e-6 relative L2 of torch's fp64 RMSprop."""
    from iif_amd import ops
    g = torch.Generator(device=DEV).manual_seed(11)
    p = torch.randn(n, device=DEV, generator=g)
    sq, buf = torch.zeros_like(p), torch.zeros_like(p)
    ga = torch.zeros_like(p) if centered else None
    ref = p.double().clone()
    d_lr = torch.zeros(1, device=DEV)
    opt = _torch_ref(ref, momentum, centered, wd, 0.0)
    for it in range(20):
        lr = f32(1e-2 * (1.0 - it / 40.0))
        d_lr.fill_(lr)
        grad = torch.randn(n, device=DEV, generator=g) * (1.0 + it % 3)
        ops.rmsprop_step(p, grad, sq, 123.0, ALPHA, EPS, wd, momentum, momentum_buf=buf, grad_avg=ga, grad_scale=0.5,
                         d_lr=d_lr)
        ref.grad = grad.double() * 0.5
        opt.param_groups[0]["lr"] = lr
        opt.step()
    st = opt.state[ref]
    assert float(st["step"]) == 20
    assert rel_l2(p, ref) <= 1e-6
    assert rel_l2(sq, st["square_avg"]) <= 1e-6
    if momentum > 0:
        assert rel_l2(buf, st["momentum_buffer"]) <= 1e-6
    else:
        assert not buf.any()                       # never touched
    if centered:
        assert rel_l2(ga, st["grad_avg"]) <= 1e-6


def test_kernel_deterministic_and_refuses_misalignment():
    from iif_amd import _lib, ops
    n = 1 << 20
    g = torch.Generator(device=DEV).manual_seed(3)
    p0, grads = torch.randn(n + 4, device=DEV, generator=g), torch.randn(n + 4, device=DEV, generator=g)
    outs = []
    for _ in range(2):
        p, sq, buf, ga = p0[:n].clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        for _ in range(3):
            ops.rmsprop_step(p, grads[:n], sq, 1e-2, ALPHA, EPS, 1e-4, 0.9, momentum_buf=buf, grad_avg=ga)
        outs.append((p, sq, buf, ga))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    before = p0.clone()
    ptr = _lib.ptr
    rc = _lib.lib().iif_rmsprop_step(ptr(p0) + 4, ptr(grads), ptr(sq), ptr(buf), 0, n, 1e-2, 0, ALPHA, EPS, 1e-4, 0.9, 0,
                                     1.0, _lib.stream_ptr())
    assert rc == -2                                # IIF_EUNSUPPORTED, nothing launched
    torch.cuda.synchronize()
    assert torch.equal(p0, before)


def _real_mask(net, arena):
    real = torch.zeros_like(arena, dtype=torch.bool)
    for v in net._arena_views(real):
        v.fill_(True)
    return real


def _iif(C, dev=DEV):
    from iif_amd.custom import IIFLoss
    counts = [max(int(1000 * (5 / 1000) ** (i / (C - 1.0))), 1) for i in range(C)]
    return counts, IIFLoss(DS(counts), variant="raw")


@pytest.mark.parametrize("arch,C,B,hw,centered", [("resnet20", 10, 8, 32, True), ("resnet50", 100, 4, 64, False)])
def test_engine_matches_torch_on_its_own_gradients(arch, C, B, hw, centered):
    """Each step's gradient arena, seen through _arena_views, steps an fp64 torch RMSprop copy of the parameters: the
    engine's parameters and state agree per tensor to 1e-6 relative L2, and the padding lanes of every arena stay 0."""
    from iif_amd import resnet_cifar, resnet_pytorch
    torch.manual_seed(0)
    if arch == "resnet20":
        net = resnet_cifar.resnet20(num_classes=C, use_norm="None", compute_dtype=torch.float32)
    else:
        net = resnet_pytorch.resnet50(num_classes=C, use_norm="None", pretrained="None", compute_dtype=torch.float32)
    net.train()
    counts, crit = _iif(C)
    x, y = _data(B, hw, counts, seed=4)
    x, y = x.to(DEV), y.to(DEV)
    ref = [p.detach().double().clone() for p in net.parameters()]
    opt = torch.optim.RMSprop(ref, lr=1e-3, alpha=f32(ALPHA), eps=f32(EPS), weight_decay=f32(1e-4), momentum=f32(0.9),
                              centered=centered, foreach=False)
    for it in range(3):
        net.loss_and_backward(x, y, crit)
        grads = [v.detach().double().clone() for v in net._arena_views(net._grad_arena)]
        net.rmsprop_step(1e-3, ALPHA, EPS, 1e-4, 0.9, centered=centered)
        for r, gr in zip(ref, grads):
            r.grad = gr
        opt.step()
    torch.cuda.synchronize()
    views = {"square_avg": net._arena_views(net._sq_arena), "momentum_buffer": net._arena_views(net._mom_arena)}
    if centered:
        views["grad_avg"] = net._arena_views(net._gavg_arena)
    for i, (p, r) in enumerate(zip(net.parameters(), ref)):
        assert rel_l2(p, r) <= 1e-6, (i, rel_l2(p, r))
        for k, vs in views.items():
            assert rel_l2(vs[i], opt.state[r][k]) <= 1e-6, (i, k, rel_l2(vs[i], opt.state[r][k]))
    arenas = [net._arena, net._sq_arena, net._mom_arena] + ([net._gavg_arena] if centered else [])
    pad = ~_real_mask(net, net._arena)
    assert pad.any()
    for a in arenas:
        assert not a[pad].any()


@pytest.mark.parametrize("arch,C,B,hw", [("resnet32", 100, 8, 32), ("resnet50", 1000, 8, 64)])
def test_fp32_loss_curve_against_oracle(arch, C, B, hw):
    """forward -> fused IIF loss -> backward -> ONE fused RMSprop launch, 4 steps at lr 1e-3, against the CPU oracle's
    gradients stepped by torch.optim.RMSprop with the reference's constants, given the same ReLU decisions
    (test_resnet_gpu.py: test_fp32_loss_curve_fused_step): loss within 1e-4, final weights within 5e-4.

    The loss is compared relative to the first step's loss, not to its own value: RMSprop's first steps move every weight
    by about lr / sqrt(1 - alpha) whatever its gradient, and on 8 images the ResNet-50's IIF loss falls to ~5e-4 after one
    step, where the fp32 rounding of two implementations (measured 3e-7 absolute, 6.6e-4 of that small value) is no longer
    1e-4 of the loss itself."""
    from iif_amd.custom import IIFLoss
    counts = [max(int(1000 * (5 / 1000) ** (i / (C - 1.0))), 1) for i in range(C)]
    net, sd = _build(arch, C, torch.float32)
    if arch not in R.CIFAR_ARCHS:
        net.load_state_dict(damp_residual_branches(sd, arch))
    x, y = _data(B, hw, counts, seed=9)
    table = O.iif_tables(counts)["raw"]
    crit = IIFLoss(DS(counts), variant="raw")
    ref_sd = {k: v.clone() for k, v in sd.items()}
    keys = R.trainable_keys(ref_sd)
    opt = torch.optim.RMSprop([ref_sd[k] for k in keys], lr=1e-3, alpha=ALPHA, eps=EPS, weight_decay=1e-4, momentum=0.9)
    xd, yd = x.to(DEV), y.to(DEV)
    net.train()
    scale = None
    for it in range(4):
        loss, _ = net.loss_and_backward(xd, yd, crit)
        masks = R.ReluMasks(gpu_relu_masks(net))
        net.rmsprop_step(1e-3, ALPHA, EPS, 1e-4, 0.9)
        ref_loss, _, grads = R.loss_and_grads(ref_sd, x, y, table, arch, relu_masks=masks)
        for k in keys:
            ref_sd[k].grad = grads[k]
        with torch.no_grad():
            opt.step()
        assert masks.disagree <= 1e-4 * masks.total and masks.worst <= 1e-4
        scale = abs(ref_loss.item()) if scale is None else scale
        assert abs(loss.item() - ref_loss.item()) <= 1e-4 * scale, (it, loss.item(), ref_loss.item(), scale)
    for k, v in net.state_dict().items():
        if v.is_floating_point():
            assert relerr(v, ref_sd[k]) <= 5e-4, (k, relerr(v, ref_sd[k]))


def test_head_only_leaves_backbone_and_its_state_alone():
    from iif_amd import resnet_cifar
    torch.manual_seed(1)
    net = resnet_cifar.resnet20(num_classes=10, use_norm="None", compute_dtype=torch.float32)
    net.train()
    net.select_training_param()
    counts, crit = _iif(10)
    x, y = _data(8, 32, counts, seed=2)
    x, y = x.to(DEV), y.to(DEV)
    head = net.block_offsets()["head"]
    body, tail = net._arena[:head].clone(), net._arena[head:].clone()
    for _ in range(3):
        net.loss_and_backward(x, y, crit)
        net.rmsprop_step(1e-3)
    torch.cuda.synchronize()
    assert torch.equal(net._arena[:head], body)
    assert not net._sq_arena[:head].any() and not net._mom_arena[:head].any()
    assert not torch.equal(net._arena[head:], tail) and net._sq_arena[head:].any()
    sd = net.rmsprop_state_dict(1e-3)
    n = len(list(net.parameters()))
    assert sorted(sd["state"]) == [n - 2, n - 1] and float(sd["state"][n - 1]["step"]) == 3


def test_mixing_sgd_and_rmsprop_on_one_engine_raises():
    from iif_amd import resnet_cifar
    counts, crit = _iif(10)
    x, y = _data(4, 32, counts, seed=3)
    x, y = x.to(DEV), y.to(DEV)
    for first, second in (("sgd", "rmsprop"), ("rmsprop", "sgd")):
        net = resnet_cifar.resnet20(num_classes=10, use_norm="None", compute_dtype=torch.float32)
        net.train()
        step = {"sgd": lambda: net.sgd_step(0.01), "rmsprop": lambda: net.rmsprop_step(1e-3)}
        net.loss_and_backward(x, y, crit)
        step[first]()
        net.loss_and_backward(x, y, crit)
        before = (net._arena.clone(), net._mom_arena.clone())
        with pytest.raises(RuntimeError, match="one optimizer"):
            step[second]()
        torch.cuda.synchronize()
        assert torch.equal(net._arena, before[0]) and torch.equal(net._mom_arena, before[1])


# ------------------------------------------------------------------------------------------------ the trainer
TRAIN = ["--model", "resnet20", "--dset_name", "cifar10", "--classif", "iif", "--iif", "raw", "-b", "16", "--max-iters", "4",
         "-j", "0", "--print-freq", "1", "--compute-dtype", "f32", "--lr", "0.001"]


def _run(cmd, env=None, ok=True):
    r = subprocess.run(cmd, env=env or dict(os.environ), capture_output=True, text=True, timeout=600, cwd=ROOT)
    if ok:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    return r


def _losses(stdout):
    import re
    return [float(v) for v in re.findall(r"loss: ([-+0-9.einfa]+)", stdout)]


def test_train_cli_rmsprop_checkpoint_and_resume(tmp_path):
    """``python -m iif_amd.train --opt rmsprop``: finite losses, a checkpoint whose optimizer entry loads into
    torch.optim.RMSprop as the reference builds it, ``--resume`` continuing from it (step counts carry on), and an SGD
    checkpoint refused under ``--opt rmsprop`` with the mismatch named."""
    out = tmp_path / "out"
    r = _run([sys.executable, "-m", "iif_amd.train", "--opt", "RMSprop", "--epochs", "1", "--output-dir", str(out)] + TRAIN)
    losses = _losses(r.stdout)
    assert len(losses) >= 3 and all(np.isfinite(losses)), r.stdout[-2000:]
    ckpt = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert ckpt["epoch"] == 0
    params = [torch.nn.Parameter(v.clone()) for k, v in ckpt["model"].items() if "running" not in k and "num_batches" not in k]
    opt = torch.optim.RMSprop(params, lr=0.001, momentum=0.9, weight_decay=1e-4, eps=0.0316, alpha=0.9)
    opt.load_state_dict(ckpt["optimizer"])
    assert len(opt.state) == len(params)
    for p in params:
        st = opt.state[p]
        assert float(st["step"]) == 4 and st["square_avg"].shape == p.shape and st["momentum_buffer"].shape == p.shape
        assert torch.isfinite(st["square_avg"]).all() and st["square_avg"].any()
    # resume: epoch 1 starts from the checkpoint's weights and RMSprop state
    out2 = tmp_path / "out2"
    _run([sys.executable, "-m", "iif_amd.train", "--opt", "rmsprop", "--epochs", "2", "--resume", str(out / "checkpoint.pth"),
          "--output-dir", str(out2)] + TRAIN)
    ck2 = torch.load(out2 / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert ck2["epoch"] == 1
    assert all(float(st["step"]) == 8 for st in ck2["optimizer"]["state"].values())
    # an SGD checkpoint under --opt rmsprop names the mismatch instead of failing later
    sgd = dict(ckpt)
    sgd_opt = torch.optim.SGD(params, lr=0.001, momentum=0.9)
    for p in params:
        p.grad = torch.zeros_like(p)
    sgd_opt.step()
    sgd["optimizer"] = sgd_opt.state_dict()
    torch.save(sgd, tmp_path / "sgd.pth")
    r = _run([sys.executable, "-m", "iif_amd.train", "--opt", "rmsprop", "--epochs", "2", "--resume", str(tmp_path / "sgd.pth")]
             + TRAIN, ok=False)
    assert r.returncode != 0 and "optimizer state mismatch" in r.stderr and "SGD state" in r.stderr, r.stderr[-2000:]


def _torchrun(port, *args):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2",
               IIF_REHEARSE_ONE_GPU="1", IIF_DDP_BACKEND="gloo")
    return _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                 "127.0.0.1", "--master-port", str(port), os.path.join(HERE, "rmsprop_ddp_worker.py")] + [str(a) for a in args],
                env=env)


def test_two_ranks_same_batch_equal_single_process_bit_for_bit(tmp_path):
    """The reducer sums two equal gradients and grad_scale 1/2 folds the average into the RMSprop launch: parameters,
    square_avg and momentum match the single-process run exactly (one-GPU rehearsal over gloo)."""
    sys.path.insert(0, HERE)
    import rmsprop_ddp_worker
    _torchrun(29571, "same", tmp_path, 4)
    ranks = [torch.load(tmp_path / ("rank%d.pt" % r), weights_only=False) for r in (0, 1)]
    rmsprop_ddp_worker.run(str(tmp_path / "single.pt"), 4, False)
    single = torch.load(tmp_path / "single.pt", weights_only=False)
    for got in ranks:
        for k in ("params", "sq", "mom"):
            assert torch.equal(got[k], single[k]), k
        assert got["losses"] == single["losses"]


@pytest.mark.parametrize("extra,port", [([], 29572), (["--bf16-buckets"], 29573)])
def test_train_cli_rmsprop_two_ranks(tmp_path, extra, port):
    """``iif_amd.train.main --opt rmsprop`` on two ranks (torch.distributed.run, gloo, both on GPU 0), with fp32 and with bf16
    gradient buckets: both ranks end with the same parameters and RMSprop state, and the checkpoint is finite."""
    out = tmp_path / "out"
    _torchrun(port, "cli", tmp_path, "--opt", "rmsprop", "--epochs", "1", "--output-dir", out, *(TRAIN + extra))
    r0, r1 = [torch.load(tmp_path / ("rank%d.pt" % r), weights_only=False) for r in (0, 1)]
    for k in ("params", "sq", "mom"):
        assert torch.equal(r0[k], r1[k]), k
    assert torch.isfinite(r0["params"]).all() and r0["sq"].any()
    ckpt = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert all(float(st["step"]) == 4 for st in ckpt["optimizer"]["state"].values())
