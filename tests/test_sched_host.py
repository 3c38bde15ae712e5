"""The host side of the learning-rate schedule and the EMA weights (no GPU): optim.LRSchedule's formula and
refusals, the trainer's argument errors, and the ``ema_state_dict`` key of the checkpoint."""
import math

import pytest
import torch
from torch import nn

import lss_carla_amd as L
from lss_carla_amd import checkpoint, optim, predict, trainer
from lss_carla_amd.flat_params import FlatParams

W, T, WF, M = 3, 10, 0.1, 0.01
KINDS = ("constant", "linear", "cosine")


def _sched(kind):
    return optim.LRSchedule(kind, warmup_steps=W, warmup_factor=WF, total_steps=T, min_factor=M)


@pytest.mark.parametrize("kind", KINDS)
def test_factor_at_the_corners(kind):
    """s = t - 1: the warm-up starts at warmup_factor, reaches 1 at s = W where the decay starts, and the decay
    reaches min_factor at s = T and stays there."""
    sc = _sched(kind)
    assert L.LRSchedule is optim.LRSchedule
    assert sc.factor(1) == pytest.approx(WF, rel=1e-15)                       # s = 0
    assert sc.factor(W + 1) == pytest.approx(1.0, rel=1e-15)                  # s = W
    end = 1.0 if kind == "constant" else M
    assert sc.factor(T + 1) == pytest.approx(end, rel=1e-12)                  # s = T
    assert sc.factor(T + 2) == sc.factor(T + 50) == pytest.approx(end, rel=1e-12)  # past T
    assert sc.lr(2e-3, 2) == 2e-3 * sc.factor(2)
    # mid-points by hand
    assert sc.factor(2) == pytest.approx(WF + (1 - WF) / W, rel=1e-15)        # s = 1 of the warm-up
    x = (6 - W) / (T - W)                                                     # s = 6
    want = {"constant": 1.0, "linear": M + (1 - M) * (1 - x), "cosine": M + (1 - M) * 0.5 * (1 + math.cos(math.pi * x))}
    assert sc.factor(7) == pytest.approx(want[kind], rel=1e-15)


@pytest.mark.parametrize("kind", KINDS)
def test_factor_rises_over_the_warmup_and_falls_after_it(kind):
    sc = _sched(kind)
    f = [sc.factor(t) for t in range(1, T + 6)]
    assert all(a < b for a, b in zip(f[:W], f[1:W + 1]))  # s = 0 .. W: strictly rising
    tail = f[W:]
    if kind == "constant":
        assert all(v == 1.0 for v in tail)
    else:
        assert all(a > b for a, b in zip(tail[:T - W], tail[1:T - W + 1]))  # s = W .. T: strictly falling
        assert all(a >= b for a, b in zip(tail, tail[1:]))
    assert all(0.0 <= v <= 1.0 for v in f)


def test_no_warmup_and_defaults():
    sc = optim.LRSchedule()
    assert [sc.factor(t) for t in (1, 2, 1000)] == [1.0, 1.0, 1.0] and sc.code == 0
    lin = optim.LRSchedule("linear", total_steps=4)
    assert [lin.factor(t) for t in range(1, 7)] == [1.0, 0.75, 0.5, 0.25, 0.0, 0.0] and lin.code == 1
    assert optim.LRSchedule("cosine", total_steps=4).code == 2


@pytest.mark.parametrize("kw", [
    dict(kind="step"), dict(kind=1), dict(warmup_steps=-1), dict(warmup_factor=-0.1), dict(warmup_factor=1.5),
    dict(warmup_factor=float("nan")), dict(min_factor=-0.01), dict(min_factor=1.01), dict(min_factor=float("nan")),
    dict(kind="linear", warmup_steps=5, total_steps=5), dict(kind="cosine", warmup_steps=5, total_steps=4),
    dict(kind="cosine"), dict(warmup_steps=1.5),
])
def test_constructor_refuses_what_the_abi_refuses(kw):
    with pytest.raises(ValueError):
        optim.LRSchedule(**kw)


def test_abi_refuses_on_the_host_before_any_device_call():
    """lss_clip_adam_sched checks its arguments before any HIP call: made-up addresses that are never dereferenced
    exercise the refusals without a GPU (tests/test_gpu_optim_sched.py repeats them over real buffers)."""
    import ctypes

    from lss_carla_amd import _lib
    lib = _lib.load()
    n = 2
    arr = lambda *a: (ctypes.c_void_p * n)(*a)  # noqa: E731
    p, g, m, v, st, e = (arr(b, b + 0x1000) for b in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000))
    numel = (ctypes.c_int64 * n)(8, 8)

    def call(kind=2, W=3, wf=0.1, T=10, mf=0.01, ema=e, d=0.9):
        return lib.lss_clip_adam_sched(n, p, g, m, v, st, numel, 5.0, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                                       ctypes.c_void_p(0x70000), None, kind, W, wf, T, mf, None, ema, d, 1, None)

    bad = [call(kind=-1), call(kind=3), call(W=-1), call(wf=-0.5), call(wf=1.5), call(mf=-0.5), call(mf=1.5),
           call(kind=1, T=3), call(kind=2, T=2), call(d=1.0), call(d=-0.5), call(ema=arr(0x60000, None)),
           call(ema=arr(0x60000, 0x60000)), call(ema=arr(0x10000, 0x61000)), call(ema=arr(0x60000, 0x30000)),
           call(ema=arr(0x41000, 0x61000))]
    assert bad == [-1] * len(bad), bad


def test_constant_schedule_needs_no_total():
    optim.LRSchedule("constant", warmup_steps=5, total_steps=0)  # kind 0: total_steps is not looked at


@pytest.mark.parametrize("kw", [
    dict(lr_schedule="cosine", warmup_steps=-1), dict(lr_schedule="step"), dict(warmup_factor=2.0),
    dict(lr_schedule="linear", warmup_steps=4, lr_total_steps=4), dict(lr_min=1.0), dict(lr_min=-1e-6),
    dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(lr_schedule="linear", lr_total_steps=0),
])
def test_trainer_argument_errors_come_before_anything_is_built(kw, tmp_path):
    """ValueError on a machine without a GPU, from a data root that does not exist: nothing was looked for."""
    with pytest.raises(ValueError):
        trainer.train(str(tmp_path / "no_such_tree"), logdir=str(tmp_path / "log"), use_wandb=False, **kw)
    assert not (tmp_path / "log").exists()


class _Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 3)
        self.bn = nn.BatchNorm2d(4)
        self.fc = nn.Linear(4, 2)
        self.const = nn.Parameter(torch.arange(3.0), requires_grad=False)


def _setup(seed, ema):
    torch.manual_seed(seed)
    model = _Small()
    flat = FlatParams(model)
    if ema:
        flat.enable_ema()
    opt = torch.optim.Adam([flat.master], lr=1e-3)
    return model, flat, opt


def _train_a_little(model, flat, opt):
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        flat.master.grad = torch.randn(flat.master.shape, generator=g)
        opt.step()
        if flat.ema is not None:
            with torch.no_grad():
                flat.ema.lerp_(flat.master.detach(), 0.25)
    with torch.no_grad():
        model.bn.running_mean.add_(0.5)


def test_checkpoint_without_ema_has_todays_keys(tmp_path):
    model, flat, opt = _setup(0, ema=False)
    _train_a_little(model, flat, opt)
    path = tmp_path / "plain.pt"
    checkpoint.save_checkpoint(path, model, flat, opt, counter=2, epoch=0)
    assert set(torch.load(path, map_location="cpu")) == {"model_state_dict", "optimizer_state_dict", "counter", "epoch"}
    assert checkpoint.load_checkpoint(path, model, flat, opt) == (2, 0)
    with pytest.raises(RuntimeError):
        flat.tensors(source="ema")
    with pytest.raises(ValueError):
        flat.tensors(source="average")


def test_checkpoint_with_ema_gains_one_key_and_round_trips(tmp_path, capsys):
    model, flat, opt = _setup(0, ema=True)
    assert torch.equal(flat.ema, flat.master.detach()) and flat.ema.data_ptr() != flat.master.data_ptr()
    assert flat.enable_ema() is flat.ema  # idempotent: the address is fixed
    _train_a_little(model, flat, opt)
    assert not torch.equal(flat.ema, flat.master.detach())
    path = tmp_path / "ema.pt"
    checkpoint.save_checkpoint(path, model, flat, opt, counter=2, epoch=0)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "counter", "epoch", "ema_state_dict"}
    esd, msd = ck["ema_state_dict"], ck["model_state_dict"]
    assert list(esd) == list(msd)
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    views = flat.views_of(flat.ema)
    assert set(views) == trainable
    for k in msd:
        if k in trainable:
            assert torch.equal(esd[k], views[k]) and not torch.equal(esd[k], msd[k]), k
        else:
            assert torch.equal(esd[k], msd[k]), k  # constants and batch-norm statistics: the live ones
    _Small().load_state_dict(esd)  # a plain module loads it as it is
    assert predict.model_state_dict(ck, "auto") is esd and predict.model_state_dict(ck, "ema") is esd
    assert predict.model_state_dict(ck, "model") is msd and predict.model_state_dict(ck) is msd
    with pytest.raises(ValueError):
        predict.model_state_dict(ck, "best")

    # into a fresh setup, in place, bit for bit
    model2, flat2, opt2 = _setup(1, ema=True)
    ptr = flat2.ema.data_ptr()
    assert checkpoint.load_checkpoint(path, model2, flat2, opt2) == (2, 0)
    assert flat2.ema.data_ptr() == ptr and torch.equal(flat2.ema, flat.ema)
    assert torch.equal(flat2.master.detach(), flat.master.detach())
    assert "ema_state_dict" not in capsys.readouterr().out

    # a file without the key: the EMA starts from the loaded weights, and the loader says so
    model3, flat3, opt3 = _setup(0, ema=False)
    _train_a_little(model3, flat3, opt3)
    plain = tmp_path / "plain.pt"
    checkpoint.save_checkpoint(plain, model3, flat3, opt3, counter=2, epoch=0)
    checkpoint.load_checkpoint(plain, model2, flat2, opt2)
    assert flat2.ema.data_ptr() == ptr and torch.equal(flat2.ema, flat3.master.detach())
    assert "no ema_state_dict" in capsys.readouterr().out
    with pytest.raises(ValueError):
        predict.model_state_dict(torch.load(plain, map_location="cpu"), "ema")
    assert predict.model_state_dict(torch.load(plain, map_location="cpu"), "auto").keys() == msd.keys()
