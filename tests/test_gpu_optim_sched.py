"""lss_clip_adam_sched (optim.ClipAdam(opt, schedule=..., ema=...)): the learning rate computed on the device from
Adam's step count, and the EMA of the weights written by the same pass. A constant schedule is lss_clip_adam /
lss_clip_adam_guarded bit for bit; cosine and linear schedules against clip_grad_norm_ + torch's fused Adam whose
lr the test sets to LRSchedule.lr before each step (bars of tests/test_gpu_optim.py); a captured update follows the
schedule; the EMA against its float64 recurrence; a skipped step moves nothing; the ABI's refusals.
(The ragged sizes of tests/test_gpu_optim.py: tensors across 4-element boundaries of the concatenation and
across block ranges -- 75131 elements are 37 blocks of the Adam pass.)"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import _lib, optim  # noqa: E402
from lss_carla_amd.optim import LRSchedule  # noqa: E402

DEV = torch.device("cuda:0")
SIZES = [1, 3, 4, 1021, 4096, 70001, 5]
MAX_NORM = 5.0
BASE, WD = 1e-3, 1e-7
EINVAL = -1


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(DEV).requires_grad_(True) for n in SIZES], g


def _adam(ps):
    return torch.optim.Adam(ps, lr=BASE, weight_decay=WD, fused=True, capturable=True)


def _grads(g, scale=3.0):
    return [torch.randn(n, generator=g).to(DEV) * scale for n in SIZES]


def _set_grads(ps, grads):
    for p, gr in zip(ps, grads):
        if p.grad is None:
            p.grad = gr.clone()
        else:
            p.grad.copy_(gr)


def _state(ps, opt, extra=()):
    out = [p.detach().clone() for p in ps]
    for p in ps:
        out += [opt.state[p][k].detach().clone() for k in ("step", "exp_avg", "exp_avg_sq")]
    return out + [t.detach().clone() for t in extra]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _cosine():
    return LRSchedule("cosine", warmup_steps=3, warmup_factor=0.1, total_steps=10, min_factor=0.01)


@pytest.mark.parametrize("guarded", [False, True])
def test_constant_schedule_is_the_plain_update_bit_for_bit(guarded):
    ps_a, g = _params(1)
    ps_b = [p.detach().clone().requires_grad_(True) for p in ps_a]
    opt_a, opt_b = _adam(ps_a), _adam(ps_b)
    ca, cb = optim.ClipAdam(opt_a, schedule=LRSchedule()), optim.ClipAdam(opt_b)
    sk_a = torch.zeros(1, device=DEV, dtype=torch.int32) if guarded else None
    sk_b = torch.zeros(1, device=DEV, dtype=torch.int32) if guarded else None
    for scale in (10.0, 1e-3, 1.0, 3.0):  # clipped and unclipped steps
        grads = _grads(g, scale)
        _set_grads(ps_a, grads)
        _set_grads(ps_b, grads)
        ca.step(MAX_NORM, skipped=sk_a)
        cb.step(MAX_NORM, skipped=sk_b)
        assert _same(_state(ps_a, opt_a), _state(ps_b, opt_b))
    assert float(opt_a.state[ps_a[0]]["step"]) == 4.0
    assert ca.lr.item() == torch.tensor(BASE, dtype=torch.float32).item() and cb.lr is None
    if guarded:
        assert sk_a.item() == sk_b.item() == 0


@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_schedule_matches_torch_adam_with_the_host_lr(kind):
    """Warm-up (W = 3), decay and the plateau past T = 10, 12 steps."""
    sched = LRSchedule(kind, warmup_steps=3, warmup_factor=0.1, total_steps=10, min_factor=0.01)
    ps_a, g = _params(2)
    ps_b = [p.detach().clone().requires_grad_(True) for p in ps_a]
    opt_a, opt_b = _adam(ps_a), _adam(ps_b)
    ca = optim.ClipAdam(opt_a, schedule=sched)
    rel = []
    for t in range(1, 13):
        grads = _grads(g, 10.0 if t % 2 else 0.5)
        _set_grads(ps_a, grads)
        _set_grads(ps_b, grads)
        assert optim.supported(opt_a, ps_a)
        ca.step(MAX_NORM)
        opt_b.param_groups[0]["lr"] = sched.lr(BASE, t)
        torch.nn.utils.clip_grad_norm_(ps_b, MAX_NORM)
        opt_b.step()
        for p, q in zip(ps_a, ps_b):
            torch.testing.assert_close(p.detach(), q.detach(), rtol=2e-5, atol=2e-7)
        want = sched.lr(BASE, t)
        rel.append(abs(float(ca.lr.item()) - want) / want)
    print(f"{kind}: lr relative error per step {['%.1e' % r for r in rel]}")
    assert max(rel) <= 1e-6, rel
    assert opt_a.param_groups[0]["lr"] == BASE  # the base rate is not touched
    for p, q in zip(ps_a, ps_b):
        sa, sb = opt_a.state[p], opt_b.state[q]
        assert float(sa["step"]) == float(sb["step"]) == 12.0
        torch.testing.assert_close(sa["exp_avg"], sb["exp_avg"], rtol=1e-5, atol=1e-8)
        torch.testing.assert_close(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=1e-5, atol=1e-10)


def test_captured_update_follows_the_schedule():
    """One eager step, the capture, 11 replays: the rate read after each replay is the schedule's (a rate baked in
    at capture would stay at step 2's), and parameters and moments are those of 12 eager steps, bit for bit."""
    sched = _cosine()
    ps_g, g = _params(3)
    ps_e = [p.detach().clone().requires_grad_(True) for p in ps_g]
    opt_g, opt_e = _adam(ps_g), _adam(ps_e)
    cg, ce = optim.ClipAdam(opt_g, schedule=sched), optim.ClipAdam(opt_e, schedule=sched)
    seq = [_grads(g) for _ in range(12)]
    for grads in seq:
        _set_grads(ps_e, grads)
        ce.step(MAX_NORM)
    _set_grads(ps_g, seq[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cg.step(MAX_NORM)  # the eager step: the state exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cg.step(MAX_NORM)
    assert float(opt_g.state[ps_g[0]]["step"]) == 1.0  # the capture launched nothing
    lrs = [float(cg.lr.item())]
    for grads in seq[1:]:
        _set_grads(ps_g, grads)
        graph.replay()
        lrs.append(float(cg.lr.item()))
    want = [sched.lr(BASE, t) for t in range(1, 13)]
    assert len(set(lrs)) >= 10
    for got, w in zip(lrs, want):
        assert abs(got - w) <= 1e-6 * w, (lrs, want)
    assert _same(_state(ps_g, opt_g, [cg.lr]), _state(ps_e, opt_e, [ce.lr]))


def _ema_run(ema_warmup, misaligned, steps=8, decay=0.9):
    """Returns (per-step EMA lists, per-step parameter lists, initial EMA list)."""
    ps, g = _params(4)
    opt = _adam(ps)
    emas = []
    for k, p in enumerate(ps):
        if misaligned and k == 3:  # 1021 elements from element 8 of the concatenation: the vector path's tensor
            base = torch.zeros(p.numel() + 1, device=DEV)
            e = base[1:]
            assert e.data_ptr() % 16 == 4 and e.is_contiguous()
            e.copy_(p.detach())
        else:
            e = p.detach().clone()
            assert e.data_ptr() % 16 == 0
        emas.append(e)
    init = [e.clone() for e in emas]
    ca = optim.ClipAdam(opt, ema=emas, ema_decay=decay, ema_warmup=ema_warmup)
    hist_e, hist_p = [], []
    for _ in range(steps):
        _set_grads(ps, _grads(g))
        ca.step(MAX_NORM)
        hist_e.append([e.clone() for e in emas])
        hist_p.append([p.detach().clone() for p in ps])
    return hist_e, hist_p, init


@pytest.mark.parametrize("ema_warmup", [True, False])
def test_ema_follows_its_recurrence(ema_warmup):
    """e_t = e_{t-1} + (1 - d_t)(p_t - e_{t-1}) in float64 from the kernel's own parameters: rtol 2e-6, atol 1e-7
    (8 steps x at most 2 ulp per fmaf step, with room). A 4-B aligned EMA tensor (the scalar loop) gives the bits
    of an aligned one (the float4 loop)."""
    hist_e, hist_p, init = _ema_run(ema_warmup, misaligned=False)
    want = [e.double() for e in init]
    worst = 0.0
    for t, (es, ps) in enumerate(zip(hist_e, hist_p), start=1):
        d = min(0.9, (1.0 + t) / (10.0 + t)) if ema_warmup else 0.9
        want = [w + (1.0 - d) * (p.double() - w) for w, p in zip(want, ps)]
        for e, w in zip(es, want):
            worst = max(worst, float(((e.double() - w).abs() / (1e-7 + 2e-6 * w.abs())).max()))
            torch.testing.assert_close(e.double(), w, rtol=2e-6, atol=1e-7)
    print(f"ema_warmup={ema_warmup}: worst error / bar {worst:.3f}")
    assert all(not torch.equal(e, p) for e, p in zip(hist_e[-1], hist_p[-1]))
    # without the EMA the parameters are the same: the arm changes nothing else
    ps, g = _params(4)
    opt = _adam(ps)
    ca = optim.ClipAdam(opt)
    for _ in range(8):
        _set_grads(ps, _grads(g))
        ca.step(MAX_NORM)
    assert _same([p.detach() for p in ps], hist_p[-1])
    mis_e, mis_p, _ = _ema_run(ema_warmup, misaligned=True)
    for a, b in zip(mis_e, hist_e):
        assert _same(a, b)
    assert _same(mis_p[-1], hist_p[-1])


def test_guarded_skip_moves_nothing():
    """A NaN gradient entry at step 3 of 5, schedule and EMA on: everything keeps its bits, the skip is counted,
    and step 4 runs at the schedule's value for the unadvanced count (t = 3)."""
    sched = _cosine()
    ps, g = _params(5)
    opt = _adam(ps)
    emas = [p.detach().clone() for p in ps]
    skipped = torch.zeros(1, device=DEV, dtype=torch.int32)
    ca = optim.ClipAdam(opt, schedule=sched, ema=emas, ema_decay=0.9)
    lrs = []
    for it in range(1, 6):
        grads = _grads(g)
        if it == 3:
            grads[5][4097] = float("nan")
        _set_grads(ps, grads)
        before = _state(ps, opt, emas + [ca.lr]) if it > 1 else None
        ca.step(MAX_NORM, skipped=skipped)
        after = _state(ps, opt, emas + [ca.lr])
        if it == 3:
            assert _same(after, before), "a skipped step wrote something"
            assert skipped.item() == 1
        elif it > 1:
            assert not _same(after[:1], before[:1])
        lrs.append(float(ca.lr.item()))
    assert skipped.item() == 1 and float(opt.state[ps[0]]["step"]) == 4.0
    want = [sched.lr(BASE, t) for t in (1, 2, 2, 3, 4)]
    for got, w in zip(lrs, want):
        assert abs(got - w) <= 1e-6 * w, (lrs, want)
    assert all(torch.isfinite(t).all() for t in ps + emas)


def _raw_call(bufs, **over):
    """lss_clip_adam_sched on the raw ABI over `bufs` (dict of lists of tensors), arguments overridden by name."""
    lib = _lib.load()
    n = len(SIZES)
    arr = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    a = dict(kind=2, warmup_steps=3, warmup_factor=0.1, total_steps=10, min_factor=0.01, ema=bufs["ema"],
             ema_decay=0.9, skipped=bufs["skipped"])
    a.update(over)
    return lib.lss_clip_adam_sched(
        n, arr(bufs["p"]), arr(bufs["g"]), arr(bufs["m"]), arr(bufs["v"]), arr(bufs["step"]),
        (ctypes.c_int64 * n)(*SIZES), MAX_NORM, BASE, 0.9, 0.999, 1e-8, WD, _lib.ptr(bufs["partial"]),
        _lib.ptr(a["skipped"]), a["kind"], a["warmup_steps"], a["warmup_factor"], a["total_steps"], a["min_factor"],
        _lib.ptr(bufs["lr"]), None if a["ema"] is None else arr(a["ema"]), a["ema_decay"], 1,
        _lib.stream_handle(DEV))


def test_refusals_launch_nothing():
    nan = float("nan")
    mk = lambda: [torch.full((n,), nan, device=DEV) for n in SIZES]  # noqa: E731
    bufs = {"p": mk(), "g": mk(), "m": mk(), "v": mk(), "ema": mk(),
            "step": [torch.full((), nan, device=DEV) for _ in SIZES],
            "partial": torch.full((int(_lib.load().lss_clip_adam_partials()),), nan, device=DEV),
            "lr": torch.full((), nan, device=DEV), "skipped": torch.full((1,), -7, device=DEV, dtype=torch.int32)}
    ema = bufs["ema"]
    swap = lambda k, t: ema[:k] + [t] + ema[k + 1:]  # noqa: E731
    cases = [
        dict(kind=-1), dict(kind=3), dict(warmup_steps=-1), dict(warmup_factor=-0.01), dict(warmup_factor=1.01),
        dict(warmup_factor=nan), dict(min_factor=-0.01), dict(min_factor=1.01), dict(min_factor=nan),
        dict(kind=1, total_steps=3), dict(kind=2, total_steps=2), dict(ema_decay=1.0), dict(ema_decay=-0.1),
        dict(ema_decay=nan), dict(ema=swap(2, None)), dict(ema=swap(4, bufs["p"][4])), dict(ema=swap(4, bufs["p"][1])),
        dict(ema=swap(0, bufs["m"][3])), dict(ema=swap(6, bufs["v"][0])), dict(ema=swap(5, ema[1])),
    ]
    for skipped in (bufs["skipped"], None):
        for c in cases:
            assert _raw_call(bufs, skipped=skipped, **c) == EINVAL, c
    torch.cuda.synchronize()
    for k in ("p", "g", "m", "v", "ema", "step"):
        assert all(torch.isnan(t).all() for t in bufs[k]), k
    assert torch.isnan(bufs["partial"]).all() and torch.isnan(bufs["lr"]).all() and bufs["skipped"].item() == -7
    # Python's own refusals
    ps, _ = _params(6)
    opt = _adam(ps)
    with pytest.raises(ValueError):
        optim.ClipAdam(opt, ema=[p.detach().clone() for p in ps], ema_decay=1.0)
    with pytest.raises(ValueError):
        optim.ClipAdam(opt, ema=[p.detach().clone() for p in ps][:-1])
    with pytest.raises(TypeError):
        optim.ClipAdam(opt, schedule="cosine")


def test_train_step_with_a_schedule_needs_the_hip_update():
    from lss_carla_amd.train_step import TrainStep
    net = torch.nn.Linear(5, 1).to(DEV)
    params = list(net.parameters())
    x, y = torch.randn(4, 5, device=DEV), torch.randn(4, 1, device=DEV)
    opt = torch.optim.Adam(params, lr=1e-3)  # foreach: `step` on the host, optim.supported is false
    step = TrainStep(net, (x,), y, torch.nn.functional.mse_loss, opt, params, amp_dtype=None, lr_schedule=_cosine())
    with pytest.raises(RuntimeError, match="needs the HIP update"):
        step()
    ema = [p.detach().clone() for p in params]
    step = TrainStep(net, (x,), y, torch.nn.functional.mse_loss, opt, params, amp_dtype=None, ema=ema)
    with pytest.raises(RuntimeError, match="needs the HIP update"):
        step()
    assert TrainStep(net, (x,), y, torch.nn.functional.mse_loss, opt, params, amp_dtype=None).lr is None
