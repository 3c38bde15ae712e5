"""lss_clip_adam_guarded (optim.ClipAdam.step(max_norm, skipped=counter)): bit for bit lss_clip_adam while the
gradient norm is finite; a step with a +inf or a NaN gradient writes nothing -- parameters, both moments
and every step count keep their bits -- and advances the counter; the next finite step applies the bias
correction of step + 1. Eager and through one captured update graph. (Infinities and NaNs are ordinary
values of the arithmetic.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import optim  # noqa: E402

DEV = torch.device("cuda:0")
SIZES = [1, 1000, 4097]
MAX_NORM = 5.0


def _setup(seed):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g).to(DEV).requires_grad_(True) for n in SIZES]
    opt = torch.optim.Adam(ps, lr=1e-3, weight_decay=1e-7, fused=True, capturable=True)
    return ps, opt, g


def _grads(g, scale=3.0):
    return [torch.randn(n, generator=g).to(DEV) * scale for n in SIZES]


def _state(ps, opt):
    out = [p.detach().clone() for p in ps]
    for p in ps:
        out += [opt.state[p][k].detach().clone() for k in ("step", "exp_avg", "exp_avg_sq")]
    return out


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _sequence(seed):
    """finite, finite, +inf, NaN, finite, finite"""
    g = torch.Generator().manual_seed(seed)
    seq = [_grads(g) for _ in range(6)]
    seq[2][1][17] = float("inf")
    seq[3][2][4096] = float("nan")
    return seq, [False, False, True, True, False, False]


def _run(captured):
    ps_g, opt_g, _ = _setup(1)   # guarded
    ps_u, opt_u, _ = _setup(1)   # unguarded, fed the finite steps only
    skipped = torch.zeros(1, device=DEV, dtype=torch.int32)
    ca_g, ca_u = optim.ClipAdam(opt_g), optim.ClipAdam(opt_u)
    for p in ps_g + ps_u:
        p.grad = torch.zeros_like(p)
    if captured:
        # the optimizer state exists before the capture (as TrainStep's warm-up leaves it); what that
        # step moved is put back, in place
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            snap = [p.detach().clone() for p in ps_g]
            ca_g.step(MAX_NORM, skipped=skipped)
            for p, q in zip(ps_g, snap):
                p.data.copy_(q)
                for k in ("step", "exp_avg", "exp_avg_sq"):
                    opt_g.state[p][k].zero_()
        torch.cuda.current_stream().wait_stream(s)
        assert skipped.item() == 0
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ca_g.step(MAX_NORM, skipped=skipped)
        # the capture launched nothing
        assert skipped.item() == 0 and float(opt_g.state[ps_g[0]]["step"]) == 0.0
    seq, bad = _sequence(7)
    n_bad = 0
    for grads, is_bad in zip(seq, bad):
        for p, gr in zip(ps_g, grads):
            p.grad.copy_(gr)
        before = _state(ps_g, opt_g) if opt_g.state[ps_g[0]] else None
        if captured:
            graph.replay()
        else:
            ca_g.step(MAX_NORM, skipped=skipped)
        if is_bad:
            n_bad += 1
            assert _same(_state(ps_g, opt_g), before), "a skipped step wrote something"
        else:
            for p, gr in zip(ps_u, grads):
                p.grad.copy_(gr)
            ca_u.step(MAX_NORM)
            assert _same(_state(ps_g, opt_g), _state(ps_u, opt_u)), "a finite guarded step != lss_clip_adam"
        assert skipped.item() == n_bad
    # four finite steps were applied: the step after the two skipped ones used the bias correction of
    # step 3 (the unguarded twin, which never saw the bad steps, stayed bit-identical), not of step 5
    assert float(opt_g.state[ps_g[0]]["step"]) == 4.0 and skipped.item() == 2
    assert all(torch.isfinite(p).all() for p in ps_g)


def test_guarded_update_eager():
    _run(captured=False)


def test_guarded_update_through_one_captured_graph():
    _run(captured=True)


def test_unguarded_update_still_poisons():
    """Without the counter the update is lss_clip_adam: a NaN gradient poisons every parameter, as torch's."""
    ps, opt, g = _setup(3)
    grads = _grads(g)
    grads[1][5] = float("nan")
    for p, gr in zip(ps, grads):
        p.grad = gr
    optim.ClipAdam(opt).step(MAX_NORM)
    assert all(torch.isnan(p).all() for p in ps)
