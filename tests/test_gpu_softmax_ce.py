"""lss_softmax_ce (tools.SoftmaxLoss) on the MI355X: the exclusive-class loss and its gradient, both arms.

Shapes (exclusive_cases.SHAPES): (2, 3, 5, 5) and (1, 2, 1, 9) take the scalar arm, (4, 8, 16, 16), (3, 5, 1, 2056)
-- a sample spanning two blocks -- and (2, 4, 1, 8) -- one thread per sample -- the vector arm; fp32 and bf16 each.
Reference: exclusive_cases.closed_form in float64 on the logits the kernel sees. Bars, as tests/test_gpu_focal_loss.py
holds its kernel to: loss rtol 2e-6 / atol 1e-7; fp32 gradient rtol max(1e-5, 4 r32), r32 the error of the same
formula in float32 on the host, atol 1e-12; bf16 gradient after the backward 8e-3 (two bf16 roundings). Each case
prints its measured errors."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import exclusive_cases as E  # noqa: E402
from lss_carla_amd import _lib, tools as T  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16]
SCALE = 0.75  # the incoming gradient of the loss


def _module(C):
    return T.SoftmaxLoss(C, E.weights(C).tolist()).to(DEV)


def _run(fn, x, labels, valid=None):
    xd = x.to(DEV).requires_grad_(True)
    ld = labels.to(DEV)
    loss = fn(xd, ld) if valid is None else fn(xd, ld, valid.to(DEV))
    loss.backward(torch.tensor(SCALE, device=DEV))
    return loss.detach(), xd.grad


@pytest.fixture
def launched(monkeypatch):
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (calls.append(what), real(code, what))[1])
    return calls


def test_the_shapes_reach_both_arms():
    arms = {}
    for shape in E.SHAPES:
        for dtype in DTYPES:
            x, labels = E.data(shape, dtype)
            arms[(shape, dtype)] = T.softmax_ce_arm(x.to(DEV), labels.to(DEV), E.mask(shape).to(DEV))
            assert arms[(shape, dtype)] == (1 if shape in E.VECTOR else 0), (shape, dtype)
    assert set(arms.values()) == {0, 1}


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", E.SHAPES)
def test_loss_and_gradient_vs_fp64_closed_form(shape, dtype, masked, launched):
    C = shape[1]
    x, labels = E.data(shape, dtype, seed=1)
    valid = E.mask(shape, seed=1) if masked else None
    fn = _module(C)
    loss, grad = _run(fn, x, labels, valid)
    assert launched == ["lss_softmax_ce", "lss_seg_loss_masked_bwd"]
    assert grad.dtype == dtype and loss.dtype == torch.float32 and loss.shape == ()
    w = E.weights(C)
    want, wgrad = E.closed_form(x.double(), labels, valid, w)
    wgrad = SCALE * wgrad
    tol = 8e-3 if dtype == torch.bfloat16 else max(1e-5, 4 * E.formula_rounding(x, labels, valid, w))
    print(f"{shape} {dtype} masked={masked}: loss {loss.item():.9e} fp64 {want.item():.9e} rel "
          f"{abs(loss.item() - want.item()) / abs(want.item()):.2e}; grad rel err "
          f"{E.rel_err(grad.cpu().double(), wgrad):.2e} (bar {tol:.2e})")
    torch.testing.assert_close(loss.cpu().double(), want, rtol=E.LOSS_RTOL, atol=E.LOSS_ATOL)
    torch.testing.assert_close(grad.cpu().double(), wgrad, rtol=tol, atol=1e-12)
    off = ~E.counted(labels, valid, C).unsqueeze(1).expand(shape)
    assert off.any() and (grad.cpu()[off] == 0).all() and (grad.cpu()[~off] != 0).any()
    loss2, grad2 = _run(fn, x, labels, valid)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)  # two runs: equal bits
    # torch's own loss, on the fp32 cast of the logits (labels in C..254 mapped to its ignore_index)
    lab = torch.where(E.counted(labels, valid, C), labels, torch.full_like(labels, 255)).long()
    ce = torch.nn.functional.cross_entropy(x.double(), lab, weight=w.double(), ignore_index=255)
    torch.testing.assert_close(want, ce, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", E.SHAPES)
def test_no_mask_gives_the_bits_of_an_all_ones_mask(shape, dtype):
    x, labels = E.data(shape, dtype, seed=2)
    fn = _module(shape[1])
    ln, gn = _run(fn, x, labels)
    lo, go = _run(fn, x, labels, torch.ones(shape[0], *shape[2:], dtype=torch.uint8))
    assert torch.equal(ln, lo) and torch.equal(gn, go)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", E.SHAPES)
def test_non_finite_logits_under_cells_that_do_not_count(shape, dtype):
    C = shape[1]
    x, labels = E.data(shape, dtype, seed=3)
    valid = E.mask(shape, seed=3)
    fn = _module(C)
    la, ga = _run(fn, x, labels, valid)
    off = ~E.counted(labels, valid, C).unsqueeze(1).expand(shape)
    bad = x.clone()
    k = int(off.sum())
    bad[off] = torch.tensor([float("nan"), float("inf"), -float("inf")]).repeat(k // 3 + 1)[:k].to(dtype)
    lb, gb = _run(fn, bad, labels, valid)
    assert torch.isfinite(lb) and torch.equal(la, lb) and torch.equal(ga, gb) and (gb.cpu()[off] == 0).all()
    # ignored labels alone select a cell out, without a mask
    off2 = ~E.counted(labels, None, C).unsqueeze(1).expand(shape)
    bad2 = x.clone()
    bad2[off2] = float("nan")
    l1, g1 = _run(fn, x, labels)
    l2, g2 = _run(fn, bad2, labels)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 5), (4, 8, 16, 16)])
def test_zero_total_weight(shape, dtype):
    C = shape[1]
    x, labels = E.data(shape, dtype, seed=4)
    fn = _module(C)
    zero = torch.zeros(shape[0], *shape[2:], dtype=torch.uint8)
    lz, gz = _run(fn, x, labels, zero)  # no cell counts
    assert lz.item() == 0.0 and (gz == 0).all()
    ln, gn = _run(fn, torch.full(shape, float("nan"), dtype=dtype), labels, zero)
    assert ln.item() == 0.0 and (gn == 0).all()
    li, gi = _run(fn, x, torch.full_like(labels, 255))  # every label ignored
    assert li.item() == 0.0 and (gi == 0).all()
    fn.class_weight.zero_()  # every counted cell has weight 0
    lw, gw = _run(fn, x, labels)
    assert lw.item() == 0.0 and (gw == 0).all()


@pytest.mark.parametrize("shape", [(2, 4, 1, 16)])
def test_the_arms_compute_the_same_cells(shape):
    """The scalar arm (the same logits at a 4-byte offset) writes the vector arm's gradient bit for bit: one
    arithmetic per cell; the losses differ only by the order of the fold."""
    lib = _lib.load()
    B, C, H, W = shape
    plane = H * W
    x, labels = E.data(shape, torch.float32, seed=5)
    w = E.weights(C).to(DEV)
    buf = torch.zeros(x.numel() + 4, device=DEV)
    xa, xm = buf[:x.numel()], buf[1:1 + x.numel()]
    ld = labels.to(DEV)
    out = []
    for xt in (xa, xm):
        xt.copy_(x.reshape(-1))
        grad = torch.empty(x.numel(), device=DEV)
        part = torch.zeros(int(lib.lss_softmax_ce_partials(B * plane)), device=DEV)
        loss, scale = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        arm = lib.lss_softmax_ce_arm(_lib.ptr(xt), _lib.F32, _lib.ptr(ld), None, B, plane, C, _lib.ptr(grad))
        assert lib.lss_softmax_ce(_lib.ptr(xt), _lib.F32, _lib.ptr(ld), None, B, plane, C, _lib.ptr(w), _lib.ptr(part),
                                  _lib.ptr(loss), _lib.ptr(scale), _lib.ptr(grad), _lib.stream_handle(DEV)) == 0
        torch.cuda.synchronize()
        out.append((arm, loss.clone(), scale.clone(), grad.clone()))
    assert [o[0] for o in out] == [1, 0]
    assert torch.equal(out[0][3], out[1][3])
    torch.testing.assert_close(out[0][1], out[1][1], rtol=E.LOSS_RTOL, atol=E.LOSS_ATOL)
    torch.testing.assert_close(out[0][2], out[1][2], rtol=E.LOSS_RTOL, atol=0)


def test_replay_follows_weight_mask_and_labels():
    shape = (4, 8, 16, 16)
    C = shape[1]
    x, labels = E.data(shape, torch.bfloat16, seed=6)
    _, labels2 = E.data(shape, torch.bfloat16, seed=7)
    m1, m2 = E.mask(shape, seed=6), E.mask(shape, seed=7, p=0.3)
    w2 = torch.tensor([1.0, 0.5, 2.0, 0.0, 1.0, 4.0, 0.25, 1.5])
    fn = _module(C)
    a, ga = _run(fn, x, labels, m1)
    b, gb = _run(fn, x, labels, m2)
    c, gc = _run(fn, x, labels2, m2)
    fn2 = T.SoftmaxLoss(C, w2.tolist()).to(DEV)
    d, gd = _run(fn2, x, labels2, m2)
    assert len({a.item(), b.item(), c.item(), d.item()}) == 4
    xd, ld, vd = x.to(DEV).requires_grad_(True), labels.to(DEV).clone(), m1.to(DEV).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.autograd.grad(fn(xd, ld, vd), xd)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = fn(xd, ld, vd)
        (grad,) = torch.autograd.grad(loss, xd, torch.full((), SCALE, device=DEV))
    graph.replay()
    assert torch.equal(loss, a) and torch.equal(grad, ga)
    vd.copy_(m2.to(DEV))  # in place: the replay reads the same addresses
    graph.replay()
    assert torch.equal(loss, b) and torch.equal(grad, gb)
    ld.copy_(labels2.to(DEV))
    graph.replay()
    assert torch.equal(loss, c) and torch.equal(grad, gc)
    fn.class_weight.copy_(w2.to(DEV))
    graph.replay()
    assert torch.equal(loss, d) and torch.equal(grad, gd)


def test_strided_logits_or_other_label_types_take_the_torch_path(launched):
    shape = (2, 3, 5, 5)
    C = shape[1]
    x, labels = E.data(shape, torch.float32, seed=8)
    valid = E.mask(shape, seed=8)
    fn = _module(C)
    xs = x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)  # NHWC strides
    assert not xs.is_contiguous()
    got = fn(xs, labels.to(DEV), valid.to(DEV))
    (g,) = torch.autograd.grad(got, xs)
    got_b = fn(x.to(DEV), labels.to(DEV), valid.to(DEV).bool())  # a boolean mask: same values, the torch path
    assert not launched
    w = E.weights(C)
    want, wgrad = E.closed_form(x.double(), labels, valid, w)
    torch.testing.assert_close(got.detach().cpu().double(), want, rtol=E.LOSS_RTOL, atol=E.LOSS_ATOL)
    torch.testing.assert_close(got_b.cpu().double(), want, rtol=E.LOSS_RTOL, atol=E.LOSS_ATOL)
    tol = max(1e-5, 4 * E.formula_rounding(x, labels, valid, w))
    torch.testing.assert_close(g.cpu().double(), wgrad, rtol=tol, atol=1e-12)
    for bad in (lambda: fn(x.to(DEV), labels.to(DEV).long()), lambda: fn(x.to(DEV), labels.to(DEV)[:1]),
                lambda: fn(x.to(DEV)[:, :2], labels.to(DEV)), lambda: fn(x.to(DEV), labels.to(DEV), valid.to(DEV)[:1])):
        with pytest.raises(RuntimeError):
            bad()
    old = T.USE_HIP_SOFTMAX
    try:  # the switch: the torch composition on tensors the kernel would take
        T.USE_HIP_SOFTMAX = False
        off = fn(x.to(DEV), labels.to(DEV), valid.to(DEV))
        assert not launched
        torch.testing.assert_close(off.cpu().double(), want, rtol=E.LOSS_RTOL, atol=E.LOSS_ATOL)
    finally:
        T.USE_HIP_SOFTMAX = old


def test_entries_refuse_bad_arguments():
    lib = _lib.load()
    B, C, plane = 2, 3, 16
    x, grad = (torch.zeros(B * C * plane + 8, device=DEV) for _ in range(2))
    labels = torch.zeros(B * plane, device=DEV, dtype=torch.uint8)
    valid = torch.ones(B * plane, device=DEV, dtype=torch.uint8)
    w = torch.ones(C + 1, device=DEV)
    partial = torch.zeros(int(lib.lss_softmax_ce_partials(B * plane)) + 1, device=DEV)
    loss, scale = torch.zeros(2, device=DEV), torch.zeros(2, device=DEV)
    st = _lib.stream_handle(DEV)
    p = _lib.ptr
    off = lambda v, by=2: ctypes.c_void_p(v.data_ptr() + by)  # noqa: E731

    def call(xp=p(x), lp=p(labels), vp=p(valid), b=B, pl=plane, c=C, wp=p(w), part=p(partial), lo=p(loss), sc=p(scale),
             gp=p(grad), dt=_lib.F32):
        return lib.lss_softmax_ce(xp, dt, lp, vp, b, pl, c, wp, part, lo, sc, gp, st)

    assert call() == 0 and call(vp=None) == 0
    for bad in (dict(xp=None), dict(lp=None), dict(wp=None), dict(part=None), dict(lo=None), dict(sc=None),
                dict(gp=None), dict(b=0), dict(b=-1), dict(pl=0), dict(c=1), dict(c=9), dict(c=0), dict(dt=7),
                dict(pl=2 ** 62), dict(xp=off(x)), dict(gp=off(grad)), dict(wp=off(w)), dict(part=off(partial)),
                dict(lo=off(loss)), dict(sc=off(scale)), dict(xp=off(x, 1), dt=_lib.BF16)):
        assert call(**bad) == -1, bad  # LSS_CONV_EINVAL, before any launch
    assert lib.lss_softmax_ce_arm(p(x), _lib.F32, p(labels), p(valid), B, plane, C, p(grad)) == 1
    assert lib.lss_softmax_ce_arm(p(x), _lib.F32, off(labels, 4), p(valid), B, plane, C, p(grad)) == 0
    assert lib.lss_softmax_ce_arm(p(x), _lib.F32, p(labels), off(valid, 4), B, plane, C, p(grad)) == 0
    assert lib.lss_softmax_ce_arm(off(x, 8), _lib.F32, p(labels), None, B, plane, C, p(grad)) == 0
    assert lib.lss_softmax_ce_arm(p(x), _lib.F32, p(labels), None, B, plane - 1, C, p(grad)) == 0
    for bad in (dict(c=9), dict(b=0), dict(dt=5), dict(xp=None)):
        kw = dict(xp=p(x), dt=_lib.F32, b=B, c=C)
        kw.update(bad)
        assert lib.lss_softmax_ce_arm(kw["xp"], kw["dt"], p(labels), None, kw["b"], plane, kw["c"], p(grad)) == -1, bad
    assert lib.lss_softmax_ce_partials(0) == 0 and lib.lss_softmax_ce_partials(257) == 4
    torch.cuda.synchronize()
