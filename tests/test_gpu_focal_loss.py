"""tools.FocalLoss on lss_focal_logits_pc against the fp64 closed form of the logits the kernel sees.

Shapes: (2, 3, 5, 5) plane 25, a thread crosses planes; (1, 2, 1, 9) under one vector; (4, 8, 16, 16) four blocks;
(1, 1, 1, 2049) a second block holding one element. fp32 and bf16 logits, gamma in {0, 0.5, 2, 3.7} (scaled per
class), distinct (w_pos, w_neg) per class, the backward scaled by 0.75.

Bars: the project's for this loss (tests/test_gpu_loss.py) -- loss rtol 2e-6 / atol 1e-7; fp32 gradient rtol
max(1e-5, 4 r32), atol 1e-12, where r32 is the formula's own rounding: the largest relative error, over gradient
elements above 1e-12, of an fp32 CPU evaluation of the closed form against fp64 on the same inputs (the factor 4:
the device's expf / log1pf are a few ulp off the host's); bf16 gradient 8e-3 (one rounding). Each case prints r32
and the kernel's measured errors."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import focal_cases as C  # noqa: E402
from lss_carla_amd import _lib, tools as T  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(2, 3, 5, 5), (1, 2, 1, 9), (4, 8, 16, 16), (1, 1, 1, 2049)]
DTYPES = [torch.float32, torch.bfloat16]


def _module(rows):
    fn = T.FocalLoss(len(rows)).to(DEV)
    fn.focal_params.copy_(torch.tensor(rows))
    return fn, fn.focal_params.cpu().tolist()  # the fp32 rows the kernel reads


def _run(fn, x, t, scale=0.75):
    xd = x.to(DEV).requires_grad_(True)
    loss = fn(xd, t.to(DEV))
    loss.backward(torch.tensor(scale, device=DEV))
    return loss.detach(), xd.grad


def _grad_tol(x, t, rows, dtype):
    if dtype == torch.bfloat16:
        return 8e-3, None
    r32 = C.formula_rounding(x, t, rows)
    return max(1e-5, 4 * r32), r32


def _rel_err(got, want):
    big = want.abs() > 1e-12
    return ((got - want).abs()[big] / want.abs()[big]).max().item() if big.any() else 0.0


@pytest.fixture
def launched(monkeypatch):
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (calls.append(what), real(code, what))[1])
    return calls


@pytest.mark.parametrize("gamma", C.GAMMAS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_focal_vs_fp64_closed_form(shape, dtype, gamma, launched):
    x, t = C.data(shape, dtype, seed=1)
    fn, rows = _module(C.rows(shape[1], gamma))
    loss, grad = _run(fn, x, t)
    assert launched == ["lss_focal_logits_pc", "lss_bce_logits_bwd"]
    assert grad.dtype == dtype and loss.dtype == torch.float32 and loss.shape == ()
    want, wgrad = C.closed_form(x.double(), t.double(), rows)
    wgrad = 0.75 * wgrad
    tol, r32 = _grad_tol(x, t, rows, dtype)
    print(f"{shape} {dtype} gamma {gamma}: loss {loss.item():.9e} fp64 {want.item():.9e} rel "
          f"{abs(loss.item() - want.item()) / max(abs(want.item()), 1e-300):.2e}; r32 {r32} grad rel err "
          f"{_rel_err(grad.cpu().double(), wgrad):.2e} (bar {tol:.2e})")
    torch.testing.assert_close(loss.cpu().double(), want, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    torch.testing.assert_close(grad.cpu().double(), wgrad, rtol=tol, atol=1e-12)
    assert torch.isfinite(grad).all()
    # two runs: equal bits
    loss2, grad2 = _run(fn, x, t)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_gamma_zero_is_simple_loss(shape, dtype):
    """(pw_k, 1, 0) is SimpleLoss(pw) on hard labels: within the bars of both (the expressions differ)."""
    x, t = C.data(shape, dtype, seed=2)
    K = shape[1]
    pw = [0.5 + 0.75 * k for k in range(K)]
    fn = T.FocalLoss(K, gamma=0.0, pos_weight=pw).to(DEV)
    assert fn.focal_params.cpu().tolist() == [[torch.tensor(w).item(), 1.0, 0.0] for w in pw]
    lf, gf = _run(fn, x, t)
    ls, gs = _run(T.SimpleLoss(pw if K > 1 else pw[0]).to(DEV), x, t)
    tol, _ = _grad_tol(x, t, fn.focal_params.cpu().tolist(), dtype)
    torch.testing.assert_close(lf, ls, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    torch.testing.assert_close(gf.double(), gs.double(), rtol=tol, atol=1e-12)


def test_params_are_read_on_the_device_eager_and_replayed():
    x, t = C.data((2, 3, 5, 5), torch.float32, seed=3)
    fn, _ = _module([(1.0, 1.0, 2.0)] * 3)
    a, _ = _run(fn, x, t)
    new = [(1.0, 1.0, 2.0), (3.0, 0.5, 1.0), (1.0, 1.0, 2.0)]
    fn.focal_params.copy_(torch.tensor(new))
    b, gb = _run(fn, x, t)
    want, wgrad = _run(_module(new)[0], x, t)
    assert not torch.equal(a, b) and torch.equal(b, want) and torch.equal(gb, wgrad)

    fn, _ = _module([(1.0, 1.0, 2.0)] * 3)
    xd, td = x.to(DEV).requires_grad_(True), t.to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.autograd.grad(fn(xd, td), xd)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = fn(xd, td)
        (grad,) = torch.autograd.grad(loss, xd, torch.full((), 0.75, device=DEV))
    graph.replay()
    assert torch.equal(loss, a)
    fn.focal_params.copy_(torch.tensor(new))
    graph.replay()
    assert torch.equal(loss, b) and torch.equal(grad, gb)


def test_strided_or_misaligned_logits_take_the_torch_path(launched):
    rows = C.rows(3, 2.0)
    fn, rows = _module(rows)
    x = torch.randn(4, 3, 10, 12, device=DEV).transpose(2, 3)
    t = (torch.rand(4, 3, 12, 10, device=DEV) < 0.5).float()
    got = fn(x, t)
    buf = torch.randn(2 * 3 * 5 * 5 + 1, device=DEV)
    xm = buf[1:].view(2, 3, 5, 5).requires_grad_(True)  # contiguous, 4 bytes off a 16-byte boundary
    assert xm.is_contiguous() and xm.data_ptr() % 16 == 4
    tm = (torch.rand(2, 3, 5, 5, device=DEV) < 0.5).float()
    gotm = fn(xm, tm)
    (gm,) = torch.autograd.grad(gotm, xm)
    assert not launched
    want, _ = C.closed_form(x.cpu().double(), t.cpu().double(), rows)
    wantm, wgm = C.closed_form(xm.detach().cpu().double(), tm.cpu().double(), rows)
    torch.testing.assert_close(got.cpu().double(), want, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    torch.testing.assert_close(gotm.cpu().double(), wantm, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    tol, _ = _grad_tol(xm.detach().cpu(), tm.cpu(), rows, torch.float32)
    torch.testing.assert_close(gm.cpu().double(), wgm, rtol=tol, atol=1e-12)
    with pytest.raises(RuntimeError):
        fn(torch.randn(4, 2, 5, 5, device=DEV), torch.zeros(4, 2, 5, 5, device=DEV))  # 3 classes, 2 channels


def test_entry_refuses_bad_arguments():
    lib = _lib.load()
    n, K = 64, 2
    x = torch.zeros(n + 8, device=DEV)
    t = torch.zeros(n + 8, device=DEV)
    grad = torch.zeros(n + 8, device=DEV)
    params = torch.ones(K, 3, device=DEV)
    partial = torch.zeros(int(lib.lss_bce_partials(n)), device=DEV)
    loss = torch.zeros((), device=DEV)
    st = _lib.stream_handle(DEV)
    p = _lib.ptr

    def call(xp=p(x), tp=p(t), k=K, pp=p(params), gp=p(grad), plane=n // K, count=n):
        return lib.lss_focal_logits_pc(xp, _lib.F32, tp, count, plane, k, pp, p(partial), p(loss), gp, st)

    off = lambda v: ctypes.c_void_p(v.data_ptr() + 2)  # noqa: E731
    assert call() == 0
    for bad in (dict(xp=None), dict(tp=None), dict(pp=None), dict(gp=None), dict(k=0), dict(plane=0), dict(count=0),
                dict(xp=off(x)), dict(tp=off(t)), dict(gp=off(grad)), dict(pp=off(params))):
        assert call(**bad) == -1, bad  # LSS_CONV_EINVAL, before any launch
    assert lib.lss_focal_logits_pc(p(x), 7, p(t), n, n // K, K, p(params), p(partial), p(loss), p(grad), st) == -1
    torch.cuda.synchronize()
