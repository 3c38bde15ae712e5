"""The K-channel head (lss_headk_fwd / lss_headk_bwd, models._HeadKx1 / _BnReluHeadK): a 1x1 conv to K = 2..8
output channels over channels-last bf16 rows, logits NCHW contiguous.

* Bit for bit against the one-channel kernels: each channel of the forward is lss_head1_fwd2's output for that
  channel's (w, b), with and without the batch-norm statistics; a gradient that is zero outside one channel
  gives lss_head1_bwd2's dx and partials (and zero partials for the other channels).
* Against fp64 of the same bf16-rounded operands: |y - y64| <= 2^-8 |y64| + C 2^-23 sum_c |in w| (one bf16
  rounding + the fp32 accumulation bound), dx likewise with K terms, dW / db within P 2^-23 sum |terms| plus
  one rounding to the gradient's dtype.
* models.bn_relu_head1 with K = 3 against its unfused form, the eligibility edges, and the C ABI's refusals.

Shapes: one row; P = 255; one row past a block; HW = 195 with two images (a block straddles the boundary)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import _lib, models as M, norm as Nm  # noqa: E402

DEV = torch.device("cuda:0")
CL = torch.channels_last
SHAPES = [(1, 1, 1), (1, 15, 17), (1, 1, 257), (2, 15, 13)]
CS = [64, 128]
KS = [2, 3, 8]
EINVAL = -1

_CASES = {}


def _case(C, shape):
    """x (N, C, H, W) channels-last bf16, a batch norm's saved statistics over it, and `inp` = the map the
    batch norm's ReLU apply stores, bf16(relu(fmaf(x, scale, shift))) -- from lss_bn_fwd2 itself. Made once."""
    key = (C, shape)
    if key not in _CASES:
        N, H, W = shape
        lib = _lib.load()
        g = torch.Generator().manual_seed(C + N * 7 + H * 31 + W)
        x = (torch.randn(N, C, H, W, generator=g) * 1.5 + 0.3).bfloat16().to(DEV).contiguous(memory_format=CL)
        gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
        beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
        groups = int(lib.lss_bn_groups(N, C, H * W, Nm.NHWC))
        partial = torch.empty(C, groups, 2, device=DEV)
        stats = torch.empty(4, C, device=DEV)
        inp = torch.empty_like(x)
        _lib.check(lib.lss_bn_fwd2(_lib.ptr(x), None, _lib.BF16, Nm.NHWC, N, C, H * W, _lib.ptr(gamma), _lib.ptr(beta),
                                   1e-5, 0.1, None, None, None, Nm.ACT["relu"], groups, _lib.ptr(partial),
                                   _lib.ptr(stats[0]), _lib.ptr(stats[1]), _lib.ptr(stats[2]), _lib.ptr(stats[3]),
                                   _lib.ptr(inp), None, _lib.stream_handle(DEV)), "lss_bn_fwd2")
        torch.cuda.synchronize()
        _CASES[key] = (x, stats, inp)
    return _CASES[key]


def _params(C, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(K, C, generator=g) * 0.2).bfloat16().float().to(DEV)  # bf16-rounded weights, as fp32
    b = torch.randn(K, generator=g).bfloat16().float().to(DEV)
    return w, b


def _rows(t):
    """(N, C, H, W) channels-last -> (P, C) rows, as fp64 on the CPU."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().cpu()


def _headk_fwd(x, w, b, stats):
    N, C, H, W = x.shape
    K = w.shape[0]
    y = torch.empty(N, K, H, W, device=DEV, dtype=torch.bfloat16)
    _lib.check(_lib.load().lss_headk_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), N * H * W, H * W, C, K,
                                         _lib.ptr(stats), _lib.ptr(y), _lib.stream_handle(DEV)), "lss_headk_fwd")
    return y


def _headk_bwd(x, dy, w, stats):
    N, C, H, W = x.shape
    K, P = w.shape[0], N * H * W
    lib = _lib.load()
    dx = torch.empty_like(x)
    part = torch.empty(int(lib.lss_head1_blocks(P)), K, C + 1, device=DEV)
    _lib.check(lib.lss_headk_bwd(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(w), P, H * W, C, K, _lib.ptr(stats), _lib.ptr(dx),
                                 _lib.ptr(part), _lib.stream_handle(DEV)), "lss_headk_bwd")
    return dx, part


def _head1_fwd(x, w1, b1, stats):
    N, C, H, W = x.shape
    y = torch.empty(N, 1, H, W, device=DEV, dtype=torch.bfloat16)
    _lib.check(_lib.load().lss_head1_fwd2(_lib.ptr(x), _lib.ptr(w1), _lib.ptr(b1), N * H * W, C, _lib.ptr(stats),
                                          _lib.ptr(y), _lib.stream_handle(DEV)), "lss_head1_fwd2")
    return y


def _head1_bwd(x, g1, w1, stats):
    N, C, H, W = x.shape
    P = N * H * W
    lib = _lib.load()
    dx = torch.empty_like(x)
    part = torch.empty(int(lib.lss_head1_blocks(P)), C + 1, device=DEV)
    _lib.check(lib.lss_head1_bwd2(_lib.ptr(x), _lib.ptr(g1), _lib.ptr(w1), P, C, _lib.ptr(stats), _lib.ptr(dx),
                                  _lib.ptr(part), _lib.stream_handle(DEV)), "lss_head1_bwd2")
    return dx, part


# ----------------------------------------------------------------------------- bit for bit vs the one-channel head
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C", CS)
def test_forward_channels_are_the_one_channel_head(C, K, shape, bn):
    x, stats, _ = _case(C, shape)
    st = stats if bn else None
    w, b = _params(C, K, seed=C + K)
    # every row of the K-head equal to (w1, b1): every channel is lss_head1_fwd2's output
    w1, b1 = w[0].contiguous(), b[:1].contiguous()
    want = _head1_fwd(x, w1, b1, st)
    got = _headk_fwd(x, w1.repeat(K, 1).contiguous(), b1.repeat(K).contiguous(), st)
    for k in range(K):
        assert torch.equal(got[:, k], want[:, 0]), k
    # distinct rows: channel k is the one-channel head of (w[k], b[k]) -- no channel reads another's weights
    got = _headk_fwd(x, w, b, st)
    for k in range(K):
        assert torch.equal(got[:, k], _head1_fwd(x, w[k].contiguous(), b[k:k + 1].contiguous(), st)[:, 0]), k
    # no bias
    got = _headk_fwd(x, w, None, st)
    assert torch.equal(got[:, K - 1], _head1_fwd(x, w[K - 1].contiguous(), None, st)[:, 0])


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C", CS)
def test_backward_of_a_one_channel_gradient_is_the_one_channel_head(C, K, shape, bn):
    x, stats, _ = _case(C, shape)
    st = stats if bn else None
    N, H, W = shape
    w, _ = _params(C, K, seed=2 * C + K)
    g = torch.Generator().manual_seed(K + H)
    g1 = torch.randn(N, 1, H, W, generator=g).bfloat16().to(DEV)
    for k in sorted({0, K // 2, K - 1}):
        dy = torch.zeros(N, K, H, W, device=DEV, dtype=torch.bfloat16)
        dy[:, k] = g1[:, 0]
        dx, part = _headk_bwd(x, dy, w, st)
        dx1, part1 = _head1_bwd(x, g1, w[k].contiguous(), st)
        assert torch.equal(dx, dx1), k
        assert torch.equal(part[:, k], part1), k
        others = [j for j in range(K) if j != k]
        assert int((part[:, others] != 0).sum()) == 0, k


# ----------------------------------------------------------------------------- vs fp64 of the bf16 operands
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C", CS)
def test_forward_and_backward_vs_fp64(C, K, shape, bn):
    x, stats, inp = _case(C, shape)
    st = stats if bn else None
    N, H, W = shape
    P = N * H * W
    w, b = _params(C, K, seed=3 * C + K)
    a64 = _rows(inp if bn else x)  # (P, C): the values the head multiplies
    w64, b64 = w.double().cpu(), b.double().cpu()
    y = _headk_fwd(x, w, b, st)
    y64 = a64 @ w64.t() + b64  # (P, K)
    mag = a64.abs() @ w64.abs().t()
    got = y.permute(0, 2, 3, 1).reshape(P, K).double().cpu()
    err = (got - y64).abs()
    bound = 2.0 ** -8 * y64.abs() + C * 2.0 ** -23 * mag
    print(f"y: worst err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())

    g = torch.Generator().manual_seed(C + K + P)
    dy = torch.randn(N, K, H, W, generator=g).bfloat16().to(DEV)
    dx, part = _headk_bwd(x, dy, w, st)
    dy64 = dy.permute(0, 2, 3, 1).reshape(P, K).double().cpu()
    dx64 = dy64 @ w64  # (P, C)
    err = (_rows(dx) - dx64).abs()
    bound = 2.0 ** -8 * dx64.abs() + K * 2.0 ** -23 * (dy64.abs() @ w64.abs())
    print(f"dx: worst err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())

    tot = part.sum(0).double().cpu()  # (K, C + 1) fp32 gradients
    dw64, db64 = dy64.t() @ a64, dy64.sum(0)
    for name, got, want, mag in (("dW", tot[:, :C], dw64, dy64.abs().t() @ a64.abs()),
                                 ("db", tot[:, C], db64, dy64.abs().sum(0))):
        err = (got - want).abs()
        bound = P * 2.0 ** -23 * mag + 2.0 ** -24 * want.abs()
        print(f"{name}: worst err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert bool((err <= bound).all()), name


# ----------------------------------------------------------------------------- module level
def _module_run(fn, bn, head, x, ctx, dout=None):
    bn, head = copy.deepcopy(bn), copy.deepcopy(head)
    xi = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    with ctx():
        y = fn(bn, head, xi)
    if dout is None:
        dout = torch.randn(y.shape, generator=torch.Generator().manual_seed(99)).to(y.device, y.dtype)
    y.backward(torch.empty_like(y).copy_(dout))
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": xi.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "dW": head.weight.grad,
            "db": head.bias.grad, "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone(),
            "num_batches_tracked": bn.num_batches_tracked.clone()}


def _bn_head(C, K, seed=0, mark=True):
    """A batch norm and a 1x1 head; mark: the head is a model's logits head (models.logits_head), as BevEncode's
    last conv is -- what lets conv1x1 / bn_relu_head1 return NCHW-contiguous logits from lss_headk_*."""
    torch.manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C) + 0.5)
        bn.bias.copy_(torch.randn(C) * 0.2)
    head = torch.nn.Conv2d(C, K, 1).to(DEV).to(memory_format=CL)
    return bn, (M.logits_head(head) if mark else head)


def _autocast():
    return torch.autocast("cuda", dtype=torch.bfloat16)


def test_bn_relu_headk_against_the_unfused_form(monkeypatch):
    """bn_relu_head1 with K = 3 under bf16 autocast against conv1x1(head, bn_act(bn, x, "relu")) with
    USE_HIP_HEADK off (the batch norm's map written, F.linear). Where a tensor is not bit-identical: y, dW and
    db within the fp64 bounds of the module docstring, computed from the bf16 operands (the unfused form's
    normalised map, the bf16 weights, the bf16 gradient; the parameter gradients are rounded to bf16 under
    autocast: 2^-8); d(x), d(gamma), d(beta) -- which go through the batch norm's backward -- at the project's
    bar for a wrapper against its stock form (tests/test_gpu_dispatch.py): an error against the fp64 CPU
    reference of at most twice the unfused form's. The running statistics must be equal."""
    N, C, H, W, K = 2, 128, 16, 24, 3
    P = N * H * W
    bn, head = _bn_head(C, K, seed=5)
    x = (torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(1)) + 0.2).bfloat16().to(DEV)
    x = x.contiguous(memory_format=CL)
    launched = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (launched.append(what), real(code, what))[1])
    got = _module_run(M.bn_relu_head1, bn, head, x, _autocast)
    assert "lss_headk_fwd" in launched and "lss_headk_bwd" in launched and "lss_bn_bwd2" in launched
    assert got["y"].shape == (N, K, H, W) and got["y"].is_contiguous() and got["y"].dtype == torch.bfloat16
    launched.clear()
    monkeypatch.setattr(M, "USE_HIP_HEADK", False)
    want = _module_run(lambda b, h, t: M.conv1x1(h, Nm.bn_act(b, t, "relu")), bn, head, x, _autocast)
    assert not [k for k in launched if "headk" in k]
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        assert torch.equal(got[k], want[k]), k
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k

    # the bf16 operands: the normalised map (what the unfused form's bn_act wrote), weights, bias, gradient
    with torch.no_grad():
        amap = Nm.bn_act(copy.deepcopy(bn), x, "relu")
    a64 = _rows(amap)
    w64 = head.weight.detach().bfloat16().reshape(K, C).double().cpu()
    b64 = head.bias.detach().bfloat16().double().cpu()
    dout = torch.randn(N, K, H, W, generator=torch.Generator().manual_seed(99)).to(DEV, torch.bfloat16)
    dy64 = dout.permute(0, 2, 3, 1).reshape(P, K).double().cpu()
    y64 = a64 @ w64.t() + b64
    checks = {
        "y": (got["y"].permute(0, 2, 3, 1).reshape(P, K), y64, 2.0 ** -8 * y64.abs()
              + C * 2.0 ** -23 * (a64.abs() @ w64.abs().t())),
        "dW": (got["dW"].reshape(K, C), dy64.t() @ a64, None),
        "db": (got["db"], dy64.sum(0), None),
    }
    for name, mag in (("dW", dy64.abs().t() @ a64.abs()), ("db", dy64.abs().sum(0))):
        g, ref, _ = checks[name]
        checks[name] = (g, ref, P * 2.0 ** -23 * mag + 2.0 ** -8 * ref.abs())
    for name, (g, ref, bound) in checks.items():
        if torch.equal(got[name], want[name]):
            continue
        err = (g.double().cpu() - ref).abs()
        print(f"{name}: worst err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert bool((err <= bound).all()), name

    # fp64 CPU reference of the whole tail, from the same bf16 input, for the gradients through the batch norm
    bn64, head64 = copy.deepcopy(bn).double().cpu(), copy.deepcopy(head).double().cpu()
    x64 = x.detach().double().cpu().requires_grad_(True)
    y_ref = head64(torch.relu(bn64(x64)))
    y_ref.backward(dout.double().cpu())
    ref = {"dx": x64.grad, "dgamma": bn64.weight.grad, "dbeta": bn64.bias.grad}
    for name in ref:
        if torch.equal(got[name], want[name]):
            continue
        ea = float((got[name].double().cpu() - ref[name]).abs().max())
        eb = float((want[name].double().cpu() - ref[name]).abs().max())
        print(f"{name}: error vs fp64 {ea:.3e} (fused) {eb:.3e} (unfused)")
        assert ea <= 2 * eb, (name, ea, eb)


def test_plain_headk_conv1x1_matches_linear():
    """conv1x1 to K = 3 channels without a batch norm in front (models._HeadKx1): NCHW logits, the fp64 bounds."""
    N, C, H, W, K = 2, 64, 9, 11, 3
    P = N * H * W
    _, head = _bn_head(C, K, seed=7)
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(2)).bfloat16().to(DEV).contiguous(memory_format=CL)
    xi = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    with _autocast():
        y = M.conv1x1(head, xi)
    assert y.is_contiguous() and y.shape == (N, K, H, W)
    dout = torch.randn(N, K, H, W, generator=torch.Generator().manual_seed(3)).bfloat16().to(DEV)
    y.backward(dout)
    a64 = _rows(x)
    w64 = head.weight.detach().bfloat16().reshape(K, C).double().cpu()
    b64 = head.bias.detach().bfloat16().double().cpu()
    dy64 = dout.permute(0, 2, 3, 1).reshape(P, K).double().cpu()
    y64 = a64 @ w64.t() + b64
    err = (y.detach().permute(0, 2, 3, 1).reshape(P, K).double().cpu() - y64).abs()
    assert bool((err <= 2.0 ** -8 * y64.abs() + C * 2.0 ** -23 * (a64.abs() @ w64.abs().t())).all())
    dx64 = dy64 @ w64
    err = (_rows(xi.grad) - dx64).abs()
    assert bool((err <= 2.0 ** -8 * dx64.abs() + K * 2.0 ** -23 * (dy64.abs() @ w64.abs())).all())
    dw64 = dy64.t() @ a64
    err = (head.weight.grad.reshape(K, C).double().cpu() - dw64).abs()
    assert head.weight.grad.dtype == torch.float32
    assert bool((err <= P * 2.0 ** -23 * (dy64.abs().t() @ a64.abs()) + 2.0 ** -8 * dw64.abs()).all())
    err = (head.bias.grad.double().cpu() - dy64.sum(0)).abs()
    assert bool((err <= P * 2.0 ** -23 * dy64.abs().sum(0) + 2.0 ** -8 * dy64.sum(0).abs()).all())


# ----------------------------------------------------------------------------- eligibility edges
def _null():
    import contextlib
    return contextlib.nullcontext()


EDGES = {
    # name: (C, K, input dtype, channels-last input, context, head marked as the logits head)
    "K=9": (64, 9, torch.bfloat16, True, _autocast, True),
    "fp32-no-autocast": (64, 3, torch.float32, True, _null, True),
    "fp16-autocast": (64, 3, torch.float16, True, lambda: torch.autocast("cuda", dtype=torch.float16), True),
    "nchw-input": (64, 3, torch.bfloat16, False, _autocast, True),
    "C=24": (24, 3, torch.bfloat16, True, _autocast, True),
    "unmarked-head": (64, 3, torch.bfloat16, True, _autocast, False),
}


@pytest.mark.parametrize("case", list(EDGES))
def test_off_the_fast_path_is_the_fallback(case, monkeypatch):
    """Outside 2 <= K <= 8, bf16, channels-last, C % 8 == 0 with 64 % (C / 8) == 0 -- or on a conv that is not
    marked as a logits head -- bn_relu_head1 is conv1x1(bn_act(x)) as before: no lss_headk launch, and the
    generic path's results bit for bit."""
    C, K, dtype, cl, ctx, mark = EDGES[case]
    bn, head = _bn_head(C, K, seed=11, mark=mark)
    x = torch.randn(2, C, 7, 9, generator=torch.Generator().manual_seed(4)).to(DEV, dtype)
    if cl:
        x = x.contiguous(memory_format=CL)
    launched = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (launched.append(what), real(code, what))[1])
    got = _module_run(M.bn_relu_head1, bn, head, x, ctx)
    assert not [k for k in launched if "headk" in k], launched
    monkeypatch.setattr(M, "USE_HIP_HEADK", False)
    want = _module_run(M.bn_relu_head1, bn, head, x, ctx)
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].stride() == want[k].stride(), k
        assert torch.equal(got[k], want[k]), k


# ----------------------------------------------------------------------------- C ABI
def test_c_abi_refuses_bad_arguments():
    lib = _lib.load()
    N, C, H, W = 1, 64, 3, 5
    P = N * H * W
    st = _lib.stream_handle(DEV)
    buf = torch.zeros(P * C + 8, device=DEV, dtype=torch.bfloat16)
    x, odd = buf[:P * C], buf[1:P * C + 1]
    assert x.data_ptr() % 16 == 0 and odd.data_ptr() % 16 == 2
    dx = torch.zeros(P * C, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(9, C, device=DEV)
    b = torch.zeros(9, device=DEV)
    y = torch.full((9 * P,), 7.0, device=DEV, dtype=torch.bfloat16)
    part = torch.zeros(9 * (C + 1), device=DEV)

    def fwd(xx, K, hw=H * W):
        return lib.lss_headk_fwd(_lib.ptr(xx), _lib.ptr(w), _lib.ptr(b), P, hw, C, K, None, _lib.ptr(y), st)

    def bwd(xx, K, dxx=dx):
        return lib.lss_headk_bwd(_lib.ptr(xx), _lib.ptr(y), _lib.ptr(w), P, H * W, C, K, None, _lib.ptr(dxx),
                                 _lib.ptr(part), st)

    assert fwd(x, 1) == EINVAL and fwd(x, 9) == EINVAL and fwd(odd, 2) == EINVAL
    assert bwd(x, 1) == EINVAL and bwd(x, 9) == EINVAL and bwd(odd, 2) == EINVAL and bwd(x, 2, odd) == EINVAL
    assert bwd(x, 2, None) == EINVAL  # dx is always written
    assert fwd(x, 2, hw=4) == EINVAL  # P is not a whole number of images
    assert lib.lss_headk_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), P, H * W, 24, 2, None, _lib.ptr(y), st) == EINVAL
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())  # refused before any launch
    assert fwd(x, 2) == 0 and bwd(x, 2) == 0
    torch.cuda.synchronize()
