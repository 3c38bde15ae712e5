"""Every HIP-backed op at the edge of its eligibility: the Python predicate in front of each kernel is
the only thing between a legal tensor and a kernel that takes a bare pointer, so each clause gets an
input that just misses it (the op must run the stock PyTorch op: no launch, same dtypes / shapes /
strides, the same values) and one that meets it (the launch spy shows the kernels).

Launch spy: ``lss_carla_amd._lib.check`` is wrapped; every wrapper reaches the library through
``_lib.check(..., "lss_xxx")`` looked up at call time, so the recorded names are the kernels an op
launched, forward and backward.

Case table (miss -> stock op, no ``lss_*`` launch of that op; meet -> the kernels in the spy)

  op / predicate                  misses                                             meets
  ------------------------------  -------------------------------------------------  ------------------------------
  norm.bn_act                     bf16 BN module (NCHW 2x8x4x6, NHWC 2x16x3x5),       bf16 / fp32 NCHW V = 8 / 4,
                                  fp16 model, fp64 model, affine=False, eval,         NHWC 2x16x3x5, +- residual,
                                  x[:, ::2] (not dense), NHWC C = 24                  unaligned x / res / dy, x[1:]
  models.conv3x3 (_flip_eligible) fp16, fp64, fp16 autocast on an fp32 conv; each    fp32 and bf16-autocast
                                  with grad on x / weight / both
  resample.upsample_cat, Up       C1 = 12, NCHW bf16, fp32 NHWC, Hi = 1, skip of      1x16x5x7 + skip 8, scale 2,
                                  another spatial size (stock torch.cat's error)      unaligned x / skip / dy
  efficientnet.squeeze_excite     HW = 6, fp32 x, NHWC x, bias=False (either conv),   2x8x2x4, unaligned x / dy,
                                  sq = 65, C = 2056                                   x[1:]
  efficientnet.pointwise_conv     HW = 9, fp16 autocast, fp32 x without autocast,     2x8x2x4 bf16 autocast,
                                  bias, stride 2                                      unaligned x / dy
  models.conv1x1 (_head1_eligible) C = 12, C = 24, NCHW, out_channels = 2, fp32 x     2x64x7x9 NHWC, unaligned
  models.bn_relu_head1            the same + a bf16 BN module                         2x64x7x9 NHWC, unaligned
  MBConvBlock depthwise 'hip'     fp64 block, fp16 block (vs 'miopen', same weights)  2x8x6x8 K3 s1 / K5 s2,
                                                                                      unaligned x / dy
  efficientnet.drop_connect_add   fp32, x NHWC + inputs NCHW, numel / N % 8 != 0,     2x8x2x4 bf16
                                  x or inputs unaligned
  models.LssDropout               fp16, p = 0, p = 1, eval, unaligned x, 12 bytes     2x8x2x4 bf16

Legal but unusual inputs (a dense view at a storage offset that is not 16-B aligned; a batch slice) must
give bit-identical results to the aligned dense copy of the same values.
"""
import contextlib
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU CI, skipped there
    pytest.skip("needs an MI355X", allow_module_level=True)

from test_gpu_robustness import _unaligned_like  # noqa: E402
from lss_carla_amd import _lib, efficientnet as E, models as M, norm as Nm, resample as R  # noqa: E402

DEV = torch.device("cuda:0")
CL = torch.channels_last
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64


@pytest.fixture
def launched(monkeypatch):
    """The ``what`` of every _lib.check call, in order: the kernels the ops under test launched."""
    seen = []
    real = _lib.check

    def spy(code, what):
        seen.append(what)
        return real(code, what)

    monkeypatch.setattr(_lib, "check", spy)
    return seen


def bf16_autocast():
    return torch.autocast("cuda", dtype=BF16)


def fp16_autocast():
    return torch.autocast("cuda", dtype=F16)


def T(shape, dtype=BF16, fmt="c", seed=0, grad=True):
    """A seeded leaf on the GPU: the same values, strides and dtype on every call."""
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV, dtype)
    if fmt == "cl":
        t = t.contiguous(memory_format=CL)
    return t.requires_grad_(grad)


def _mf(t):
    cl = t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=CL)
    return CL if cl else torch.contiguous_format


def _off16(t, grad=None):
    """The same values and strides at a storage offset that is not 16-B aligned, as a leaf."""
    grad = t.requires_grad if grad is None else grad
    return _unaligned_like(t.detach(), _mf(t)).requires_grad_(grad)


def _run(fn, mods, ins, ctx=None, seed=None, off16_dy=False):
    """y = fn(*mods, *ins) under ctx, backpropagated with a seeded gradient of y's strides. Returns the
    output, every input and parameter gradient and every buffer, by name."""
    if seed is not None:
        torch.manual_seed(seed)
    with (ctx() if ctx else contextlib.nullcontext()):
        y = fn(*mods, *ins)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(99)).to(y.device)
    dy = torch.empty_like(y).copy_(dy)
    if off16_dy:
        dy = _unaligned_like(dy, _mf(dy))
    y.backward(dy)
    if y.is_cuda:
        torch.cuda.synchronize()
    out = {"y": y.detach()}
    for i, t in enumerate(ins):
        if isinstance(t, torch.Tensor) and t.requires_grad:
            out[f"d_in{i}"] = t.grad
    for j, m in enumerate(mods):
        for n, p in m.named_parameters():
            out[f"d_m{j}.{n}"] = p.grad
        for n, b in m.named_buffers():
            out[f"m{j}.{n}"] = b.detach().clone()
    return out


def _fp64_reference(stock, mods, mk_inputs):
    mods = [copy.deepcopy(m).double().cpu() for m in mods]
    ins = [t.detach().double().cpu().requires_grad_(t.requires_grad) for t in mk_inputs()]
    return _run(stock, mods, ins)


def _err(a, ref):
    return float((a.detach().double().cpu() - ref.double()).abs().max())


def _assert_same(got, want, loose=(), reference=None):
    """Same names, dtypes, shapes, strides and bits. A name in ``loose`` (a gradient whose stock backward is
    not deterministic: MIOpen weight gradients, atomic scatters) may differ in bits if its error against
    the fp64 CPU reference is at most twice the stock result's (summation order only)."""
    assert got.keys() == want.keys(), got.keys() ^ want.keys()
    ref = None
    for k in got:
        a, b = got[k], want[k]
        if a is None or b is None:
            assert a is None and b is None, k
            continue
        assert (a.dtype, a.shape, a.stride()) == (b.dtype, b.shape, b.stride()), (k, a.dtype, b.dtype, a.stride(),
                                                                                  b.stride())
        if torch.equal(a, b):
            continue
        assert any(s in k for s in loose), f"{k}: differs from the stock result by {_err(a, b.cpu()):.3e}"
        ref = ref or reference()
        ea, eb = _err(a, ref[k]), _err(b, ref[k])
        print(f"{k}: error vs fp64 {ea:.3e} (wrapper) {eb:.3e} (stock)")
        # Measured on an MI355X (wrapper / stock): only d(x) of test_upsample_cat_falls_back differed in
        # bits (torch's bilinear backward adds atomically) -- bf16 3.062e-02 / 3.062e-02 and
        # 3.522e-02 / 3.522e-02, fp32 9.201e-07 / 9.201e-07; every MIOpen gradient came out bit-equal.
        assert ea <= 2 * eb, (k, ea, eb)


def check_fallback(launched, op, stock, mods, mk_inputs, banned="lss_", ctx=None, loose=(), seed=None):
    """op must be the stock op on this input: nothing of `banned` launched, and the same results."""
    launched.clear()
    got = _run(op, copy.deepcopy(mods), mk_inputs(), ctx, seed)
    ran = list(launched)
    assert not [k for k in ran if k.startswith(banned)], ran
    want = _run(stock, copy.deepcopy(mods), mk_inputs(), ctx, seed)
    _assert_same(got, want, loose, lambda: _fp64_reference(stock, mods, mk_inputs))
    return got


def check_unaligned(launched, op, mods, mk_inputs, expect, ctx=None, which=None, tol_keys=()):
    """The results with each input in turn (and then the gradient) at an unaligned storage offset are those
    of the aligned run, bit for bit; the aligned run launches `expect`. tol_keys: gradients whose
    determinism no test asserts (the SE weight gradients) -- equal, or within the op's fp64 tolerance."""
    launched.clear()
    base = _run(op, copy.deepcopy(mods), mk_inputs(), ctx, seed=3)
    assert set(expect) <= set(launched), (expect, launched)
    n = len(mk_inputs())
    variants = [("dy", None)] + [(f"in{i}", i) for i in (range(n) if which is None else which)]
    for name, i in variants:
        ins = mk_inputs()
        if i is not None:
            ins[i] = _off16(ins[i])
        got = _run(op, copy.deepcopy(mods), ins, ctx, seed=3, off16_dy=i is None)
        assert got.keys() == base.keys()
        for k in got:
            a, b = got[k], base[k]
            if a is None or b is None:
                assert a is None and b is None, (name, k)
                continue
            assert (a.dtype, a.shape) == (b.dtype, b.shape), (name, k)
            if any(s in k for s in tol_keys) and not torch.equal(a, b):
                rel = _err(a, b.cpu()) / max(float(b.double().abs().max()), 1e-12)
                assert rel < 5e-2, (name, k, rel)  # test_squeeze_excite_vs_fp64's bound on these gradients
                continue
            assert torch.equal(a, b), f"{name} unaligned: {k} differs by {_err(a, b.cpu()):.3e}"
    return base


# ------------------------------------------------------------------------------------------------ bn_act
def _bn(C, dtype=F32, **kw):
    torch.manual_seed(C)
    bn = nn.BatchNorm2d(C, eps=1e-3, momentum=0.1, **kw).to(DEV)
    with torch.no_grad():
        if bn.affine:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.1)
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 1.5)
    return bn.to(dtype).train()


def _bn_op(act):
    return lambda bn, x, res=None: Nm.bn_act(bn, x, act, res)


def _bn_stock(act):
    def f(bn, x, res=None):
        y = bn(x)
        if res is not None:
            y = y + res
        return {"none": y, "relu": F.relu(y), "swish": F.silu(y)}[act]
    return f


BN_FALLBACK = {  # name: (module, inputs)
    "bf16_module_nchw": (lambda: _bn(8, BF16), lambda: [T((2, 8, 4, 6))]),
    "bf16_module_nhwc": (lambda: _bn(16, BF16), lambda: [T((2, 16, 3, 5), fmt="cl")]),
    "fp16_model": (lambda: _bn(8, F16), lambda: [T((2, 8, 4, 6), F16)]),
    "fp64_model": (lambda: _bn(8, F64), lambda: [T((2, 8, 4, 6), F64)]),
    "affine_false": (lambda: _bn(8, affine=False), lambda: [T((2, 8, 4, 6), F32)]),
    "eval": (lambda: _bn(8).eval(), lambda: [T((2, 8, 4, 6), F32)]),
    "channel_slice": (lambda: _bn(8), lambda: [T((2, 16, 4, 6), F32, grad=False)[:, ::2].requires_grad_(True)]),
    "nhwc_c24": (lambda: _bn(24), lambda: [T((2, 24, 3, 5), fmt="cl")]),
}


@pytest.mark.parametrize("act", ["relu", "swish"])
@pytest.mark.parametrize("case", sorted(BN_FALLBACK))
def test_bn_act_falls_back(case, act, launched):
    """A BatchNorm2d the lss_bn_* kernels cannot take -- they read gamma / beta / running statistics as
    fp32 arrays, x as dense fp32 / bf16 -- runs stock nn.BatchNorm2d: outputs, gradients (in the
    parameters' dtype), running statistics and num_batches_tracked are the stock op's."""
    mk_bn, mk_in = BN_FALLBACK[case]
    bn = mk_bn()
    got = check_fallback(launched, _bn_op(act), _bn_stock(act), [bn], mk_in, banned="lss_bn")
    if bn.affine:
        assert got["d_m0.weight"].dtype == bn.weight.dtype and got["d_m0.bias"].dtype == bn.bias.dtype
    assert int(got["m0.num_batches_tracked"]) == (0 if case == "eval" else 1)


BN_ALIGN = [(BF16, (2, 8, 4, 6), "c"), (BF16, (2, 8, 2, 6), "c"), (F32, (2, 8, 4, 6), "c"), (BF16, (2, 16, 3, 5), "cl")]


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("dtype,shape,fmt", BN_ALIGN)
def test_bn_act_unaligned_views(dtype, shape, fmt, with_res, launched):
    """x, the residual or dy at a storage offset of one element (NCHW V = 8, V = 4, fp32; NHWC): the kernels'
    uint4 / uint2 / float4 accesses need the copy norm._BnAct makes."""
    def mk():
        return [T(shape, dtype, fmt)] + ([T(shape, dtype, fmt, seed=1)] if with_res else [])
    check_unaligned(launched, _bn_op("relu"), [_bn(shape[1])], mk, ["lss_bn_fwd2", "lss_bn_bwd2"])


def test_bn_act_batch_slice_stays_on_the_kernels(launched):
    """x[1:] of a dense buffer is dense and 16-B aligned: the kernel path, the same bits as from a copy, and
    the fp64 result within test_bn_act_vs_fp64's bf16 tolerance."""
    def op(bn, base):
        return Nm.bn_act(bn, base[1:], "swish")
    bn = _bn(8)
    launched.clear()
    got = _run(op, [copy.deepcopy(bn)], [T((3, 8, 4, 6))])
    assert launched == ["lss_bn_fwd2", "lss_bn_bwd2"]
    want = _run(lambda m, base: Nm.bn_act(m, base[1:].clone(), "swish"), [copy.deepcopy(bn)], [T((3, 8, 4, 6))])
    _assert_same(got, want)
    ref = _run(lambda m, base: F.silu(m(base[1:])), [copy.deepcopy(bn).double().cpu()],
               [T((3, 8, 4, 6)).detach().double().cpu().requires_grad_(True)])
    for k in ("y", "d_in0"):
        torch.testing.assert_close(got[k].double().cpu(), ref[k], rtol=2e-2, atol=3e-2)
    torch.testing.assert_close(got["m0.running_var"].double().cpu(), ref["m0.running_var"], rtol=1e-3, atol=1e-4)


def test_bn_entry_point_refuses_a_real_unaligned_pointer():
    """The C-ABI backstop on real memory: the call that succeeds on a tensor is LSS_CONV_EINVAL two bytes on."""
    lib = _lib.load()
    x, y = T((2, 8, 4, 6), grad=False), torch.empty(2 * 8 * 24 + 8, device=DEV, dtype=BF16)
    xs = torch.cat([x.flatten(), x.flatten()[:8]])  # room for the shifted read
    f32 = dict(device=DEV, dtype=F32)
    g, b, part, st = torch.ones(8, **f32), torch.zeros(8, **f32), torch.empty(8, 1, 2, **f32), torch.empty(4, 8, **f32)
    for off, want in ((0, 0), (2, -1), (8, -1)):
        code = lib.lss_bn_fwd2(xs.data_ptr() + off, None, _lib.BF16, _lib.NCHW, 2, 8, 24, _lib.ptr(g), _lib.ptr(b), 1e-3,
                               0.1, None, None, None, 1, 1, _lib.ptr(part), _lib.ptr(st[0]), _lib.ptr(st[1]),
                               _lib.ptr(st[2]), _lib.ptr(st[3]), _lib.ptr(y), None, _lib.stream_handle(DEV))
        assert code == want, (off, code)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- conv3x3
def _conv3(dtype=F32):
    torch.manual_seed(1)
    return nn.Conv2d(8, 8, 3, padding=1, bias=False).to(DEV, dtype)


CONV3_MISS = {"fp16": (F16, F16, None), "fp64": (F64, F64, None), "fp16_autocast": (F32, F32, fp16_autocast)}


@pytest.mark.parametrize("grads", ["x", "weight", "both"])
@pytest.mark.parametrize("case", sorted(CONV3_MISS))
def test_conv3x3_falls_back(case, grads, launched):
    """fp16 / fp64 callers and fp16 autocast are conv(x) -- the flipped-weight backward takes fp32 / bf16
    only and _Conv3x3 casts to bf16 under any autocast -- with a backward that works."""
    wdt, xdt, ctx = CONV3_MISS[case]
    conv = _conv3(wdt)
    conv.weight.requires_grad_(grads != "x")
    got = check_fallback(launched, M.conv3x3, lambda c, x: c(x), [conv], lambda: [T((2, 8, 5, 7), xdt, grad=grads != "weight")],
                         ctx=ctx, loose=("weight", "d_in0"))
    assert got["y"].dtype == (F16 if case != "fp64" else F64)
    assert (got.get("d_in0") is not None) == (grads != "weight") and (got["d_m0.weight"] is not None) == (grads != "x")


@pytest.mark.parametrize("grads", ["x", "weight", "both"])
@pytest.mark.parametrize("case", ["fp32", "bf16", "bf16_autocast"])
def test_conv3x3_eligible_runs_the_flipped_backward(case, grads, launched):
    wdt, xdt, ctx = {"fp32": (F32, F32, None), "bf16": (BF16, BF16, None), "bf16_autocast": (F32, BF16, bf16_autocast)}[case]
    conv = _conv3(wdt)
    conv.weight.requires_grad_(grads != "x")
    mk = lambda: [T((2, 8, 5, 7), xdt, grad=grads != "weight")]  # noqa: E731
    launched.clear()
    got = _run(M.conv3x3, [copy.deepcopy(conv)], mk(), ctx)
    assert launched == (["lss_conv_flip_weight"] if grads != "weight" else [])
    want = _run(lambda c, x: c(x), [copy.deepcopy(conv)], mk(), ctx)
    assert torch.equal(got["y"], want["y"])  # the same forward call
    # the backward-data is a forward conv of dy with the flipped weight: another summation order over the
    # 8 x 9 = 72 products, each operand O(1): a few ulps of the result's dtype
    tol = dict(rtol=1e-4, atol=1e-4) if case == "fp32" else dict(rtol=2e-2, atol=3e-2)
    for k in got:
        if got[k] is None:
            assert want[k] is None, k
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape
            torch.testing.assert_close(got[k].float(), want[k].float(), **tol)


# ---------------------------------------------------------------------------------- upsample_cat and Up
def _up_stock(x, skip):
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    return torch.cat([skip, up], dim=1)


UP_MISS = {  # x, skip
    "c1_12": lambda: [T((1, 12, 5, 7), fmt="cl"), T((1, 8, 10, 14), fmt="cl", seed=1)],
    "nchw": lambda: [T((1, 16, 5, 7)), T((1, 8, 10, 14), seed=1)],
    "fp32_nhwc": lambda: [T((1, 16, 5, 7), F32, "cl"), T((1, 8, 10, 14), F32, "cl", seed=1)],
    "hi_1": lambda: [T((1, 16, 1, 7), fmt="cl"), T((1, 8, 2, 14), fmt="cl", seed=1)],
}


@pytest.mark.parametrize("case", sorted(UP_MISS))
def test_upsample_cat_falls_back(case, launched):
    """(torch's bilinear backward scatters with atomics: d(x) may differ in bits between two stock runs.)"""
    check_fallback(launched, lambda x, s: R.upsample_cat(x, s, 2), _up_stock, [], UP_MISS[case], banned="lss_upsample",
                   loose=("d_in0",))


def _up_module(cin):
    torch.manual_seed(2)
    return M.Up(cin, 16).to(DEV).to(memory_format=CL).train()


def _up_stock_module(up, x1, x2):
    return up.conv(torch.cat([x2, up.up(x1)], dim=1))  # src/models.py:31-34, stock modules


@pytest.mark.parametrize("case", sorted(UP_MISS))
def test_up_forward_falls_back(case, launched):
    """Up.forward on maps lss_upsample_* cannot take: the stock upsample + cat (no lss_upsample launch), then
    the two conv-BN-ReLU stages; against the stock nn.Sequential on the same weights. Two 3x3 convs over
    <= 24 channels and two batch norms of O(1) outputs: within a few bf16 ulps (2^-8) of 1, 5e-2; fp32
    1e-3."""
    mk = UP_MISS[case]
    up = _up_module(mk()[0].shape[1] + 8)
    ctx = bf16_autocast if mk()[0].dtype == BF16 else None
    launched.clear()
    got = _run(lambda m, a, b: m(a, b), [copy.deepcopy(up)], mk(), ctx)
    assert not [k for k in launched if k.startswith("lss_upsample")], launched
    want = _run(_up_stock_module, [copy.deepcopy(up)], mk(), ctx)
    assert got["y"].dtype == want["y"].dtype and got["y"].shape == want["y"].shape
    tol = 5e-2 if ctx else 1e-3
    torch.testing.assert_close(got["y"].float(), want["y"].float(), rtol=tol, atol=tol)
    for k in ("m0.conv.1.running_mean", "m0.conv.4.running_var", "m0.conv.1.num_batches_tracked"):
        torch.testing.assert_close(got[k].float(), want[k].float(), rtol=tol, atol=tol)


def test_upsample_cat_skip_of_another_size_raises_like_torch_cat():
    x, skip = T((1, 16, 5, 7), fmt="cl"), T((1, 8, 9, 14), fmt="cl", seed=1)
    with pytest.raises(RuntimeError) as stock:
        _up_stock(x, skip)
    with pytest.raises(RuntimeError) as ours:
        R.upsample_cat(x, skip, 2)
    assert str(ours.value) == str(stock.value) and "Sizes of tensors must match" in str(ours.value)
    up = _up_module(24)
    with pytest.raises(RuntimeError) as mod, bf16_autocast():
        up(x, skip)
    assert str(mod.value) == str(stock.value)


def test_upsample_cat_unaligned_views(launched):
    """x, skip or dy at an unaligned offset: lss_upsample_* return LSS_CONV_EINVAL for such pointers, which
    was a RuntimeError in the middle of training where F.interpolate would have worked; now a copy."""
    mk = lambda: [T((1, 16, 5, 7), fmt="cl"), T((1, 8, 10, 14), fmt="cl", seed=1)]  # noqa: E731
    check_unaligned(launched, lambda x, s: R.upsample_cat(x, s, 2), [], mk, ["lss_upsample_cat_fwd2", "lss_upsample_bwd2"])


# ---------------------------------------------------------------------------------------- squeeze_excite
def _se_convs(C, sq, bias=(True, True)):
    torch.manual_seed(C + sq)
    return [nn.Conv2d(C, sq, 1, bias=bias[0]).to(DEV), nn.Conv2d(sq, C, 1, bias=bias[1]).to(DEV)]


def _se_op(red, exp, x):
    return E.squeeze_excite(x, red, exp)


def _se_stock(red, exp, x):
    s = F.adaptive_avg_pool2d(x, 1)
    s = exp(F.silu(red(s)))
    return torch.sigmoid(s) * x


SE_MISS = {  # convs, x
    "hw_6": (lambda: _se_convs(8, 2), lambda: [T((2, 8, 2, 3))]),
    "fp32_x": (lambda: _se_convs(8, 2), lambda: [T((2, 8, 2, 4), F32)]),
    "nhwc_x": (lambda: _se_convs(8, 2), lambda: [T((2, 8, 2, 4), fmt="cl")]),
    "reduce_without_bias": (lambda: _se_convs(8, 2, (False, True)), lambda: [T((2, 8, 2, 4))]),
    "expand_without_bias": (lambda: _se_convs(8, 2, (True, False)), lambda: [T((2, 8, 2, 4))]),
    "sq_65": (lambda: _se_convs(8, 65), lambda: [T((2, 8, 2, 4))]),
    "c_2056": (lambda: _se_convs(2056, 2), lambda: [T((1, 2056, 2, 2))]),
}


@pytest.mark.parametrize("case", sorted(SE_MISS))
def test_squeeze_excite_falls_back(case, launched):
    mk_mods, mk_in = SE_MISS[case]
    check_fallback(launched, _se_op, _se_stock, mk_mods(), mk_in, banned="lss_se", ctx=bf16_autocast, loose=("weight", "bias"))


def test_squeeze_excite_unaligned_views(launched):
    check_unaligned(launched, _se_op, _se_convs(8, 2), lambda: [T((2, 8, 2, 4))], ["lss_se_fwd", "lss_se_bwd", "lss_se_wgrad"],
                    tol_keys=("weight", "bias"))


def test_squeeze_excite_batch_slice_stays_on_the_kernels(launched):
    convs = _se_convs(8, 2)
    launched.clear()
    got = _run(lambda r, e, base: E.squeeze_excite(base[1:], r, e), copy.deepcopy(convs), [T((3, 8, 2, 4))])
    assert launched == ["lss_se_fwd", "lss_se_bwd", "lss_se_wgrad"]
    want = _run(lambda r, e, base: E.squeeze_excite(base[1:].clone(), r, e), copy.deepcopy(convs), [T((3, 8, 2, 4))])
    for k in ("y", "d_in0"):
        assert torch.equal(got[k], want[k]), k
    # fp64 on the bf16-rounded weights, test_squeeze_excite_vs_fp64's tolerances
    ref_convs = [copy.deepcopy(c).to(BF16).double().cpu() for c in convs]
    ref = _run(lambda r, e, base: _se_stock(r, e, base[1:]), ref_convs,
               [T((3, 8, 2, 4)).detach().double().cpu().requires_grad_(True)])
    torch.testing.assert_close(got["y"].double().cpu(), ref["y"], rtol=2e-2, atol=3e-2)
    for k in got:
        if k.startswith("d_"):
            rel = _err(got[k], ref[k]) / max(float(ref[k].abs().max()), 1e-12)
            assert rel < (2e-2 if k == "d_in0" else 5e-2), (k, rel)


# ---------------------------------------------------------------------------------------- pointwise_conv
def _pw(bias=False, stride=1):
    torch.manual_seed(3)
    return nn.Conv2d(8, 16, 1, stride=stride, bias=bias).to(DEV)


PW_MISS = {  # conv, x, autocast
    "hw_9": (_pw, lambda: [T((2, 8, 3, 3))], bf16_autocast),
    "fp16_autocast": (_pw, lambda: [T((2, 8, 2, 4), F32)], fp16_autocast),
    "fp32_no_autocast": (_pw, lambda: [T((2, 8, 2, 4), F32)], None),
    "bias": (lambda: _pw(bias=True), lambda: [T((2, 8, 2, 4))], bf16_autocast),
    "stride_2": (lambda: _pw(stride=2), lambda: [T((2, 8, 4, 4))], bf16_autocast),
}


@pytest.mark.parametrize("case", sorted(PW_MISS))
def test_pointwise_conv_falls_back(case, launched):
    mk_conv, mk_in, ctx = PW_MISS[case]
    check_fallback(launched, E.pointwise_conv, lambda c, x: c(x), [mk_conv()], mk_in, banned="lss_pw", ctx=ctx,
                   loose=("weight", "bias", "d_in0"))


def test_pointwise_conv_unaligned_views(launched):
    """(lss_pw_wrw reads the saved activations in 8-B vectors and refuses other pointers: an unaligned x took
    the framework forward and then failed in the backward.)"""
    check_unaligned(launched, E.pointwise_conv, [_pw()], lambda: [T((2, 8, 2, 4))], ["lss_pw_conv", "lss_pw_wrw"],
                    ctx=bf16_autocast)


# ------------------------------------------------------------------------- conv1x1 / bn_relu_head1
def _head(C, out=1):
    torch.manual_seed(4)
    return nn.Conv2d(C, out, 1).to(DEV)


def _linear_1x1(conv, x):
    """models.conv1x1 off the lss_head1 kernels: the GEMM over channels-last pixels it documents."""
    w = conv.weight.reshape(conv.out_channels, conv.in_channels)
    return F.linear(x.permute(0, 2, 3, 1), w, conv.bias).permute(0, 3, 1, 2)


HEAD_MISS = {  # head, x, autocast
    "c_12": (lambda: _head(12), lambda: [T((2, 12, 3, 5), fmt="cl")], bf16_autocast),
    "c_24": (lambda: _head(24), lambda: [T((2, 24, 3, 5), fmt="cl")], bf16_autocast),  # 64 % (C / 8) != 0
    "nchw": (lambda: _head(16), lambda: [T((2, 16, 3, 5))], bf16_autocast),
    "two_outputs": (lambda: _head(16, 2), lambda: [T((2, 16, 3, 5), fmt="cl")], bf16_autocast),
    "fp32_no_autocast": (lambda: _head(16), lambda: [T((2, 16, 3, 5), F32, "cl")], None),
}


@pytest.mark.parametrize("case", sorted(HEAD_MISS))
def test_conv1x1_falls_back(case, launched):
    mk_head, mk_in, ctx = HEAD_MISS[case]
    check_fallback(launched, M.conv1x1, _linear_1x1, [mk_head()], mk_in, banned="lss_head1", ctx=ctx,
                   loose=("weight", "bias"))


@pytest.mark.parametrize("case", sorted(HEAD_MISS))
def test_bn_relu_head1_falls_back(case, launched):
    """Off the fused tail, bn_relu_head1 is conv1x1(bn_act(x)): no lss_head1 launch, the batch norm on its
    own kernels where it is eligible (bit-identical to bn_act alone by construction)."""
    mk_head, mk_in, ctx = HEAD_MISS[case]
    head = mk_head()
    bn = _bn(head.in_channels)
    check_fallback(launched, lambda b, h, x: M.bn_relu_head1(b, h, x), lambda b, h, x: _linear_1x1(h, Nm.bn_act(b, x, "relu")),
                   [bn, head], mk_in, banned="lss_head1", ctx=ctx, loose=("m1.weight", "m1.bias"))


def test_bn_relu_head1_with_a_bf16_batch_norm(launched):
    """model.to(bfloat16): the batch norm's parameters are bf16 arrays, which lss_bn_fwd2 would read as fp32
    (twice their size). The batch norm runs stock nn.BatchNorm2d -- its statistics and its gradients, in
    bf16, are the stock module's bit for bit -- and only the head stays on lss_head1_*."""
    bn, head = _bn(16, BF16), _head(16).to(BF16)
    mk = lambda: [T((2, 16, 3, 5), fmt="cl")]  # noqa: E731
    launched.clear()
    got = _run(lambda b, h, x: M.bn_relu_head1(b, h, x), [copy.deepcopy(bn), copy.deepcopy(head)], mk())
    assert not [k for k in launched if k.startswith("lss_bn")] and "lss_head1_fwd" in launched, launched
    want = _run(lambda b, h, x: h(F.relu(b(x))), [copy.deepcopy(bn), copy.deepcopy(head)], mk())
    for k in ("m0.running_mean", "m0.running_var", "m0.num_batches_tracked"):
        assert torch.equal(got[k], want[k]), k
    for k in got:  # a 16-term dot product per pixel in fp32, rounded to bf16 once: a few bf16 ulps
        if k.startswith("d_") or k == "y":
            assert got[k].dtype == BF16 and got[k].shape == want[k].shape, k
            torch.testing.assert_close(got[k].float(), want[k].float(), rtol=2e-2, atol=3e-2)


def test_head1_unaligned_views(launched):
    """The head shape (2, 64, 7, 9), channels-last rows read as uint4: conv1x1 and the fused BN + ReLU + head."""
    mk = lambda: [T((2, 64, 7, 9), fmt="cl")]  # noqa: E731
    check_unaligned(launched, M.conv1x1, [_head(64)], mk, ["lss_head1_fwd", "lss_head1_bwd"])
    check_unaligned(launched, lambda b, h, x: M.bn_relu_head1(b, h, x), [_bn(64), _head(64)], mk,
                    ["lss_bn_fwd2", "lss_head1_fwd2", "lss_head1_bwd2", "lss_bn_bwd_rank1"])


# ------------------------------------------------------------------------------- MBConvBlock depthwise
def _block(K, stride, expand, dtype=F32, impl="hip"):
    torch.manual_seed(5)
    blk = E.MBConvBlock(K, stride, expand, 8, 8, image_size=(6, 8)).to(DEV, dtype).train()
    blk.depthwise_impl = impl
    return blk


@pytest.mark.parametrize("dtype", [F64, F16])
def test_mbconv_depthwise_falls_back_for_fp64_and_fp16(dtype, launched):
    """_HipDepthwise computed fp64 / fp16 callers in fp32 and returned fp32 maps and gradients; such blocks now
    take the module's own conv (the 'miopen' branch), dtypes in = dtypes out."""
    blk = _block(3, 1, 2, dtype)

    def stock(m, x):
        m.depthwise_impl = "miopen"
        return m(x)
    got = check_fallback(launched, lambda m, x: m(x), stock, [blk], lambda: [T((2, 8, 6, 8), dtype)],
                         loose=("weight", "bias", "d_in0"))
    assert all(v.dtype == dtype for k, v in got.items() if k == "y" or k.startswith("d_"))


@pytest.mark.parametrize("K,stride", [(3, 1), (5, 2)])
def test_mbconv_depthwise_unaligned_views(K, stride, launched):
    """The depthwise branch (expand ratio 1: the block's input is the depthwise conv's) under bf16 autocast."""
    check_unaligned(launched, lambda m, x: m(x), [_block(K, stride, 1)], lambda: [T((2, 8, 6, 8))],
                    ["lss_dwconv_fwd", "lss_dwconv_bwd_data", "lss_dwconv_bwd_weight2"], ctx=bf16_autocast,
                    tol_keys=("_se_",))


# ---------------------------------------------------------------------------- drop_connect_add, dropout
DROP_MISS = {
    "fp32": lambda: [T((2, 8, 2, 4), F32), T((2, 8, 2, 4), F32, seed=1)],
    "mixed_formats": lambda: [T((2, 8, 2, 4), fmt="cl"), T((2, 8, 2, 4), seed=1)],
    "per_sample_12": lambda: [T((2, 3, 2, 2)), T((2, 3, 2, 2), seed=1)],
    "unaligned_x": lambda: [_off16(T((2, 8, 2, 4))), T((2, 8, 2, 4), seed=1)],
    "unaligned_inputs": lambda: [T((2, 8, 2, 4)), _off16(T((2, 8, 2, 4), seed=1))],
}


@pytest.mark.parametrize("case", sorted(DROP_MISS))
def test_drop_connect_add_falls_back(case, launched):
    check_fallback(launched, lambda x, r: E.drop_connect_add(x, r, 0.2, True), lambda x, r: E.drop_connect(x, 0.2, True) + r,
                   [], DROP_MISS[case], banned="lss_scale_add", seed=7)


def test_drop_connect_add_eligible_launches(launched):
    _run(lambda x, r: E.drop_connect_add(x, r, 0.2, True), [], [T((2, 8, 2, 4)), T((2, 8, 2, 4), seed=1)])
    assert launched == ["lss_scale_add", "lss_scale_add"]


@pytest.mark.parametrize("case", ["fp16", "p0", "p1", "eval", "unaligned", "bytes_12"])
def test_lss_dropout_falls_back(case, launched):
    p = {"p0": 0.0, "p1": 1.0}.get(case, 0.2)
    d = M.LssDropout(p).train(case != "eval")
    stock = nn.Dropout(p).train(case != "eval")

    def mk():
        x = T((2, 3, 1, 1) if case == "bytes_12" else (2, 8, 2, 4), F16 if case == "fp16" else BF16)
        return [_off16(x) if case == "unaligned" else x]
    check_fallback(launched, lambda x: d(x), lambda x: stock(x), [], mk, banned="lss_dropout", seed=7)


def test_lss_dropout_eligible_launches(launched):
    _run(lambda x: M.LssDropout(0.2).train()(x), [], [T((2, 8, 2, 4))])
    assert launched == ["lss_dropout", "lss_dropout"]
