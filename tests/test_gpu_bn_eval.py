"""Eval-mode batch norm on the HIP kernels (lss_bn_eval, lss_bn_eval_coef; ABI 28): inference as
src/explore.py:244-246, 317-328 runs the network -- model.eval(), no_grad.

* every vector width, layout and grid regime of lss_bn_eval against fp64, over act x residual x dtype, through
  the C ABI into a NaN-filled output, and norm.bn_act giving the same bits;
* the module's buffers and parameters untouched; the dispatch guards (norm.eval_eligible); sample independence
  (what partial batches rest on); unaligned views and the entry point's alignment check;
* BevEncode's eval tail (models.bn_relu_head1) without the normalised map, bit-identical to the unfused
  sequence; the MBConv identity skip inside bn2's pass; the whole model against its fp32 stock forward.

Tolerances are tests/test_gpu_convs.py::test_bn_act_vs_fp64's: fp32 rtol 1e-4 / atol 1e-4, bf16 rtol 2e-2 /
atol 3e-2 (one bf16 rounding of a value of a few units is 2^-9 relative)."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import _lib, efficientnet as E, models as M, norm as Nm  # noqa: E402
from lss_carla_amd import synthetic as syn  # noqa: E402

DEV = torch.device("cuda:0")
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
CL = torch.channels_last
TOL = {F32: dict(rtol=1e-4, atol=1e-4), BF16: dict(rtol=2e-2, atol=3e-2)}
ACTS = ("none", "relu", "swish")


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


def randomise(bn: nn.BatchNorm2d, seed: int) -> None:
    g = torch.Generator(device="cpu").manual_seed(seed)
    C = bn.num_features
    with torch.no_grad():
        if bn.affine:
            bn.weight.copy_(torch.empty(C).uniform_(0.5, 1.5, generator=g))
            bn.bias.copy_(torch.empty(C).normal_(0, 0.1, generator=g))
        if bn.track_running_stats:
            bn.running_mean.copy_(torch.empty(C).normal_(0, 1, generator=g))
            bn.running_var.copy_(torch.empty(C).uniform_(0.5, 1.5, generator=g))


def _bn(C, **kw):
    bn = nn.BatchNorm2d(C, eps=1e-3, momentum=0.1, **kw).to(DEV)
    randomise(bn, C)
    return bn.eval()


def _act(z, act):
    return {"none": z, "relu": F.relu(z), "swish": z * torch.sigmoid(z)}[act]


# (layout, shape): V = 1 | V = 8 bf16, 4 fp32 | bf16 V = 4 | C % 8 != 0 | several chunks per channel |
# NHWC 2 and 32 channel groups per row | NHWC many blocks | and, for the grid the kernels actually use (at most
# 1,024 blocks): NCHW with more (channel, chunk) units than blocks, so blocks stride over units; NHWC with more
# rows than 1,024 blocks take in one iteration (135,200 rows of 8 octets: 132 or 133 rows per block, 128 per iteration)
CASES = [("nchw", (2, 16, 5, 7)), ("nchw", (2, 8, 4, 6)), ("nchw", (2, 8, 2, 6)), ("nchw", (3, 40, 4, 11)),
         ("nchw", (3, 32, 64, 176)), ("nhwc", (2, 16, 3, 5)), ("nhwc", (2, 256, 5, 5)), ("nhwc", (3, 64, 100, 100)),
         ("nchw", (2, 1040, 4, 6)), ("nhwc", (2, 64, 260, 260))]


@functools.lru_cache(maxsize=None)
def _inputs(layout, shape, dtype):
    """(x, residual, bn, {(act, with_res): fp64 reference}) of one case, made once and left unchanged."""
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g).to(DEV, dtype)
    r = torch.randn(*shape, generator=g).to(DEV, dtype)
    if layout == "nhwc":
        x, r = x.contiguous(memory_format=CL), r.contiguous(memory_format=CL)
    bn = _bn(shape[1])
    v = lambda t: t.double().view(1, -1, 1, 1)  # noqa: E731
    z = (x.double() - v(bn.running_mean)) / torch.sqrt(v(bn.running_var) + bn.eps) * v(bn.weight) + v(bn.bias)
    want = {(a, wr): _act(z + r.double() if wr else z, a) for a in ACTS for wr in (False, True)}
    return x, r, bn, want


def _call(x, r, bn, act, y, layout):
    N, C, H, W = x.shape
    return _lib.load().lss_bn_eval(_lib.ptr(x), _lib.ptr(r), _lib.dtype_code(x.dtype),
                                   _lib.NHWC if layout == "nhwc" else _lib.NCHW, N, C, H * W, _lib.ptr(bn.weight),
                                   _lib.ptr(bn.bias), _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var),
                                   float(bn.eps), Nm.ACT[act], _lib.ptr(y), _lib.stream_handle(DEV))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("layout,shape", CASES, ids=[f"{l}-{'x'.join(map(str, s))}" for l, s in CASES])
def test_bn_eval_vs_fp64(layout, shape, act, with_res, dtype):
    x, r, bn, want = _inputs(layout, shape, dtype)
    res = r if with_res else None
    y = torch.full_like(x, float("nan"))
    assert _call(x, res, bn, act, y, layout) == 0
    assert not torch.isnan(y).any(), "an element the kernel did not write"
    torch.testing.assert_close(y.double(), want[(act, with_res)], **TOL[dtype])
    with torch.no_grad():
        got = Nm.bn_act(bn, x, act, res)
    assert got.dtype == dtype and got.stride() == x.stride() and torch.equal(got, y)


def test_entry_point_rejects_bad_arguments():
    x, r, bn, _ = _inputs("nchw", (2, 8, 4, 6), BF16)
    y = torch.empty_like(x)
    lib = _lib.load()
    args = lambda **kw: [kw.get("x", _lib.ptr(x)), None, kw.get("dtype", _lib.BF16), kw.get("layout", _lib.NCHW), 2,  # noqa: E731
                         kw.get("C", 8), 24, _lib.ptr(bn.weight), _lib.ptr(bn.bias),
                         kw.get("rm", _lib.ptr(bn.running_mean)), _lib.ptr(bn.running_var), 1e-3, kw.get("act", 1),
                         kw.get("y", _lib.ptr(y)), _lib.stream_handle(DEV)]
    assert lib.lss_bn_eval(*args()) == 0
    for bad in (dict(x=None), dict(y=None), dict(rm=None), dict(dtype=2), dict(layout=2), dict(act=3), dict(C=0),
                dict(layout=_lib.NHWC, C=24)):
        assert lib.lss_bn_eval(*args(**bad)) == -1, bad
    st = torch.empty(4, 8, device=DEV)
    coef = lambda **kw: [_lib.ptr(bn.weight), _lib.ptr(bn.bias), _lib.ptr(bn.running_mean),  # noqa: E731
                         kw.get("rv", _lib.ptr(bn.running_var)), 1e-3, kw.get("C", 8), kw.get("st", _lib.ptr(st)),
                         _lib.stream_handle(DEV)]
    assert lib.lss_bn_eval_coef(*coef()) == 0
    for bad in (dict(rv=None), dict(st=None), dict(C=0), dict(st=st.data_ptr() + 2)):
        assert lib.lss_bn_eval_coef(*coef(**bad)) == -1, bad
    torch.cuda.synchronize()
    rstd = torch.rsqrt(bn.running_var.double() + 1e-3)
    scale = bn.weight.double() * rstd
    want = torch.stack([bn.running_mean.double(), rstd, scale, bn.bias.double() - bn.running_mean.double() * scale])
    torch.testing.assert_close(st.double(), want, rtol=1e-5, atol=1e-6)
    assert torch.equal(st[0], bn.running_mean)


def test_buffers_and_parameters_unchanged(launched):
    bn = _bn(16)
    before = copy.deepcopy(bn.state_dict())
    x = torch.randn(2, 16, 5, 7, device=DEV)
    with torch.no_grad():
        Nm.bn_act(bn, x, "swish", x)
        Nm.bn_act(bn, x.to(BF16).contiguous(memory_format=CL), "relu")
    torch.cuda.synchronize()
    assert launched == ["lss_bn_eval", "lss_bn_eval"]
    after = bn.state_dict()
    assert set(after) == {"weight", "bias", "running_mean", "running_var", "num_batches_tracked"}
    for k, v in before.items():
        assert torch.equal(v, after[k]), k


# ------------------------------------------------------------------------------------------------ dispatch
def test_eval_without_gradients_takes_the_eval_kernel_and_training_the_training_one(launched):
    bn = _bn(8)
    x = torch.randn(2, 8, 4, 6, device=DEV)
    with torch.no_grad():
        y = Nm.bn_act(bn, x, "relu")
    assert launched == ["lss_bn_eval"] and not y.requires_grad
    launched.clear()
    y2 = Nm.bn_act(bn, x.clone(), "relu")  # grad mode on, nothing requires grad ... but gamma / beta do
    assert launched == [] and y2.requires_grad
    bn.requires_grad_(False)
    y3 = Nm.bn_act(bn, x, "relu")  # grad mode on, no tensor wants a gradient
    assert launched == ["lss_bn_eval"] and torch.equal(y3, y)
    launched.clear()
    bn.requires_grad_(True).train()
    Nm.bn_act(bn, x, "relu")
    assert launched == ["lss_bn_fwd2"]


FALLBACK = {
    "nhwc_c24": (lambda: _bn(24), lambda: torch.randn(2, 24, 3, 5, device=DEV).contiguous(memory_format=CL), {}),
    "bf16_module": (lambda: _bn(8).to(BF16), lambda: torch.randn(2, 8, 4, 6, device=DEV, dtype=BF16), {}),
    "affine_false": (lambda: _bn(8, affine=False), lambda: torch.randn(2, 8, 4, 6, device=DEV), {}),
    "no_running_stats": (lambda: _bn(8, track_running_stats=False), lambda: torch.randn(2, 8, 4, 6, device=DEV), {}),
    "switch_eval_off": (lambda: _bn(8), lambda: torch.randn(2, 8, 4, 6, device=DEV), {"USE_HIP_BN_EVAL": False}),
    "switch_bn_off": (lambda: _bn(8), lambda: torch.randn(2, 8, 4, 6, device=DEV), {"USE_HIP_BN": False}),
}


@pytest.mark.parametrize("case", sorted(FALLBACK))
def test_ineligible_cases_stay_on_the_stock_op(case, launched, monkeypatch):
    mk_bn, mk_x, switches = FALLBACK[case]
    for k, v in switches.items():
        monkeypatch.setattr(Nm, k, v)
    bn, x = mk_bn(), mk_x()
    with torch.no_grad():
        got = Nm.bn_act(bn, x, "swish", x)
        want = F.silu(bn(x) + x)
    assert not [w for w in launched if w.startswith("lss_bn")], launched
    assert torch.equal(got, want)


@pytest.mark.parametrize("fmt", ["nchw", "nhwc"])
def test_sample_independence(fmt):
    """bn_act(bn, x[:1]) == bn_act(bn, x)[:1] bit for bit: no op across samples in eval mode."""
    bn = _bn(16)
    x = torch.randn(3, 16, 6, 8, device=DEV).to(BF16)
    if fmt == "nhwc":
        x = x.contiguous(memory_format=CL)
    with torch.no_grad():
        full = Nm.bn_act(bn, x, "swish", x)
        one = Nm.bn_act(bn, x[:1], "swish", x[:1])
    assert torch.equal(one, full[:1])


# ------------------------------------------------------------------------------------------------ alignment
def _shifted(t):
    """The same values and strides at a storage offset of one element."""
    fmt = CL if (not t.is_contiguous() and t.is_contiguous(memory_format=CL)) else torch.contiguous_format
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].as_strided(t.shape, t.stride())
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous(memory_format=fmt)
    return v


@pytest.mark.parametrize("which", ["x", "residual"])
@pytest.mark.parametrize("dtype,shape,fmt", [(BF16, (2, 8, 4, 6), "nchw"), (BF16, (2, 8, 2, 6), "nchw"),
                                             (F32, (2, 8, 4, 6), "nchw"), (BF16, (2, 16, 3, 5), "nhwc")])
def test_unaligned_views_give_the_aligned_bits(dtype, shape, fmt, which, launched):
    x, r, bn, _ = _inputs(fmt, shape, dtype)
    with torch.no_grad():
        want = Nm.bn_act(bn, x, "relu", r)
        got = Nm.bn_act(bn, _shifted(x) if which == "x" else x, "relu", _shifted(r) if which == "residual" else r)
    assert launched == ["lss_bn_eval", "lss_bn_eval"] and torch.equal(got, want)


def test_entry_point_refuses_a_real_unaligned_pointer():
    """The C-ABI backstop on real memory: the call that succeeds on a tensor is LSS_CONV_EINVAL two bytes on."""
    lib = _lib.load()
    x = torch.randn(2 * 8 * 24 + 8, device=DEV).to(BF16)  # room for the shifted read
    y = torch.empty(2 * 8 * 24 + 8, device=DEV, dtype=BF16)
    bn = _bn(8)
    for xo, ro, yo, want in ((0, None, 0, 0), (2, None, 0, -1), (8, None, 0, -1), (0, 2, 0, -1), (0, None, 2, -1),
                             (0, 0, 0, 0)):
        code = lib.lss_bn_eval(x.data_ptr() + xo, None if ro is None else x.data_ptr() + ro, _lib.BF16, _lib.NCHW, 2, 8,
                               24, _lib.ptr(bn.weight), _lib.ptr(bn.bias), _lib.ptr(bn.running_mean),
                               _lib.ptr(bn.running_var), 1e-3, 1, y.data_ptr() + yo, _lib.stream_handle(DEV))
        assert code == want, (xo, ro, yo, code)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ eval tail
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("shape", [(2, 16, 3, 5), (1, 128, 10, 10)], ids=["2x16x3x5", "1x128x10x10"])
def test_eval_tail_is_the_unfused_sequence_without_the_map(shape, K, launched):
    bn = _bn(shape[1])
    torch.manual_seed(K)
    head = M.logits_head(nn.Conv2d(shape[1], K, 1)).to(DEV)
    x = torch.randn(*shape, device=DEV).to(BF16).contiguous(memory_format=CL)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        got = M.bn_relu_head1(bn, head, x)
        assert launched == ["lss_bn_eval_coef", "lss_head1_fwd2" if K == 1 else "lss_headk_fwd"]
        launched.clear()
        want = M.conv1x1(head, Nm.bn_act(bn, x, "relu"))
        assert launched == ["lss_bn_eval", "lss_head1_fwd" if K == 1 else "lss_headk_fwd"]
    assert got.shape == (shape[0], K, shape[2], shape[3]) and got.dtype == BF16
    assert torch.equal(got, want)
    # with gradients wanted the tail stays where it was (stock BN in eval mode)
    launched.clear()
    with torch.autocast("cuda", dtype=BF16):
        M.bn_relu_head1(bn, head, x)
    assert "lss_bn_eval_coef" not in launched and "lss_bn_eval" not in launched


# ------------------------------------------------------------------------------------------------ MBConv skip
def test_mbconv_skip_rides_in_bn2(launched, monkeypatch):
    torch.manual_seed(3)
    blk = E.MBConvBlock(3, 1, 6, 24, 24, image_size=(8, 22)).to(DEV)
    for i, bn in enumerate((blk._bn0, blk._bn1, blk._bn2)):
        randomise(bn, 100 + i)
    blk.eval()
    x = torch.randn(2, 24, 8, 22, device=DEV).to(BF16)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        on = blk(x, drop_connect_rate=0.2)
        assert launched.count("lss_bn_eval") == 3, launched
        monkeypatch.setattr(Nm, "USE_HIP_BN_EVAL", False)
        launched.clear()
        off = blk(x, drop_connect_rate=0.2)
        assert not [w for w in launched if w.startswith("lss_bn")], launched
    assert on.shape == off.shape == x.shape and on.dtype == off.dtype
    torch.testing.assert_close(on.double(), off.double(), **TOL[BF16])
    # training mode is untouched: bn2 without a residual, then the drop-connect add
    blk.train()
    launched.clear()
    monkeypatch.setattr(Nm, "USE_HIP_BN_EVAL", True)
    with torch.autocast("cuda", dtype=BF16):
        blk(x, drop_connect_rate=0.2)
    assert launched.count("lss_bn_fwd2") == 3 and "lss_bn_eval" not in launched and "lss_scale_add" in launched


# ------------------------------------------------------------------------------------------------ whole model
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}


def test_whole_model_bf16_error_no_worse_than_the_stock_sequence(launched, monkeypatch):
    """e_on <= 2 e_off against the fp32 stock eval logits: the fused kernels round less often than BN, add,
    activation as three ops; the factor 2 covers two equally valid bf16 roundings diverging through ~70 layers."""
    old = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    try:
        torch.manual_seed(0)
        model = L.compile_model(GC, DAC, outC=1).to(DEV)
        model.bevencode.to(memory_format=CL)
        model.camencode.up1.to(memory_format=CL)
        for i, m in enumerate(m for m in model.modules() if isinstance(m, nn.BatchNorm2d)):
            randomise(m, 1000 + i)
        model.eval()
        B, N, fd = 2, 6, DAC["final_dim"]
        rig = syn.make_rig(B, N, fd, seed=0)
        inputs = (syn.make_images(B, N, fd, seed=0).to(DEV), *(rig[k].to(DEV) for k in
                                                               ("rots", "trans", "intrins", "post_rots", "post_trans")))
        with torch.no_grad():
            monkeypatch.setattr(Nm, "USE_HIP_BN_EVAL", False)
            ref = model(*inputs).double()
            with torch.autocast("cuda", dtype=BF16):
                off = model(*inputs).double()
            assert "lss_bn_eval" not in launched
            monkeypatch.setattr(Nm, "USE_HIP_BN_EVAL", True)
            launched.clear()
            with torch.autocast("cuda", dtype=BF16):
                on = model(*inputs).double()
        n_eval = launched.count("lss_bn_eval")
        e_off, e_on = (off - ref).abs().max().item(), (on - ref).abs().max().item()
        print(f"whole model, bf16 against fp32 stock eval logits (max |logit| {ref.abs().max().item():.4g}): "
              f"e_off {e_off:.6g}, e_on {e_on:.6g}; {n_eval} lss_bn_eval launches, tail "
              f"{'fused' if 'lss_bn_eval_coef' in launched else 'unfused'}")
        assert torch.isfinite(ref).all() and torch.isfinite(on).all()
        assert n_eval >= 60 and "lss_bn_eval_coef" in launched
        assert e_on <= 2 * e_off, (e_on, e_off)
    finally:
        torch.backends.cudnn.benchmark = old
