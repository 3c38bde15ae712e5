"""Every kernel-selection arm of lss_bn_fwd2 / lss_bn_bwd2 on the GPU, against a plain fp64 restatement of training
batch norm from the rounded inputs (tests/arm_cases.py's batch-norm section).

tests/test_host.py proves through the host-only query lss_bn_arm, which the launchers themselves switch on, that the
cases reach every arm, that the bars leave fp32 arithmetic 4x room and that they notice one left-out element. The
cases call the C ABI directly, so ngroups is the case's choice and the shapes stay tiny. Every output buffer starts
as NaN and is compared whole. The backward is handed the REFERENCE's output (rounded) and statistics, not the
forward kernel's, so a forward bug cannot hide a backward one.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import ctypes  # noqa: E402

import arm_cases as A  # noqa: E402
from lss_carla_amd import _lib, norm as Nm  # noqa: E402
from test_gpu_dispatch_arms import DEV, _DT, _nan, _within  # noqa: E402

_CODE = {A.F32: _lib.F32, A.BF16: _lib.BF16}
_WORKSPACE = []


def _sync_words() -> torch.Tensor:
    """The tests' own sync workspace: zero-filled once, left zero-filled by every call (asserted)."""
    if not _WORKSPACE:
        _WORKSPACE.append(torch.zeros(int(_lib.load().lss_bn_sync_words()), device=DEV, dtype=torch.int32))
    return _WORKSPACE[0]


@functools.lru_cache(maxsize=None)
def _reference(case, dtype, combo):
    """(inputs, fp64 reference) of one case: made once, shared by the forward and the backward test, left unchanged."""
    ins = A.bn_inputs(case, dtype, combo)
    return ins, A.bn_reference(ins, combo, dtype)


def _to_dev(a: np.ndarray, case, dtype) -> torch.Tensor:
    """A (C, N * HW) array as the case's tensor: (N, C, HW) for NCHW, (N * HW, C) for NHWC."""
    if case.layout == 1:
        a = a.T
    else:
        a = a.reshape(case.C, case.N, -1).transpose(1, 0, 2)
    return A.rounded(np.ascontiguousarray(a), dtype).to(DEV)


def _to_cm(t: torch.Tensor, case) -> torch.Tensor:
    """The inverse of _to_dev, still a tensor (for _within)."""
    if case.layout == 1:
        return t.reshape(-1, case.C).T
    return t.reshape(case.N, case.C, -1).permute(1, 0, 2).reshape(case.C, -1)


def _f32(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _arm(pas, case, dtype, act) -> str:
    a = _lib.BnArm()
    assert _lib.load().lss_bn_arm(pas, _CODE[dtype], case.layout, case.N, case.C, case.H * case.W, A.ACT[act], case.G,
                                  int(case.sync), ctypes.byref(a)) == 0
    return A.bn_arm_name(a.family, a.v, a.it, a.relu)


def _params(pas):
    out = []
    for case in A.BN_CASES:
        for dtype in (A.F32, A.BF16):
            for combo in A.bn_combos(case, pas):
                name = "%s-%s-%s-%s%s%s" % (A.bn_case_arm(case, dtype, pas, combo.act), _DT[dtype], A.bn_id(case),
                                            combo.act, "+res" if combo.res else "", "-ynull" if combo.y == "null" else "")
                out.append(pytest.param(case, dtype, combo, id=name))
    return out


def _forward(case, dtype, combo, running=True):
    lib = _lib.load()
    ins, ref = _reference(case, dtype, combo)
    C, G = case.C, case.G
    x = _to_dev(ins["x"], case, dtype)
    res = _to_dev(ins["res"], case, dtype) if combo.res else None
    y = None if combo.y == "null" else _nan(x.shape, dtype)
    gamma, beta = _f32(ins["gamma"]), _f32(ins["beta"])
    rm, rv = (_f32(ins["rm"]), _f32(ins["rv"])) if running else (None, None)
    count = torch.full((1,), 7, device=DEV, dtype=torch.int64) if running else None
    partial, stats = _nan((C, G, 2), torch.float32), _nan((4, C), torch.float32)
    sync = _sync_words() if case.sync else None
    _lib.check(lib.lss_bn_fwd2(_lib.ptr(x), _lib.ptr(res), _CODE[dtype], case.layout, case.N, C, case.H * case.W,
                               _lib.ptr(gamma), _lib.ptr(beta), A.BN_EPS, A.BN_MOM, _lib.ptr(rm), _lib.ptr(rv),
                               _lib.ptr(count), A.ACT[combo.act], G, _lib.ptr(partial), _lib.ptr(stats[0]),
                               _lib.ptr(stats[1]), _lib.ptr(stats[2]), _lib.ptr(stats[3]), _lib.ptr(y), _lib.ptr(sync),
                               _lib.stream_handle(DEV)), "lss_bn_fwd2")
    torch.cuda.synchronize()
    if sync is not None:
        assert int(sync.abs().sum()) == 0, "cluster counters not re-zeroed"
    return ins, ref, y, stats, rm, rv, count


def _check_forward(case, dtype, combo, arm, running=True):
    ins, ref, y, stats, rm, rv, count = _forward(case, dtype, combo, running)
    bars = A.bn_fwd_bars(ref, ins)
    for row, name in enumerate(("mean", "rstd", "scale", "shift")):
        _within(stats[row], ref[name], bars[name], "%s: saved %s" % (arm, name))
    if running:
        _within(rm, ref["run_mean"], bars["run_mean"], arm + ": running mean")
        _within(rv, ref["run_var"], bars["run_var"], arm + ": running var")
        assert int(count) == 8
    if y is not None:
        _within(_to_cm(y, case), ref["y"], A.bn_map_bar(ref["y"], dtype), arm + ": y")


def _check_backward(case, dtype, combo, arm, sums=True):
    lib = _lib.load()
    ins, ref = _reference(case, dtype, combo)
    C, G = case.C, case.G
    x, dy = _to_dev(ins["x"], case, dtype), _to_dev(ins["dy"], case, dtype)
    y = _to_dev(ref["y_in"], case, dtype) if combo.act == "relu" and combo.y == "y" else None
    stats = _f32(ref["stats_in"])
    partial, coef = _nan((C, G, 2), torch.float32), _nan((C, 2), torch.float32)
    dgamma, dbeta = (_nan((C,), torch.float32), _nan((C,), torch.float32)) if sums else (None, None)
    dx = _nan(x.shape, dtype)
    dres = _nan(x.shape, dtype) if combo.res else None
    sync = _sync_words() if case.sync else None
    _lib.check(lib.lss_bn_bwd2(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(y), _CODE[dtype], case.layout, case.N, C,
                               case.H * case.W, _lib.ptr(stats[2]), _lib.ptr(stats[3]), _lib.ptr(stats[0]),
                               _lib.ptr(stats[1]), A.ACT[combo.act], G, _lib.ptr(partial), _lib.ptr(coef),
                               _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(dx), _lib.ptr(dres), _lib.ptr(sync),
                               _lib.stream_handle(DEV)), "lss_bn_bwd2")
    torch.cuda.synchronize()
    if sync is not None:
        assert int(sync.abs().sum()) == 0, "cluster counters not re-zeroed"
    bars = A.bn_bwd_bars(ref, ins, combo)
    if sums:
        _within(dbeta, ref["dbeta"], bars["dbeta"], arm + ": dbeta")
        _within(dgamma, ref["dgamma"], bars["dgamma"], arm + ": dgamma")
    near = A.bn_near_zero(ref, combo)  # (the recomputing ReLU arm alone: test_host.py caps their number)
    _within(_to_cm(dx, case), ref["dx"], np.where(near, np.inf, A.bn_map_bar(ref["dx"], dtype)), arm + ": dx")
    if dres is not None:
        _within(_to_cm(dres, case), ref["dres"], A.bn_map_bar(ref["dres"], dtype), arm + ": dresidual")


@pytest.mark.parametrize("case,dtype,combo", _params(A.BN_FWD))
def test_bn_fwd_arm(case, dtype, combo):
    arm = _arm(A.BN_FWD, case, dtype, combo.act)
    assert arm == A.bn_case_arm(case, dtype, A.BN_FWD, combo.act)
    _check_forward(case, dtype, combo, arm)


@pytest.mark.parametrize("case,dtype,combo", _params(A.BN_BWD))
def test_bn_bwd_arm(case, dtype, combo):
    arm = _arm(A.BN_BWD, case, dtype, combo.act)
    assert arm == A.bn_case_arm(case, dtype, A.BN_BWD, combo.act)
    _check_backward(case, dtype, combo, arm)


# one case per family for the nullable arguments: no running statistics and no counter; no dgamma / dbeta
# (residual and dresidual NULL: every combination without a residual above)
_NULLABLE = [next(c for c in A.BN_CASES if c.bf16.startswith(f) and c.N * c.H * c.W > 256)
             for f in ("nhwc", "cluster<8,6", "cluster<8,8", "fused_reg", "fused<", "two_pass")]


@pytest.mark.parametrize("case", _NULLABLE, ids=lambda c: c.bf16 + "-" + A.bn_id(c))
def test_bn_arm_nullable_arguments(case):
    combo = A.BnCombo("relu", True, "y")
    _check_forward(case, A.BF16, combo, case.bf16 + " without running statistics", running=False)
    _check_backward(case, A.BF16, combo, A.bn_case_arm(case, A.BF16, A.BN_BWD, "relu") + " without dgamma / dbeta",
                    sums=False)


# ----------------------------------------------------------------------------- through norm.bn_act
@pytest.fixture
def launched(monkeypatch):
    seen = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (seen.append(what), real(code, what))[1])
    return seen


def _module(case, ins):
    bn = torch.nn.BatchNorm2d(case.C, eps=A.BN_EPS, momentum=A.BN_MOM).to(DEV).train()
    with torch.no_grad():
        for t, k in ((bn.weight, "gamma"), (bn.bias, "beta"), (bn.running_mean, "rm"), (bn.running_var, "rv")):
            t.copy_(_f32(ins[k]))
    return bn


_PY = [pytest.param(c, dt, id="%s-%s-%s" % (A.bn_case_arm(c, dt, A.BN_FWD), _DT[dt], A.bn_id(c)))
       for c in A.BN_CASES if c.py for dt in (A.F32, A.BF16)]


@pytest.mark.parametrize("case,dtype", _PY)
def test_bn_act_takes_the_arm_with_the_groups_lss_bn_groups_picks(case, dtype, launched):
    """The same cases through norm.bn_act (its own ngroups, workspace and saved tensors): same reference, same
    bars; the backward here reads the forward kernel's own output and statistics."""
    assert _lib.load().lss_bn_groups(case.N, case.C, case.H * case.W, case.layout) == case.G
    for combo in A.BN_COMBOS_NCHW:
        ins, ref = _reference(case, dtype, combo)
        bn = _module(case, ins)
        shape = (case.N, case.C, case.H, case.W)
        x = _to_dev(ins["x"], case, dtype).reshape(shape).requires_grad_(True)
        res = _to_dev(ins["res"], case, dtype).reshape(shape).requires_grad_(True) if combo.res else None
        del launched[:]
        y = Nm.bn_act(bn, x, combo.act, res)
        y.backward(_to_dev(ins["dy"], case, dtype).reshape(shape))
        torch.cuda.synchronize()
        assert launched == ["lss_bn_fwd2", "lss_bn_bwd2"]
        fb, bb = A.bn_fwd_bars(ref, ins), A.bn_bwd_bars(ref, ins, combo)
        what = A.bn_case_arm(case, dtype, A.BN_FWD) + " " + combo.act
        _within(_to_cm(y.detach(), case), ref["y"], A.bn_map_bar(ref["y"], dtype), what + ": y")
        _within(bn.running_mean, ref["run_mean"], fb["run_mean"], what + ": running mean")
        _within(bn.running_var, ref["run_var"], fb["run_var"], what + ": running var")
        _within(_to_cm(x.grad, case), ref["dx"], A.bn_map_bar(ref["dx"], dtype), what + ": dx")
        _within(bn.bias.grad, ref["dbeta"], bb["dbeta"], what + ": dbeta")
        _within(bn.weight.grad, ref["dgamma"], bb["dgamma"], what + ": dgamma")
        if combo.res:
            _within(_to_cm(res.grad, case), ref["dres"], A.bn_map_bar(ref["dres"], dtype), what + ": dresidual")
        assert int(bn.num_batches_tracked) == 1
    assert int(Nm._sync(DEV)[:-1].abs().sum()) == 0


def test_bn_act_swish_with_a_residual_trains_on_the_stock_ops(launched):
    """The backward kernels take swish's slope without the residual (lss_bn_bwd2 refuses the combination), so
    bn_act does not hand it to them: fp32 against the same reference, the project's fp32 tolerance."""
    case = next(c for c in A.BN_CASES if c.note == "groups of 2 and 3 images" and c.H * c.W == 8)
    combo = A.BnCombo("swish", True, "y")
    ins = A.bn_inputs(case, A.F32, combo)
    bn = _module(case, ins)
    shape = (case.N, case.C, case.H, case.W)
    x = _to_dev(ins["x"], case, A.F32).reshape(shape).requires_grad_(True)
    res = _to_dev(ins["res"], case, A.F32).reshape(shape).requires_grad_(True)
    dy = _to_dev(ins["dy"], case, A.F32).reshape(shape)
    y = Nm.bn_act(bn, x, "swish", res)
    y.backward(dy)
    assert not [w for w in launched if w.startswith("lss_bn")], launched
    xr, rr = x.detach().cpu().double().requires_grad_(True), res.detach().cpu().double().requires_grad_(True)
    w, b = (torch.from_numpy(ins[k]).requires_grad_(True) for k in ("gamma", "beta"))
    yr = torch.nn.functional.silu(torch.nn.functional.batch_norm(xr, None, None, w, b, training=True, eps=A.BN_EPS) + rr)
    yr.backward(dy.cpu().double())
    for got, want in ((y, yr), (x.grad, xr.grad), (res.grad, rr.grad), (bn.weight.grad, w.grad), (bn.bias.grad, b.grad)):
        torch.testing.assert_close(got.detach().cpu().double(), want.detach(), **A.F32_TOL)
