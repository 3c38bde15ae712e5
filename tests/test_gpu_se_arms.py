"""Every launch class of lss_se_fwd / lss_se_bwd / lss_se_wgrad on the GPU, stage by stage against a plain fp64
restatement of the contract (tests/arm_cases.py's squeeze-excite section).

tests/test_gpu_se_tails.py compares the tails with the launch sequence, which share their __device__ bodies; here every
buffer of the C ABI is compared with a value computed in numpy from the buffers that feed it: m from x, r from the
kernel's m, h from its r, sig from its h, y from its sig; t from dy and x, de from the kernel's t, dh_part and dr from
its de, dm from its dr, dx from its dm. Each of those buffers is checked itself, so nothing escapes, and an error
cannot hide behind the tolerance of a later stage. lss_se_bwd is handed the REFERENCE's r and sig and lss_se_wgrad the
reference's de, h, dr, m, so a forward bug cannot hide a backward one. The bars are per element and derived in
arm_cases.py; tests/test_host.py proves through lss_se_arm that the cases reach every class, that an fp32 evaluation
keeps 4x room under every bar and that every bar notices one left-out term. Every output starts as NaN.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import arm_cases as A  # noqa: E402
from lss_carla_amd import _lib  # noqa: E402
from lss_carla_amd import efficientnet as E  # noqa: E402

DEV = torch.device("cuda:0")
FWD = ("m", "r", "h", "sig", "y")
BWD = ("t", "de", "dr", "dm", "dx")
WGRAD = ("dw1", "db1", "dw2", "db2")
WORST = {}  # buffer -> the largest |error| / bar seen in this module (printed when the module is done)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nse_arms worst error / bar: " + " ".join("%s=%.4f" % kv for kv in sorted(WORST.items())))


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(inputs, fp64 reference) of one case: made once, shared, left unchanged."""
    ins = A.se_inputs(case.N, case.C, case.HW, case.sq)
    return ins, A.se_reference(ins)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _f32(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _np(t) -> np.ndarray:
    return t.detach().double().cpu().numpy()


def _arm(pas, N, C, HW, sq):
    a = _lib.SeArm()
    assert _lib.load().lss_se_arm(pas, N, C, HW, sq, ctypes.byref(a)) == 0
    return a


def _wgrad(de, h, dr, m, o):
    N, C = de.shape
    p = _lib.ptr
    _lib.check(_lib.load().lss_se_wgrad(p(de), p(h), p(dr), p(m), N, C, h.shape[1], p(o["dw1"]), p(o["db1"]), p(o["dw2"]),
                                        p(o["db2"]), _lib.stream_handle(DEV)), "lss_se_wgrad")


def _run(ins, setting, fed=None):
    """Forward, backward and weight gradients through the C ABI under one lss_se_tails setting, every output
    NaN-filled first. fed: the reference whose r, sig the backward and whose de, h, dr, m the weight gradients are
    handed; None: the kernels' own (what the autograd wrapper does). Returns the buffers and the two reports of
    lss_se_arm taken under the same setting."""
    lib = _lib.load()
    N, C, HW = ins["x"].shape
    sq = ins["w1"].shape[0]
    x, dy = (A.rounded(ins[k], A.BF16).to(DEV) for k in ("x", "dy"))
    w1, b1, w2, b2 = (_f32(ins[k]) for k in ("w1", "b1", "w2", "b2"))
    o = {"m": _nan(N, C), "r": _nan(N, sq), "h": _nan(N, sq), "sig": _nan(N, C),
         "y": _nan(N, C, HW, dtype=torch.bfloat16), "t": _nan(N, C), "dh_part": _nan(N, (C + 63) // 64, sq),
         "de": _nan(N, C), "dr": _nan(N, sq), "dm": _nan(N, C), "dx": _nan(N, C, HW, dtype=torch.bfloat16),
         "dw1": _nan(sq, C), "db1": _nan(sq), "dw2": _nan(C, sq), "db2": _nan(C)}
    p, st = _lib.ptr, _lib.stream_handle(DEV)
    prev = lib.lss_se_tails(int(setting))
    try:
        arms = _arm(A.SE_FWD, N, C, HW, sq), _arm(A.SE_BWD, N, C, HW, sq)
        _lib.check(lib.lss_se_fwd(p(x), N, C, HW, p(w1), p(b1), p(w2), p(b2), sq, p(o["m"]), p(o["r"]), p(o["h"]),
                                  p(o["sig"]), p(o["y"]), st), "lss_se_fwd")
        r, sig = (o["r"], o["sig"]) if fed is None else (_f32(fed["r"]), _f32(fed["sig"]))
        _lib.check(lib.lss_se_bwd(p(dy), p(x), N, C, HW, p(w1), p(w2), sq, p(r), p(sig), p(o["t"]), p(o["dh_part"]),
                                  p(o["de"]), p(o["dr"]), p(o["dm"]), p(o["dx"]), st), "lss_se_bwd")
        four = [o[k] if fed is None else _f32(fed[k]) for k in ("de", "h", "dr", "m")]
        _wgrad(*four, o)
    finally:
        lib.lss_se_tails(prev)
    torch.cuda.synchronize()
    return o, arms


def _note(rooms):
    for k, v in rooms.items():
        WORST[k] = max(WORST.get(k, 0.0), v)


@pytest.mark.parametrize("case", A.SE_CASES, ids=A.se_id)
def test_se_arm_stages(case):
    ins, ref = _reference(case)
    runs = {}
    for setting in A.se_settings(case):
        o, (fa, ba) = _run(ins, setting, fed=ref)
        what = "%s setting %d" % (A.se_id(case), setting)
        # the routing the query reports, seen from outside: only the sequence stores the chunk partials
        limit = lambda pas: 4096 if pas else 1024  # noqa: E731
        for pas, a in ((A.SE_FWD, fa), (A.SE_BWD, ba)):
            tails = setting != A.SE_OFF and case.N <= A.SE_BANK_IMAGES and \
                (setting == A.SE_FORCED or case.C * case.sq <= limit(pas))
            assert (a.tails, a.launches) == ((1, 2) if tails else (0, 4)), (what, pas)
        assert bool(torch.isnan(o["dh_part"]).all()) if ba.tails else not torch.isnan(o["dh_part"]).any(), what
        for k in FWD + BWD + WGRAD:
            assert not torch.isnan(o[k]).any(), (what, k, "NaN left")
        for k in ("m", "r", "h", "sig"):  # fp32 buffers that hold bf16 values
            assert not (_bits(o[k]) & 0xFFFF).any(), (what, k, "not a bf16 value")
        buf = {k: _np(v) for k, v in o.items()}
        rooms = A.se_rooms(ins, buf, ref, dh_part=not ba.tails)
        fed4 = [ref[k].astype(np.float32) for k in ("de", "h", "dr", "m")]
        rooms.update(A.se_wgrad_rooms(fed4, buf))
        print(what, {k: round(v, 4) for k, v in rooms.items()})
        _note(rooms)
        assert all(v <= 1.0 for v in rooms.values()), (what, {k: v for k, v in rooms.items() if not v <= 1.0})
        runs[setting] = o
    first = runs[A.SE_OFF]
    for setting, o in runs.items():
        for k in FWD + BWD + WGRAD:
            assert torch.equal(_bits(o[k]), _bits(first[k])), (A.se_id(case), setting, k, "settings differ")


@pytest.mark.parametrize("N,C,sq", A.SE_WGRAD_CASES)
def test_se_wgrad_arm(N, C, sq):
    fed4 = A.se_wgrad_inputs(N, C, sq)
    o = {"dw1": _nan(sq, C), "db1": _nan(sq), "dw2": _nan(C, sq), "db2": _nan(C)}
    _wgrad(*(_f32(a) for a in fed4), o)
    torch.cuda.synchronize()
    for k in WGRAD:
        assert not torch.isnan(o[k]).any(), k
    rooms = A.se_wgrad_rooms(fed4, {k: _np(v) for k, v in o.items()})
    print((N, C, sq), {k: round(v, 4) for k, v in rooms.items()})
    _note(rooms)
    assert all(v <= 1.0 for v in rooms.values()), rooms


@pytest.mark.parametrize("note", A.SE_AUTOGRAD)
def test_squeeze_excite_autograd_equals_the_c_abi(note):
    """efficientnet.squeeze_excite through autograd: what it returns is the C ABI's buffers bit for bit after the
    wrapper's reshapes and casts (the C ABI run chained on its own buffers, as the wrapper chains them)."""
    case = A.se_case(note)
    ins, _ = _reference(case)
    N, C, sq = case.N, case.C, case.sq
    H = 2 if case.HW % 2 == 0 else 1
    red, exp = torch.nn.Conv2d(C, sq, 1).to(DEV), torch.nn.Conv2d(sq, C, 1).to(DEV)
    with torch.no_grad():
        red.weight.copy_(_f32(ins["w1"]).reshape(sq, C, 1, 1))
        red.bias.copy_(_f32(ins["b1"]))
        exp.weight.copy_(_f32(ins["w2"]).reshape(C, sq, 1, 1))
        exp.bias.copy_(_f32(ins["b2"]))
    x = A.rounded(ins["x"], A.BF16).to(DEV).reshape(N, C, H, case.HW // H).requires_grad_(True)
    dy = A.rounded(ins["dy"], A.BF16).to(DEV).reshape(x.shape)
    y = E.squeeze_excite(x, red, exp)
    assert isinstance(y.grad_fn, E._HipSqueezeExcite._backward_cls)
    grads = torch.autograd.grad(y, [x, red.weight, red.bias, exp.weight, exp.bias], dy)
    torch.cuda.synchronize()
    lib = _lib.load()
    current = lib.lss_se_tails(1)
    lib.lss_se_tails(current)
    o, _ = _run(ins, current)
    for got, k in zip((y,) + grads, ("y", "dx", "dw1", "db1", "dw2", "db2")):
        assert got.dtype == o[k].dtype and not torch.isnan(got).any(), k
        assert torch.equal(_bits(got.detach().reshape(o[k].shape).contiguous()), _bits(o[k])), k
