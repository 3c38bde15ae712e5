"""lss_confusion_accum (tools.confusion_accumulate) and lss_argmax_classes (tools.argmax_classes) on the MI355X:
exact confusion counts and the argmax map against numpy restatements (exclusive_cases), the loss total against the
float64 closed form, n_valid on one captured graph, accumulation over calls, and the two-class case against
lss_bce_iou_accum's IoU of x_1 - x_0 > 0."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import exclusive_cases as E  # noqa: E402
from lss_carla_amd import _lib, tools as T  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16]


def _with_nans(x, seed):
    """Some cells with a NaN channel (the first, a middle one, the last), one cell all NaN, one all -inf."""
    B, C, H, W = x.shape
    cells = x.permute(0, 2, 3, 1).reshape(-1, C).clone()
    n = cells.shape[0]
    cells[8 % n, 0] = float("nan")
    cells[9 % n, C // 2] = float("nan")
    cells[10 % n, C - 1] = float("nan")
    cells[11 % n] = float("nan")
    cells[12 % n] = -float("inf")
    return cells.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def _loss_total(x, labels, valid, w, nv):
    if nv == 0:
        return 0.0
    loss, _ = E.closed_form(x[:nv].double(), labels[:nv], None if valid is None else valid[:nv], w)
    return nv * loss.item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", E.SHAPES)
def test_argmax_map_vs_the_restatement(shape, dtype):
    x, _ = E.data(shape, dtype, seed=1)
    x = _with_nans(x, 1)
    got = T.argmax_classes(x.to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (shape[0],) + shape[2:]
    want = E.argmax_rule(x.float().numpy())
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(T.argmax_classes_host(x), want)
    flat = want.reshape(-1)
    n = flat.size
    assert flat[0] == 0 and flat[3 % n] == 0 and flat[4 % n] == 0  # ties: the lowest class
    assert flat[11 % n] == 0 and flat[12 % n] == 0                 # all NaN, all -inf
    if n > 12:
        assert flat[8] != 0                                        # a NaN in channel 0 never wins


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", E.SHAPES)
def test_counts_and_loss_total_accumulate_over_two_calls(shape, dtype, masked):
    B, C = shape[0], shape[1]
    w = E.weights(C)
    xa, la = E.data(shape, dtype, seed=2)
    xb, lb = E.data(shape, dtype, seed=3)
    va, vb = (E.mask(shape, seed=2), E.mask(shape, seed=3)) if masked else (None, None)
    totals = torch.zeros(1 + C * C, device=DEV, dtype=torch.float64)
    dv = lambda v: None if v is None else v.to(DEV)  # noqa: E731
    T.confusion_accumulate(xa.to(DEV), la.to(DEV), totals, None, w.to(DEV), valid=dv(va))
    first = totals.cpu().clone()
    conf_a = E.confusion_counts(xa, la, va, B)
    assert np.array_equal(first[1:].numpy().reshape(C, C), conf_a.astype(np.float64))
    nvb = max(B - 1, 1)
    nv = torch.tensor([nvb], device=DEV, dtype=torch.int32)
    T.confusion_accumulate(xb.to(DEV), lb.to(DEV), totals, nv, w.to(DEV), valid=dv(vb))
    got = totals.cpu()
    conf = conf_a + E.confusion_counts(xb, lb, vb, nvb)
    assert np.array_equal(got[1:].numpy().reshape(C, C), conf.astype(np.float64))
    assert np.trace(conf) > 0 and conf.sum() > np.trace(conf)  # right and wrong cells both
    want = _loss_total(xa, la, va, w, B) + _loss_total(xb, lb, vb, w, nvb)
    print(f"{shape} {dtype} masked={masked}: loss total {got[0].item():.9e} fp64 {want:.9e} rel "
          f"{abs(got[0].item() - want) / abs(want):.2e}")
    assert got[0].item() == pytest.approx(want, rel=E.LOSS_RTOL, abs=E.LOSS_ATOL)
    info = T.confusion_summary(got, C, B + nvb, cells=(B + nvb) * shape[2] * shape[3] if masked else None)
    assert info["confusion"] == conf.tolist() and info["loss"] == pytest.approx(want / (B + nvb), rel=E.LOSS_RTOL)
    assert ("valid_fraction" in info) == masked
    if masked:
        assert info["valid_fraction"] == pytest.approx(conf.sum() / ((B + nvb) * shape[2] * shape[3]))


def test_n_valid_of_zero_partial_and_full_on_one_graph():
    shape = (4, 8, 16, 16)
    B, C = shape[0], shape[1]
    x, labels = E.data(shape, torch.bfloat16, seed=4)
    x = _with_nans(x, 4)
    labels.view(-1)[8:13] = 255  # the cells with non-finite logits do not count: the loss total stays finite
    valid = E.mask(shape, seed=4)
    w = E.weights(C)
    xd, ld, vd, wd = x.to(DEV), labels.to(DEV), valid.to(DEV), w.to(DEV)
    nv = torch.zeros(1, device=DEV, dtype=torch.int32)
    totals = torch.zeros(1 + C * C, device=DEV, dtype=torch.float64)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.confusion_accumulate(xd, ld, totals, nv, wd, valid=vd)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        T.confusion_accumulate(xd, ld, totals, nv, wd, valid=vd)
    for n in (0, 3, B, B + 5, -2):  # (clamped to 0..B)
        totals.zero_()
        nv.fill_(n)
        graph.replay()
        k = min(max(n, 0), B)
        got = totals.cpu()
        assert np.array_equal(got[1:].numpy().reshape(C, C), E.confusion_counts(x, labels, valid, k).astype(np.float64))
        assert got[0].item() == pytest.approx(_loss_total(x, labels, valid, w, k), rel=E.LOSS_RTOL, abs=E.LOSS_ATOL)
    totals.zero_()
    nv.fill_(0)
    graph.replay()
    assert (totals == 0).all()


@pytest.mark.parametrize("shape", [(2, 2, 5, 5), (2, 2, 16, 16)])
def test_two_classes_match_the_sigmoid_iou_of_the_logit_difference(shape):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(shape, generator=g)
    d = (x[:, 1] - x[:, 0]).unsqueeze(1).contiguous()
    assert (d != 0).all()  # no ties
    labels = (torch.rand(shape[0], *shape[2:], generator=g) < 0.4).to(torch.uint8)
    totals = torch.zeros(5, device=DEV, dtype=torch.float64)
    T.confusion_accumulate(x.to(DEV), labels.to(DEV), totals, None, torch.ones(2, device=DEV))
    info = T.confusion_summary(totals, 2, shape[0])
    bce = torch.zeros(3, device=DEV, dtype=torch.float64)
    T.val_accumulate(d.to(DEV), labels.float().unsqueeze(1).to(DEV), bce, pos_weight=1.0)
    _, inter, union = bce.tolist()
    assert info["iou"] == inter / union and info["iou_per_class"][1] == inter / union
    pred = d.squeeze(1).numpy() > 0
    lab = labels.numpy() != 0
    assert inter == (pred & lab).sum() and union == (pred | lab).sum()


def test_entries_refuse_bad_arguments():
    lib = _lib.load()
    B, C, plane = 2, 3, 16
    x = torch.zeros(B * C * plane + 8, device=DEV)
    labels = torch.zeros(B * plane, device=DEV, dtype=torch.uint8)
    out = torch.zeros(B * plane, device=DEV, dtype=torch.uint8)
    w = torch.ones(C + 1, device=DEV)
    nv = torch.ones(2, device=DEV, dtype=torch.int32)
    totals = torch.zeros(2 + C * C, device=DEV, dtype=torch.float64)
    nbytes = int(lib.lss_confusion_partial_bytes(B * plane, C))
    assert nbytes == 16 + 4 * C * C and lib.lss_confusion_partial_bytes(0, C) == 0
    assert lib.lss_confusion_partial_bytes(10, 1) == 0 and lib.lss_confusion_partial_bytes(10, 9) == 0
    partial = torch.zeros(nbytes // 8 + 2, device=DEV, dtype=torch.float64)
    st = _lib.stream_handle(DEV)
    p = _lib.ptr
    off = lambda v, by=2: ctypes.c_void_p(v.data_ptr() + by)  # noqa: E731

    def accum(xp=p(x), lp=p(labels), vp=None, b=B, pl=plane, c=C, np_=p(nv), wp=p(w), tp=p(totals), part=p(partial),
              dt=_lib.F32):
        return lib.lss_confusion_accum(xp, dt, lp, vp, b, pl, c, np_, wp, tp, part, st)

    assert accum() == 0 and accum(np_=None) == 0 and accum(vp=p(out)) == 0
    for bad in (dict(xp=None), dict(lp=None), dict(wp=None), dict(tp=None), dict(part=None), dict(b=0), dict(pl=0),
                dict(c=1), dict(c=9), dict(dt=7), dict(pl=2 ** 62), dict(xp=off(x)), dict(wp=off(w)), dict(np_=off(nv)),
                dict(tp=off(totals, 4)), dict(part=off(partial, 4))):
        assert accum(**bad) == -1, bad

    def argmax(xp=p(x), b=B, pl=plane, c=C, op=p(out), dt=_lib.F32):
        return lib.lss_argmax_classes(xp, dt, b, pl, c, op, st)

    assert argmax() == 0
    for bad in (dict(xp=None), dict(op=None), dict(b=0), dict(pl=0), dict(c=1), dict(c=9), dict(dt=7), dict(xp=off(x))):
        assert argmax(**bad) == -1, bad
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        T.confusion_accumulate(x[:B * C * plane].view(B, C, 4, 4), labels.view(B, 4, 4).float(), totals[:1 + C * C], None,
                               w[:C])
    with pytest.raises(RuntimeError):
        T.confusion_accumulate(x[:B * C * plane].view(B, C, 4, 4), labels.view(B, 4, 4), totals[:C * C], None, w[:C])
    with pytest.raises(RuntimeError):
        T.argmax_classes(x[:B * C * plane].view(B, C, 4, 4).cpu())
