"""The per-class loss and metrics of a multi-class BEV head: SimpleLoss with one pos_weight per class on
lss_bce_logits_pc, tools.val_accumulate / EvalStep totals per class on lss_bce_iou_accum_pc, get_val_info's
per-class IoU.

Bars: the project's for this loss (tests/test_gpu_loss.py) -- loss rtol 2e-6 / atol 1e-7 against fp64
BCEWithLogitsLoss(pos_weight=(K, 1, 1)), gradient rtol 1e-5 (fp32) or 8e-3 (bf16: the fp32 gradient rounded
once); equal class weights reproduce the one-weight kernel bit for bit; counts are exact."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import tools as T  # noqa: E402
from lss_carla_amd.train_step import EvalStep  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(2, 3, 5, 5), (1, 2, 1, 9), (4, 8, 16, 16)]  # plane 25: threads cross planes; under one vector; 4 blocks
DTYPES = [torch.float32, torch.bfloat16]
RTOL, ATOL = 2e-6, 1e-7


def _data(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = (torch.randn(shape, generator=g) * 4).to(dtype)
    x.view(-1)[:3] = torch.tensor([60.0, -60.0, 0.0]).to(dtype)  # saturated logits and zero
    t = (torch.rand(shape, generator=g) < 0.3).float()
    return x, t


def _weights(K):
    return [0.5 + 0.75 * k for k in range(K)]


def _run(loss_fn, x, t, scale=0.75):
    xd = x.to(DEV).requires_grad_(True)
    loss = loss_fn(xd, t.to(DEV))
    loss.backward(torch.tensor(scale, device=DEV))
    return loss.detach(), xd.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_equal_class_weights_are_the_one_weight_kernel_bit_for_bit(shape, dtype, monkeypatch):
    x, t = _data(shape, dtype)
    launched = []
    from lss_carla_amd import _lib
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (launched.append(what), real(code, what))[1])
    l1, g1 = _run(T.SimpleLoss(2.13).to(DEV), x, t)
    lk, gk = _run(T.SimpleLoss([2.13] * shape[1]).to(DEV), x, t)
    assert launched.count("lss_bce_logits") == 1 and launched.count("lss_bce_logits_pc") == 1
    assert torch.equal(l1, lk) and torch.equal(g1, gk)
    assert gk.dtype == dtype and lk.dtype == torch.float32 and lk.shape == ()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_distinct_class_weights_vs_fp64(shape, dtype):
    x, t = _data(shape, dtype, seed=1)
    K = shape[1]
    w = _weights(K)
    loss, grad = _run(T.SimpleLoss(w).to(DEV), x, t)
    xr = x.double().requires_grad_(True)
    ref = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(w, dtype=torch.float64).view(K, 1, 1))(xr, t.double())
    (ref * 0.75).backward()
    print(f"loss {loss.item():.9f} fp64 {ref.item():.9f}")
    torch.testing.assert_close(loss.cpu().double(), ref.detach(), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(grad.cpu().double(), xr.grad, rtol=1e-5 if dtype == torch.float32 else 8e-3, atol=1e-12)
    # two runs: equal bits
    loss2, grad2 = _run(T.SimpleLoss(w).to(DEV), x, t)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_class_weights_are_read_on_the_device():
    """The K weights are a device buffer: changing it in place changes the next call (no re-capture needed)."""
    x, t = _data((2, 3, 5, 5), torch.float32, seed=2)
    fn = T.SimpleLoss([1.0, 1.0, 1.0]).to(DEV)
    a, _ = _run(fn, x, t)
    fn.pos_weight_classes.copy_(torch.tensor([1.0, 3.0, 1.0]))
    b, _ = _run(fn, x, t)
    want, _ = _run(T.SimpleLoss([1.0, 3.0, 1.0]).to(DEV), x, t)
    assert not torch.equal(a, b) and torch.equal(b, want)


def test_non_contiguous_logits_take_torch_path(monkeypatch):
    from lss_carla_amd import _lib
    launched = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (launched.append(what), real(code, what))[1])
    x = torch.randn(4, 3, 10, 12, device=DEV).transpose(2, 3)
    t = (torch.rand(4, 3, 12, 10, device=DEV) < 0.5).float()
    w = _weights(3)
    fn = T.SimpleLoss(w).to(DEV)
    got = fn(x, t)
    assert not launched
    want = F.binary_cross_entropy_with_logits(x, t, pos_weight=torch.tensor(w, device=DEV).view(3, 1, 1))
    torch.testing.assert_close(got, want)
    with pytest.raises(RuntimeError):
        fn(torch.randn(4, 2, 5, 5, device=DEV), torch.zeros(4, 2, 5, 5, device=DEV))  # 3 weights, 2 channels


# ----------------------------------------------------------------------------- validation totals per class
def _val_reference(x, t, nv, w):
    """fp64 on the CPU from the logits the kernel sees: (loss x samples, K intersections, K unions)."""
    K = x.shape[1]
    if nv == 0:
        return 0.0, [0] * K, [0] * K
    xs, ts = x[:nv].double(), t[:nv].double()
    loss = F.binary_cross_entropy_with_logits(xs, ts, pos_weight=torch.tensor(w, dtype=torch.float64).view(K, 1, 1),
                                              reduction="sum").item() / x[0].numel()
    p, q = xs > 0, ts != 0
    return loss, (p & q).sum(dim=(0, 2, 3)).tolist(), (p | q).sum(dim=(0, 2, 3)).tolist()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 3, 5, 5), (3, 3, 50, 50), (2, 8, 16, 16)])
def test_val_accumulate_per_class(shape, dtype):
    B, K = shape[:2]
    x, t = _data(shape, dtype, seed=3)
    x = x / 2
    xd, td = x.to(DEV), t.to(DEV)
    w = _weights(K)
    wd = torch.tensor(w, device=DEV)
    for nv in (0, 1, B, None):
        loss, inter, union = _val_reference(x, t, B if nv is None else nv, w)
        n_valid = None if nv is None else torch.tensor([nv], device=DEV, dtype=torch.int32)
        totals = torch.zeros(1 + 2 * K, device=DEV, dtype=torch.float64)
        T.val_accumulate(xd, td, totals, n_valid=n_valid, pos_weight=wd)
        got = totals.tolist()
        print(f"nv {nv}: got {got} want {loss} {inter} {union}")
        assert got[0] == pytest.approx(loss, rel=RTOL, abs=ATOL)
        assert got[1:1 + K] == inter and got[1 + K:] == union
        T.val_accumulate(xd, td, totals, n_valid=n_valid, pos_weight=w)  # a list of weights; accumulates
        assert totals.tolist()[1:] == [2 * v for v in inter + union]
        again = torch.zeros(1 + 2 * K, device=DEV, dtype=torch.float64)
        T.val_accumulate(xd, td, again, n_valid=n_valid, pos_weight=wd)
        assert torch.equal(again, torch.tensor(got, device=DEV, dtype=torch.float64))
    if nv is None:
        assert sum(inter) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 1, 1, 63), (3, 1, 50, 50), (2, 1, 200, 200)])
def test_one_class_totals_are_todays_entry_bit_for_bit(shape, dtype):
    """K = 1 through lss_bce_iou_accum_pc (a device weight) == lss_bce_iou_accum (the float), all three totals."""
    x, t = _data(shape, dtype, seed=4)
    xd, td = x.to(DEV), t.to(DEV)
    for nv in (1, shape[0]):
        n_valid = torch.tensor([nv], device=DEV, dtype=torch.int32)
        a = torch.zeros(3, device=DEV, dtype=torch.float64)
        b = torch.zeros(3, device=DEV, dtype=torch.float64)
        T.val_accumulate(xd, td, a, n_valid=n_valid, pos_weight=2.13)
        T.val_accumulate(xd, td, b, n_valid=n_valid, pos_weight=torch.tensor([2.13], device=DEV))
        assert torch.equal(a, b) and a[2].item() > 0


def test_captured_per_class_accumulate_follows_n_valid():
    B, K = 3, 3
    x, t = _data((B, K, 30, 30), torch.bfloat16, seed=5)
    xd, td = x.to(DEV), t.to(DEV)
    w = _weights(K)
    wd = torch.tensor(w, device=DEV)
    n_valid = torch.tensor([B], device=DEV, dtype=torch.int32)
    totals = torch.zeros(1 + 2 * K, device=DEV, dtype=torch.float64)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.val_accumulate(xd, td, totals, n_valid=n_valid, pos_weight=wd)  # the scratch exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        T.val_accumulate(xd, td, totals, n_valid=n_valid, pos_weight=wd)
    for nv in (B, 1, 0):
        totals.zero_()
        n_valid.fill_(nv)
        graph.replay()
        loss, inter, union = _val_reference(x, t, nv, w)
        got = totals.tolist()
        assert got[0] == pytest.approx(loss, rel=RTOL, abs=ATOL)
        assert got[1:1 + K] == inter and got[1 + K:] == union


# ----------------------------------------------------------------------------- get_val_info / EvalStep.read
class _Fixed(torch.nn.Module):
    """A 'model' that returns fixed logits for the batch size it is given."""

    def __init__(self, preds):
        super().__init__()
        self.preds = preds

    def forward(self, x, *rig):
        return self.preds[:x.shape[0]]


def _loader(labels, B):
    z = torch.zeros(B, 1)

    class Loader(list):
        dataset = list(range(B))

    return Loader([(z, z, z, z, z, z, labels)])


def test_get_val_info_and_eval_step_per_class():
    B, K = 2, 3
    g = torch.Generator().manual_seed(6)
    preds = torch.randn(B, K, 8, 8, generator=g).to(DEV)
    labels = (torch.rand(B, K, 8, 8, generator=g) < 0.4).float().to(DEV)
    preds[:, 1] = -1.0
    labels[:, 1] = 0.0  # class 1: an empty union
    w = _weights(K)
    p, q = preds > 0, labels != 0
    inter, union = (p & q).sum(dim=(0, 2, 3)).tolist(), (p | q).sum(dim=(0, 2, 3)).tolist()
    want = [inter[0] / union[0], None, inter[2] / union[2]]
    model = _Fixed(preds)
    info = T.get_val_info(model, _loader(labels, B), T.SimpleLoss(w).to(DEV), DEV, use_tqdm=False)
    assert set(info) == {"loss", "iou", "iou_per_class"}
    assert info["iou_per_class"] == want and info["iou"] == (want[0] + want[2]) / 2
    ref = F.binary_cross_entropy_with_logits(preds.double(), labels.double(),
                                             pos_weight=torch.tensor(w, device=DEV, dtype=torch.float64).view(K, 1, 1))
    assert info["loss"] == pytest.approx(ref.item(), rel=RTOL, abs=ATOL)

    z = torch.zeros(B, 1, device=DEV)
    ev = EvalStep(model, model, (z,) * 6, labels, pos_weight=w, amp_dtype=None, n_samples=B)
    assert ev.totals.shape == (1 + 2 * K,)
    ev()
    got = ev.read()
    assert set(got) == {"loss", "iou", "iou_per_class"}
    assert got["iou_per_class"] == want and got["iou"] == info["iou"]
    assert got["loss"] == pytest.approx(ref.item(), rel=RTOL, abs=ATOL)

    # every class empty: the reference's ZeroDivisionError
    neg = _Fixed(-torch.ones(B, K, 8, 8, device=DEV))
    empty = torch.zeros(B, K, 8, 8, device=DEV)
    with pytest.raises(ZeroDivisionError):
        T.get_val_info(neg, _loader(empty, B), T.SimpleLoss(w).to(DEV), DEV, use_tqdm=False)
    ev = EvalStep(neg, neg, (z,) * 6, empty, pos_weight=w, amp_dtype=None, n_samples=B)
    ev()
    with pytest.raises(ZeroDivisionError):
        ev.read()

    # one class: the same floats as the reference's dict, plus the list
    ev1 = EvalStep(_Fixed(preds[:, :1].contiguous()), _Fixed(preds[:, :1].contiguous()), (z,) * 6,
                   labels[:, :1].contiguous(), pos_weight=2.13, amp_dtype=None, n_samples=B)
    assert ev1.totals.shape == (3,)
    ev1()
    r1 = ev1.read()
    assert r1["iou"] == inter[0] / union[0] and r1["iou_per_class"] == [r1["iou"]]


def test_get_batch_iou_per_class_stays_on_the_device():
    g = torch.Generator().manual_seed(7)
    preds = torch.randn(2, 3, 8, 8, generator=g).to(DEV)
    labels = (torch.rand(2, 3, 8, 8, generator=g) < 0.4).float().to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        i, u = T.get_batch_iou_per_class(preds, labels)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert i.shape == (3,) and u.shape == (3,) and i.is_cuda
    p, q = preds > 0, labels != 0
    assert i.tolist() == (p & q).sum(dim=(0, 2, 3)).tolist() and u.tolist() == (p | q).sum(dim=(0, 2, 3)).tolist()
