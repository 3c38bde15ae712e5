"""lss_seg_metrics_accum (tools.seg_metrics_accumulate): validation in one pass for either loss and a ladder of
thresholds. Every count equals a numpy count over the same fp32 thetas exactly (strict >, a logit equal to a
theta is not counted, its successor is); the loss total is within the project's bar for this loss (rtol 2e-6 /
atol 1e-7, tests/test_gpu_loss.py) of the fp64 closed form; with (pw_k, 1, 0) and theta = 0 the counts are
lss_bce_iou_accum_pc's; one captured launch serves any n_valid; EvalStep without the new options launches what it
launched and returns what it returned; Predictor's per-class thresholds are the metric's predicate."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import focal_cases as C  # noqa: E402
import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import _lib, predict as P, tools as T  # noqa: E402
from lss_carla_amd.train_step import EvalStep  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(3, 3, 5, 5), (3, 3, 50, 50), (2, 8, 16, 16), (2, 1, 200, 200)]
DTYPES = [torch.float32, torch.bfloat16]
RTOL, ATOL = C.LOSS_RTOL, C.LOSS_ATOL


def _ladder(T_):
    """T_ ascending probabilities; 7: the usual 0.35 ... 0.65."""
    if T_ == 1:
        return [0.5]
    if T_ == 7:
        return [0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65]
    return [round(0.1 + 0.05 * i, 2) for i in range(T_)]


def _thetas(probs):
    return torch.tensor([P.threshold_logit(v) for v in probs], dtype=torch.float32)


def _reference(x, t, nv, rows, thetas):
    """The 1 + K + 2 K T totals from numpy counts (fp32 compares) and the fp64 closed form, over x[:nv]."""
    K, Tn = x.shape[1], len(thetas)
    if nv == 0:
        return [0.0] * (1 + K + 2 * K * Tn)
    xs, ts = x[:nv].float().numpy(), t[:nv].numpy()
    th = thetas.numpy()
    mean, _ = C.closed_form(x[:nv].double(), t[:nv].double(), rows)
    loss = mean.item() * xs.size / x[0].numel()
    q = ts != 0
    Pk = [int(q[:, k].sum()) for k in range(K)]
    TP = [int(((xs[:, k] > th[j]) & q[:, k]).sum()) for k in range(K) for j in range(Tn)]
    PP = [int((xs[:, k] > th[j]).sum()) for k in range(K) for j in range(Tn)]
    return [loss] + Pk + TP + PP


def _rows(K, gamma=2.0):
    return torch.tensor(C.rows(K, gamma), dtype=torch.float32)


@pytest.mark.parametrize("Tn", [1, 7, 16])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_counts_are_numpys_and_the_loss_is_the_closed_form(shape, dtype, Tn):
    B, K = shape[:2]
    x, t = C.data(shape, dtype, seed=3)
    x = x / 4  # most logits inside the ladder's range of +-2.2
    thetas = _thetas(_ladder(Tn))
    rows = _rows(K)
    xd, td, rd, thd = x.to(DEV), t.to(DEV), rows.to(DEV), thetas.to(DEV)
    n = 1 + K + 2 * K * Tn
    for nv in (0, 1, B, None):
        want = _reference(x, t, B if nv is None else nv, rows.tolist(), thetas)
        n_valid = None if nv is None else torch.tensor([nv], device=DEV, dtype=torch.int32)
        totals = torch.zeros(n, device=DEV, dtype=torch.float64)
        T.seg_metrics_accumulate(xd, td, totals, n_valid, rd, thd)
        got = totals.tolist()
        print(f"{shape} {dtype} T {Tn} nv {nv}: loss {got[0]:.12e} fp64 {want[0]:.12e}")
        assert got[0] == pytest.approx(want[0], rel=RTOL, abs=ATOL)
        assert got[1:] == want[1:]
        T.seg_metrics_accumulate(xd, td, totals, n_valid, rd, thd)  # accumulates
        assert totals.tolist()[1:] == [2 * v for v in want[1:]]
        again = torch.zeros(n, device=DEV, dtype=torch.float64)
        T.seg_metrics_accumulate(xd, td, again, n_valid, rd, thd)
        assert torch.equal(again, torch.tensor(got, device=DEV, dtype=torch.float64))  # two runs: equal bits
    assert sum(want[1 + K:1 + K + K * Tn]) > 0  # some true positives in the full batch


def test_a_logit_equal_to_a_threshold_is_not_counted_and_its_successor_is():
    probs = _ladder(7)
    thetas = _thetas(probs)
    K, Tn = 2, 7
    up = torch.nextafter(thetas, torch.full_like(thetas, float("inf")))
    x = torch.full((1, K, 4, 8), -30.0)
    x[0, 0].view(-1)[:Tn] = thetas  # class 0: one logit on each threshold
    x[0, 1].view(-1)[:Tn] = up      # class 1: one just above each
    t = torch.ones_like(x)
    totals = torch.zeros(1 + K + 2 * K * Tn, device=DEV, dtype=torch.float64)
    T.seg_metrics_accumulate(x.to(DEV), t.to(DEV), totals, None, _rows(K).to(DEV), thetas.to(DEV))
    Pk, TP, PP = T.seg_metrics_counts(totals, K, Tn)
    assert Pk == [32.0, 32.0]
    # theta_i > theta_j exactly for i > j: Tn - 1 - j logits of class 0, and Tn - j of class 1 (theta_j's successor too)
    assert TP[0] == [float(Tn - 1 - j) for j in range(Tn)] and PP[0] == TP[0]
    assert TP[1] == [float(Tn - j) for j in range(Tn)] and PP[1] == TP[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_gamma_zero_and_theta_zero_are_the_bce_entry(shape, dtype):
    B, K = shape[:2]
    x, t = C.data(shape, dtype, seed=4)
    x = x / 2
    xd, td = x.to(DEV), t.to(DEV)
    pw = torch.tensor([0.5 + 0.75 * k for k in range(K)], device=DEV)
    rows = torch.stack([pw, torch.ones_like(pw), torch.zeros_like(pw)], dim=1).contiguous()
    theta = torch.zeros(1, device=DEV)
    for nv in (1, B):
        n_valid = torch.tensor([nv], device=DEV, dtype=torch.int32)
        a = torch.zeros(1 + 2 * K, device=DEV, dtype=torch.float64)
        b = torch.zeros(1 + K + 2 * K, device=DEV, dtype=torch.float64)
        T.val_accumulate(xd, td, a, n_valid=n_valid, pos_weight=pw)
        T.seg_metrics_accumulate(xd, td, b, n_valid, rows, theta)
        a, (Pk, TP, PP) = a.tolist(), T.seg_metrics_counts(b, K, 1)
        assert [TP[k][0] for k in range(K)] == a[1:1 + K]
        assert [PP[k][0] + Pk[k] - TP[k][0] for k in range(K)] == a[1 + K:]
        assert b[0].item() == pytest.approx(a[0], rel=RTOL, abs=ATOL)
        assert sum(a[1 + K:]) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_misaligned_logits_are_read_an_element_at_a_time(dtype):
    """Logits that start one element into a larger buffer (contiguous, off every 16-byte boundary): the entry takes
    the guarded element loads for the whole call. Counts and loss against the reference above."""
    shape, Tn = (3, 3, 5, 5), 7
    B, K = shape[:2]
    x, t = C.data(shape, dtype, seed=6)
    x = x / 4
    buf = torch.zeros(x.numel() + 1, device=DEV, dtype=dtype)
    buf[1:] = x.to(DEV).view(-1)
    xm = buf[1:].view(shape)
    assert xm.is_contiguous() and xm.data_ptr() % 16 != 0
    thetas, rows = _thetas(_ladder(Tn)), _rows(K)
    for nv in (1, B, None):
        want = _reference(x, t, B if nv is None else nv, rows.tolist(), thetas)
        n_valid = None if nv is None else torch.tensor([nv], device=DEV, dtype=torch.int32)
        totals = torch.zeros(1 + K + 2 * K * Tn, device=DEV, dtype=torch.float64)
        T.seg_metrics_accumulate(xm, t.to(DEV), totals, n_valid, rows.to(DEV), thetas.to(DEV))
        got = totals.tolist()
        print(f"{dtype} nv {nv}: loss {got[0]:.12e} fp64 {want[0]:.12e}")
        assert got[0] == pytest.approx(want[0], rel=RTOL, abs=ATOL)
        assert got[1:] == want[1:]
    assert sum(want[1 + K:1 + K + K * Tn]) > 0


def test_captured_accumulate_follows_n_valid():
    B, K, Tn = 3, 3, 7
    x, t = C.data((B, K, 30, 30), torch.bfloat16, seed=5)
    x = x / 4
    thetas, rows = _thetas(_ladder(Tn)), _rows(K)
    xd, td, rd, thd = x.to(DEV), t.to(DEV), rows.to(DEV), thetas.to(DEV)
    n_valid = torch.tensor([B], device=DEV, dtype=torch.int32)
    totals = torch.zeros(1 + K + 2 * K * Tn, device=DEV, dtype=torch.float64)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.seg_metrics_accumulate(xd, td, totals, n_valid, rd, thd)  # the scratch exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        T.seg_metrics_accumulate(xd, td, totals, n_valid, rd, thd)
    for nv in (B, 1, 0):
        totals.zero_()
        n_valid.fill_(nv)
        graph.replay()
        want = _reference(x, t, nv, rows.tolist(), thetas)
        got = totals.tolist()
        assert got[0] == pytest.approx(want[0], rel=RTOL, abs=ATOL) and got[1:] == want[1:]


def test_entry_refuses_bad_arguments():
    lib = _lib.load()
    B, K, plane, Tn = 2, 2, 32, 3
    x = torch.zeros(B * K * plane, device=DEV)
    t = torch.zeros_like(x)
    rows, thetas = _rows(K).to(DEV), torch.tensor([-1.0, 0.0, 1.0], device=DEV)
    totals = torch.zeros(1 + K + 2 * K * Tn, device=DEV, dtype=torch.float64)
    assert lib.lss_seg_metrics_partial_bytes(x.numel(), K, Tn) == 8 + 4 * 2 * K * (Tn + 1)
    assert lib.lss_seg_metrics_partial_bytes(x.numel(), K, 17) == 0 and lib.lss_seg_metrics_partial_bytes(x.numel(), 33, 1) == 0
    partial = torch.zeros(int(lib.lss_seg_metrics_partial_bytes(x.numel(), K, Tn)) // 8, device=DEV, dtype=torch.float64)
    p, st = _lib.ptr, _lib.stream_handle(DEV)

    def call(xp=p(x), k=K, pl=plane, rp=p(rows), thp=p(thetas), tn=Tn, tot=p(totals), per=K * plane):
        return lib.lss_seg_metrics_accum(xp, _lib.F32, p(t), per, B, None, pl, k, rp, thp, tn, tot, p(partial), st)

    assert call() == 0
    for bad in (dict(xp=None), dict(rp=None), dict(thp=None), dict(tot=None), dict(k=0), dict(k=33, pl=2, per=66),
                dict(tn=0), dict(tn=17), dict(pl=31)):
        assert call(**bad) == -1, bad  # LSS_CONV_EINVAL, before any launch
    once = torch.zeros_like(totals)
    T.seg_metrics_accumulate(x.view(B, K, 4, 8), t.view(B, K, 4, 8), once, None, rows, thetas)
    assert torch.equal(totals, once)  # the refused calls added nothing


# ----------------------------------------------------------------------------- EvalStep / Predictor
class _Fixed(torch.nn.Module):
    def __init__(self, preds):
        super().__init__()
        self.preds = preds

    def forward(self, x, *rig):
        return self.preds[:x.shape[0]]


@pytest.fixture
def launched(monkeypatch):
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (calls.append(what), real(code, what))[1])
    return calls


def test_eval_step_without_the_options_is_todays(launched):
    B, K = 2, 3
    g = torch.Generator().manual_seed(6)
    preds = torch.randn(B, K, 8, 8, generator=g).to(DEV)
    labels = (torch.rand(B, K, 8, 8, generator=g) < 0.4).float().to(DEV)
    w = [0.5, 1.25, 2.0]
    model = _Fixed(preds)
    z = torch.zeros(B, 1, device=DEV)
    ev = EvalStep(model, model, (z,) * 6, labels, pos_weight=w, amp_dtype=None, n_samples=B, loss=None, thresholds=None)
    ev()
    assert launched == ["lss_bce_iou_accum_pc"] and ev.totals.shape == (1 + 2 * K,)
    today = ev.read()
    assert set(today) == {"loss", "iou", "iou_per_class"}
    direct = torch.zeros(1 + 2 * K, device=DEV, dtype=torch.float64)
    T.val_accumulate(preds, labels, direct, pos_weight=w)
    assert torch.equal(ev.totals, direct)

    # a ladder: the new entry alone; today's keys keep their values (the 0.5 column), the summary's are added
    del launched[:]
    ladder = [0.35, 0.45, 0.55, 0.65]  # (0.5 is added for today's keys and left out of the report)
    ev2 = EvalStep(model, model, (z,) * 6, labels, pos_weight=w, amp_dtype=None, n_samples=B, thresholds=ladder)
    ev2()
    assert launched == ["lss_seg_metrics_accum"] and ev2.columns == [0.35, 0.45, 0.5, 0.55, 0.65]
    got = ev2.read()
    assert set(got) == set(today) | {"iou_at", "iou_max_per_class", "best_threshold_per_class", "iou_max"}
    assert got["iou"] == today["iou"] and got["iou_per_class"] == today["iou_per_class"]
    assert got["loss"] == pytest.approx(today["loss"], rel=RTOL, abs=ATOL)
    assert len(got["iou_at"]) == 4 and all(len(r) == K for r in got["iou_at"])
    p, q = preds.cpu(), labels.cpu() != 0
    for j, v in enumerate(ladder):
        m = p > _thetas([v])[0]
        want = [((m & q)[:, k].sum().item() / (m | q)[:, k].sum().item()) for k in range(K)]
        assert got["iou_at"][j] == want
    assert got["iou_max_per_class"] == [max(r[k] for r in got["iou_at"]) for k in range(K)]
    assert got["iou_max"] == sum(got["iou_max_per_class"]) / K

    # the focal loss: "loss" is the focal loss, the IoU keys are unchanged
    focal = T.FocalLoss(K, gamma=2.0, alpha=[0.25, 0.5, 0.75]).to(DEV)
    ev3 = EvalStep(model, model, (z,) * 6, labels, pos_weight=w, amp_dtype=None, n_samples=B, loss=focal)
    ev3()
    got3 = ev3.read()
    assert set(got3) == set(today) and got3["iou"] == today["iou"]
    want, _ = C.closed_form(preds.cpu().double(), labels.cpu().double(), focal.focal_params.cpu().tolist())
    assert got3["loss"] == pytest.approx(want.item(), rel=RTOL, abs=ATOL)
    assert got3["loss"] == pytest.approx(focal(preds, labels).item(), rel=1e-5)

    # every class empty: the reference's ZeroDivisionError, as today
    neg, empty = _Fixed(-torch.ones(B, K, 8, 8, device=DEV)), torch.zeros(B, K, 8, 8, device=DEV)
    ev4 = EvalStep(neg, neg, (z,) * 6, empty, pos_weight=w, amp_dtype=None, n_samples=B, thresholds=ladder)
    ev4()
    with pytest.raises(ZeroDivisionError):
        ev4.read()


def test_predictor_per_class_thresholds_are_the_metrics_predicate():
    GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
          "dbound": [4.0, 45.0, 1.0]}
    DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
           "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
    K, B = 3, 2
    probs = [0.35, 0.5, 0.65]
    torch.manual_seed(0)
    model = L.compile_model(GC, DAC, outC=K).to(DEV)
    with pytest.raises(ValueError, match="2 thresholds for 3"):
        L.Predictor(model, B, DEV, threshold=[0.4, 0.6], graph=False)
    with pytest.raises(ValueError):
        L.Predictor(model, B, DEV, threshold=[0.4, 0.6, 1.0], graph=False)
    p = L.Predictor(model, B, DEV, threshold=probs, graph=False)
    thetas = _thetas(probs)
    assert p.thetas.dtype == torch.float32 and torch.equal(p.thetas.cpu(), thetas) and p.logit is None
    # fixed logits in the place of a forward's: some exactly on their class's threshold, some just above
    g = torch.Generator().manual_seed(8)
    logits = torch.randn(B, K, 200, 200, generator=g)
    up = torch.nextafter(thetas, torch.full_like(thetas, float("inf")))
    for k in range(K):
        logits[0, k, 0, :8] = thetas[k]
        logits[1, k, 0, :8] = up[k]
    labels = (torch.rand(B, K, 200, 200, generator=g) < 0.3).float()
    labels[:, :, 0, :8] = 1.0
    for dtype in DTYPES:
        x = logits.to(dtype).to(DEV)
        p._out, p._b = x, B
        masks = p.masks()
        assert masks.dtype == torch.uint8 and masks.shape == (B, K, 200, 200)
        totals = torch.zeros(1 + K + 2 * K * K, device=DEV, dtype=torch.float64)
        T.seg_metrics_accumulate(x, labels.to(DEV), totals, None, _rows(K).to(DEV), thetas.to(DEV))
        _, TP, PP = T.seg_metrics_counts(totals, K, K)
        tp = (masks.bool() & (labels.to(DEV) != 0)).sum(dim=(0, 2, 3)).tolist()
        assert tp == [TP[k][k] for k in range(K)] and masks.sum(dim=(0, 2, 3)).tolist() == [PP[k][k] for k in range(K)]
        if dtype == torch.float32:
            assert not masks[0, :, 0, :8].any() and masks[1, :, 0, :8].all()
    p1 = L.Predictor(L.compile_model(GC, DAC, outC=1).to(DEV), B, DEV, threshold=0.7, graph=False)
    assert p1.thetas is None and p1.logit == P.threshold_logit(0.7)  # a float: today's path
