"""The focal loss and the threshold ladder on the host: tools.FocalLoss's torch path (the closed form, through an
autograd.Function) against the definition in fp64, why the closed form is used (fp64 autograd through
(1 - p_t) ** gamma is NaN at a saturated, correctly classified element for 0 < gamma < 1), the argument errors,
the (alpha, gamma, pos_weight) -> (w_pos, w_neg, gamma) rows, tools.seg_metrics_summary on hand-made totals and
the command lines' flag parsing."""
import math

import pytest
import torch

import focal_cases as C
from lss_carla_amd import predict as P, tools as T, trainer

SHAPE = (2, 3, 5, 5)


@pytest.mark.parametrize("gamma", C.GAMMAS)
def test_cpu_fallback_matches_the_closed_form_in_fp64(gamma):
    x, t = C.data(SHAPE, torch.float32)
    r = C.rows(SHAPE[1], gamma)
    fn = T.FocalLoss(SHAPE[1], gamma=[v[2] for v in r], pos_weight=[v[0] for v in r])
    with torch.no_grad():
        fn.focal_params[:, 1] = torch.tensor([v[1] for v in r])  # distinct w_neg too
    xr = x.clone().requires_grad_(True)
    loss = fn(xr, t)
    loss.backward(torch.tensor(0.75))
    r32 = [tuple(float(v) for v in row) for row in fn.focal_params.tolist()]  # the fp32 rows the module holds
    want, grad = C.closed_form(x.double(), t.double(), r32)
    assert {(60.0, 1.0), (-60.0, 0.0), (0.0, 1.0)} <= set(zip(x.view(-1).tolist(), t.view(-1).tolist()))
    assert loss.dtype == torch.float32 and loss.shape == () and xr.grad.dtype == torch.float32
    torch.testing.assert_close(loss.double(), want, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    # fp32 arithmetic: the formula's own rounding (measured against fp64 on these inputs), and no less than 1e-5
    tol = max(1e-5, 4 * C.formula_rounding(x, t, r32))
    torch.testing.assert_close(xr.grad.double(), 0.75 * grad, rtol=tol, atol=1e-12)
    assert torch.isfinite(xr.grad).all()


def test_closed_form_is_finite_where_autograd_of_the_power_is_nan():
    x, t = C.data(SHAPE, torch.float32)
    r = C.rows(SHAPE[1], 0.5)
    sat = ((x == 60) & (t == 1)) | ((x == -60) & (t == 0))
    assert sat.sum().item() == 2
    xa = x.double().requires_grad_(True)
    C.naive(xa, t.double(), r).backward()
    assert torch.isnan(xa.grad[sat]).all()  # inf * 0 in pow's backward
    xr = x.clone().requires_grad_(True)
    fn = T.FocalLoss(SHAPE[1], gamma=[v[2] for v in r], pos_weight=[v[0] for v in r])
    fn(xr, t).backward()
    assert torch.isfinite(xr.grad).all() and (xr.grad[sat].abs() < 1e-36).all()  # exp(-90) w / n, not NaN
    # away from saturation the closed form is the naive form's derivative
    x2 = x.double().clamp(-20, 20)
    xb = x2.clone().requires_grad_(True)
    lb = C.naive(xb, t.double(), r, subtract=False)
    lb.backward()
    lc, gc = C.closed_form(x2, t.double(), r)
    torch.testing.assert_close(lc, lb.detach(), rtol=1e-8, atol=0)
    torch.testing.assert_close(gc, xb.grad, rtol=1e-8, atol=1e-300)


def test_bf16_and_one_class_on_the_torch_path():
    x, t = C.data((3, 1, 4, 7), torch.bfloat16)
    fn = T.FocalLoss(1, gamma=2.0, alpha=0.25)
    xr = x.clone().requires_grad_(True)
    loss = fn(xr, t)
    loss.backward()
    want, grad = C.closed_form(x.double(), t.double(), [(0.25, 0.75, 2.0)])
    assert xr.grad.dtype == torch.bfloat16
    torch.testing.assert_close(loss.double(), want, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    torch.testing.assert_close(xr.grad.double(), grad, rtol=8e-3, atol=1e-12)
    flat = T.FocalLoss(1, gamma=2.0, alpha=0.25)(x.view(-1), t.view(-1))  # one class: any shape
    torch.testing.assert_close(flat, loss.detach(), rtol=1e-6, atol=0)


def test_rows_from_alpha_gamma_pos_weight():
    assert T.focal_rows(2, gamma=2.0) == [(1.0, 1.0, 2.0)] * 2
    assert T.focal_rows(1, gamma=0.0, pos_weight=2.13) == [(2.13, 1.0, 0.0)]  # SimpleLoss(pw)
    assert T.focal_rows(2, gamma=[1.0, 3.0], alpha=0.25) == [(0.25, 0.75, 1.0), (0.25, 0.75, 3.0)]
    assert T.focal_rows(2, gamma=2, alpha=[0.25, 0.5]) == [(0.25, 0.75, 2.0), (0.5, 0.5, 2.0)]
    assert T.focal_rows(3, 1.5, None, [1.0, 2.0, 3.0]) == [(1.0, 1.0, 1.5), (2.0, 1.0, 1.5), (3.0, 1.0, 1.5)]
    fn = T.FocalLoss(3, gamma=2.0, alpha=[0.25, 0.5, 0.75])
    assert fn.computes_in_fp32 is True and fn.focal_params.shape == (3, 3) and fn.focal_params.dtype == torch.float32
    assert fn.focal_params.tolist() == [[0.25, 0.75, 2.0], [0.5, 0.5, 2.0], [0.75, 0.25, 2.0]]
    assert "focal_params" not in fn.state_dict()  # non-persistent
    assert T.FocalLoss(2).focal_params.tolist() == [[1.0, 1.0, 2.0]] * 2


def test_argument_errors():
    for kw in (dict(gamma=-0.1), dict(gamma=[1.0, -1.0]), dict(gamma=float("nan")), dict(alpha=0.0), dict(alpha=1.0),
               dict(alpha=[0.5, 1.5]), dict(alpha=0.25, pos_weight=2.0), dict(gamma=[1.0, 2.0, 3.0]),
               dict(alpha=[0.25]), dict(pos_weight=[1.0, 2.0, 3.0])):
        with pytest.raises(ValueError):
            T.FocalLoss(2, **kw)
    with pytest.raises(ValueError):
        T.FocalLoss(0)
    fn = T.FocalLoss(3)
    with pytest.raises(RuntimeError):
        fn(torch.zeros(2, 2, 4, 4), torch.zeros(2, 2, 4, 4))  # 3 classes, 2 channels
    with pytest.raises(RuntimeError):
        fn(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 5))
    with pytest.raises(RuntimeError, match="device tensors only"):
        T.seg_metrics_accumulate(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2), torch.zeros(4, dtype=torch.float64),
                                 None, torch.ones(1, 3), torch.zeros(1))


def _totals(loss, P, TP, PP):
    return [loss] + list(P) + [v for row in TP for v in row] + [v for row in PP for v in row]


def test_summary_on_hand_made_totals():
    th = [0.4, 0.45, 0.5, 0.55, 0.6]
    # class 0: IoU 0.5 at 0.45 and at 0.55 (equally near 0.5: the lower), less elsewhere
    # class 1: IoU 0.25 at 0.4 and 0.6 and 0.5: 0.5 is nearest; class 2: nothing anywhere (every union 0)
    P = [10, 8, 0]
    TP = [[4, 5, 4, 5, 2], [2, 1, 2, 1, 2], [0, 0, 0, 0, 0]]
    PP = [[10, 5, 4, 5, 2], [2, 8, 2, 8, 2], [0, 0, 0, 0, 0]]
    s = T.seg_metrics_summary(_totals(6.0, P, TP, PP), 3, th, 4)
    assert set(s) == {"loss", "iou_at", "iou_max_per_class", "best_threshold_per_class", "iou_max"}
    assert s["loss"] == 1.5
    assert s["iou_at"][0] == [4 / 16, 2 / 8, None] and s["iou_at"][1] == [5 / 10, 1 / 15, None]
    assert s["iou_at"][2] == [4 / 10, 2 / 8, None] and len(s["iou_at"]) == 5
    assert s["iou_max_per_class"] == [0.5, 0.25, None]
    assert s["best_threshold_per_class"] == [0.45, 0.5, None]
    assert s["iou_max"] == (0.5 + 0.25) / 2
    # a tensor of totals; one threshold; the distance to 0.5 decides before the lower one does
    s1 = T.seg_metrics_summary(torch.tensor(_totals(1.0, [3], [[2, 2]], [[3, 3]]), dtype=torch.float64), 1, [0.3, 0.6], 1)
    assert s1["best_threshold_per_class"] == [0.6] and s1["iou_max"] == 0.5
    # nothing at all, no samples: None, never an exception
    s0 = T.seg_metrics_summary([0.0] * (1 + 2 + 2 * 2 * 1), 2, [0.5], 0)
    assert s0 == {"loss": None, "iou_at": [[None, None]], "iou_max_per_class": [None, None],
                  "best_threshold_per_class": [None, None], "iou_max": None}
    assert T.seg_metrics_summary([], 2, [0.5], 0) == s0
    P_, TP_, PP_ = T.seg_metrics_counts(_totals(6.0, P, TP, PP), 3, 5)
    assert P_ == [10.0, 8.0, 0.0] and TP_[1] == [2.0, 1.0, 2.0, 1.0, 2.0] and PP_[0] == [10.0, 5.0, 4.0, 5.0, 2.0]


def test_iou_of_the_half_column_is_todays_summary():
    """EvalStep.read's existing keys come from the 0.5 column: intersection TP, union PP + P - TP."""
    P, TP, PP = [10, 0], [[4, 3], [0, 0]], [[9, 5], [0, 0]]
    cols = [0.35, 0.5]
    c = cols.index(0.5)
    got = T.iou_summary([TP[k][c] for k in range(2)], [PP[k][c] + P[k] - TP[k][c] for k in range(2)])
    assert got == {"iou": 3 / 12, "iou_per_class": [3 / 12, None]}
    s = T.seg_metrics_summary(_totals(0.0, P, TP, PP), 2, cols, 1)
    assert s["iou_at"][c] == got["iou_per_class"]


def test_flag_parsing():
    assert trainer.parse_per_class("2.0", "--focal_gamma") == 2.0
    assert trainer.parse_per_class("2.0,1.5, 0.5") == [2.0, 1.5, 0.5]
    with pytest.raises(ValueError):
        trainer.parse_per_class(" , ")
    assert trainer.parse_thresholds(None) is None and trainer.parse_thresholds("") is None
    assert trainer.parse_thresholds("0.35,0.4,0.45,0.5,0.55,0.6,0.65") == [0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65]
    assert trainer.parse_thresholds("0.6,0.4,0.6") == [0.4, 0.6] and trainer.parse_thresholds([0.7, 0.3]) == [0.3, 0.7]
    for bad in ("0.0,0.5", "0.5,1.0", ",".join(str(0.03 * i) for i in range(1, 18))):
        with pytest.raises(ValueError):
            trainer.parse_thresholds(bad)
    # the loss: pos_weight is the reference's 2.13 for BCE and w_pos for the focal loss, unless alpha is given
    assert trainer._loss_setup("bce", None, 2.0, None) == (2.13, None)
    assert trainer._loss_setup("bce", [1.0, 2.0], 2.0, None) == ([1.0, 2.0], None)
    assert trainer._loss_setup("focal", None, 2.0, None) == (1.0, {"gamma": 2.0, "alpha": None, "pos_weight": None})
    assert trainer._loss_setup("focal", 3.0, [1.0, 2.0], None)[1] == {"gamma": [1.0, 2.0], "alpha": None, "pos_weight": 3.0}
    assert trainer._loss_setup("focal", None, 2.0, 0.25)[1] == {"gamma": 2.0, "alpha": 0.25, "pos_weight": None}
    for bad in (("focal", 2.13, 2.0, 0.25), ("bce", None, 2.0, 0.25), ("dice", None, 2.0, None)):
        with pytest.raises(ValueError):
            trainer._loss_setup(*bad)
    # both given: refused before anything is built (no GPU is looked for, no directory made)
    with pytest.raises(ValueError, match="give one"):
        trainer.train("/nonexistent", loss="focal", pos_weight=2.0, focal_alpha=0.25, logdir="/nonexistent/run")
    with pytest.raises(ValueError):
        trainer.train("/nonexistent", loss="focal", focal_gamma=-1.0, logdir="/nonexistent/run")

    seen = {}
    real = trainer.train
    trainer.train = lambda **kw: seen.update(kw)
    try:
        trainer.main(["--dataroot", "/data", "--loss", "focal", "--focal_gamma", "2,1,0.5", "--focal_alpha", "0.25",
                      "--iou_thresholds", "0.4,0.5,0.6", "--label_groups", "0;1;2"])
        assert (seen["loss"], seen["focal_gamma"], seen["focal_alpha"], seen["iou_thresholds"], seen["pos_weight"]) == \
            ("focal", [2.0, 1.0, 0.5], 0.25, [0.4, 0.5, 0.6], None)
        trainer.main(["--dataroot", "/data", "--loss", "focal", "--pos_weight", "3.0"])
        assert seen["pos_weight"] == 3.0 and seen["focal_alpha"] is None and seen["focal_gamma"] == 2.0
        trainer.main(["--dataroot", "/data"])
        assert (seen["loss"], seen["pos_weight"], seen["iou_thresholds"], seen["focal_alpha"]) == ("bce", 2.13, None, None)
    finally:
        trainer.train = real

    base = ["--modelf", "m.pt", "--dataroot", "/data", "--out", "o"]
    a = P.parser().parse_args(base)
    assert (a.loss, a.focal_gamma, a.focal_alpha, a.iou_thresholds, a.threshold, a.pos_weight) == \
        ("bce", "2.0", None, None, 0.5, None)
    a = P.parser().parse_args(base + ["--loss", "focal", "--focal_gamma", "2,1", "--focal_alpha", "0.25,0.5",
                                      "--iou_thresholds", "0.4,0.5,0.6", "--threshold", "0.4,0.6"])
    assert a.loss == "focal" and a.threshold == [0.4, 0.6] and a.iou_thresholds == "0.4,0.5,0.6"
    assert P.threshold_arg("0.35") == 0.35 and P.threshold_arg("0.5,0.4,0.35") == [0.5, 0.4, 0.35]
    for bad in (base + ["--loss", "dice"], base + ["--threshold", "x"]):
        with pytest.raises(SystemExit):
            P.parser().parse_args(bad)
    assert math.isclose(P.threshold_logit(0.35), math.log(0.35 / 0.65))
