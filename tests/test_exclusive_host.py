"""Exclusive classes on the host: tools.SoftmaxLoss's torch form against F.cross_entropy in float64, the confusion
summary on hand-made matrices, the paint-order class map restated in numpy, and the argument errors of the trainer,
predict and the Predictor -- none of it needs a GPU."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import exclusive_cases as E
from lss_carla_amd import _lib, predict as P, simbev, tools as T


def _ce64(x, labels, valid, w):
    C = x.shape[1]
    lab = torch.where(E.counted(labels, valid, C), labels, torch.full_like(labels, 255)).long()
    xd = x.double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(xd, lab, weight=w.double(), ignore_index=255, reduction="mean")
    (g,) = torch.autograd.grad(loss, xd)
    return loss.detach(), g


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 5), (1, 2, 1, 9), (2, 8, 4, 8)])
def test_softmax_loss_on_cpu_vs_cross_entropy_fp64(shape, masked):
    C = shape[1]
    x, labels = E.data(shape, torch.float32, seed=1)
    valid = E.mask(shape, seed=1) if masked else None
    w = E.weights(C)
    fn = T.SoftmaxLoss(C, w.tolist())
    assert fn.exclusive and fn.computes_in_fp32 and fn.class_weight.dtype == torch.float32
    xr = x.clone().requires_grad_(True)
    loss = fn(xr, labels) if valid is None else fn(xr, labels, valid)
    loss.backward(torch.tensor(0.75))
    want, wgrad = _ce64(x, labels, valid, w)
    torch.testing.assert_close(loss.detach().double(), want, rtol=E.LOSS_RTOL, atol=E.LOSS_ATOL)
    tol = max(1e-5, 4 * E.formula_rounding(x, labels, valid, w))
    torch.testing.assert_close(xr.grad.double(), 0.75 * wgrad, rtol=tol, atol=1e-12)
    off = ~E.counted(labels, valid, C).unsqueeze(1).expand(shape)
    assert off.any() and (xr.grad[off] == 0).all()
    # float64 logits: the module computes in float64, and the tests' closed form is the same numbers
    l64 = fn(x.double(), labels) if valid is None else fn(x.double(), labels, valid)
    c64, g64 = E.closed_form(x.double(), labels, valid, w)
    torch.testing.assert_close(l64, want, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(c64, want, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(g64, wgrad, rtol=1e-9, atol=1e-15)
    # non-finite logits under cells that do not count change nothing
    bad = x.clone()
    bad[off] = float("nan")
    lb = fn(bad, labels) if valid is None else fn(bad, labels, valid)
    assert torch.equal(lb, loss.detach())


def test_softmax_loss_zero_total_weight_and_bad_arguments():
    shape = (2, 3, 5, 5)
    x, labels = E.data(shape, torch.float32, seed=2)
    fn = T.SoftmaxLoss(3)
    assert fn.class_weight.tolist() == [1.0, 1.0, 1.0]
    xr = x.clone().requires_grad_(True)
    loss = fn(xr, labels, torch.zeros(2, 5, 5, dtype=torch.uint8))
    loss.backward()
    assert loss.item() == 0.0 and (xr.grad == 0).all()
    assert fn(x, torch.full_like(labels, 255)).item() == 0.0
    fn.class_weight.zero_()
    assert fn(x, labels).item() == 0.0
    for bad in (dict(classes=1), dict(classes=9), dict(classes=3, weight=[1.0, 2.0]),
                dict(classes=2, weight=[1.0, -1.0]), dict(classes=2, weight=[1.0, float("nan")])):
        with pytest.raises(ValueError):
            T.SoftmaxLoss(**bad)
    fn = T.SoftmaxLoss(3)
    for call in (lambda: fn(x, labels.long()), lambda: fn(x, labels[:1]), lambda: fn(x[:, :2], labels),
                 lambda: fn(x, labels, torch.ones(1, 5, 5, dtype=torch.uint8))):
        with pytest.raises(RuntimeError):
            call()


def test_confusion_summary_on_hand_made_matrices():
    # classes: background, 1, 2 (never labelled nor predicted), 3
    conf = [[50, 5, 0, 0], [10, 30, 0, 0], [0, 0, 0, 0], [4, 0, 0, 1]]
    totals = [12.0] + [v for row in conf for v in row]
    info = T.confusion_summary(totals, 4, 8)
    assert info["loss"] == 1.5 and info["confusion"] == conf
    iou0, iou1, iou3 = 50 / 69, 30 / 45, 1 / 5
    assert info["iou_per_class"] == [iou0, iou1, None, iou3]
    assert info["iou"] == (iou1 + iou3) / 2                   # the background is not in it
    assert info["miou_all"] == (iou0 + iou1 + iou3) / 3
    assert info["pixel_acc"] == 81 / 100
    assert info["precision_per_class"] == [50 / 64, 30 / 35, None, 1.0]
    assert info["recall_per_class"] == [50 / 55, 30 / 40, None, 1 / 5]
    assert "valid_fraction" not in info
    assert T.confusion_summary(totals, 4, 8, cells=400)["valid_fraction"] == 0.25
    # only background seen: no foreground IoU, nothing raises
    only_bg = T.confusion_summary([0.0, 7, 0, 0, 0], 2, 1)
    assert only_bg["iou"] is None and only_bg["miou_all"] == 1.0 and only_bg["iou_per_class"] == [1.0, None]
    # nothing at all, no samples, short and tensor totals: nothing raises
    empty = T.confusion_summary([], 3, 0, cells=0)
    assert empty["loss"] is None and empty["iou"] is None and empty["miou_all"] is None and empty["pixel_acc"] is None
    assert empty["valid_fraction"] is None and empty["confusion"] == [[0] * 3] * 3
    assert T.confusion_summary(torch.tensor(totals, dtype=torch.float64), 4, 8)["confusion"] == conf


def test_class_index_restatement_on_a_painted_example():
    """Road everywhere in a band, a vehicle on the road, a pedestrian beside it: the later group wins."""
    bev = np.zeros((1, 8, 4, 6), dtype=np.uint8)
    bev[0, 0, 1:3, :] = 200          # channel 0: road, npz rows 1..2
    bev[0, 2, 1, 2:4] = 1            # channel 2: a vehicle on the road
    bev[0, 7, 0, 5] = 9              # channel 7: a pedestrian off the road
    bev[0, 7, 2, 0] = 9              # and one on it
    groups = [[0], [1, 2, 3], [6, 7]]
    want = np.array([[0, 0, 0, 0, 0, 0],
                     [3, 1, 1, 1, 1, 1],     # x row 1 = npz row 2 (flipud)
                     [1, 1, 2, 2, 1, 1],
                     [0, 0, 0, 0, 0, 3]], dtype=np.uint8)
    assert np.array_equal(E.class_index_ref(bev, groups)[0], want)
    planes = np.stack([np.any(bev[:, g] > 0, axis=1)[:, ::-1] for g in groups], axis=1)
    assert np.array_equal(simbev.class_index_from_masks(planes)[0], want)
    assert np.array_equal(simbev.class_index_from_masks(torch.from_numpy(planes.astype(np.float32)))[0], want)
    # the other paint order: the road covers the vehicle
    assert E.class_index_ref(bev, [[1, 2, 3], [0]])[0, 2, 2] == 2
    assert simbev.exclusive_bits(groups) == [1, 14, 192]
    with pytest.raises(ValueError):
        simbev.exclusive_bits([[0]] * 8)
    with pytest.raises(RuntimeError):
        simbev.class_index(torch.from_numpy(bev), groups)  # host maps: no CPU fallback


def test_argmax_rule_on_the_host():
    nan, inf = float("nan"), float("inf")
    rows = [([1.0, 2.0, 2.0], 1), ([3.0, 3.0, 3.0], 0), ([nan, 1.0, 0.0], 1), ([1.0, nan, 2.0], 2),
            ([nan, nan, nan], 0), ([-inf, -inf, -inf], 0), ([-inf, nan, -5.0], 2), ([0.0, inf, nan], 1)]
    x = torch.tensor([r for r, _ in rows]).t().reshape(1, 3, 1, len(rows))
    want = [w for _, w in rows]
    assert T.argmax_classes_host(x).reshape(-1).tolist() == want
    assert E.argmax_rule(x.numpy()).reshape(-1).tolist() == want


def test_entries_check_their_arguments_before_any_hip_call():
    """Made-up addresses that are never dereferenced: every refusal comes before a launch."""
    lib = _lib.load()
    a = lambda v: ctypes.c_void_p(v)  # noqa: E731
    ok = dict(x=a(4096), lab=a(8192), w=a(12288), part=a(16384), loss=a(20480), scale=a(24576), grad=a(32768))
    assert lib.lss_softmax_ce_arm(ok["x"], _lib.F32, ok["lab"], None, 2, 16, 3, ok["grad"]) == 1
    assert lib.lss_softmax_ce_arm(ok["x"], _lib.BF16, ok["lab"], a(8196), 2, 16, 3, ok["grad"]) == 0
    assert lib.lss_softmax_ce_arm(ok["x"], _lib.F32, ok["lab"], None, 2, 15, 3, ok["grad"]) == 0
    assert lib.lss_softmax_ce_arm(a(4100), _lib.F32, ok["lab"], None, 2, 16, 3, ok["grad"]) == 0
    for C in (1, 9, 0, -3):
        assert lib.lss_softmax_ce_arm(ok["x"], _lib.F32, ok["lab"], None, 2, 16, C, ok["grad"]) == -1
        assert lib.lss_softmax_ce(ok["x"], _lib.F32, ok["lab"], None, 2, 16, C, ok["w"], ok["part"], ok["loss"],
                                  ok["scale"], ok["grad"], None) == -1
        assert lib.lss_argmax_classes(ok["x"], _lib.F32, 2, 16, C, ok["lab"], None) == -1
        assert lib.lss_confusion_accum(ok["x"], _lib.F32, ok["lab"], None, 2, 16, C, None, ok["w"], ok["part"],
                                       ok["grad"], None) == -1
    assert lib.lss_softmax_ce(None, _lib.F32, ok["lab"], None, 2, 16, 3, ok["w"], ok["part"], ok["loss"], ok["scale"],
                              ok["grad"], None) == -1
    assert lib.lss_softmax_ce(a(4098), _lib.F32, ok["lab"], None, 2, 16, 3, ok["w"], ok["part"], ok["loss"],
                              ok["scale"], ok["grad"], None) == -1
    assert lib.lss_softmax_ce(ok["x"], _lib.F32, ok["lab"], None, 2, 2 ** 62, 3, ok["w"], ok["part"], ok["loss"],
                              ok["scale"], ok["grad"], None) == -1
    host = (ctypes.c_uint32 * 8)(*([1] * 8))
    hp = ctypes.cast(host, ctypes.c_void_p)
    assert lib.lss_simbev_class_index(ok["x"], 1, 8, 4, 4, hp, 8, None, ok["lab"], None) == -1   # K > 7
    assert lib.lss_simbev_class_index(ok["x"], 1, 8, 4, 4, hp, 0, None, ok["lab"], None) == -1
    assert lib.lss_simbev_class_index(None, 1, 8, 4, 4, hp, 2, None, ok["lab"], None) == -1
    assert lib.lss_simbev_class_index(ok["x"], 1, 8, 4, 4, hp, 2, None, None, None) == -1
    assert lib.lss_simbev_class_index(ok["x"], 1, 8, 4, 4, None, 2, None, ok["lab"], None) == -1
    assert lib.lss_simbev_class_index(ok["x"], 1, 8, (1 << 23) + 1, 4, hp, 2, None, ok["lab"], None) == -1
    assert lib.lss_simbev_class_index(ok["x"], 1, 8, 4, 4, hp, 2, a(4098), ok["lab"], None) == -1
    assert lib.lss_softmax_ce_partials(512) == 4 and lib.lss_confusion_partial_bytes(512, 4) == 2 * (16 + 64)


def test_predictor_refuses_a_threshold_with_exclusive_classes():
    for th in ([0.5, 0.4, 0.3], 0.4, (0.5,)):
        with pytest.raises(ValueError, match="exclusive"):
            P.Predictor(torch.nn.Linear(1, 1), 2, "cpu", threshold=th, exclusive=True)


GROUPS = [[0], [1, 2, 3]]


@pytest.mark.parametrize("kw, match", [
    (dict(exclusive=True), "label_groups"),
    (dict(exclusive=True, label_groups=[[0]] * 8), "1..7"),
    (dict(exclusive=True, label_groups=GROUPS, pos_weight=2.13), "pos_weight"),
    (dict(exclusive=True, label_groups=GROUPS, pos_weight=[1.0, 2.0]), "pos_weight"),
    (dict(exclusive=True, label_groups=GROUPS, loss="focal"), "focal"),
    (dict(exclusive=True, label_groups=GROUPS, focal_gamma=1.0), "focal_gamma"),
    (dict(exclusive=True, label_groups=GROUPS, focal_alpha=0.25), "focal_alpha"),
    (dict(exclusive=True, label_groups=GROUPS, iou_thresholds=[0.4, 0.5]), "iou_thresholds"),
    (dict(exclusive=True, label_groups=GROUPS, class_weight=[1.0, 2.0]), "class_weight"),
    (dict(exclusive=True, label_groups=GROUPS, class_weight=[1.0, 2.0, -1.0]), "class_weight"),
    (dict(label_groups=GROUPS, class_weight=[1.0, 2.0, 3.0]), "exclusive"),
])
def test_trainer_argument_errors_come_before_anything_is_built(kw, match, tmp_path):
    from lss_carla_amd import trainer
    with pytest.raises(ValueError, match=match):  # (gpuid -1 would be the next error: nothing was looked for or built)
        trainer.train(str(tmp_path / "no_such_tree"), gpuid=-1, logdir=str(tmp_path / "log"), use_wandb=False, **kw)
    assert not (tmp_path / "log").exists()


def test_trainer_accepts_an_exclusive_run_up_to_the_gpu_check(tmp_path):
    from lss_carla_amd import trainer
    with pytest.raises(RuntimeError, match="MI355X"):
        trainer.train(str(tmp_path / "no_such_tree"), gpuid=-1, logdir=str(tmp_path / "log"), use_wandb=False,
                      exclusive=True, label_groups=GROUPS, class_weight=[0.5, 1.0, 2.0])
    assert trainer._exclusive_setup(GROUPS, None) == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="exclusive"):
        trainer.main(["--dataroot", "x", "--gpuid", "-1", "--class_weight", "1,1"])
    for extra in (["--pos_weight", "2.0"], ["--loss", "focal"], ["--focal_gamma", "1.5"], ["--iou_thresholds", "0.4"],
                  ["--class_weight", "1,1"]):
        with pytest.raises(ValueError):
            trainer.main(["--dataroot", "x", "--gpuid", "-1", "--exclusive", "1", "--label_groups", "0;1,2,3"] + extra)
    with pytest.raises(ValueError, match="label_groups"):
        trainer.main(["--dataroot", "x", "--gpuid", "-1", "--exclusive", "1"])


@pytest.mark.parametrize("extra, match", [
    (["--exclusive", "1"], "label_groups"),
    (["--exclusive", "1", "--label_groups", "0;1", "--threshold", "0.4"], "threshold"),
    (["--exclusive", "1", "--label_groups", "0;1", "--threshold", "0.5,0.4,0.3"], "threshold"),
    (["--exclusive", "1", "--label_groups", "0;1", "--pos_weight", "2"], "pos_weight"),
    (["--exclusive", "1", "--label_groups", "0;1", "--loss", "focal"], "focal"),
    (["--exclusive", "1", "--label_groups", "0;1", "--focal_alpha", "0.25"], "focal_alpha"),
    (["--exclusive", "1", "--label_groups", "0;1", "--iou_thresholds", "0.4,0.5"], "iou_thresholds"),
    (["--exclusive", "1", "--label_groups", "0;1", "--class_weight", "1,1"], "class_weight"),
    (["--class_weight", "1,1"], "exclusive"),
])
def test_predict_argument_errors_come_before_anything_is_built(extra, match, tmp_path):
    a = P.parser().parse_args(["--modelf", "no_such.pt", "--dataroot", "x", "--out", str(tmp_path / "out"), "--gpuid",
                               "-1"] + extra)
    with pytest.raises(ValueError, match=match):
        P.predict(a)
    assert not (tmp_path / "out").exists()
