"""Host-side pieces of lss_carla_amd.predict (no GPU): the command line's arguments, checkpoint-format
detection, the head-width check, the threshold -> logit conversion, the error without a GPU, and the dispatch
guard of the eval-mode batch norm on CPU tensors."""
import math

import pytest
import torch
from torch import nn

import lss_carla_amd as L
from lss_carla_amd import norm, predict as P


def test_argument_parsing():
    a = P.parser().parse_args(["--modelf", "m.pt", "--dataroot", "/data", "--out", "o"])
    assert (a.modelf, a.dataroot, a.out) == ("m.pt", "/data", "o")
    assert a.bsz == 4 and a.dtype == "bf16" and a.graph == 1 and a.label_groups is None and a.threshold == 0.5
    a = P.parser().parse_args(["--modelf", "m.pt", "--dataroot", "/data", "--out", "o", "--bsz", "8", "--dtype", "fp32",
                               "--graph", "0", "--label_groups", "0;1,2,3", "--final_h", "64", "--final_w", "192"])
    assert a.bsz == 8 and a.dtype == "fp32" and a.graph == 0 and a.label_groups == "0;1,2,3"
    gc, dac = P.confs(a)
    assert dac["final_dim"] == (64, 192) and dac["Ncams"] == 6 and gc["dbound"] == [4.0, 45.0, 1.0]
    for bad in (["--dataroot", "/data", "--out", "o"], ["--modelf", "m", "--dataroot", "d", "--out", "o", "--dtype", "fp16"],
                ["--modelf", "m", "--dataroot", "d", "--out", "o", "--graph", "2"]):
        with pytest.raises(SystemExit):
            P.parser().parse_args(bad)


def test_checkpoint_format_detection():
    sd = {"bevencode.up2.4.weight": torch.zeros(3, 128, 1, 1), "dx": torch.zeros(3)}
    assert P.checkpoint_format(sd) == "state_dict" and P.model_state_dict(sd) is sd
    wrapped = {"model_state_dict": sd, "optimizer_state_dict": {}, "counter": 7, "epoch": 0}
    assert P.checkpoint_format(wrapped) == "trainer" and P.model_state_dict(wrapped) is sd
    for bad in ([1, 2], {}, {"counter": 3}, {"model_state_dict": {"w": 1}}, None):
        with pytest.raises(ValueError):
            P.model_state_dict(bad)
    P.check_head(sd, 3)
    P.check_head({"dx": torch.zeros(3)}, 1)  # no head in the dict: load_state_dict's business
    with pytest.raises(RuntimeError, match="3 output classes.*the model has 1"):
        P.check_head(sd, 1)


def test_threshold_to_logit():
    assert P.threshold_logit(0.5) == 0.0
    assert P.threshold_logit(0.7) == pytest.approx(math.log(0.7 / 0.3), rel=1e-12)
    assert P.threshold_logit(0.25) == pytest.approx(-P.threshold_logit(0.75), rel=1e-12)
    for t in (0.1, 0.5, 0.9):
        assert torch.sigmoid(torch.tensor(P.threshold_logit(t), dtype=torch.float64)).item() == pytest.approx(t, rel=1e-12)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            P.threshold_logit(bad)


def test_clear_error_without_a_gpu(monkeypatch):
    assert L.Predictor is P.Predictor
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        P.Predictor(nn.Identity(), 2, "cpu")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        P.Predictor(nn.Identity(), 2, "cuda:0")
    a = P.parser().parse_args(["--modelf", "m.pt", "--dataroot", "/data", "--out", "o"])
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        P.predict(a)


def test_eval_batch_norm_guard_on_the_host():
    """CPU tensors never reach lss_bn_eval; the guard is false for them and bn_act is the stock op."""
    bn = nn.BatchNorm2d(8).eval()
    x = torch.randn(2, 8, 4, 6)
    assert norm.USE_HIP_BN_EVAL is True and not norm.eval_eligible(bn, x)
    with torch.no_grad():
        assert torch.equal(norm.bn_act(bn, x, "relu", x), torch.relu(bn(x) + x))
    assert norm.no_grad_wanted(x) and not norm.no_grad_wanted(x, bn.weight)
    with torch.no_grad():
        assert norm.no_grad_wanted(x, bn.weight)
