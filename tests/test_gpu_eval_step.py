"""train_step.EvalStep: the validation step captured as one HIP graph over the stager's static tensors,
against tools.val_totals under the same autocast -- over the val split with a stager of the batch's size,
and with a 3-sample stager fed the 2-sample batch (n_valid = 2, read on the device). Bars of
tests/test_gpu_val.py: loss rel 1e-6, intersection and union equal."""
import os

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import parallel, simbev, tools as T  # noqa: E402
from lss_carla_amd.flat_params import FlatParamGroups, lss_backward_groups  # noqa: E402
from lss_carla_amd.staging import BatchStager  # noqa: E402
from lss_carla_amd.train_step import EvalStep  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.join(GOLDEN, "simbev_small")
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
PW = 2.13


@pytest.fixture(scope="module")
def setup():
    old = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    _, vl = simbev.compile_data("", ROOT, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV)
    raws = list(vl.loader)
    torch.manual_seed(0)
    model = L.compile_model(GC, DAC, outC=1).to(DEV)
    model.bevencode.to(memory_format=torch.channels_last)
    model.train()
    parallel.freeze_unused(model)
    flat = FlatParamGroups(model, lss_backward_groups(), cast_dtype=torch.bfloat16)
    forward = flat.bind(model)
    # the reference: tools.val_totals over finish_batch's tensors, same autocast, the model in eval mode
    model.eval()
    model.static_inverses = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        want = [t.item() for t in T.val_totals(forward, [simbev.finish_batch(r, DAC["final_dim"], DEV) for r in raws],
                                               T.SimpleLoss(PW).to(DEV), DEV)]
    model.train()
    yield model, forward, raws, len(vl.dataset), want
    torch.backends.cudnn.benchmark = old


@pytest.mark.parametrize("B", [2, 3], ids=["full_batch", "two_of_three_samples"])
def test_captured_eval_step_matches_val_totals(setup, B):
    model, forward, raws, n_val, want = setup
    assert n_val == 2 and len(raws) == 1 and want[2] > 0
    st = BatchStager(DAC["final_dim"], B, 6, (DAC["H"], DAC["W"]), GC, DEV)
    model.static_inverses = (st.hinv.pinv, st.hinv.kinv)
    ev = EvalStep(model, forward, st.inputs, st.binimgs, n_valid=st.n_valid, pos_weight=PW,
                  amp_dtype=torch.bfloat16, n_samples=n_val)
    st.stage(raws[0])
    st.commit()
    ev.capture(warmup=1)
    assert ev.captured and model.training, "the capture must restore the module's mode"
    assert ev.totals.tolist() == [0.0, 0.0, 0.0]
    for _ in range(2):  # reset -> replay per batch -> read, twice: the totals restart
        ev.reset()
        for i, raw in enumerate(raws):
            if i:
                st.stage(raw)
                st.commit()
            ev()
        got = ev.totals.tolist()
        info = ev.read()
        print(f"B={B}: captured totals {got}, val_totals {want}")
        assert got[0] == pytest.approx(want[0], rel=1e-6) and got[1] == want[1] and got[2] == want[2]
        assert info["loss"] == pytest.approx(want[0] / n_val, rel=1e-6)
        assert info["iou"] == want[1] / want[2]
    model.static_inverses = None


def test_eager_eval_step_and_empty_union():
    """An eager EvalStep over a toy forward: get_val_info's definitions, ZeroDivisionError on an empty union."""
    x = torch.full((2, 1, 5, 5), -1.0, device=DEV)
    y = torch.zeros(2, 1, 5, 5, device=DEV)
    net = torch.nn.Identity()
    ev = EvalStep(net, lambda a: a, (x,), y, pos_weight=PW, amp_dtype=None, n_samples=2)
    ev()
    with pytest.raises(ZeroDivisionError):
        ev.read()
    y[0, 0, 1, 1] = 1.0
    x[0, 0, 1, 1] = 2.0
    x[1, 0, 0, 0] = 3.0
    ev.reset()
    ev()
    info = ev.read()
    want = torch.nn.functional.binary_cross_entropy_with_logits(x.double().cpu(), y.double().cpu(),
                                                                pos_weight=torch.tensor([PW], dtype=torch.float64))
    assert info["iou"] == 0.5 and info["loss"] == pytest.approx(want.item(), rel=2e-6)
