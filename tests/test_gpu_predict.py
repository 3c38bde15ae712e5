"""predict.Predictor and the command line's entry function on the MI355X: the graph replay against the eager
eval / no_grad / autocast forward, partial batches, the outputs, the module's state, both checkpoint formats,
and ``python -m lss_carla_amd.predict``'s work over tests/golden/simbev_small against tools.get_val_info
(bars of tests/test_gpu_val.py: loss rel 1e-6, intersection and union equal)."""
import copy
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import predict as P, simbev, tools as T  # noqa: E402
from lss_carla_amd import synthetic as syn  # noqa: E402

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
ROOT = os.path.join(GOLDEN, "simbev_small")
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
B, N = 2, 6
RIG = ("rots", "trans", "intrins", "post_rots", "post_trans")


def _model(seed, outC=1):
    torch.manual_seed(seed)
    m = L.compile_model(GC, DAC, outC=outC).to(DEV)
    m.bevencode.to(memory_format=torch.channels_last)
    m.camencode.up1.to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():  # running statistics a trained network would have (fresh ones are 0 / 1)
        for bn in (x for x in m.modules() if isinstance(x, nn.BatchNorm2d)):
            bn.running_mean.copy_(torch.empty(bn.num_features).normal_(0, 0.1, generator=g))
            bn.running_var.copy_(torch.empty(bn.num_features).uniform_(0.5, 1.5, generator=g))
    return m.train()


def _host_inputs(seed, b=B):
    rig = syn.make_rig(b, N, DAC["final_dim"], seed=seed)
    return (syn.make_images(b, N, DAC["final_dim"], seed=seed), *(rig[k] for k in RIG))


def _eager(model, inputs):
    """The plain eval / no_grad / autocast forward (host torch.inverse inside, as the reference)."""
    was = model.training
    model.eval()
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
            return model(*(t.to(DEV) for t in inputs))
    finally:
        model.train(was)


@pytest.fixture(scope="module")
def setup():
    """cudnn.benchmark off as in tests/test_gpu_eval_step.py, and cudnn.deterministic on: two eager bf16 forwards
    of this model over the same inputs already differ in the last bits of some 3 x 3 convolutions' outputs
    (MIOpen's default solvers; the fp32 forward repeats exactly), which a bit-for-bit comparison of two forwards
    would otherwise be a test of."""
    old = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    model = _model(0)
    state = copy.deepcopy(model.state_dict())
    p = L.Predictor(model, B, DEV, amp_dtype=BF16, threshold=0.5, graph=True)
    assert model.training, "construction must restore the module's mode"
    yield model, p, state
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = old


def test_replay_matches_eager_and_inputs_are_refreshed(setup):
    model, p, state = setup
    for seed in (0, 1):  # the second rig differs: static inputs and inverses are refreshed per call
        inputs = _host_inputs(seed)
        got = p(*inputs)
        assert p.graph is not None and got.shape == (B, 1, 200, 200)
        want = _eager(model, inputs)
        assert torch.equal(got, want), f"rig {seed}: max diff {(got.float() - want.float()).abs().max().item()}"
    assert not torch.equal(_eager(model, _host_inputs(0)), _eager(model, _host_inputs(1)))
    # state after calls: the mode flag and every parameter and buffer
    assert model.training
    now = model.state_dict()
    assert list(now) == list(state)
    for k, v in state.items():
        assert torch.equal(v, now[k]), k


def test_partial_batch_and_outputs(setup):
    model, p, _ = setup
    inputs = _host_inputs(2)
    full = p(*inputs).clone()
    assert torch.equal(p.masks(), (full > 0).to(torch.uint8)) and p.masks().dtype == torch.uint8
    assert torch.equal(p.probs(), full.float().sigmoid()) and p.probs().dtype == torch.float32
    one = p(*(t[:1] for t in inputs))
    assert one.shape == (1, 1, 200, 200) and torch.equal(one, full[:1])
    assert p.masks().shape == (1, 1, 200, 200) and p.probs().shape == (1, 1, 200, 200)
    dev_in = tuple(t.to(DEV) for t in inputs)  # device tensors too
    assert torch.equal(p(*dev_in), full)
    with pytest.raises(ValueError):
        p(*(torch.cat([t, t]) for t in inputs))
    p7 = L.Predictor(_model(4), B, DEV, threshold=0.7, graph=False)  # eager, another threshold
    out = p7(*inputs)
    assert p7.graph is None and torch.equal(p7.masks(), (out > float(np.log(0.7 / (1.0 - 0.7)))).to(torch.uint8))


def test_load_both_formats_and_wrong_head(setup, tmp_path):
    model, p, _ = setup
    inputs = _host_inputs(3)
    before = p(*inputs).clone()
    other = _model(7)
    sd = {k: v.detach().cpu().clone() for k, v in other.state_dict().items()}
    want = _eager(other, inputs)
    assert not torch.equal(want, before)
    plain, wrapped = tmp_path / "plain.pt", tmp_path / "wrapped.pt"
    torch.save(sd, plain)
    torch.save({"model_state_dict": sd, "counter": 5, "epoch": 1}, wrapped)
    for path in (plain, wrapped):
        with torch.no_grad():  # scramble a weight so each load is seen to act
            model.bevencode.up2[4].weight.add_(1.0)
        p.refresh()
        assert not torch.equal(p(*inputs), want)
        p.load(path)
        assert torch.equal(p(*inputs), want), path
    # a head of another width: refused before anything is loaded or captured
    wide = _model(9, outC=3)
    bad = tmp_path / "wide.pt"
    torch.save({k: v.detach().cpu() for k, v in wide.state_dict().items()}, bad)
    kept = copy.deepcopy(model.state_dict())
    with pytest.raises(RuntimeError, match="3 output classes"):
        p.load(bad)
    for k, v in kept.items():
        assert torch.equal(v, model.state_dict()[k]), k
    fresh = L.Predictor(_model(11), B, DEV)
    with pytest.raises(RuntimeError, match="3 output classes"):
        fresh.load(bad)
    assert fresh.graph is None


def test_command_line_entry_function(tmp_path):
    old = torch.backends.cudnn.benchmark
    try:
        model = _model(5)
        ckpt = tmp_path / "model.pt"
        torch.save(model.state_dict(), ckpt)
        out = tmp_path / "pred"
        a = P.parser().parse_args(["--modelf", str(ckpt), "--dataroot", ROOT, "--out", str(out), "--bsz", "2",
                                   "--dtype", "fp32", "--nworkers", "0", "--miopen_find", "0"])
        info = P.predict(a, grid_conf=GC, data_aug_conf=DAC)
        _, vl = simbev.compile_data("", ROOT, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV)
        n_val = len(vl.dataset)
        files = sorted(f for f in os.listdir(out) if f.endswith(".npy"))
        assert files == sorted(f"{i}.npy" for i in range(n_val)) and n_val > 0
        for f in files:
            m = np.load(out / f)
            assert m.shape == (1, 200, 200) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}
        on_disk = json.load(open(out / "metrics.json"))
        assert on_disk == json.loads(json.dumps(info)) and on_disk["samples"] == n_val
        # get_val_info on the same model (fp32, eager), and the totals it divides
        ref_model = L.compile_model(GC, DAC, outC=1).to(DEV)
        ref_model.load_state_dict(torch.load(ckpt))
        ref_model.bevencode.to(memory_format=torch.channels_last)
        ref_model.camencode.up1.to(memory_format=torch.channels_last)
        loss_fn = T.SimpleLoss(2.13).to(DEV)
        want = T.get_val_info(ref_model, vl, loss_fn, DEV, use_tqdm=False)
        ref_model.eval()
        _, inter, union = (t.item() for t in T.val_totals(ref_model, vl, loss_fn, DEV))
        print(f"predict: {on_disk}; get_val_info: {want}; totals {inter} / {union}")
        assert on_disk["loss"] == pytest.approx(want["loss"], rel=1e-6)
        assert on_disk["intersection"] == [inter] and on_disk["union"] == [union]
        assert on_disk["iou"] == pytest.approx(want["iou"], rel=1e-12)
    finally:
        torch.backends.cudnn.benchmark = old
