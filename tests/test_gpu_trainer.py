"""trainer.train on the SimBEV test tree (tests/golden/simbev_small): the captured step fed by the stager
against an eager TrainStep on simbev.finish_batch's tensors over two consecutive different batches (bars of
tests/test_gpu_captured_step.py: loss rtol 1e-5 / atol 1e-6, camencode.depthnet.weight's gradient within
1e-3 relative, every gradient within 2e-2); a full two-epoch run with validation and checkpoints; resume.

The comparison runs with ``torch.backends.cudnn.deterministic`` on (MIOpen's deterministic-solver attribute;
``benchmark`` stays off). At this shape (2 x 6 x 64 x 192, no find results) the solvers MIOpen otherwise
picks are not reproducible run to run, forward included: measured on an MI355X without the attribute, two
replays of the SAME graph from the same masters, inputs and seed differ in 17.6 k of the 80 k logits (max
3.1e-2), by 4.1e-3 - 7.2e-3 relative in camencode.depthnet.weight's gradient and by O(1) in the trunk's
_bn2.bias gradients (mathematically zero: the next batch norm removes a constant shift; norm ~1e-5, pure
rounding noise), and two eager steps differ likewise (2.6e-3 - 6.0e-3) -- no comparison of two runs can meet
1e-3 there, captured or not. With the attribute set, replay, second replay and eager step agree bit for bit
in the features, the BEV, the logits, the loss and every gradient, so the bars below hold with room."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import simbev, trainer  # noqa: E402
from lss_carla_amd.train_step import TrainStep  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.join(GOLDEN, "simbev_small")
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
KW = dict(H=56, W=120, resize_lim=(1.6, 1.8), final_dim=(64, 192), rot_lim=(-5.4, 5.4), rand_flip=True,
          bot_pct_lim=(0.0, 0.22), bsz=2, nworkers=0, use_wandb=False, miopen_find=False)


@pytest.fixture(autouse=True)
def _no_find():
    old = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    yield
    torch.backends.cudnn.benchmark = old


@pytest.fixture
def deterministic_solvers():
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def test_captured_step_over_the_stager_matches_eager_on_finish_batch(deterministic_solvers):
    tl, _ = simbev.compile_data("", ROOT, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV)
    np.random.seed(0)
    torch.manual_seed(0)
    raws = list(tl.loader)[:2]
    ctx = trainer.build_step(GC, DAC, 2, DEV)
    model, flat, masters, opt, stager, step = (ctx[k] for k in ("model", "flat", "masters", "opt", "stager", "step"))
    stager.stage(raws[0])
    stager.commit()
    step.capture(warmup=2)
    assert step.captured and step.skipped is not None and step.static_preds is not None
    snap = [m.detach().clone() for m in masters]

    def restore():
        with torch.no_grad():
            for m, s in zip(masters, snap):
                m.copy_(s)

    def graph_grads():
        out = {}
        for grp, gg in zip(flat.groups, step.graph_grads):
            out.update(grp.views_of(gg))
        return out

    losses = []
    for i, raw in enumerate(raws):
        stager.stage(raw)
        stager.commit()
        restore()
        torch.cuda.manual_seed(1000 + i)
        step()
        torch.cuda.synchronize()
        rep_loss = step.static_loss.clone()
        rep = {k: v.detach().clone() for k, v in graph_grads().items()}
        preds = step.static_preds.clone()
        # eager, from the same masters and the same Philox stream, on finish_batch's tensors (its host
        # copies of the rig feed the reference's host torch.inverse)
        restore()
        want = simbev.finish_batch(raw, DAC["final_dim"], DEV)
        model.static_inverses = None
        try:
            eager = TrainStep(ctx["forward"], want[:6], want[6], ctx["loss_fn"], opt, masters, all_reduce=False,
                              amp_dtype=torch.bfloat16, max_grad_norm=5.0, keep_preds=True)
            torch.cuda.manual_seed(1000 + i)
            loss_e = eager.forward_backward().detach()
            torch.cuda.synchronize()
        finally:
            model.static_inverses = (stager.hinv.pinv, stager.hinv.kinv)
        eag = flat.views(grads=True)
        print(f"batch {i}: loss captured {rep_loss.item():.7f} eager {loss_e.item():.7f}")
        k = "camencode.depthnet.weight"
        rel = ((rep[k] - eag[k]).norm() / eag[k].norm()).item()
        diffs = []
        for name, e in eag.items():
            en = e.norm().item()
            if en < 1e-6:
                continue
            diffs.append((((rep[name] - e).norm() / en).item(), name))
        diffs.sort(reverse=True)
        print(f"batch {i}: depthnet.weight grad rel diff {rel:.3e}; worst {diffs[:3]}")
        torch.testing.assert_close(rep_loss, loss_e, rtol=1e-5, atol=1e-6)
        assert rel < 1e-3, (i, rel)
        assert len(diffs) > 100 and diffs[0][0] < 2e-2, diffs[0]
        assert preds.shape == stager.binimgs.shape and torch.isfinite(preds.float()).all()
        losses.append(rep_loss.item())
    assert losses[0] != losses[1]
    assert step.skipped.item() == 0


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    logdir = tmp_path_factory.mktemp("run1")
    old = torch.backends.cudnn.benchmark
    seen = {}

    def on_start(ctx):
        seen["initial"] = {k: v.detach().cpu().clone() for k, v in ctx["flat"].views().items()}
        seen["counter"], seen["epoch"] = ctx["counter"], ctx["epoch"]

    out = trainer.train(ROOT, nepochs=2, val_step=3, save_step=4, seed=0, logdir=str(logdir), loss_step=2,
                        on_start=on_start, **KW)
    torch.backends.cudnn.benchmark = old
    return logdir, out, seen


def test_full_run_writes_checkpoints_and_metrics(full_run):
    logdir, out, seen = full_run
    assert out["counter"] == 8 and out["epoch"] == 2 and out["skipped"] == 0
    assert (seen["counter"], seen["epoch"]) == (0, 0)
    for name in ("model_000004.pt", "model_000008.pt", "model_final.pt", "model_best.pt"):
        assert (logdir / name).exists(), name
    events = [json.loads(line) for line in open(logdir / "metrics.jsonl")]
    train_ev = [e for e in events if e["event"] == "train"]
    val_ev = [e for e in events if e["event"] == "val"]
    final = [e for e in events if e["event"] == "final"]
    assert [e["counter"] for e in train_ev] == [2, 4, 6, 8]
    assert all(math.isfinite(e["loss"]) and e["loss"] > 0 for e in train_ev)
    assert [e["counter"] for e in val_ev] == [3, 6]
    assert all(math.isfinite(e["loss"]) and 0.0 <= e["iou"] <= 1.0 for e in val_ev)
    assert len(final) == 1 and final[0]["skipped"] == 0 and final[0]["counter"] == 8
    assert math.isfinite(final[0]["loss"])
    ck = torch.load(logdir / "model_final.pt", map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "counter", "epoch"}
    assert ck["counter"] == 8 and ck["epoch"] == 2
    best = torch.load(logdir / "model_best.pt", map_location="cpu")
    assert best["counter"] in (3, 6) and best["val_iou"] == max(e["iou"] for e in val_ev)
    mid = torch.load(logdir / "model_000004.pt", map_location="cpu")
    assert mid["counter"] == 4 and mid["epoch"] == 0
    steps = {float(e["step"]) for e in mid["optimizer_state_dict"]["state"].values()}
    assert steps == {4.0}, "the capture's warm-up steps must not count"
    # training moved the parameters, and every one of them is finite
    for k, v in ck["model_state_dict"].items():
        assert torch.isfinite(v.float()).all(), k
    moved = sum(int(not torch.equal(v, ck["model_state_dict"][k])) for k, v in seen["initial"].items())
    assert moved > len(seen["initial"]) // 2, (moved, len(seen["initial"]))


def test_resume_starts_from_the_checkpoint(full_run, tmp_path):
    logdir, _, _ = full_run
    path = logdir / "model_000004.pt"
    ck = torch.load(path, map_location="cpu")
    seen = {}

    def on_start(ctx):
        flat, opt = ctx["flat"], ctx["opt"]
        seen["counter"], seen["epoch"] = ctx["counter"], ctx["epoch"]
        seen["params"] = {k: v.detach().cpu().clone() for k, v in flat.views().items()}
        avg, sq, step = {}, {}, {}
        for grp in flat.groups:
            st = opt.state[grp.master]
            avg.update({k: v.detach().cpu().clone() for k, v in grp.views_of(st["exp_avg"]).items()})
            sq.update({k: v.detach().cpu().clone() for k, v in grp.views_of(st["exp_avg_sq"]).items()})
            step.update({k: float(st["step"]) for k in grp.views_of(st["exp_avg"])})
        seen["avg"], seen["sq"], seen["step"] = avg, sq, step
        seen["names"] = [n for n, _ in ctx["model"].named_parameters()]
        seen["buffers"] = {k: v.detach().cpu().clone() for k, v in ctx["model"].state_dict().items()}

    out = trainer.train(ROOT, nepochs=2, val_step=3, save_step=4, seed=0, logdir=str(tmp_path), loss_step=2,
                        resume=str(path), max_steps=1, on_start=on_start, **KW)
    assert (seen["counter"], seen["epoch"]) == (4, ck["epoch"]) and out["counter"] == 5
    # before its first step: masters, Adam state and buffers bit-equal to the file's contents
    for k, v in ck["model_state_dict"].items():
        assert torch.equal(seen["buffers"][k], v), k
    state = ck["optimizer_state_dict"]["state"]
    assert len(state) == len(seen["params"])
    for name in seen["params"]:
        e = state[seen["names"].index(name)]
        assert torch.equal(seen["params"][name], ck["model_state_dict"][name]), name
        assert torch.equal(seen["avg"][name], e["exp_avg"]) and torch.equal(seen["sq"][name], e["exp_avg_sq"]), name
        assert seen["step"][name] == float(e["step"]) == 4.0
    assert (tmp_path / "model_final.pt").exists()
    assert torch.load(tmp_path / "model_final.pt", map_location="cpu")["counter"] == 5
