"""trainer.build_step / trainer.train with loss="focal" and three class groups on tests/golden/simbev_small, at
the sizes of tests/test_gpu_trainer_multiclass.py: the captured step fed by the stager against an eager TrainStep
on simbev.finish_batch's tensors from the same masters (that file's comparison and bars: loss rtol 1e-5 / atol
1e-6, camencode.depthnet.weight's gradient within 1e-3 relative, every gradient within 2e-2, MIOpen's
deterministic solvers on); a short run with a threshold ladder writes the ladder's keys into its ``val`` events and
a ``config`` event, a best checkpoint, and resumes; predict on the result writes the ladder's keys and masks at one
threshold per class. (That the loss decreases over four steps is not asserted.)"""
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

from lss_carla_amd import predict as P, simbev, tools, trainer  # noqa: E402
from lss_carla_amd.train_step import TrainStep  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.join(GOLDEN, "simbev_small")
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
KW = dict(H=56, W=120, resize_lim=(1.6, 1.8), final_dim=(64, 192), rot_lim=(-5.4, 5.4), rand_flip=True,
          bot_pct_lim=(0.0, 0.22), bsz=2, nworkers=0, use_wandb=False, miopen_find=False)
GROUPS = [[0], [1, 2, 3], [6, 7]]
GAMMA = [2.0, 1.0, 0.5]
ALPHA = [0.25, 0.5, 0.75]
LADDER = [0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65]


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


def test_captured_focal_step_matches_eager_on_finish_batch(deterministic_solvers, monkeypatch):
    from lss_carla_amd import _lib
    launched = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (launched.append(what), real(code, what))[1])
    tl, _ = simbev.compile_data("", ROOT, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV,
                                label_groups=GROUPS)
    np.random.seed(0)
    torch.manual_seed(0)
    raws = list(tl.loader)[:2]
    ctx = trainer.build_step(GC, DAC, 2, DEV, label_groups=GROUPS, loss="focal", focal_gamma=GAMMA, focal_alpha=ALPHA,
                             iou_thresholds=LADDER)
    model, flat, masters, opt, stager, step = (ctx[k] for k in ("model", "flat", "masters", "opt", "stager", "step"))
    assert isinstance(ctx["loss_fn"], tools.FocalLoss) and ctx["loss_fn"].focal_params.is_cuda
    assert ctx["loss_fn"].focal_params.cpu().tolist() == [[0.25, 0.75, 2.0], [0.5, 0.5, 1.0], [0.75, 0.25, 0.5]]
    assert ctx["evaluate"].params is ctx["loss_fn"].focal_params and ctx["evaluate"].columns == LADDER
    assert model.bevencode.up2[4].out_channels == 3 and stager.binimgs.shape == (2, 3, 200, 200)
    stager.stage(raws[0])
    stager.commit()
    step.capture(warmup=2)
    assert "lss_focal_logits_pc" in launched and "lss_bce_logits_bwd" in launched
    assert "lss_bce_logits_pc" not in launched and "lss_bce_logits" not in launched
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
        restore()
        want = simbev.finish_batch(raw, DAC["final_dim"], DEV, label_groups=GROUPS)
        assert torch.equal(want[6], stager.binimgs)
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
        assert preds.shape == stager.binimgs.shape == (2, 3, 200, 200) and torch.isfinite(preds.float()).all()
        # the step's loss is the focal loss of the logits it kept
        ref = tools._FocalTorch.apply(preds, stager.binimgs, ctx["loss_fn"].focal_params)
        torch.testing.assert_close(rep_loss, ref, rtol=1e-5, atol=1e-6)
        losses.append(rep_loss.item())
    assert losses[0] != losses[1]
    assert step.skipped.item() == 0


@pytest.fixture(scope="module")
def short_run(tmp_path_factory):
    logdir = tmp_path_factory.mktemp("run_focal")
    old = torch.backends.cudnn.benchmark
    out = trainer.train(ROOT, nepochs=1, val_step=2, save_step=4, seed=0, logdir=str(logdir), loss_step=2, iou_step=2,
                        label_groups=GROUPS, loss="focal", focal_gamma=GAMMA, focal_alpha=ALPHA, iou_thresholds=LADDER,
                        **KW)
    torch.backends.cudnn.benchmark = old
    return logdir, out


def test_short_run_writes_the_ladder_and_the_config(short_run):
    logdir, out = short_run
    assert out["counter"] == 4 and out["skipped"] == 0
    events = [json.loads(line) for line in open(logdir / "metrics.jsonl")]
    assert events[0]["event"] == "config" and events[0]["loss"] == "focal" and events[0]["iou_thresholds"] == LADDER
    assert events[0]["focal_gamma"] == GAMMA and events[0]["focal_alpha"] == ALPHA and events[0]["label_groups"] == GROUPS
    val_ev = [e for e in events if e["event"] == "val"]
    assert [e["counter"] for e in val_ev] == [2, 4]
    for e in val_ev:
        assert math.isfinite(e["loss"]) and e["loss"] > 0
        per, best, at = e["iou_per_class"], e["iou_max_per_class"], e["best_threshold_per_class"]
        assert len(per) == len(best) == len(at) == 3
        for k in range(3):  # every group has labels in the val split: a union at every threshold
            assert per[k] is not None and 0.0 <= per[k] <= best[k] <= 1.0 and at[k] in LADDER
        assert e["iou"] == pytest.approx(sum(per) / 3, rel=1e-12)
        assert e["iou_max"] == pytest.approx(sum(best) / 3, rel=1e-12) and e["iou_max"] >= e["iou"]
    assert all(math.isfinite(e["loss"]) for e in events if e["event"] == "train")
    ck = torch.load(logdir / "model_best.pt", map_location="cpu")
    assert ck["model_state_dict"]["bevencode.up2.4.weight"].shape == (3, 128, 1, 1)
    assert ck["val_iou"] == pytest.approx(max(e["iou"] for e in val_ev), rel=1e-12)  # chosen by iou, not iou_max
    assert (logdir / "model_000004.pt").exists() and (logdir / "model_final.pt").exists()


def test_resume_and_predict_with_thresholds_per_class(short_run, tmp_path, deterministic_solvers):
    logdir, _ = short_run
    path = logdir / "model_000004.pt"
    ck = torch.load(path, map_location="cpu")
    seen = {}

    def on_start(ctx):
        seen["counter"] = ctx["counter"]
        seen["head"] = ctx["flat"].views()["bevencode.up2.4.weight"].detach().cpu().clone()

    out = trainer.train(ROOT, nepochs=2, val_step=100, save_step=100, seed=0, logdir=str(tmp_path / "resumed"),
                        resume=str(path), max_steps=1, on_start=on_start, label_groups=GROUPS, loss="focal",
                        focal_gamma=GAMMA, focal_alpha=ALPHA, **KW)
    assert seen["counter"] == 4 and out["counter"] == 5 and math.isfinite(out["loss"])
    assert torch.equal(seen["head"], ck["model_state_dict"]["bevencode.up2.4.weight"])

    pred = tmp_path / "pred"
    a = P.parser().parse_args(["--modelf", str(path), "--dataroot", ROOT, "--out", str(pred), "--bsz", "2",
                               "--nworkers", "0", "--miopen_find", "0", "--label_groups", "0;1,2,3;6,7",
                               "--loss", "focal", "--focal_gamma", "2.0,1.0,0.5", "--focal_alpha", "0.25,0.5,0.75",
                               "--iou_thresholds", "0.35,0.4,0.45,0.5,0.55,0.6,0.65", "--threshold", "0.4,0.5,0.6"])
    info = P.predict(a, grid_conf=GC, data_aug_conf=DAC)
    on_disk = json.load(open(pred / "metrics.json"))
    assert on_disk == json.loads(json.dumps(info))
    assert info["loss_kind"] == "focal" and info["iou_thresholds"] == LADDER and info["threshold"] == [0.4, 0.5, 0.6]
    assert info["classes"] == 3 and info["samples"] == 2 and math.isfinite(info["loss"]) and info["loss"] > 0
    assert len(info["iou_at"]) == len(LADDER) and all(len(r) == 3 for r in info["iou_at"])
    assert info["iou_per_class"] == info["iou_at"][LADDER.index(0.5)]
    assert info["iou_max_per_class"] == [max(r[k] for r in info["iou_at"]) for k in range(3)]
    assert all(v in LADDER for v in info["best_threshold_per_class"])
    # the masks are the K-threshold predicate: their per-class positive fractions fall as the thresholds rise past
    # what a single 0.5 gives, and class 1 (at 0.5) carries exactly the 0.5 column's predicted positives
    masks = np.stack([np.load(pred / f"{i}.npy") for i in range(2)])
    assert masks.shape == (2, 3, 200, 200) and masks.dtype == np.uint8 and set(np.unique(masks)) <= {0, 1}
    # (two forwards of this model agree bit for bit only under MIOpen's deterministic solvers: the fixture)
    a5 = P.parser().parse_args(["--modelf", str(path), "--dataroot", ROOT, "--out", str(tmp_path / "pred5"), "--bsz", "2",
                                "--nworkers", "0", "--miopen_find", "0", "--label_groups", "0;1,2,3;6,7"])
    info5 = P.predict(a5, grid_conf=GC, data_aug_conf=DAC)
    masks5 = np.stack([np.load(tmp_path / "pred5" / f"{i}.npy") for i in range(2)])
    assert info5["loss_kind"] == "bce" and "iou_at" not in info5
    assert info5["iou_per_class"] == info["iou_per_class"]  # the 0.5 column is today's predicate
    assert np.array_equal(masks[:, 1], masks5[:, 1])
    assert (masks[:, 0] >= masks5[:, 0]).all() and (masks[:, 2] <= masks5[:, 2]).all()
