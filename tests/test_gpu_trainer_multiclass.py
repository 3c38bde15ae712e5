"""trainer.build_step / trainer.train with label_groups=[[0], [1, 2, 3]] (two output classes) on a synthetic
SimBEV tree with boxes in channels 0-3, at the sizes of tests/test_gpu_trainer.py: the captured step fed by the
stager against an eager TrainStep on simbev.finish_batch's tensors (that test's comparison and bars: loss
rtol 1e-5 / atol 1e-6, camencode.depthnet.weight's gradient within 1e-3 relative, every gradient within 2e-2,
MIOpen's deterministic solvers on); a short run writes per-class IoUs and a two-class checkpoint, resumes from
it, and refuses a one-class checkpoint."""
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import simbev, synthetic, trainer  # noqa: E402
from lss_carla_amd.train_step import TrainStep  # noqa: E402

DEV = torch.device("cuda:0")
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
KW = dict(H=56, W=120, resize_lim=(1.6, 1.8), final_dim=(64, 192), rot_lim=(-5.4, 5.4), rand_flip=True,
          bot_pct_lim=(0.0, 0.22), bsz=2, nworkers=0, use_wandb=False, miopen_find=False)
GROUPS = [[0], [1, 2, 3]]
PW = [1.0, 2.13]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    d = tmp_path_factory.mktemp("simbev_multiclass")
    assert synthetic.make_simbev_tree(str(d), n_scenes=5, per_scene=2, H=56, W=120, seed=1,
                                      box_classes=(0, 1, 2, 3)) == 10
    return str(d)


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


def test_captured_two_class_step_matches_eager_on_finish_batch(root, deterministic_solvers, monkeypatch):
    from lss_carla_amd import _lib
    launched = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (launched.append(what), real(code, what))[1])
    tl, _ = simbev.compile_data("", root, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV,
                                label_groups=GROUPS)
    np.random.seed(0)
    torch.manual_seed(0)
    raws = list(tl.loader)[:2]
    ctx = trainer.build_step(GC, DAC, 2, DEV, label_groups=GROUPS, pos_weight=PW)
    model, flat, masters, opt, stager, step = (ctx[k] for k in ("model", "flat", "masters", "opt", "stager", "step"))
    assert model.bevencode.up2[4].out_channels == 2 and stager.binimgs.shape == (2, 2, 200, 200)
    stager.stage(raws[0])
    stager.commit()
    step.capture(warmup=2)
    # the step ran the K-channel head, the per-class loss and the class-group labels
    for name in ("lss_headk_fwd", "lss_headk_bwd", "lss_bce_logits_pc", "lss_simbev_class_masks"):
        assert name in launched, name
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
        assert preds.shape == stager.binimgs.shape == (2, 2, 200, 200) and torch.isfinite(preds.float()).all()
        assert eag["bevencode.up2.4.weight"].shape == (2, 128, 1, 1)
        losses.append(rep_loss.item())
    assert losses[0] != losses[1]
    assert step.skipped.item() == 0


@pytest.fixture(scope="module")
def short_run(root, tmp_path_factory):
    logdir = tmp_path_factory.mktemp("run_multiclass")
    old = torch.backends.cudnn.benchmark
    out = trainer.train(root, nepochs=1, val_step=2, save_step=4, seed=0, logdir=str(logdir), loss_step=2, iou_step=2,
                        label_groups=GROUPS, pos_weight=PW, **KW)
    torch.backends.cudnn.benchmark = old
    return logdir, out


def test_short_run_writes_per_class_iou_and_a_two_class_checkpoint(short_run):
    logdir, out = short_run
    assert out["counter"] == 4 and out["skipped"] == 0
    events = [json.loads(line) for line in open(logdir / "metrics.jsonl")]
    val_ev = [e for e in events if e["event"] == "val"]
    iou_ev = [e for e in events if e["event"] == "train_iou"]
    assert [e["counter"] for e in val_ev] == [2, 4] and [e["counter"] for e in iou_ev] == [2, 4]
    for e in val_ev + iou_ev:
        per = e["iou_per_class"]
        assert len(per) == 2 and all(v is None or 0.0 <= v <= 1.0 for v in per)
        seen = [v for v in per if v is not None]
        if seen:
            assert e["iou"] == pytest.approx(sum(seen) / len(seen), rel=1e-12)
    assert all(math.isfinite(e["loss"]) for e in val_ev)
    ck = torch.load(logdir / "model_000004.pt", map_location="cpu")
    assert ck["model_state_dict"]["bevencode.up2.4.weight"].shape == (2, 128, 1, 1)
    assert ck["model_state_dict"]["bevencode.up2.4.bias"].shape == (2,)
    assert (logdir / "model_best.pt").exists() and (logdir / "model_final.pt").exists()


def test_resume_two_class_and_refuse_one_class(short_run, root, tmp_path):
    logdir, _ = short_run
    path = logdir / "model_000004.pt"
    ck = torch.load(path, map_location="cpu")
    seen = {}

    def on_start(ctx):
        seen["counter"] = ctx["counter"]
        seen["head"] = ctx["flat"].views()["bevencode.up2.4.weight"].detach().cpu().clone()

    out = trainer.train(root, nepochs=2, val_step=100, save_step=100, seed=0, logdir=str(tmp_path / "resumed"),
                        resume=str(path), max_steps=1, on_start=on_start, label_groups=GROUPS, pos_weight=PW, **KW)
    assert seen["counter"] == 4 and out["counter"] == 5
    assert torch.equal(seen["head"], ck["model_state_dict"]["bevencode.up2.4.weight"])

    # a one-class checkpoint (a bare state dict, as the reference also saves) against a two-class run, and the
    # two-class checkpoint against the default one-class run: refused with both numbers, before any capture
    one = tmp_path / "one_class.pt"
    torch.save(L.compile_model(GC, DAC, outC=1).state_dict(), one)
    captured = []
    with pytest.raises(RuntimeError, match=r"1 output classes.*ask for 2"):
        trainer.train(root, nepochs=1, seed=0, logdir=str(tmp_path / "refused"), resume=str(one), max_steps=1,
                      on_start=captured.append, label_groups=GROUPS, pos_weight=PW, **KW)
    with pytest.raises(RuntimeError, match=r"2 output classes.*ask for 1"):
        trainer.train(root, nepochs=1, seed=0, logdir=str(tmp_path / "refused1"), resume=str(path), max_steps=1,
                      on_start=captured.append, **KW)
    assert not captured
