"""trainer.train with a learning-rate schedule and EMA weights on the SimBEV test tree (tests/golden/simbev_small; the
sizes and keywords of tests/test_gpu_trainer.py's full run: bsz 2, 64 x 192, 8 steps): the captured update follows the
schedule, validation runs on the averaged weights, the checkpoint carries ``ema_state_dict``, a resumed run continues
the schedule and the EMA, and Predictor.load chooses between the two sets of weights. One run and one resume,
module-scoped."""
import json
import os

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import synthetic as syn, trainer  # noqa: E402
from lss_carla_amd.optim import LRSchedule  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.join(GOLDEN, "simbev_small")
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
KW = dict(H=56, W=120, resize_lim=(1.6, 1.8), final_dim=(64, 192), rot_lim=(-5.4, 5.4), rand_flip=True,
          bot_pct_lim=(0.0, 0.22), bsz=2, nworkers=0, use_wandb=False, miopen_find=False)
SCHED_KW = dict(lr_schedule="cosine", warmup_steps=2, lr_total_steps=8, ema_decay=0.9, graph=True)
SCHED = LRSchedule("cosine", warmup_steps=2, warmup_factor=0.0, total_steps=8, min_factor=0.0)
LR = 1e-3


def _events(logdir):
    return [json.loads(line) for line in open(os.path.join(str(logdir), "metrics.jsonl"))]


def _start_state(ctx):
    flat = ctx["flat"]
    return {"counter": ctx["counter"], "epoch": ctx["epoch"],
            "params": {k: v.detach().cpu().clone() for k, v in flat.views().items()},
            "ema": {k: v.detach().cpu().clone() for k, v in flat.views(ema=True).items()}}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    old = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    logdir, resumed = tmp_path_factory.mktemp("sched"), tmp_path_factory.mktemp("sched_resume")
    seen, seen_r = {}, {}
    out = trainer.train(ROOT, nepochs=2, val_step=3, save_step=4, seed=0, logdir=str(logdir), loss_step=2,
                        on_start=lambda ctx: seen.update(_start_state(ctx)), **SCHED_KW, **KW)
    out_r = trainer.train(ROOT, nepochs=2, val_step=3, save_step=4, seed=0, logdir=str(resumed), loss_step=1,
                          resume=str(logdir / "model_000004.pt"), max_steps=1,
                          on_start=lambda ctx: seen_r.update(_start_state(ctx)), **SCHED_KW, **KW)
    torch.backends.cudnn.benchmark = old
    return {"logdir": logdir, "out": out, "seen": seen, "resumed": resumed, "out_r": out_r, "seen_r": seen_r}


def test_run_follows_the_schedule_and_validates_on_the_ema(runs):
    logdir, out, seen = runs["logdir"], runs["out"], runs["seen"]
    assert out["counter"] == 8 and out["skipped"] == 0 and seen["counter"] == 0
    events = _events(logdir)
    assert events[0]["event"] == "config" and events[0]["lr_schedule"] == "cosine" and events[0]["ema_decay"] == 0.9
    assert events[0]["lr_total_steps"] == 8 and events[0]["warmup_steps"] == 2
    train_ev = [e for e in events if e["event"] == "train"]
    assert [e["counter"] for e in train_ev] == [2, 4, 6, 8]
    for e in train_ev:
        want = SCHED.lr(LR, e["counter"])  # no step was skipped: Adam's count is the loop's counter
        print(f"counter {e['counter']}: lr {e['lr']:.9e} schedule {want:.9e}")
        assert abs(e["lr"] - want) <= 1e-6 * want, (e, want)
    val_ev = [e for e in events if e["event"] == "val"]
    assert [e["counter"] for e in val_ev] == [3, 6] and all(e["weights"] == "ema" for e in val_ev)
    best = torch.load(logdir / "model_best.pt", map_location="cpu")
    assert best["val_iou"] == max(e["iou"] for e in val_ev) and "ema_state_dict" in best
    # the capture's warm-up is undone for the EMA too: at counter 0 it is the initial masters
    assert set(seen["ema"]) == set(seen["params"])
    for k, v in seen["params"].items():
        assert torch.equal(seen["ema"][k], v), k


def test_checkpoint_carries_the_ema(runs):
    logdir, seen = runs["logdir"], runs["seen"]
    mid = torch.load(logdir / "model_000004.pt", map_location="cpu")
    assert set(mid) == {"model_state_dict", "optimizer_state_dict", "counter", "epoch", "ema_state_dict"}
    msd, esd = mid["model_state_dict"], mid["ema_state_dict"]
    assert list(esd) == list(msd)
    assert all(torch.isfinite(v.float()).all() for v in esd.values())
    assert {float(e["step"]) for e in mid["optimizer_state_dict"]["state"].values()} == {4.0}
    differ = 0
    for k in msd:
        if k in seen["params"]:
            if not torch.equal(msd[k], seen["params"][k]):  # the parameter moved: its average lags behind it
                assert not torch.equal(esd[k], msd[k]), k
                differ += 1
        else:
            assert torch.equal(esd[k], msd[k]), k  # buffers, constants, frozen parameters: the live values
    assert differ > len(seen["params"]) // 2, (differ, len(seen["params"]))


def test_resume_continues_the_schedule_and_the_ema(runs):
    mid = torch.load(runs["logdir"] / "model_000004.pt", map_location="cpu")
    seen_r, out_r = runs["seen_r"], runs["out_r"]
    assert seen_r["counter"] == 4 and out_r["counter"] == 5
    for k, v in seen_r["ema"].items():
        assert torch.equal(v, mid["ema_state_dict"][k]), k
        assert torch.equal(seen_r["params"][k], mid["model_state_dict"][k]), k
    train_ev = [e for e in _events(runs["resumed"]) if e["event"] == "train"]
    assert [e["counter"] for e in train_ev] == [5]
    want = SCHED.lr(LR, 5)
    assert abs(train_ev[0]["lr"] - want) <= 1e-6 * want and abs(train_ev[0]["lr"] - SCHED.lr(LR, 1)) > 1e-4
    assert "ema_state_dict" in torch.load(runs["resumed"] / "model_final.pt", map_location="cpu")


def test_predictor_chooses_the_weights(runs, tmp_path):
    old = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    try:
        path = runs["logdir"] / "model_final.pt"
        bare = tmp_path / "ema_only.pt"
        torch.save(torch.load(path, map_location="cpu")["ema_state_dict"], bare)
        model = L.compile_model(GC, DAC, outC=1).to(DEV)
        model.bevencode.to(memory_format=torch.channels_last)
        model.camencode.up1.to(memory_format=torch.channels_last)
        p = L.Predictor(model, 2, DEV, graph=False)
        rig = syn.make_rig(2, 6, DAC["final_dim"], seed=1)
        inputs = (syn.make_images(2, 6, DAC["final_dim"], seed=1),
                  *(rig[k] for k in ("rots", "trans", "intrins", "post_rots", "post_trans")))
        got = {}
        for name, (f, w) in {"ema": (path, "ema"), "model": (path, "model"), "auto": (path, "auto"),
                             "bare": (bare, "auto")}.items():
            p.load(f, weights=w)
            got[name] = p(*inputs).float().clone()
        assert all(torch.isfinite(v).all() for v in got.values())
        assert not torch.equal(got["ema"], got["model"])
        assert torch.equal(got["auto"], got["ema"]) and torch.equal(got["bare"], got["ema"])
        with pytest.raises(ValueError):
            p.load(bare, weights="ema")
    finally:
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = old
