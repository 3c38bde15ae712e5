"""trainer.train(ncams=k) on a synthetic SimBEV tree (synthetic.make_simbev_tree): the reference's ``Ncams`` -- k
random cameras per training sample, validation at all six -- over two stagers and two captured shapes; the eager
loop follows the captured one's losses (bar of tests/test_gpu_trainer.py between captured and eager: rtol 1e-5 /
atol 1e-6, cudnn.deterministic on as there); resume at another k; the valid-cell mask; and
``python -m lss_carla_amd.predict --drop_cams / --drop_each`` on the run's checkpoint."""
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import predict as P, simbev, synthetic as syn, trainer  # noqa: E402

DEV = torch.device("cuda:0")
KW = dict(H=56, W=120, resize_lim=(1.6, 1.8), final_dim=(64, 192), rot_lim=(-5.4, 5.4), rand_flip=True,
          bot_pct_lim=(0.0, 0.22), bsz=2, nworkers=0, use_wandb=False, miopen_find=False)
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.0, 1.0), "final_dim": (64, 192), "rot_lim": (0.0, 0.0), "H": 56, "W": 120,
       "rand_flip": False, "bot_pct_lim": (0.0, 0.0), "Ncams": 6}


@pytest.fixture(scope="module", autouse=True)
def _deterministic():
    old = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    yield
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = old


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("tree")
    assert syn.make_simbev_tree(str(root), n_scenes=5, per_scene=2, H=56, W=120) == 10  # 8 train, 2 val samples
    return str(root)


def _events(logdir):
    return [json.loads(line) for line in open(logdir / "metrics.jsonl")]


def _run(tree, logdir, ncams, graph, **kw):
    seen = {}

    def on_start(ctx):
        seen["train_N"], seen["val_N"] = ctx["stager"].N, ctx["val_stager"].N
        seen["same"] = ctx["val_stager"] is ctx["stager"]
        seen["imgs"] = tuple(ctx["stager"].imgs.shape)
        seen["captured"] = ctx["step"].captured
        torch.cuda.manual_seed(4321)  # the dropouts' Philox stream from the first timed step on, captured or eager

    args = dict(nepochs=1, val_step=2, save_step=100, seed=0, loss_step=1, logdir=str(logdir), ncams=ncams,
                graph=graph, on_start=on_start)
    args.update(KW)
    args.update(kw)
    out = trainer.train(tree, **args)
    return out, seen


@pytest.fixture(scope="module")
def run5(tree, tmp_path_factory):
    logdir = tmp_path_factory.mktemp("ncams5")
    out, seen = _run(tree, logdir, 5, True)
    return logdir, out, seen


def test_train_ncams5_captured_validates_at_six_cameras(run5):
    logdir, out, seen = run5
    assert out["counter"] == 4 and out["skipped"] == 0 and math.isfinite(out["loss"])
    assert seen["captured"] and (seen["train_N"], seen["val_N"]) == (5, 6) and not seen["same"]
    assert seen["imgs"] == (2, 5, 3, 64, 192)
    ev = _events(logdir)
    train_ev = [e for e in ev if e["event"] == "train"]
    val_ev = [e for e in ev if e["event"] == "val"]
    assert [e["counter"] for e in train_ev] == [1, 2, 3, 4]
    assert all(math.isfinite(e["loss"]) and e["loss"] > 0 for e in train_ev)
    assert [e["counter"] for e in val_ev] == [2, 4]
    assert all(math.isfinite(e["loss"]) and e["loss"] > 0 and 0.0 <= e["iou"] <= 1.0 for e in val_ev)
    assert (logdir / "model_best.pt").exists() and (logdir / "model_final.pt").exists()
    ck = torch.load(logdir / "model_final.pt", map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "counter", "epoch"}  # checkpoints do not change
    # Predictor.load takes the best checkpoint as any other, at N = 6
    model = L.compile_model(GC, DAC, outC=1).to(DEV)
    p = L.Predictor(model, 2, DEV, graph=False)
    p.load(logdir / "model_best.pt")
    rig = syn.make_rig(2, 6, (64, 192), seed=0)
    out6 = p(syn.make_images(2, 6, (64, 192), seed=0), *(rig[k] for k in p.RIG))
    assert out6.shape == (2, 1, 200, 200) and torch.isfinite(out6.float()).all()


def test_eager_loop_follows_the_captured_losses(tree, run5, tmp_path):
    logdir, _, _ = run5
    out, seen = _run(tree, tmp_path, 5, False)
    assert not seen["captured"] and (seen["train_N"], seen["val_N"]) == (5, 6)
    cap, eag = _events(logdir), _events(tmp_path)
    for kind in ("train", "val"):
        a = [e["loss"] for e in cap if e["event"] == kind]
        b = [e["loss"] for e in eag if e["event"] == kind]
        print(kind, "captured", a, "eager", b)
        assert len(a) == len(b) and len(a) >= 2
        torch.testing.assert_close(torch.tensor(b, dtype=torch.float64), torch.tensor(a, dtype=torch.float64),
                                   rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("ncams,graph", [(6, False), (3, True)])
def test_resume_of_a_five_camera_checkpoint_at_another_count(tree, run5, tmp_path, ncams, graph):
    logdir, _, _ = run5
    out, seen = _run(tree, tmp_path, ncams, graph, resume=str(logdir / "model_final.pt"), nepochs=2, max_steps=2,
                     val_step=2)
    assert out["counter"] == 6 and out["skipped"] == 0 and math.isfinite(out["loss"])
    assert (seen["train_N"], seen["val_N"]) == (ncams, 6) and seen["same"] == (ncams == 6)
    val_ev = [e for e in _events(tmp_path) if e["event"] == "val"]
    assert [e["counter"] for e in val_ev] == [6] and math.isfinite(val_ev[0]["loss"])
    assert torch.load(tmp_path / "model_final.pt", map_location="cpu")["counter"] == 6


def test_ncams5_with_the_fov_mask_reports_valid_fraction(tree, tmp_path):
    out, seen = _run(tree, tmp_path, 5, True, valid_mask="fov", max_steps=2)
    assert out["counter"] == 2 and math.isfinite(out["loss"]) and (seen["train_N"], seen["val_N"]) == (5, 6)
    ev = _events(tmp_path)
    cfg = [e for e in ev if e["event"] == "config"]
    assert cfg and cfg[0]["valid_mask"] == "fov" and cfg[0]["num_cameras"] == 5
    val_ev = [e for e in ev if e["event"] == "val"]
    assert len(val_ev) == 1 and 0.0 < val_ev[0]["valid_fraction"] <= 1.0 and math.isfinite(val_ev[0]["loss"])


def test_fov_mask_of_a_five_camera_batch_misses_the_dropped_cameras_cells():
    """Each stager's mask comes from the cameras its batch holds: the same rig staged with five of its cameras
    marks fewer cells valid than with all six, and never one the six do not."""
    rig = syn.make_rig(2, 6, (64, 192), seed=0)
    out = torch.empty(2, 200, 200, device=DEV, dtype=torch.uint8)
    six = simbev.valid_mask(simbev.fov_cameras(**rig), rig["post_trans"], GC, (64, 192), out=out).clone()
    keep = [0, 1, 2, 4, 5]
    sub = {k: v[:, keep].contiguous() for k, v in rig.items()}
    five = simbev.valid_mask(simbev.fov_cameras(**sub), sub["post_trans"], GC, (64, 192), out=out)
    assert (five <= six).all() and int(five.sum()) < int(six.sum())


def test_ncams6_returns_the_same_stager_for_validation():
    ctx = trainer.build_step(GC, DAC, 2, DEV, ncams=6)
    assert ctx["val_stager"] is ctx["stager"] and ctx["stager"].N == 6
    assert ctx["step"].inverses is None and ctx["evaluate"].inverses is None
    ctx5 = trainer.build_step(GC, {**DAC, "Ncams": 5}, 2, DEV, ncams=5)
    assert ctx5["stager"].N == 5 and ctx5["val_stager"].N == 6 and ctx5["val_stager"] is not ctx5["stager"]
    assert ctx5["step"].inverses[0] is ctx5["stager"].hinv.pinv
    assert ctx5["evaluate"].inverses[0] is ctx5["val_stager"].hinv.pinv
    assert ctx5["evaluate"].labels is ctx5["val_stager"].binimgs and ctx5["step"].labels is ctx5["stager"].binimgs
    with pytest.raises(ValueError, match="ncams"):
        trainer.build_step(GC, DAC, 2, DEV, ncams=7)


def _predict(tree, run5, out, *extra):
    logdir, _, _ = run5
    a = P.parser().parse_args(["--modelf", str(logdir / "model_best.pt"), "--dataroot", tree, "--out", str(out),
                               "--bsz", "2", "--nworkers", "0", "--H", "56", "--W", "120", "--final_h", "64",
                               "--final_w", "192", "--miopen_find", "0", *extra])
    return P.predict(a)


def test_predict_drop_cams_and_drop_each(tree, run5, tmp_path):
    base = _predict(tree, run5, tmp_path / "base")
    assert "dropped_cams" not in base and "drop_each" not in base
    front = _predict(tree, run5, tmp_path / "front", "--drop_cams", "front")
    assert front["dropped_cams"] == ["front"] and "drop_each" not in front
    assert math.isfinite(front["loss"]) and front["samples"] == 2
    assert front["loss"] != base["loss"]
    each = _predict(tree, run5, tmp_path / "each", "--drop_each", "1", "--valid_mask", "fov")
    assert each["dropped_cams"] == [] and list(each["drop_each"]) == simbev.CAMERA_ORDER
    for name, e in each["drop_each"].items():
        assert {"loss", "iou", "intersection", "union", "valid_fraction"} <= set(e), name
        assert math.isfinite(e["loss"]) and e["valid_fraction"] < each["valid_fraction"], name
    # the normal pass is the unmasked run's, and masks are written for it only
    assert sorted(p.name for p in (tmp_path / "each").glob("*.npy")) == ["0.npy", "1.npy"]
    on_disk = json.load(open(tmp_path / "each" / "metrics.json"))
    assert on_disk["drop_each"]["front"]["loss"] == each["drop_each"]["front"]["loss"]
    # the entry for a camera equals a separate --drop_cams run for it
    alone = _predict(tree, run5, tmp_path / "alone", "--drop_cams", "front", "--valid_mask", "fov")
    got = each["drop_each"]["front"]
    for k in ("loss", "iou", "intersection", "union", "valid_fraction"):
        assert got[k] == alone[k], (k, got[k], alone[k])
    plain = _predict(tree, run5, tmp_path / "plain", "--drop_each", "1")
    for k in ("loss", "iou", "intersection", "union"):
        assert plain["drop_each"]["front"][k] == front[k], k
        assert plain[k] == base[k], k
