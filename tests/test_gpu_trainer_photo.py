"""trainer.train with the photometric augmentation on a synthetic SimBEV tree (synthetic.make_simbev_tree), every
photo_* option on, together with the BEV-space augmentation and the valid-cell mask: finite losses, the settings in
the config event, validation batches bit-equal to a run without the option, resume; and
``python -m lss_carla_amd.predict --photo`` on the run's checkpoint. ``cudnn.deterministic`` is on, as in
tests/test_gpu_trainer.py and tests/test_gpu_trainer_ncams.py: at this shape the solvers MIOpen otherwise picks are not
reproducible under replay (measured here too: without the attribute a captured run of this tree skips two of four
steps for a non-finite gradient with the option off as well as on; the eager loop skips none)."""
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import predict as P, synthetic as syn, trainer  # noqa: E402

KW = dict(H=56, W=120, resize_lim=(1.6, 1.8), final_dim=(64, 192), rot_lim=(-5.4, 5.4), rand_flip=True,
          bot_pct_lim=(0.0, 0.22), bsz=2, nworkers=0, use_wandb=False, miopen_find=False)
PHOTO = dict(photo_brightness=32.0, photo_contrast=(0.5, 1.5), photo_saturation=(0.5, 1.5), photo_hue=18.0,
             photo_noise=(0.0, 8.0), photo_prob=0.75, photo_per_camera=True)
# metrics.json of a plain run, as it was before the option existed
PLAIN_KEYS = {"loss", "iou", "iou_per_class", "loss_kind", "threshold", "intersection", "union", "samples", "classes",
              "dtype", "graph", "bsz", "frames_per_s"}


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


def _run(tree, logdir, **kw):
    """train(); returns (summary, what on_start saw, the images of every committed batch in order)."""
    seen, commits = {}, []

    def on_start(ctx):
        st = ctx["stager"]
        seen["photo"], seen["same"], seen["captured"] = st.photo, ctx["val_stager"] is st, ctx["step"].captured
        commit = st.commit

        def recording_commit():
            b = commit()
            commits.append(st.imgs[:b].clone())
            return b

        st.commit = recording_commit

    args = dict(nepochs=1, val_step=2, save_step=100, seed=0, loss_step=1, logdir=str(logdir), on_start=on_start)
    args.update(KW)
    args.update(kw)
    return trainer.train(tree, **args), seen, commits


@pytest.fixture(scope="module")
def photo_run(tree, tmp_path_factory):
    logdir = tmp_path_factory.mktemp("photo")
    out, seen, commits = _run(tree, logdir, graph=True, bev_rot_lim=(-20.0, 20.0), valid_mask="grid", **PHOTO)
    return logdir, out, seen, commits


def test_every_option_on_trains_and_records_its_settings(photo_run):
    logdir, out, seen, commits = photo_run
    assert out["counter"] == 4 and out["skipped"] == 0 and math.isfinite(out["loss"])
    assert seen["photo"] and seen["same"] and seen["captured"]
    ev = _events(logdir)
    cfg = [e for e in ev if e["event"] == "config"]
    assert len(cfg) == 1
    assert {k: cfg[0][k] for k in PHOTO} == {"photo_brightness": 32.0, "photo_contrast": [0.5, 1.5],
                                             "photo_saturation": [0.5, 1.5], "photo_hue": 18.0,
                                             "photo_noise": [0.0, 8.0], "photo_prob": 0.75, "photo_per_camera": True}
    assert cfg[0]["bev_rot_lim"] == [-20.0, 20.0] and cfg[0]["valid_mask"] == "grid"
    train_ev = [e for e in ev if e["event"] == "train"]
    val_ev = [e for e in ev if e["event"] == "val"]
    assert [e["counter"] for e in train_ev] == [1, 2, 3, 4] and [e["counter"] for e in val_ev] == [2, 4]
    assert all(math.isfinite(e["loss"]) and e["loss"] > 0 for e in train_ev + val_ev)
    ck = torch.load(logdir / "model_final.pt", map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "counter", "epoch"}  # checkpoints do not change


def test_validation_batches_are_those_of_a_run_without_the_option(tree, photo_run, tmp_path):
    _, _, _, with_photo = photo_run
    _, seen, plain = _run(tree, tmp_path, graph=False, bev_rot_lim=(-20.0, 20.0), valid_mask="grid", max_steps=2)
    assert not seen["photo"]
    # (the first commit precedes on_start) recorded: training batch 2, validation, [3, 4, validation]
    assert len(plain) == 2 and len(with_photo) == 5
    assert torch.equal(with_photo[1], plain[1]) and torch.equal(with_photo[4], plain[1])  # validation: not augmented
    assert not torch.equal(with_photo[0], plain[0])                                       # training: augmented
    assert [e for e in _events(tmp_path) if e["event"] == "config"][0].keys().isdisjoint(PHOTO)


def test_resume_continues(tree, photo_run, tmp_path):
    logdir, _, _, _ = photo_run
    out, seen, _ = _run(tree, tmp_path, graph=True, resume=str(logdir / "model_final.pt"), nepochs=2, max_steps=2,
                        **PHOTO)
    assert out["counter"] == 6 and out["skipped"] == 0 and math.isfinite(out["loss"]) and seen["photo"]
    assert torch.load(tmp_path / "model_final.pt", map_location="cpu")["counter"] == 6


def test_exclusive_classes_and_a_camera_subset_take_the_option(tree, tmp_path):
    out, seen, _ = _run(tree, tmp_path, graph=False, max_steps=2, ncams=5, exclusive=True,
                        label_groups=[[0], [1, 2, 3]], photo_noise=(2.0, 4.0), photo_per_camera=False)
    assert out["counter"] == 2 and math.isfinite(out["loss"]) and seen["photo"] and not seen["same"]
    cfg = [e for e in _events(tmp_path) if e["event"] == "config"][0]
    assert cfg["photo_noise"] == [2.0, 4.0] and cfg["photo_per_camera"] is False and cfg["exclusive"] is True


def _predict(tree, photo_run, out, *extra):
    logdir = photo_run[0]
    a = P.parser().parse_args(["--modelf", str(logdir / "model_best.pt"), "--dataroot", tree, "--out", str(out),
                               "--bsz", "2", "--nworkers", "0", "--H", "56", "--W", "120", "--final_h", "64",
                               "--final_w", "192", "--miopen_find", "0", *extra])
    return P.predict(a)


def test_predict_photo_shifts_every_image(tree, photo_run, tmp_path):
    base = _predict(tree, photo_run, tmp_path / "base")
    assert set(base) == PLAIN_KEYS and set(json.load(open(tmp_path / "base" / "metrics.json"))) == PLAIN_KEYS
    dusk = _predict(tree, photo_run, tmp_path / "dusk", "--photo", "brightness=-40,noise=8")
    assert dusk["photo"] == {"brightness": -40.0, "noise": 8.0} and set(dusk) == PLAIN_KEYS | {"photo"}
    assert json.load(open(tmp_path / "dusk" / "metrics.json"))["photo"] == dusk["photo"]
    assert math.isfinite(dusk["loss"]) and dusk["loss"] != base["loss"] and dusk["samples"] == base["samples"] == 2
    again = _predict(tree, photo_run, tmp_path / "again", "--photo", "brightness=-40,noise=8")
    assert again["loss"] == dusk["loss"] and again["intersection"] == dusk["intersection"]  # a fixed seed: repeatable
    neutral = _predict(tree, photo_run, tmp_path / "neutral", "--photo", "brightness=0")
    assert neutral["loss"] == base["loss"] and neutral["union"] == base["union"]
    with pytest.raises(ValueError):
        _predict(tree, photo_run, tmp_path / "bad", "--photo", "gamma=2")
