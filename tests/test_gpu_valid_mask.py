"""The valid-cell mask on the MI355X: lss_simbev_valid_mask (simbev.valid_mask) bit for bit against the numpy
restatement of tests/valid_mask_cases.py on small grids (one partly empty block, rows shorter than a wave), one and
three samples, one and six cameras, one and three heights, fov and grid modes, no / identity / rotated index matrices;
its agreement with the label warp's out-of-grid zero; the stager, the trainer and predict with the option on, on the
committed fixture and on a synthetic tree."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import bev_aug_cases as C
import valid_mask_cases as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import _lib, predict as P, simbev, synthetic as syn, trainer  # noqa: E402
from lss_carla_amd.staging import BatchStager  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.join(GOLDEN, "simbev_small")
KW = dict(H=56, W=120, resize_lim=(1.6, 1.8), final_dim=(64, 192), rot_lim=(-5.4, 5.4), rand_flip=True,
          bot_pct_lim=(0.0, 0.22), bsz=2, nworkers=0, use_wandb=False, miopen_find=False)


@pytest.fixture(autouse=True)
def _no_find():
    old = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    yield
    torch.backends.cudnn.benchmark = old


def _mask(c, mode="fov", **kw):
    """simbev.valid_mask on a case's inputs into a buffer of 7s: every byte must come back written."""
    n = len(c["want"])
    out = torch.full((n, c["X"], c["Y"]), 7, device=DEV, dtype=torch.uint8)
    got = simbev.valid_mask(torch.from_numpy(c["cams"]), torch.from_numpy(c["q"]), c["grid_conf"], V.FINAL_DIM,
                            c["heights"], index_mats=c["mats"], mode=mode, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy()


# ----------------------------------------------------------------------------- the kernel against the restatement
@pytest.mark.parametrize("grid,n,N,heights,mats", V.gpu_cases())
def test_fov_mask_matches_the_restatement_bit_for_bit(grid, n, N, heights, mats):
    c = V.case(grid, n, N, heights, mats)
    want = c["want"]
    assert 0.05 <= want.mean() <= 0.95
    got = _mask(c)
    assert set(np.unique(got)) <= {0, 1}
    np.testing.assert_array_equal(got, want)
    if mats == "identity":  # the identity's output is the NULL output
        null = V.case(grid, n, N, heights, "null")
        np.testing.assert_array_equal(got, _mask(null))
        np.testing.assert_array_equal(got, null["want"])
    # device inputs and a (n, N, 3) post_trans give the same mask
    q3 = np.concatenate([c["q"], np.zeros_like(c["q"][..., :1])], axis=-1)
    got_d = simbev.valid_mask(torch.from_numpy(c["cams"]).to(DEV), torch.from_numpy(q3).to(DEV), c["grid_conf"],
                              V.FINAL_DIM, c["heights"], mode="fov",
                              index_mats=None if c["mats"] is None else torch.from_numpy(c["mats"]).to(DEV))
    np.testing.assert_array_equal(got_d.cpu().numpy(), want)


@pytest.mark.parametrize("mats", [m for m in V.MATS if m != "null"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("grid", V.GPU_GRIDS)
def test_grid_mask_matches_the_restatement_and_the_label_warp(grid, n, mats):
    c = V.case(grid, n, 6, "one", mats, mode="grid")
    X, Y = c["X"], c["Y"]
    got = _mask(c, "grid")
    np.testing.assert_array_equal(got, c["want"])
    np.testing.assert_array_equal(got, V.in_grid_ref(c["mats"], X, Y).astype(np.uint8))
    # without cameras: n from the matrices
    alone = simbev.valid_mask(None, None, c["grid_conf"], V.FINAL_DIM, index_mats=torch.from_numpy(c["mats"]).to(DEV),
                              mode="grid")
    np.testing.assert_array_equal(alone.cpu().numpy(), got)
    # the label warp of an all-ones map writes 0 exactly where the mask is 0
    bev = torch.ones(n, 8, X, Y, device=DEV, dtype=torch.uint8)
    labels = simbev.class_masks(bev, C.THREE, index_mats=c["mats"]).cpu().numpy()
    for k in range(3):
        np.testing.assert_array_equal(labels[:, k], got.astype(np.float32))
    if mats == "identity" or (mats == "rot90" and X == Y):
        assert got.all()
    else:
        assert 0 < got.mean() < 1
    # no matrices: all ones
    ones = torch.zeros(n, X, Y, device=DEV, dtype=torch.uint8)
    simbev.valid_mask(None, None, c["grid_conf"], V.FINAL_DIM, mode="grid", out=ones)
    assert bool(ones.all())


def test_grid_mode_scale_leaves_the_outer_rings_out():
    X = Y = 16
    gc = V.grid_conf(X, Y, 6.25)
    m = simbev.label_index_matrix(simbev.bev_aug_matrix(0.0, 0.8, False, False), gc)[None]
    got = simbev.valid_mask(None, None, gc, V.FINAL_DIM, index_mats=torch.from_numpy(m).to(DEV), mode="grid")[0].cpu().numpy()
    want = np.zeros((X, Y), dtype=np.uint8)
    want[2:-2, 2:-2] = 1  # a centre c cells out has its source at c / 0.8: inside while c < 6.4
    np.testing.assert_array_equal(got, want)


def test_nan_cameras_and_nan_matrices_are_unseen():
    c = V.case("5x7", 3, 6)
    cams = c["cams"].copy()
    cams[0] = np.nan                      # sample 0: every camera NaN
    cams[1, :, 6:9] = 0.0                 # sample 1: d = o_2 only -- a constant depth, possibly outside the bounds
    cams[1, :, 11] = 0.0                  # ... d = 0: 0 / 0 and x / 0
    bad = dict(c, cams=cams)
    bad["want"] = V.valid_mask_ref(cams, c["q"], c["X"], c["Y"], *V.grid_args(c["X"], c["Y"], c["cell"]), c["heights"],
                                   V.DBOUND[0], V.DBOUND[1], V.FINAL_DIM)
    got = _mask(bad)
    np.testing.assert_array_equal(got, bad["want"])
    assert not got[0].any() and not got[1].any() and got[2].any()
    mats = np.stack([V.EYE] * 3).copy()
    mats[1, 0, 2] = np.nan
    got = _mask(dict(c, mats=mats))
    np.testing.assert_array_equal(got[0], c["want"][0])
    assert not got[1].any()


def test_entry_refuses_without_launching():
    lib = _lib.load()
    n, N, X, Y = 2, 6, 5, 7
    cams = torch.zeros(n, N, 16, device=DEV)
    q = torch.zeros(n, N, 2, device=DEV)
    mats = torch.from_numpy(np.stack([V.EYE] * n)).to(DEV)
    out = torch.full((n, X, Y), 7, device=DEV, dtype=torch.uint8)
    hz = (ctypes.c_float * 9)(*([0.0] * 9))
    hp = ctypes.cast(hz, ctypes.c_void_p)
    st = _lib.stream_handle(DEV)
    p = _lib.ptr

    def call(cams=p(cams), q=p(q), n=n, N=N, X=X, Y=Y, heights=hp, nh=1, d_lo=4.0, d_hi=45.0, fH=64, fW=192,
             mats=p(mats), mode=1, out=p(out)):
        return lib.lss_simbev_valid_mask(cams, q, n, N, X, Y, -32.0, 16.0, -48.0, 16.0, heights, nh, d_lo, d_hi, fH, fW,
                                         mats, mode, out, st)

    bad = [call(out=None), call(n=0), call(n=65536), call(X=0), call(Y=-1), call(X=(1 << 23) + 1), call(Y=(1 << 23) + 1),
           call(mode=2), call(nh=9), call(nh=9, mode=0), call(d_lo=0.0), call(d_hi=4.0), call(d_lo=float("nan")),
           call(cams=None), call(q=None), call(heights=None), call(N=0), call(N=257), call(nh=0), call(fH=0), call(fW=0)]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool((out == 7).all())  # nothing was launched
    assert call() == 0 and call(mode=0, cams=None, q=None, heights=None, nh=0, N=0) == 0 and call(mats=None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        simbev.valid_mask(cams, q, V.grid_conf(X, Y, 16.0), V.FINAL_DIM, heights=(0.0,) * 9)
    with pytest.raises(RuntimeError):
        simbev.valid_mask(None, None, V.grid_conf(X, Y, 16.0), V.FINAL_DIM, mode="fov", out=out)
    with pytest.raises(RuntimeError):
        simbev.valid_mask(cams, q[:1], V.grid_conf(X, Y, 16.0), V.FINAL_DIM)
    with pytest.raises(RuntimeError):
        simbev.valid_mask(cams, q, V.grid_conf(X, Y, 16.0), V.FINAL_DIM, out=out[:1])


# ----------------------------------------------------------------------------- the stager on the fixture
def _ref_for_raw(raw, gc, heights=(0.0,), mode="fov", mats=None):
    """The restated mask of a raw batch: the package's camera blocks of its host rig, the restatement's arithmetic."""
    X, Y = int((gc["xbound"][1] - gc["xbound"][0]) / gc["xbound"][2]), int((gc["ybound"][1] - gc["ybound"][0]) / gc["ybound"][2])
    f = np.float32
    x0, dx = f(gc["xbound"][0] + gc["xbound"][2] / 2.0), f(gc["xbound"][2])
    y0, dy = f(gc["ybound"][0] + gc["ybound"][2] / 2.0), f(gc["ybound"][2])
    cams = simbev.fov_cameras(*raw[1:5]).numpy()
    q = raw[5].numpy()[..., :2].copy()
    return V.valid_mask_ref(cams, q, X, Y, x0, dx, y0, dy, heights, gc["dbound"][0], gc["dbound"][1], C.DAC["final_dim"],
                            mats, mode)


@pytest.fixture(scope="module")
def raws():
    kw = dict(bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV)
    tl, vl = simbev.compile_data("", ROOT, {**C.DAC, **C.BEV_ON, "valid_mask": "fov"}, C.GC, **kw)
    tl_off, vl_off = simbev.compile_data("", ROOT, C.DAC, C.GC, **kw)
    assert tl.valid_mask_conf == ("fov", C.GC, (0.0,)) and tl_off.valid_mask_conf is None
    np.random.seed(3)
    torch.manual_seed(3)
    train = list(tl.loader)[:2]
    np.random.seed(3)
    torch.manual_seed(3)
    plain = list(tl_off.loader)[:2]
    return {"train": train, "plain": plain, "val": list(vl_off.loader), "tl": tl, "vl_off": vl_off}


def _stager(**kw):
    return BatchStager(C.DAC["final_dim"], 2, 6, (C.DAC["H"], C.DAC["W"]), C.GC, DEV, **kw)


def test_stager_mask_is_the_restatement_and_partial_batches_leave_the_rest(raws, monkeypatch):
    launched = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (launched.append(what), real(code, what))[1])
    st = _stager(bev_aug=True, valid_mask="fov")
    assert st.valid.dtype == torch.uint8 and tuple(st.valid.shape) == (2, 200, 200) and bool(st.valid.all())
    a, b = raws["train"]
    st.stage(a)
    assert st.commit() == 2
    torch.cuda.synchronize()
    assert launched.count("lss_simbev_valid_mask") == 1
    want = _ref_for_raw(a, C.GC, mats=a[8].numpy())
    np.testing.assert_array_equal(st.valid.cpu().numpy(), want)
    assert 0.05 <= want.mean() <= 0.95
    assert (want <= V.in_grid_ref(a[8].numpy(), 200, 200)).all() and not V.in_grid_ref(a[8].numpy(), 200, 200).all()
    # finish_batch carries the same mask after the labels
    fin = simbev.finish_batch(a, C.DAC["final_dim"], DEV, bev_aug=True, valid_mask_conf=("fov", C.GC, (0.0,)))
    assert len(fin) == 8 and torch.equal(fin[7], st.valid) and torch.equal(fin[6], st.binimgs)
    # a partial batch leaves sample 1 as it was
    before = st.valid.clone()
    one = tuple(t[:1] for t in b)
    st.stage(one)
    assert st.commit() == 1
    torch.cuda.synchronize()
    np.testing.assert_array_equal(st.valid[:1].cpu().numpy(), _ref_for_raw(one, C.GC, mats=one[8].numpy()))
    assert torch.equal(st.valid[1:], before[1:]) and not torch.equal(st.valid[:1], before[:1])
    # grid mode, three heights
    sg = _stager(bev_aug=True, valid_mask="grid")
    sg.stage(a)
    sg.commit()
    s3 = _stager(bev_aug=True, valid_mask="fov", fov_z=(0.0, 1.5, -1.0))
    s3.stage(a)
    s3.commit()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(sg.valid.cpu().numpy(), V.in_grid_ref(a[8].numpy(), 200, 200).astype(np.uint8))
    np.testing.assert_array_equal(s3.valid.cpu().numpy(), _ref_for_raw(a, C.GC, (0.0, 1.5, -1.0), mats=a[8].numpy()))


def test_stager_masks_validation_batches_and_is_todays_when_off(raws, monkeypatch):
    launched = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (launched.append(what), real(code, what))[1])
    off, on = _stager(), _stager(valid_mask="fov")
    assert off.valid is None
    for raw in raws["val"]:
        off.stage(raw)
        off.commit()
    assert "lss_simbev_valid_mask" not in launched
    fin = simbev.finish_batch(raws["val"][-1], C.DAC["final_dim"], DEV)
    assert len(fin) == 7
    torch.cuda.synchronize()
    assert torch.equal(off.binimgs, fin[6])
    for raw in raws["val"]:
        on.stage(raw)
        on.commit()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(on.valid.cpu().numpy(), _ref_for_raw(raw, C.GC))  # no matrices: all in the grid
    for x, y in zip(on.inputs + (on.binimgs,), off.inputs + (off.binimgs,)):
        assert torch.equal(x, y)  # the other static tensors are bit-identical
    # the training batches of the same seed without the option: labels as today
    plain = _stager()
    plain.stage(raws["plain"][0])
    plain.commit()
    torch.cuda.synchronize()
    assert torch.equal(plain.binimgs, simbev.finish_batch(raws["plain"][0], C.DAC["final_dim"], DEV)[6])
    with pytest.raises(ValueError):
        _stager(valid_mask="bogus")


# ----------------------------------------------------------------------------- trainer and predict
def _events(logdir):
    return [json.loads(line) for line in open(os.path.join(str(logdir), "metrics.jsonl"))]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("simbev_tree")
    assert syn.make_simbev_tree(str(root), n_scenes=5, per_scene=2, H=56, W=120, seed=1) == 10
    return str(root)


@pytest.fixture(scope="module")
def masked_run(tree, tmp_path_factory):
    logdir = tmp_path_factory.mktemp("masked_run")
    launched = []
    real = _lib.check
    _lib.check = lambda code, what: (launched.append(what), real(code, what))[1]
    try:
        out = trainer.train(tree, nepochs=1, seed=0, graph=True, max_steps=4, loss_step=1, iou_step=2, val_step=4,
                            save_step=4, logdir=str(logdir), valid_mask="fov", bev_rot_lim=(-20.0, 20.0), **KW)
    finally:
        _lib.check = real
    return logdir, out, launched


def test_trainer_runs_masked_and_reports_the_valid_fraction(tree, masked_run):
    logdir, out, launched = masked_run
    assert out["counter"] == 4 and out["skipped"] == 0 and math.isfinite(out["loss"])
    assert "lss_seg_loss_masked" in launched and "lss_seg_loss_masked_bwd" in launched
    assert "lss_seg_metrics_accum_masked" in launched and "lss_simbev_valid_mask" in launched
    assert "lss_bce_logits" not in launched and "lss_bce_iou_accum" not in launched
    events = _events(logdir)
    cfg = events[0]
    assert cfg["event"] == "config" and cfg["valid_mask"] == "fov" and cfg["fov_z"] == [0.0]
    assert cfg["bev_rot_lim"] == [-20.0, 20.0]
    losses = [e["loss"] for e in events if e["event"] == "train"]
    assert len(losses) == 4 and all(math.isfinite(v) and v > 0 for v in losses)
    ious = [e for e in events if e["event"] == "train_iou"]
    assert len(ious) == 2 and all(0.0 <= e["iou"] <= 1.0 for e in ious)
    vals = [e for e in events if e["event"] == "val"]
    assert len(vals) == 1
    # the mean of the restated mask over the val split (validation carries the identity: every cell in the grid)
    gc = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
          "dbound": [4.0, 45.0, 1.0]}
    ds = simbev.SegmentationData(tree, is_train=False, data_aug_conf=C.DAC, grid_conf=gc)
    masks = [_ref_for_raw(tuple(t[None] for t in ds[i]), gc) for i in range(len(ds))]
    want = float(np.mean([m.mean() for m in masks]))
    assert 0.05 <= want <= 0.95
    for e in vals:
        assert e["valid_fraction"] == pytest.approx(want, rel=1e-12)
        assert math.isfinite(e["loss"]) and e["loss"] > 0 and 0.0 <= e["iou"] <= 1.0
    assert (logdir / "model_000004.pt").exists() and (logdir / "model_best.pt").exists()


def test_resume_continues_and_predict_counts_valid_cells_only(tree, masked_run, tmp_path):
    logdir, _, _ = masked_run
    path = logdir / "model_000004.pt"
    seen = {}
    out = trainer.train(tree, nepochs=2, val_step=100, save_step=100, seed=0, logdir=str(tmp_path / "resumed"),
                        resume=str(path), max_steps=1, on_start=lambda ctx: seen.update(counter=ctx["counter"]),
                        valid_mask="fov", bev_rot_lim=(-20.0, 20.0), **KW)
    assert seen["counter"] == 4 and out["counter"] == 5 and math.isfinite(out["loss"])

    pred = tmp_path / "pred"
    a = P.parser().parse_args(["--modelf", str(path), "--dataroot", tree, "--out", str(pred), "--bsz", "2",
                               "--nworkers", "0", "--miopen_find", "0", "--valid_mask", "fov", "--fov_z", "0.0,1.5"])
    info = P.predict(a, grid_conf=C.GC, data_aug_conf=C.DAC)
    assert json.load(open(pred / "metrics.json")) == json.loads(json.dumps(info))
    assert info["valid_mask"] == "fov" and info["fov_z"] == [0.0, 1.5] and info["samples"] == 2
    masks = np.stack([np.load(pred / f"{i}.npy") for i in range(2)])
    valid = np.stack([np.load(pred / "valid" / f"{i}.npy") for i in range(2)])
    assert masks.shape == (2, 1, 200, 200) and valid.shape == (2, 200, 200) and valid.dtype == np.uint8
    assert info["valid_fraction"] == pytest.approx(valid.mean(), rel=1e-12) and 0.05 <= valid.mean() <= 0.95
    # the IoU recomputed on the host from the saved masks, the labels and the saved valid masks
    ds = simbev.SegmentationData(tree, is_train=False, data_aug_conf=C.DAC, grid_conf=C.GC)
    labels = np.stack([C.plain_labels(ds[i][-1].numpy()[None], C.VEHICLE)[0] for i in range(2)])
    on = valid[:, None].astype(bool)
    p, q = masks.astype(bool) & on, (labels != 0) & on
    inter, union = int((p & q).sum()), int((p | q).sum())
    assert info["intersection"] == [float(inter)] and info["union"] == [float(union)] and union > 0
    assert info["iou"] == pytest.approx(inter / union, rel=1e-12)
    ds_raw = [tuple(t[None] for t in ds[i]) for i in range(2)]
    np.testing.assert_array_equal(valid, np.concatenate([_ref_for_raw(r, C.GC, (0.0, 1.5)) for r in ds_raw]))
    # without the flag: today's keys and files
    a0 = P.parser().parse_args(["--modelf", str(path), "--dataroot", tree, "--out", str(tmp_path / "pred0"), "--bsz", "2",
                                "--nworkers", "0", "--miopen_find", "0"])
    info0 = P.predict(a0, grid_conf=C.GC, data_aug_conf=C.DAC)
    assert "valid_fraction" not in info0 and "valid_mask" not in info0 and not (tmp_path / "pred0" / "valid").exists()
    assert np.load(tmp_path / "pred0" / "0.npy").shape == (1, 200, 200)
