"""Exclusive classes end to end on the MI355X, at the sizes of tests/test_gpu_trainer_multiclass.py: the stager's
class-map labels, the captured TrainStep with tools.SoftmaxLoss against the eager step (that test's bars: loss rtol
1e-5 / atol 1e-6), EvalStep.read() against a numpy evaluation of its logits, a short trainer run with the valid-cell
mask and the BEV-space augmentation on (events, resume, a refused checkpoint), predict's class maps against its
metrics.json, and a default (sigmoid) step that launches none of the new kernels and computes what the untouched
entries compute."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import exclusive_cases as E  # noqa: E402
import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import _lib, predict as P, simbev, synthetic, tools as T, trainer  # noqa: E402
from lss_carla_amd.staging import BatchStager  # noqa: E402
from lss_carla_amd.train_step import EvalStep, TrainStep  # noqa: E402

DEV = torch.device("cuda:0")
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
KW = dict(H=56, W=120, resize_lim=(1.6, 1.8), final_dim=(64, 192), rot_lim=(-5.4, 5.4), rand_flip=True,
          bot_pct_lim=(0.0, 0.22), bsz=2, nworkers=0, use_wandb=False, miopen_find=False)
GROUPS = [[0], [1, 2, 3]]   # background, then two groups: C = 3
CW = [0.5, 1.0, 2.0]
NEW = ("lss_softmax_ce", "lss_confusion_accum", "lss_argmax_classes", "lss_simbev_class_index")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    d = tmp_path_factory.mktemp("simbev_exclusive")
    assert synthetic.make_simbev_tree(str(d), n_scenes=5, per_scene=2, H=56, W=120, seed=1,
                                      box_classes=(0, 1, 2, 3)) == 10
    return str(d)


@pytest.fixture(autouse=True)
def _solvers():
    old = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    yield
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = old


@pytest.fixture
def launched(monkeypatch):
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (calls.append(what), real(code, what))[1])
    return calls


@pytest.fixture(scope="module")
def raws(root):
    tl, vl = simbev.compile_data("", root, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV,
                                 label_groups=GROUPS, exclusive=True)
    assert tl.exclusive and vl.exclusive
    np.random.seed(0)
    torch.manual_seed(0)
    return list(tl.loader)[:2], tl


def _fresh_model(outC, state=None):
    m = L.compile_model(GC, DAC, outC=outC)
    if state is not None:
        m.load_state_dict(state)
    m = m.to(DEV)
    m.bevencode.to(memory_format=torch.channels_last)
    m.camencode.up1.to(memory_format=torch.channels_last)
    return m


class _SyncErrors:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")


def test_stager_and_loader_labels_are_the_class_index(raws, launched):
    batches, tl = raws
    st = BatchStager(DAC["final_dim"], 2, 6, (DAC["H"], DAC["W"]), GC, DEV, label_groups=GROUPS, exclusive=True)
    assert st.binimgs.dtype == torch.uint8 and tuple(st.binimgs.shape) == (2, 200, 200)
    st.stage(batches[0])  # (first use: the resize tables of these sizes are uploaded)
    st.commit()
    with _SyncErrors():
        st.stage(batches[1])
        st.commit()
    torch.cuda.synchronize()
    assert "lss_simbev_class_index" in launched and "lss_simbev_class_masks" not in launched
    bev = batches[1][-1]
    want = simbev.class_index(bev.to(DEV), GROUPS)
    assert torch.equal(st.binimgs, want) and np.array_equal(want.cpu().numpy(), E.class_index_ref(bev.numpy(), GROUPS))
    values = set(np.unique(want.cpu().numpy()).tolist())
    assert values <= {0, 1, 2} and 0 in values and len(values) > 1
    fin = simbev.finish_batch(batches[1], DAC["final_dim"], DEV, label_groups=GROUPS, exclusive=True)
    assert fin[6].dtype == torch.uint8 and torch.equal(fin[6], want)
    with pytest.raises(ValueError):
        BatchStager(DAC["final_dim"], 2, 6, (DAC["H"], DAC["W"]), GC, DEV, exclusive=True)  # no label_groups
    with pytest.raises(ValueError):
        simbev.finish_batch(batches[1], DAC["final_dim"], DEV, exclusive=True)


def test_captured_step_matches_eager_lowers_the_loss_and_eval_reads_its_logits(raws, launched):
    batches, _ = raws
    ctx = trainer.build_step(GC, DAC, 2, DEV, label_groups=GROUPS, exclusive=True, class_weight=CW, n_val=2)
    model, flat, masters, opt, stager, step = (ctx[k] for k in ("model", "flat", "masters", "opt", "stager", "step"))
    assert model.bevencode.up2[4].out_channels == 3 and ctx["loss_fn"].exclusive
    assert ctx["loss_fn"].class_weight.tolist() == CW and stager.binimgs.dtype == torch.uint8
    stager.stage(batches[0])
    stager.commit()
    snap = [m.detach().clone() for m in masters]
    step.capture(warmup=2)
    for name in ("lss_headk_fwd", "lss_headk_bwd", "lss_softmax_ce", "lss_seg_loss_masked_bwd",
                 "lss_simbev_class_index"):
        assert name in launched, name
    assert "lss_bce_logits" not in launched and "lss_bce_logits_pc" not in launched
    with torch.no_grad():
        for m, s in zip(masters, snap):
            m.copy_(s)
    torch.cuda.manual_seed(1000)
    step()
    torch.cuda.synchronize()
    rep_loss = step.static_loss.clone()
    rep = {}
    for grp, gg in zip(flat.groups, step.graph_grads):
        rep.update({k: v.detach().clone() for k, v in grp.views_of(gg).items()})
    with torch.no_grad():
        for m, s in zip(masters, snap):
            m.copy_(s)
    want = simbev.finish_batch(batches[0], DAC["final_dim"], DEV, label_groups=GROUPS, exclusive=True)
    assert torch.equal(want[6], stager.binimgs)
    model.static_inverses = None
    try:
        eager = TrainStep(ctx["forward"], want[:6], want[6], ctx["loss_fn"], opt, masters, all_reduce=False,
                          amp_dtype=torch.bfloat16, max_grad_norm=5.0, keep_preds=True)
        torch.cuda.manual_seed(1000)
        loss_e = eager.forward_backward().detach()
        torch.cuda.synchronize()
    finally:
        model.static_inverses = (stager.hinv.pinv, stager.hinv.kinv)
    eag = flat.views(grads=True)
    k = "camencode.depthnet.weight"
    rel = ((rep[k] - eag[k]).norm() / eag[k].norm()).item()
    print(f"loss captured {rep_loss.item():.7f} eager {loss_e.item():.7f}; depthnet.weight grad rel diff {rel:.3e}")
    torch.testing.assert_close(rep_loss, loss_e, rtol=1e-5, atol=1e-6)
    assert rel < 1e-3 and eag["bevencode.up2.4.weight"].shape == (3, 128, 1, 1)
    # the loss of the step's own logits, from the float64 closed form
    logits = step.static_preds.float().cpu()
    ref, _ = E.closed_form(logits.double(), stager.binimgs.cpu(), None, torch.tensor(CW))
    assert rep_loss.item() == pytest.approx(ref.item(), rel=E.LOSS_RTOL, abs=E.LOSS_ATOL)
    losses = [rep_loss.item()]
    for _ in range(5):
        step()
        losses.append(step.static_loss.item())
    print("losses over six steps on one batch:", losses)
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0] and step.skipped.item() == 0

    evaluate = ctx["evaluate"]
    assert evaluate.exclusive and evaluate.totals.numel() == 1 + 9
    with pytest.raises(ValueError):
        EvalStep(model, ctx["forward"], stager.inputs, stager.binimgs, loss=ctx["loss_fn"], thresholds=[0.4])
    stager.n_valid.fill_(2)
    evaluate.capture(warmup=1)
    assert "lss_confusion_accum" in launched and "lss_bce_iou_accum_pc" not in launched
    for nv in (2, 1):
        evaluate.reset()
        stager.n_valid.fill_(nv)
        evaluate()
        info = evaluate.read(n_samples=nv)
        x = evaluate.static_preds.float().cpu()
        labels = stager.binimgs.cpu()
        conf = E.confusion_counts(x, labels, None, nv)
        loss64, _ = E.closed_form(x[:nv].double(), labels[:nv], None, torch.tensor(CW))
        assert info["confusion"] == conf.tolist() and conf.sum() == nv * 200 * 200
        assert info["loss"] == pytest.approx(loss64.item(), rel=E.LOSS_RTOL, abs=E.LOSS_ATOL)
        tp = np.diag(conf).astype(float)
        union = conf.sum(0) + conf.sum(1) - np.diag(conf)
        per = [tp[c] / union[c] if union[c] > 0 else None for c in range(3)]
        assert info["iou_per_class"] == per and info["pixel_acc"] == tp.sum() / conf.sum()
        fg = [v for v in per[1:] if v is not None]
        assert info["iou"] == (sum(fg) / len(fg) if fg else None) and "valid_fraction" not in info


@pytest.fixture(scope="module")
def short_run(root, tmp_path_factory):
    logdir = tmp_path_factory.mktemp("run_exclusive")
    seen = []
    real = _lib.check
    _lib.check = lambda code, what: (seen.append(what), real(code, what))[1]
    try:
        out = trainer.train(root, nepochs=2, val_step=3, save_step=6, seed=0, logdir=str(logdir), loss_step=1,
                            iou_step=2, max_steps=6, label_groups=GROUPS, exclusive=True, class_weight=CW,
                            valid_mask="grid", bev_rot_lim=(-20.0, 20.0), **KW)
    finally:
        _lib.check = real
    return logdir, out, seen


def test_short_run_writes_the_confusion_keys(short_run):
    logdir, out, seen = short_run
    assert out["counter"] == 6 and out["skipped"] == 0 and math.isfinite(out["loss"])
    for name in NEW[:2] + NEW[3:]:
        assert name in seen, name
    assert "lss_simbev_valid_mask" in seen and "lss_seg_metrics_accum_masked" not in seen
    events = [json.loads(line) for line in open(logdir / "metrics.jsonl")]
    cfg = events[0]
    assert cfg["event"] == "config" and cfg["exclusive"] is True and cfg["class_weight"] == CW
    assert cfg["label_groups"] == GROUPS and cfg["valid_mask"] == "grid" and cfg["pos_weight"] is None
    val_ev = [e for e in events if e["event"] == "val"]
    iou_ev = [e for e in events if e["event"] == "train_iou"]
    assert [e["counter"] for e in val_ev] == [3, 6] and [e["counter"] for e in iou_ev] == [2, 4, 6]
    for e in val_ev + iou_ev:
        for key in trainer.EXCLUSIVE_KEYS:
            assert key in e, key
        conf = np.array(e["confusion"])
        assert conf.shape == (3, 3) and conf.sum() > 0
        fg = [v for v in e["iou_per_class"][1:] if v is not None]
        assert e["iou"] == (pytest.approx(sum(fg) / len(fg), rel=1e-12) if fg else None)
        assert e["pixel_acc"] == pytest.approx(np.trace(conf) / conf.sum(), rel=1e-12)
    for e in val_ev:
        assert math.isfinite(e["loss"]) and e["valid_fraction"] == 1.0  # validation is never augmented
        assert np.array(e["confusion"]).sum() == 2 * 200 * 200
    assert any(np.array(e["confusion"]).sum() < 2 * 200 * 200 for e in iou_ev)  # rotated corners are masked out
    losses = [e["loss"] for e in events if e["event"] == "train"]
    assert len(losses) == 6 and all(math.isfinite(v) for v in losses)
    ck = torch.load(logdir / "model_000006.pt", map_location="cpu")
    assert ck["model_state_dict"]["bevencode.up2.4.weight"].shape == (3, 128, 1, 1)
    assert (logdir / "model_final.pt").exists()


def test_resume_and_refuse_another_head_width(short_run, root, tmp_path):
    logdir, _, _ = short_run
    path = logdir / "model_000006.pt"
    seen = {}
    out = trainer.train(root, nepochs=3, val_step=100, save_step=100, seed=0, logdir=str(tmp_path / "resumed"),
                        resume=str(path), max_steps=1, on_start=lambda c: seen.update(counter=c["counter"]),
                        label_groups=GROUPS, exclusive=True, class_weight=CW, valid_mask="grid",
                        bev_rot_lim=(-20.0, 20.0), **KW)
    assert seen["counter"] == 6 and out["counter"] == 7
    two = tmp_path / "two_class.pt"
    torch.save(L.compile_model(GC, DAC, outC=2).state_dict(), two)  # the sigmoid run of the same groups
    captured = []
    with pytest.raises(RuntimeError, match=r"2 output classes.*ask for 3"):
        trainer.train(root, nepochs=1, seed=0, logdir=str(tmp_path / "refused"), resume=str(two), max_steps=1,
                      on_start=captured.append, label_groups=GROUPS, exclusive=True, **KW)
    with pytest.raises(RuntimeError, match=r"3 output classes.*ask for 2"):
        trainer.train(root, nepochs=1, seed=0, logdir=str(tmp_path / "refused2"), resume=str(path), max_steps=1,
                      on_start=captured.append, label_groups=GROUPS, **KW)
    assert not captured


def test_predict_writes_class_maps_that_give_its_confusion_matrix(root, tmp_path, launched):
    torch.manual_seed(5)
    model = L.compile_model(GC, DAC, outC=3)
    ckpt = tmp_path / "model.pt"
    torch.save(model.state_dict(), ckpt)
    out = tmp_path / "pred"
    a = P.parser().parse_args(["--modelf", str(ckpt), "--dataroot", root, "--out", str(out), "--bsz", "2", "--dtype",
                               "fp32", "--nworkers", "0", "--miopen_find", "0", "--exclusive", "1", "--label_groups",
                               "0;1,2,3", "--class_weight", "0.5,1,2", "--drop_each", "1"])
    info = P.predict(a, grid_conf=GC, data_aug_conf=DAC)
    assert "lss_argmax_classes" in launched and "lss_confusion_accum" in launched
    on_disk = json.load(open(out / "metrics.json"))
    assert on_disk == json.loads(json.dumps(info)) and on_disk["exclusive"] is True and on_disk["classes"] == 3
    _, vl = simbev.compile_data("", root, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV)
    n_val = len(vl.dataset)
    files = sorted(os.listdir(out / "preds"))
    assert files == sorted(f"{i}.npy" for i in range(n_val)) and n_val > 0 and on_disk["samples"] == n_val
    conf = np.zeros((3, 3), dtype=np.int64)
    i = 0
    for raw in vl.loader:
        labels = E.class_index_ref(raw[-1].numpy(), GROUPS)
        for lab in labels:
            pred = np.load(out / "preds" / f"{i}.npy")
            assert pred.shape == (200, 200) and pred.dtype == np.uint8 and pred.max() <= 2
            np.add.at(conf, (lab.astype(np.int64).ravel(), pred.astype(np.int64).ravel()), 1)
            i += 1
    assert i == n_val and on_disk["confusion"] == conf.tolist()
    assert set(on_disk["drop_each"]) == set(simbev.CAMERA_ORDER)
    for entry in on_disk["drop_each"].values():
        assert np.array(entry["confusion"]).sum() == conf.sum() and "iou" in entry and "pixel_acc" in entry
    # the Predictor's outputs of the last batch agree among themselves
    p = L.Predictor(_fresh_model(3, model.state_dict()), 2, DEV, amp_dtype=None, graph=False, exclusive=True)
    fin = simbev.finish_batch(next(iter(vl.loader)), DAC["final_dim"], DEV)
    logits = p(*fin[:6])
    cls, probs, masks = p.classes(), p.probs(), p.masks()
    assert np.array_equal(cls.cpu().numpy(), E.argmax_rule(logits.float().cpu().numpy()))
    assert tuple(masks.shape) == (2, 2, 200, 200) and masks.dtype == torch.uint8
    assert torch.equal(masks[:, 0], (cls == 1).to(torch.uint8)) and torch.equal(masks[:, 1], (cls == 2).to(torch.uint8))
    torch.testing.assert_close(probs.sum(dim=1), torch.ones_like(probs[:, 0]))
    with pytest.raises(RuntimeError):
        L.Predictor(_fresh_model(1), 2, DEV, graph=False).classes()


def test_default_step_launches_no_new_kernel_and_computes_what_the_sigmoid_entries_compute(raws, launched):
    batches, _ = raws
    torch.manual_seed(3)
    ctx = trainer.build_step(GC, DAC, 2, DEV, n_val=2)
    stager, step, evaluate = ctx["stager"], ctx["step"], ctx["evaluate"]
    assert stager.binimgs.dtype == torch.float32 and tuple(stager.binimgs.shape) == (2, 1, 200, 200)
    assert not stager.exclusive and not evaluate.exclusive
    stager.stage(batches[0])
    stager.commit()
    torch.cuda.manual_seed(7)
    loss = step.forward_backward().detach()
    evaluate.eager()
    torch.cuda.synchronize()
    assert not set(launched) & set(NEW) and "lss_bce_logits" in launched and "lss_bce_iou_accum" in launched
    assert torch.equal(stager.binimgs, simbev.class_masks(batches[0][-1].to(DEV), None))
    # the loss of the step's logits through the untouched entry, called directly
    lib = _lib.load()
    x = step.static_preds.contiguous()
    n = x.numel()
    partial = torch.empty(int(lib.lss_bce_partials(n)), device=DEV)
    again = torch.empty((), device=DEV)
    grad = torch.empty_like(x)
    assert lib.lss_bce_logits(_lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(stager.binimgs), n, 2.13, _lib.ptr(partial),
                              _lib.ptr(again), _lib.ptr(grad), _lib.stream_handle(DEV)) == 0
    torch.cuda.synchronize()
    assert torch.equal(again, loss)
    totals = torch.zeros(3, device=DEV, dtype=torch.float64)
    T.val_accumulate(evaluate.static_preds, stager.binimgs, totals, n_valid=stager.n_valid, pos_weight=2.13)
    assert torch.equal(totals, evaluate.totals)
    p = L.Predictor(_fresh_model(1), 2, DEV, graph=False)  # (a module no training step is bound to)
    assert not p.exclusive
    out = p(*simbev.finish_batch(batches[0], DAC["final_dim"], DEV)[:6])
    assert torch.equal(p.masks(), (out > 0).to(torch.uint8)) and torch.equal(p.probs(), out.float().sigmoid())
    assert not set(launched) & set(NEW)
