"""Host-side pieces of multi-class training (no GPU): the trainer's --label_groups / --pos_weight parsing,
SimpleLoss with one weight per class on the CPU, synthetic.make_simbev_tree's default tree unchanged by
box_classes, and the K-channel head kernels' descriptors (no scratch, no spills)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from lss_carla_amd import _lib, simbev, synthetic, tools as T, trainer
from test_kernel_resources import _kernel_notes


# ----------------------------------------------------------------------------- command line
def test_label_groups_parsing():
    assert trainer.parse_label_groups("0;1,2,3;6,7") == [[0], [1, 2, 3], [6, 7]]
    assert trainer.parse_label_groups(" 1, 2 ,3 ") == [[1, 2, 3]]
    assert trainer.parse_label_groups(None) is None and trainer.parse_label_groups("") is None
    for bad in ("0;;1", "0;", "a,b"):
        with pytest.raises(ValueError):
            trainer.parse_label_groups(bad)


def test_pos_weight_parsing():
    assert trainer.parse_pos_weight("2.13") == 2.13 and isinstance(trainer.parse_pos_weight("2.13"), float)
    assert trainer.parse_pos_weight("1.0,2.13,5.0") == [1.0, 2.13, 5.0]
    with pytest.raises(ValueError):
        trainer.parse_pos_weight("")
    with pytest.raises(ValueError):
        trainer.parse_pos_weight("1.0,x")


def test_class_setup_pairs_weights_with_groups():
    assert trainer._class_setup(None, 2.13) == (None, 1, 2.13)
    assert trainer._class_setup(None, [2.13]) == (None, 1, 2.13)
    assert trainer._class_setup([[0], (1, 2, 3)], 2.13) == ([[0], [1, 2, 3]], 2, 2.13)
    assert trainer._class_setup([[0], [1, 2, 3]], [1.0, 2.0]) == ([[0], [1, 2, 3]], 2, [1.0, 2.0])
    with pytest.raises(ValueError):
        trainer._class_setup([[0], [1, 2, 3]], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        trainer._class_setup([[0], []], 2.13)
    with pytest.raises(ValueError):
        trainer._class_setup([[c] for c in range(9)], 2.13)  # more groups than the label kernel takes


def test_group_bits():
    assert simbev.group_bits([[1, 2, 3], [0], [31]]) == [0b1110, 1, 1 << 31]
    for bad in ([], [[]], [[32]], [[-1]], [[1.5]]):
        with pytest.raises(ValueError):
            simbev.group_bits(bad)


def test_cli_passes_groups_and_weights(monkeypatch):
    seen = {}
    monkeypatch.setattr(trainer, "train", lambda **kw: seen.update(kw))
    trainer.main(["--dataroot", "/data", "--label_groups", "0;1,2,3", "--pos_weight", "1.0,2.13"])
    assert seen["label_groups"] == [[0], [1, 2, 3]] and seen["pos_weight"] == [1.0, 2.13]
    trainer.main(["--dataroot", "/data"])
    assert seen["label_groups"] is None and seen["pos_weight"] == 2.13


# ----------------------------------------------------------------------------- loss and metrics on the CPU
def test_simple_loss_with_class_weights_on_cpu_is_torchs():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 5, 7, generator=g, requires_grad=True)
    t = (torch.rand(2, 3, 5, 7, generator=g) < 0.3).float()
    w = [0.5, 2.13, 4.0]
    fn = T.SimpleLoss(w)
    got = fn(x, t)
    want = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(w).view(3, 1, 1))(x, t)
    assert torch.equal(got, want)
    got.backward()
    g1 = x.grad.clone()
    x.grad = None
    want.backward()
    assert torch.equal(g1, x.grad)
    assert torch.equal(T.SimpleLoss(w)(x.detach().bfloat16(), t), fn(x.detach().bfloat16().float(), t))
    # a float stays the reference's module
    assert torch.equal(T.SimpleLoss(2.13)(x, t), torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([2.13]))(x, t))
    with pytest.raises(RuntimeError):
        fn(torch.zeros(2, 2, 5, 7), torch.zeros(2, 2, 5, 7))
    with pytest.raises(ValueError):
        T.SimpleLoss([])


def test_iou_summary():
    assert T.iou_summary([3.0], [4.0]) == {"iou": 0.75, "iou_per_class": [0.75]}
    assert T.iou_summary([1.0, 0.0, 3.0], [2.0, 0.0, 4.0]) == {"iou": 0.625, "iou_per_class": [0.5, None, 0.75]}
    with pytest.raises(ZeroDivisionError):
        T.iou_summary([0.0], [0.0])
    with pytest.raises(ZeroDivisionError):
        T.iou_summary([0.0, 0.0], [0.0, 0.0])


def test_get_val_info_per_class_on_cpu():
    g = torch.Generator().manual_seed(1)
    preds = torch.randn(2, 2, 6, 6, generator=g)
    labels = (torch.rand(2, 2, 6, 6, generator=g) < 0.4).float()

    class Model(torch.nn.Module):
        def forward(self, x, *rig):
            return preds

    class Loader(list):
        dataset = [0, 1]

    z = torch.zeros(2, 1)
    info = T.get_val_info(Model(), Loader([(z, z, z, z, z, z, labels)]), T.SimpleLoss([1.0, 2.0]), torch.device("cpu"),
                          use_tqdm=False)
    p, q = preds > 0, labels != 0
    want = [((p & q)[:, k].sum() / (p | q)[:, k].sum()).item() for k in range(2)]
    assert set(info) == {"loss", "iou", "iou_per_class"}
    assert info["iou_per_class"] == pytest.approx(want) and info["iou"] == pytest.approx(sum(want) / 2)


# ----------------------------------------------------------------------------- synthetic trees
def _parent_bevs_and_meta(root, n_scenes, per_scene, H, W, seed, n_classes=8, X=200, Y=200):
    """make_simbev_tree as it was before box_classes existed, without the files: the same generator, the same
    draws in the same order (six images' worth per sample, then twelve boxes in classes 1-3); returns
    ({npz path relative to root: bev}, {meta path: records})."""
    rng = np.random.default_rng(seed)
    rig = synthetic.make_rig(1, 6, (H, W), seed=seed)
    extr = np.tile(np.eye(4), (6, 1, 1))
    extr[:, :3, :3] = rig["rots"][0].double().numpy()
    extr[:, :3, 3] = rig["trans"][0].double().numpy()
    fx = W / (2.0 * math.tan(math.radians(synthetic.HFOV_DEG / 2.0)))
    K = [[fx, 0.0, W / 2.0], [0.0, fx, H / 2.0], [0.0, 0.0, 1.0]]
    cams = [f"RGB-CAM_{c.upper()}" for c in simbev.CAMERA_ORDER]
    bevs, metas = {}, {}
    for s in range(n_scenes):
        d = os.path.join("SimBEV_cvt_label", f"scene_{s:04d}", "yaw0pitch0")
        meta = []
        for k in range(per_scene):
            tok = f"s{s}_{k}"
            for _ in cams:
                rng.integers(0, 256, size=(H // 8 + 1, W // 8 + 1, 3), dtype=np.uint8)
            bev = np.zeros((n_classes, X, Y), dtype=np.uint8)
            for _ in range(12):
                cls = int(rng.integers(1, 4))
                x0, y0 = int(rng.integers(0, X - 10)), int(rng.integers(0, Y - 5))
                bev[cls, x0:x0 + 9, y0:y0 + 4] = 1
            bevs[os.path.join(d, f"bev_{tok}.npz")] = bev
            meta.append({"token": tok, "images": [f"sweeps/{c}/{tok}.jpg" for c in cams], "intrinsics": [K] * 6,
                         "extrinsics": extr.tolist(), "bev": f"bev_{tok}.npz"})
        metas[os.path.join(d, "meta.json")] = meta
    return bevs, metas


def test_default_tree_is_unchanged(tmp_path):
    args = dict(n_scenes=1, per_scene=2, H=16, W=24, seed=3)
    assert synthetic.make_simbev_tree(str(tmp_path / "a"), **args) == 2
    assert synthetic.make_simbev_tree(str(tmp_path / "b"), box_classes=[1, 2, 3], **args) == 2  # spelled out
    bevs, metas = _parent_bevs_and_meta(str(tmp_path), **args)
    assert len(bevs) == 2
    for name in ("a", "b"):
        for rel, want in bevs.items():
            got = np.load(tmp_path / name / rel)["bev"]
            assert got.dtype == want.dtype and np.array_equal(got, want), rel
        for rel, want in metas.items():
            assert json.load(open(tmp_path / name / rel)) == json.loads(json.dumps(want)), rel
    for rel in bevs:  # and the two trees' files are the same bytes
        assert (tmp_path / "a" / rel).read_bytes() == (tmp_path / "b" / rel).read_bytes()
    jpgs = sorted(p.relative_to(tmp_path / "a") for p in (tmp_path / "a" / "sweeps").rglob("*.jpg"))
    assert len(jpgs) == 12
    for rel in jpgs:
        assert (tmp_path / "a" / rel).read_bytes() == (tmp_path / "b" / rel).read_bytes()


def test_box_classes_place_boxes_in_those_channels(tmp_path):
    synthetic.make_simbev_tree(str(tmp_path), n_scenes=1, per_scene=3, H=16, W=24, seed=0, box_classes=(0, 5))
    used = np.zeros(8, dtype=bool)
    for p in (tmp_path / "SimBEV_cvt_label").rglob("*.npz"):
        used |= np.load(p)["bev"].any(axis=(1, 2))
    assert used.tolist() == [True, False, False, False, False, True, False, False]
    with pytest.raises(ValueError):
        synthetic.make_simbev_tree(str(tmp_path / "bad"), 1, 1, H=16, W=24, box_classes=(8,))


# ----------------------------------------------------------------------------- kernel descriptors
def test_headk_kernels_use_no_scratch():
    """Every <lanes per row, K> instance of the K-channel head (7 row widths x K = 2..8, forward and backward)
    keeps its weights and accumulators in registers: no private segment, no spilled VGPRs."""
    kernels = _kernel_notes(_lib.LIB_PATH)
    for name in ("k_headk_fwd", "k_headk_bwd"):
        mine = {k: v for k, v in kernels.items() if name in k}
        assert len(mine) >= 49, (name, len(mine))
        bad = {k: v for k, v in mine.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)}
        assert not bad, bad
    other = {}
    for name, least in (("k_sig_loss_fwd", 8), ("k_bce_iou_pc", 2), ("k_class_masks", 2)):  # (the loss template: 4 x 2 dtypes)
        mine = {k: v for k, v in kernels.items() if name in k}
        assert len(mine) >= least, (name, sorted(mine))
        other.update(mine)
    assert not {k: v for k, v in other.items() if v.get("private_segment_fixed_size", 0)}, other
