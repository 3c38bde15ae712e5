"""Camera dropout, host side: argument errors of ``train(ncams=)`` and ``--drop_cams``, the parsing of
``--drop_cams``, ``simbev.fov_cameras(alive=)`` (a dead camera's block is all zeros, and a numpy restatement of
``lss_simbev_valid_mask``'s projection shows that a zero block sees no cell), and the loader's camera subset
(``Ncams`` = 3: three sorted distinct cameras per training sample, all six in validation). No GPU."""
import numpy as np
import pytest
import torch

from lss_carla_amd import predict, simbev, synthetic as syn, trainer
from lss_carla_amd.tools import gen_dx_bx


@pytest.mark.parametrize("ncams", [0, 7, -1, 2.5, "5", None, True])
def test_train_rejects_a_bad_ncams_before_anything_else(ncams, tmp_path):
    # (a dataroot that does not exist and no GPU: the argument error comes first)
    with pytest.raises(ValueError, match="ncams"):
        trainer.train(str(tmp_path / "nowhere"), ncams=ncams, logdir=str(tmp_path / "log"), use_wandb=False)
    assert not (tmp_path / "log").exists()


@pytest.mark.parametrize("ncams", [1, 3, 5, 6, np.int64(5)])
def test_ncams_one_to_six_pass_the_argument_check(ncams):
    """(That such a run trains is tests/test_gpu_trainer_ncams.py's.)"""
    got = trainer._check_ncams(ncams)
    assert got == int(ncams) and type(got) is int


def test_parse_drop_cams():
    assert predict.parse_drop_cams(None) == []
    assert predict.parse_drop_cams("") == []
    assert predict.parse_drop_cams("front") == [1]
    assert predict.parse_drop_cams("front,back_left") == [1, 3]
    assert predict.parse_drop_cams("back_left, front ,front") == [1, 3]
    assert predict.parse_drop_cams("5,0") == [0, 5]
    assert predict.parse_drop_cams("back,2") == [2, 4]
    assert predict.parse_drop_cams([3, "front_left"]) == [0, 3]
    assert [simbev.CAMERA_ORDER[i] for i in predict.parse_drop_cams("front,back_left")] == ["front", "back_left"]


@pytest.mark.parametrize("text", ["frnt", "front,rear", "6", "-1", "front;back", "1.5"])
def test_parse_drop_cams_rejects_unknown_names_and_indices(text):
    with pytest.raises(ValueError, match="drop_cams"):
        predict.parse_drop_cams(text)


def test_predict_cli_has_the_flags_and_a_bad_name_fails_before_the_gpu(tmp_path):
    a = predict.parser().parse_args(["--modelf", "m", "--dataroot", "d", "--out", "o", "--drop_cams", "front,back_left",
                                     "--drop_each", "1"])
    assert a.drop_cams == "front,back_left" and a.drop_each == 1
    d = predict.parser().parse_args(["--modelf", "m", "--dataroot", "d", "--out", "o"])
    assert d.drop_cams is None and d.drop_each == 0
    # a bad name: ValueError from predict() itself, before the GPU is asked for, a file is read or --out is made
    out = tmp_path / "out"
    bad = predict.parser().parse_args(["--modelf", str(tmp_path / "none.pt"), "--dataroot", str(tmp_path), "--out", str(out),
                                       "--drop_cams", "front,rear"])
    with pytest.raises(ValueError, match="drop_cams"):
        predict.predict(bad)
    assert not out.exists()


# ----------------------------------------------------------------------------- fov_cameras(alive=)
def _np_valid(cams, post_trans, gc, final_dim, z=0.0):
    """``lss_simbev_valid_mask``'s "fov" test restated in numpy (float64): cell centre p at height z; camera point
    c = M p + o, depth d = c_2 in [d_lo, d_hi) with d_lo > 0, pixel P (c_0 / d, c_1 / d) + post_trans inside the
    image. (n, X, Y) bool."""
    dx, bx, nx = (np.asarray(v, dtype=np.float64) for v in gen_dx_bx(gc["xbound"], gc["ybound"], gc["zbound"]))
    X, Y = int(nx[0]), int(nx[1])
    d_lo, d_hi = float(gc["dbound"][0]), float(gc["dbound"][1])
    fH, fW = final_dim
    xs = bx[0] + dx[0] * np.arange(X)
    ys = bx[1] + dx[1] * np.arange(Y)
    p = np.stack(np.broadcast_arrays(xs[:, None], ys[None, :], np.full((X, Y), z)), -1)  # (X, Y, 3)
    cams = np.asarray(cams, dtype=np.float64)
    q = np.asarray(post_trans, dtype=np.float64)[..., :2]
    n, N = cams.shape[:2]
    out = np.zeros((n, X, Y), dtype=bool)
    for i in range(n):
        for c in range(N):
            M, o, P = cams[i, c, :9].reshape(3, 3), cams[i, c, 9:12], cams[i, c, 12:16].reshape(2, 2)
            cp = p @ M.T + o
            d = cp[..., 2]
            ok = (d >= d_lo) & (d < d_hi)
            with np.errstate(divide="ignore", invalid="ignore"):
                uv = np.stack((cp[..., 0] / d, cp[..., 1] / d), -1) @ P.T + q[i, c]
            ok &= (uv[..., 0] >= 0) & (uv[..., 0] <= fW - 1) & (uv[..., 1] >= 0) & (uv[..., 1] <= fH - 1)
            out[i] |= ok
    return out


def test_fov_cameras_alive_zeroes_dead_blocks_and_a_zero_block_sees_nothing():
    fd = (128, 352)
    rig = syn.make_rig(2, 6, fd, seed=3)
    full = simbev.fov_cameras(**rig)
    assert full.shape == (2, 6, 16) and full.dtype == torch.float32
    assert torch.equal(simbev.fov_cameras(**rig, alive=None), full)
    assert torch.equal(simbev.fov_cameras(**rig, alive=torch.ones(6, dtype=torch.uint8)), full)
    one = simbev.fov_cameras(**rig, alive=[1, 0, 1, 1, 1, 1])  # (N,): every sample
    assert not one[:, 1].any() and torch.equal(one[:, [0, 2, 3, 4, 5]], full[:, [0, 2, 3, 4, 5]])
    per = torch.tensor([[1, 1, 1, 0, 1, 1], [0, 1, 1, 1, 1, 0]], dtype=torch.bool)  # (b, N): per sample
    got = simbev.fov_cameras(**rig, alive=per)
    assert torch.equal(got[per], full[per]) and not got[~per].any()
    assert got.is_contiguous()
    with pytest.raises(ValueError, match="alive"):
        simbev.fov_cameras(**rig, alive=[1, 0, 1])
    # what the mask kernel makes of it: dead cameras add no cell, and with every camera dead no cell is valid
    gc = syn.grid_conf()
    v_full = _np_valid(full, rig["post_trans"], gc, fd)
    v_got = _np_valid(got, rig["post_trans"], gc, fd)
    assert v_full.mean() > 0.25
    want = np.zeros_like(v_full)
    for i in range(2):
        keep = [c for c in range(6) if per[i, c]]
        want[i] = _np_valid(full[i:i + 1, keep], rig["post_trans"][i:i + 1, keep], gc, fd)[0]
    np.testing.assert_array_equal(v_got, want)
    assert (v_got <= v_full).all() and (v_got != v_full).any()
    none = simbev.fov_cameras(**rig, alive=torch.zeros(6))
    assert not none.any() and not _np_valid(none, rig["post_trans"], gc, fd).any()


# ----------------------------------------------------------------------------- the loader's subset
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("tree")
    n = syn.make_simbev_tree(str(root), n_scenes=5, per_scene=2, H=28, W=60, X=200, Y=200)
    assert n == 10
    return str(root)


def test_loader_draws_three_sorted_cameras_in_training_and_six_in_validation(tree):
    dac = {"resize_lim": (1.0, 1.0), "final_dim": (32, 64), "rot_lim": (0.0, 0.0), "H": 28, "W": 60,
           "rand_flip": False, "bot_pct_lim": (0.0, 0.0), "Ncams": 3}
    gc = syn.grid_conf()
    train = simbev.SegmentationData(tree, is_train=True, data_aug_conf=dac, grid_conf=gc)
    val = simbev.SegmentationData(tree, is_train=False, data_aug_conf=dac, grid_conf=gc)
    np.random.seed(0)
    seen = set()
    for _ in range(8):
        cams = train.choose_cams()
        assert len(cams) == 3 and cams == sorted(set(cams)) and all(0 <= c < 6 for c in cams)
        seen.add(tuple(cams))
    assert len(seen) > 1, "the subset is drawn per sample"
    assert val.choose_cams() == list(range(6))
    np.random.seed(1)
    want = sorted(np.random.choice(list(range(6)), 3, replace=False).tolist())
    np.random.seed(1)
    s = train[0]
    assert s[0].shape[0] == 3 and s[0].dtype == torch.uint8          # three decoded images
    for t in s[1:6]:
        assert t.shape[0] == 3
    # the rig rows are those of the drawn cameras, in ascending camera order
    ext = np.array(train.samples[0]["extrinsics"])
    np.testing.assert_allclose(s[2].numpy(), ext[want][:, :3, 3].astype(np.float32))
    v = val[0]
    assert v[0].shape[0] == 6 and all(t.shape[0] == 6 for t in v[1:6])
