"""The host side of the BEV-space augmentation (no GPU): the draws leave numpy's generator as they found it when the
option is off and only follow the image augmentation's when it is on; the matrices against float64 constructions;
the numpy restatement of the label warp (tests/bev_aug_cases.py) exact on the grid's pure symmetries -- the CPU gate
of tests/test_gpu_bev_aug.py's symmetry test --; the refusals of the C entry, of label_index_matrix and of the
trainer's arguments."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import bev_aug_cases as C
from conftest import GOLDEN
from lss_carla_amd import _lib, simbev, trainer

SMALL = os.path.join(GOLDEN, "simbev_small")


def _train_conf():
    dac = json.loads(str(np.load(os.path.join(GOLDEN, "simbev_ref.npz"))["train_aug"]))
    dac["final_dim"] = tuple(dac["final_dim"])
    for k in ("resize_lim", "rot_lim", "bot_pct_lim"):
        dac[k] = tuple(dac[k])
    return dac


def _dataset(extra, is_train=True):
    return simbev.SegmentationData(SMALL, is_train=is_train, data_aug_conf={**_train_conf(), **extra}, grid_conf=C.GC)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ----------------------------------------------------------------------------- RNG neutrality
@pytest.mark.parametrize("extra", [{}, C.BEV_NEUTRAL], ids=["absent", "neutral"])
def test_option_off_is_the_reference_loader_draw_for_draw(extra):
    """The golden samples of the reference's loader under the same seeds, element for element, and the generator left
    where the image augmentation's draws alone leave it."""
    z = np.load(os.path.join(GOLDEN, "simbev_ref.npz"))
    ds = _dataset(extra)
    assert not ds.bev_aug and not simbev.bev_aug_enabled(ds.data_aug_conf)
    for i in range(len(ds)):
        np.random.seed(100 + i)
        raw = ds[i]
        after = np.random.get_state()
        assert len(raw) == 9  # today's tuple: nothing before the BEV map
        for name, t in zip(("rots", "trans", "intrins", "post_rots", "post_trans"), raw[1:6]):
            np.testing.assert_array_equal(t.numpy(), z[f"train{i}_{name}"], err_msg=f"{i} {name}")
        np.random.seed(100 + i)
        want = simbev.draw_augmentation(ds.data_aug_conf, True)
        assert _same_state(after, np.random.get_state())
        assert raw[6].tolist() == [*want[1], *want[2], int(want[3])] and float(raw[7]) == float(want[4])


def test_off_draws_nothing():
    np.random.seed(5)
    before = np.random.get_state()
    assert simbev.draw_bev_augmentation({}, True) == (0.0, 1.0, False, False)
    assert simbev.draw_bev_augmentation(C.BEV_NEUTRAL, True) == (0.0, 1.0, False, False)
    assert simbev.draw_bev_augmentation(C.BEV_ON, False) == (0.0, 1.0, False, False)  # validation never augments
    assert _same_state(before, np.random.get_state())


@pytest.mark.parametrize("flip", [True, False])
def test_option_on_draws_after_the_image_augmentation(flip):
    """The image augmentation's values are the off run's; then angle, scale and (only with bev_flip) the two coins;
    the rig is the off run's composed with A and the extra element is A's label index matrix."""
    on = {**C.BEV_ON, "bev_flip": flip}
    ds_off, ds_on = _dataset({}), _dataset(on)
    assert ds_on.bev_aug
    for i in range(len(ds_on)):
        np.random.seed(100 + i)
        off = ds_off[i]
        np.random.seed(100 + i)
        got = ds_on[i]
        after = np.random.get_state()
        np.random.seed(100 + i)
        simbev.draw_augmentation(ds_on.data_aug_conf, True)
        theta = np.random.uniform(*on["bev_rot_lim"])
        scale = np.random.uniform(*on["bev_scale_lim"])
        fx, fy = (bool(np.random.choice([0, 1])), bool(np.random.choice([0, 1]))) if flip else (False, False)
        assert _same_state(after, np.random.get_state())
        assert len(got) == 10 and got[-1].dtype == torch.uint8 and torch.equal(got[-1], off[-1])  # the BEV map stays last
        for k in (0, 3, 4, 5, 6, 7):  # images, intrins, post_rots, post_trans, the image augmentation
            assert torch.equal(got[k], off[k]), k
        A = simbev.bev_aug_matrix(theta, scale, fx, fy)
        rots, trans = simbev.compose_rig(A, off[1], off[2])
        assert torch.equal(got[1], rots) and torch.equal(got[2], trans)
        assert not torch.equal(got[1], off[1])
        assert got[8].dtype == torch.float32 and got[8].shape == (2, 3)
        np.testing.assert_array_equal(got[8].numpy(), simbev.label_index_matrix(A, C.GC))


def test_validation_samples_carry_the_identity_and_the_rig_as_it_is():
    off, on = _dataset({}, is_train=False), _dataset(C.BEV_ON, is_train=False)
    np.random.seed(1)
    before = np.random.get_state()
    a, b = off[0], on[0]
    assert _same_state(before, np.random.get_state())
    assert len(a) == 9 and len(b) == 10
    for x, y in zip(a[:8] + a[8:], b[:8] + b[9:]):
        assert torch.equal(x, y)
    np.testing.assert_array_equal(b[8].numpy(), np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32))


def test_vizdata_keeps_its_placeholder_and_the_map_last():
    ds = simbev.VizData(SMALL, is_train=True, data_aug_conf={**_train_conf(), **C.BEV_ON}, grid_conf=C.GC)
    np.random.seed(2)
    raw = ds[0]
    assert len(raw) == 11 and raw[8].shape == (3, 0) and raw[9].shape == (2, 3) and raw[10].dtype == torch.uint8


# ----------------------------------------------------------------------------- matrix algebra
@pytest.mark.parametrize("theta,scale,fx,fy", [(0.0, 1.0, False, False), (20.0, 0.95, True, False),
                                               (-22.5, 1.1, False, True), (137.0, 0.5, True, True)])
def test_bev_aug_matrix_against_float64(theta, scale, fx, fy):
    A = simbev.bev_aug_matrix(theta, scale, fx, fy)
    assert A.dtype == np.float32 and A.shape == (3, 3)
    t = math.radians(theta)
    want = np.zeros((3, 3))
    sx, sy = (-1.0 if fx else 1.0), (-1.0 if fy else 1.0)
    want[0] = [scale * math.cos(t) * sx, -scale * math.sin(t) * sy, 0.0]
    want[1] = [scale * math.sin(t) * sx, scale * math.cos(t) * sy, 0.0]
    want[2, 2] = scale  # z is scaled as well
    np.testing.assert_array_equal(A, want.astype(np.float32))
    if (theta, scale, fx, fy) == (0.0, 1.0, False, False):
        np.testing.assert_array_equal(A, np.eye(3, dtype=np.float32))


def test_compose_rig_moves_camera_points_by_A():
    g = torch.Generator().manual_seed(0)
    rots, trans = torch.randn(2, 6, 3, 3, generator=g), torch.randn(2, 6, 3, generator=g) * 2
    x = torch.randn(2, 6, 50, 3, generator=g) * 30
    A = simbev.bev_aug_matrix(20.0, 0.95, True, False)
    r2, t2 = simbev.compose_rig(A, rots, trans)
    assert r2.dtype == torch.float32 and r2.shape == rots.shape and t2.shape == trans.shape
    got = torch.einsum("bnij,bnpj->bnpi", r2.double(), x.double()) + t2.double()[:, :, None]
    ego = torch.einsum("bnij,bnpj->bnpi", rots.double(), x.double()) + trans.double()[:, :, None]
    want = torch.einsum("ij,bnpj->bnpi", torch.from_numpy(A).double(), ego)
    # fp32 rounding of the composed matrices: |x| <= ~150 times 3 products of eps 6e-8 each, well under 1e-3
    assert (got - want).abs().max().item() < 1e-3
    one_r, one_t = simbev.compose_rig(A, rots[0], trans[0])  # a sample's (N, 3, 3) / (N, 3), as the dataset calls it
    assert torch.equal(one_r, r2[0]) and torch.equal(one_t, t2[0])


def test_label_index_matrix_identity_and_formula():
    eye = simbev.label_index_matrix(np.eye(3, dtype=np.float32), C.GC)
    assert eye.dtype == np.float32
    np.testing.assert_array_equal(eye, np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32))
    # M = D^-1 A2^-1 D, b = D^-1 (A2^-1 lo - lo) on a grid whose two axes differ
    gc = {"xbound": [-30.0, 50.0, 0.5], "ybound": [-20.0, 20.0, 0.25], "zbound": [-10.0, 10.0, 20.0]}
    A = simbev.bev_aug_matrix(20.0, 0.95, True, False)
    inv = np.linalg.inv(A[:2, :2].astype(np.float64))
    D, lo = np.diag([0.5, 0.25]), np.array([-30.0, -20.0])
    want = np.concatenate([np.linalg.inv(D) @ inv @ D, (np.linalg.inv(D) @ (inv @ lo - lo))[:, None]], axis=1)
    got = simbev.label_index_matrix(A, gc)
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=1e-6)  # one rounding to fp32
    # a cell centre goes where the metric map sends it: output centre p', source A2^-1 p'
    u = np.array([10.5, 100.5])
    src = inv @ (lo + D @ u)
    np.testing.assert_allclose(got[:, :2].astype(np.float64) @ u + got[:, 2], (src - lo) / np.diag(D), atol=1e-4)


@pytest.mark.parametrize("bad", [simbev.bev_aug_matrix(0.0, 0.0, False, False),
                                 np.full((3, 3), np.nan, dtype=np.float32),
                                 np.array([[1, 0, 0], [0, np.inf, 0], [0, 0, 1]], dtype=np.float32),
                                 np.array([[1, 2, 0], [2, 4, 0], [0, 0, 1]], dtype=np.float32)])
def test_label_index_matrix_refuses_singular_and_non_finite(bad):
    with pytest.raises(ValueError):
        simbev.label_index_matrix(bad, C.GC)


# ----------------------------------------------------------------------------- the restatement on pure symmetries
def _mats(theta, fx, fy, gc, n):
    m = simbev.label_index_matrix(simbev.bev_aug_matrix(theta, 1.0, fx, fy), gc)
    return np.repeat(m[None], n, axis=0)


# (a quarter turn maps a grid onto itself only when it is square)
@pytest.mark.parametrize("X,Y,name", [(X, Y, name) for X, Y in [(12, 12), (200, 200), (12, 20)] for name in C.SYMMETRIES
                                      if X == Y or name not in C.SQUARE_ONLY])
def test_restatement_is_exact_on_pure_symmetries(X, Y, name):
    (theta, fx, fy), fn = C.SYMMETRIES[name]
    bev = C.bev_maps(2, 8, X, Y, seed=X + Y)
    plain = C.plain_labels(bev, C.THREE)
    got = C.warp_labels(bev, C.THREE, _mats(theta, fx, fy, C.grid_conf(X, Y), 2))
    want = np.stack([np.stack([fn(plain[b, k]) for k in range(3)]) for b in range(2)])
    np.testing.assert_array_equal(got, want)
    assert 0.2 < plain.mean() < 0.8  # dense enough that a wrong gather cannot pass by chance


def test_restatement_identity_outside_and_nan():
    bev = C.bev_maps(2, 8, 13, 7, seed=4)
    eye = np.repeat(np.array([[[1, 0, 0], [0, 1, 0]]], dtype=np.float32), 2, axis=0)
    np.testing.assert_array_equal(C.warp_labels(bev, C.THREE, eye), C.plain_labels(bev, C.THREE))
    far = eye.copy()
    far[0, 0, 2] = 13.0          # every source row of sample 0 at or past X
    far[1, 1, 2] = np.nan        # a NaN position is outside
    np.testing.assert_array_equal(C.warp_labels(bev, C.THREE, far), np.zeros((2, 3, 13, 7), dtype=np.float32))


# ----------------------------------------------------------------------------- refusals
def test_abi_refuses_on_the_host_before_any_device_call():
    """lss_simbev_class_masks_warp checks its arguments before any HIP call: made-up addresses that are never
    dereferenced exercise the refusals without a GPU."""
    lib = _lib.load()
    bev, mats, out = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000))

    def call(bits=(0b1110,), bev=bev, n=1, C_=8, X=3, Y=5, K=None, mats=mats, out=out, groups=True):
        host = (ctypes.c_uint32 * len(bits))(*bits)
        return lib.lss_simbev_class_masks_warp(bev, n, C_, X, Y, ctypes.cast(host, ctypes.c_void_p) if groups else None,
                                               len(bits) if K is None else K, mats, out, None)

    bad = [call(mats=None), call(bev=None), call(out=None), call(groups=False), call(n=0), call(X=0), call(Y=-1),
           call(C_=0), call(C_=33), call(K=0), call(bits=(1,) * 9), call(bits=(0b1110, 0)), call(bits=(1 << 8,)),
           call(X=(1 << 23) + 1), call(Y=(1 << 23) + 1)]
    assert bad == [-1] * len(bad), bad


@pytest.mark.parametrize("kw", [dict(bev_scale_lim=(0.0, 1.0)), dict(bev_scale_lim=(1.1, 0.9)),
                                dict(bev_rot_lim=(10.0, -10.0)), dict(bev_rot_lim=(0.0, float("nan"))),
                                dict(bev_rot_lim=(0.0, 1.0, 2.0))])
def test_trainer_argument_errors_come_before_anything_is_built(kw, tmp_path):
    with pytest.raises(ValueError):
        trainer.train(str(tmp_path / "no_such_tree"), logdir=str(tmp_path / "log"), use_wandb=False, **kw)
    assert not (tmp_path / "log").exists()


def test_command_line_pairs():
    assert trainer.parse_pair("-22.5,22.5") == (-22.5, 22.5) and trainer.parse_pair("1, 1") == (1.0, 1.0)
    for bad in ("1", "1,2,3", ""):
        with pytest.raises(ValueError):
            trainer.parse_pair(bad, "--bev_rot_lim")
    assert simbev.bev_aug_enabled({"bev_flip": True}) and simbev.bev_aug_enabled({"bev_rot_lim": (0.0, 5.0)})
    assert not simbev.bev_aug_enabled({}) and not simbev.bev_aug_enabled(C.BEV_NEUTRAL)
