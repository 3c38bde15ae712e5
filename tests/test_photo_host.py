"""Photometric augmentation, host side (no GPU): photo_matrix's algebra, the Philox and noise restatements of
tests/photo_cases.py, the draws (count, order, what the option leaves alone), the record layout against the header,
and the command-line parsing."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import photo_cases as C
from conftest import GOLDEN, REPO
from lss_carla_amd import _lib, simbev

ROOT = os.path.join(GOLDEN, "simbev_small")
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (0.6, 0.9), "final_dim": (32, 88), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
BEV = {"bev_rot_lim": (-20.0, 20.0), "bev_scale_lim": (0.9, 1.1), "bev_flip": True}
PHOTO = {"photo_brightness_lim": (-32.0, 32.0), "photo_contrast_lim": (0.5, 1.5), "photo_saturation_lim": (0.5, 1.5),
         "photo_hue_lim": (-18.0, 18.0), "photo_noise_lim": (0.0, 8.0)}


# ----------------------------------------------------------------------------- photo_matrix
def test_neutral_record_is_exactly_identity():
    M, t = simbev.photo_matrix(0.0, 1.0, 1.0, 0.0)
    assert M.dtype == np.float32 and t.dtype == np.float32
    assert np.array_equal(M, np.eye(3, dtype=np.float32)) and np.array_equal(t, np.zeros(3, dtype=np.float32))
    rec = simbev.photo_record()
    assert rec.shape == (16,) and rec.dtype == np.float32
    assert np.array_equal(rec.view(np.uint32), C.record().view(np.uint32)) and not rec[12:].any()


def test_saturation_zero_makes_every_row_luma():
    M, t = simbev.photo_matrix(saturation=0.0)
    want = np.array([0.299, 0.587, 0.114], dtype=np.float32)
    for r in range(3):
        assert np.array_equal(M[r], want)
    assert not t.any()


def test_hue_full_turn_is_the_identity():
    M, t = simbev.photo_matrix(hue_deg=360.0)
    assert np.abs(M.astype(np.float64) - np.eye(3)).max() < 1e-6 and np.abs(t).max() < 1e-6
    M90, _ = simbev.photo_matrix(hue_deg=90.0)
    assert np.abs(M90.astype(np.float64) - np.eye(3)).max() > 0.1  # (a quarter turn is not)
    np.testing.assert_allclose(M90.astype(np.float64) @ np.ones(3), np.ones(3), atol=1e-5)  # greys keep their grey


@pytest.mark.parametrize("alpha", [0.5, 0.8, 1.5])
def test_contrast_leaves_mid_grey_fixed(alpha):
    M, t = simbev.photo_matrix(contrast=alpha)
    v = M.astype(np.float64) @ np.full(3, 127.5) + t.astype(np.float64)
    np.testing.assert_allclose(v, 127.5, atol=1e-4)


@pytest.mark.parametrize("args", [(20.0, 1.0, 1.0, 0.0), (-300.0, 1.0, 1.0, 0.0), (12.5, 0.7, 1.0, 0.0),
                                  (0.0, 1.0, 0.4, 0.0), (0.0, 1.0, 1.0, -18.0), (-31.0, 1.4, 0.6, 17.0)])
def test_photo_matrix_equals_the_restatement(args):
    M, t = simbev.photo_matrix(*args)
    Mw, tw = C.photo_matrix(*args)
    assert np.array_equal(M, Mw) and np.array_equal(t, tw)


def test_order_is_brightness_then_contrast():
    _, t = simbev.photo_matrix(brightness=10.0, contrast=2.0)
    np.testing.assert_allclose(t, 2.0 * (10.0 - 127.5) + 127.5)  # (contrast acts on the shifted offset)


def test_photo_matrix_is_exported_and_refuses_non_finite():
    import lss_carla_amd as L
    assert L.photo_matrix is simbev.photo_matrix
    with pytest.raises(ValueError):
        simbev.photo_matrix(brightness=float("nan"))


# ----------------------------------------------------------------------------- Philox and the noise
def test_philox_known_answer():
    w = C.philox4x32_10((0, 0), np.zeros((1, 4), dtype=np.uint64))[0]
    assert [f"{int(x):08x}" for x in w] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    # Random123's second published vector: all-ones counter and key
    w = C.philox4x32_10((0xFFFFFFFF, 0xFFFFFFFF), np.full((1, 4), 0xFFFFFFFF, dtype=np.uint64))[0]
    assert [f"{int(x):08x}" for x in w] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]


def test_noise_restatement_statistics():
    z = C.noise_z((12345, 678), 2, 64 * 64)
    assert z.shape == (64 * 64, 3) and z.dtype == np.float32
    n = z.size
    mean, std, peak = float(z.mean(dtype=np.float64)), float(z.std(dtype=np.float64)), float(np.abs(z).max())
    print("noise z: mean", mean, "std", std, "max |z|", peak)
    assert abs(mean) < 5.0 / math.sqrt(n) and 5.0 / math.sqrt(n) < 0.0452
    assert abs(std - 1.0) < 0.04
    assert peak <= 3.46
    assert float(C.INV_STD) == float(np.float32(0.006765875))
    assert not np.array_equal(z, C.noise_z((12345, 678), 1, 64 * 64))  # the image index is in the counter
    assert not np.array_equal(z, C.noise_z((12346, 678), 2, 64 * 64))


# ----------------------------------------------------------------------------- the draws
def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _dataset(conf, train):
    return simbev.SegmentationData(ROOT, is_train=train, data_aug_conf=conf, grid_conf=GC)


@pytest.mark.parametrize("bev", [False, True])
def test_without_photo_keys_the_sample_draws_what_it_drew(bev):
    conf = {**DAC, **(BEV if bev else {})}
    ds = _dataset(conf, True)
    assert ds.photo is False and simbev.photo_enabled(conf) is False
    np.random.seed(11)
    raw, index_mat, photo = ds._image_data(ds.samples[0], list(range(6)))
    got = np.random.get_state()
    assert photo is None and (index_mat is not None) == bev
    np.random.seed(11)
    simbev.draw_augmentation(conf, True)
    if bev:
        simbev.draw_bev_augmentation(conf, True)
    assert _state_equal(got, np.random.get_state())
    np.random.seed(11)
    sample = ds[0]
    assert len(sample) == (10 if bev else 9)  # 8 image-side elements, [index matrix,] the BEV map


@pytest.mark.parametrize("per_camera, units", [(1, 6), (0, 1)])
def test_draw_count_is_fixed_whatever_the_coins_say(per_camera, units):
    states = []
    for prob in (0.0, 0.5, 1.0):
        conf = {**DAC, **PHOTO, "photo_prob": prob, "photo_per_camera": per_camera}
        ds = _dataset(conf, True)
        np.random.seed(5)
        _, _, photo = ds._image_data(ds.samples[0], list(range(6)))
        states.append(np.random.get_state())
        assert photo.shape == (6, 16) and photo.dtype == torch.float32
        if prob == 0.0:  # every coin fails: the colour part is neutral, the noise is still drawn
            assert torch.equal(photo[:, :12], torch.from_numpy(C.record()[:12]).expand(6, 12))
            assert (photo[:, 12] >= 0).all() and (photo[:, 12] <= 8.0).all() and photo[:, 12].max() > 0
        if not per_camera:
            assert all(torch.equal(photo[0].view(torch.int32), photo[i].view(torch.int32)) for i in range(6))
        else:
            assert len({tuple(r.tolist()) for r in photo.view(torch.int32)[:, 13:15]}) == 6  # a key per camera
    assert _state_equal(states[0], states[1]) and _state_equal(states[1], states[2])
    # and the count is the stated one: after the sample's own draws, per unit 4 x (coin, value), sigma, two words
    conf = {**DAC, **PHOTO, "photo_per_camera": per_camera}
    np.random.seed(5)
    simbev.draw_augmentation(conf, True)
    for _ in range(units):
        for _ in range(9):
            np.random.uniform(0.0, 1.0)
        np.random.randint(0, 1 << 32, dtype=np.uint32)
        np.random.randint(0, 1 << 32, dtype=np.uint32)
    assert _state_equal(states[1], np.random.get_state())


def test_draw_order_and_values():
    conf = {**DAC, **PHOTO, "photo_prob": 1.0}
    np.random.seed(9)
    got = simbev.draw_photo_augmentation(conf, True)
    np.random.seed(9)
    want = []
    for name in ("photo_brightness_lim", "photo_contrast_lim", "photo_saturation_lim", "photo_hue_lim"):
        assert np.random.uniform(0.0, 1.0) < 1.0
        want.append(float(np.random.uniform(*PHOTO[name])))
    want.append(float(np.random.uniform(*PHOTO["photo_noise_lim"])))
    want += [int(np.random.randint(0, 1 << 32, dtype=np.uint32)) for _ in range(2)]
    assert list(got) == want


def test_validation_is_neutral_and_draws_nothing():
    conf = {**DAC, **PHOTO}
    ds = _dataset(conf, False)
    assert ds.photo is True
    np.random.seed(3)
    before = np.random.get_state()
    sample = ds[0]
    assert _state_equal(before, np.random.get_state())
    assert len(sample) == 10 and sample[8].shape == (6, 16)  # the records sit directly before the BEV map
    assert torch.equal(sample[8].view(torch.int32), torch.from_numpy(np.stack([C.record()] * 6)).view(torch.int32))
    assert simbev.draw_photo_augmentation(conf, False) == simbev.PHOTO_NEUTRAL


def test_records_sit_before_the_index_matrix_with_bev_aug():
    ds = _dataset({**DAC, **BEV, **PHOTO}, True)
    np.random.seed(2)
    sample = ds[0]
    assert len(sample) == 11 and sample[8].shape == (6, 16) and sample[9].shape == (2, 3) and sample[10].dim() == 3
    tl, vl = simbev.compile_data("", ROOT, {**DAC, **BEV, **PHOTO}, GC, bsz=2, nworkers=0,
                                 parser_name="segmentationdata", device="cpu")
    assert tl.photo and vl.photo and tl.bev_aug and vl.bev_aug
    tl, vl = simbev.compile_data("", ROOT, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device="cpu")
    assert not tl.photo and not vl.photo


def test_photo_fixed_is_validations_only():
    fixed = {"brightness": -40.0, "contrast": 0.8, "noise": 8.0, "seed": (7 << 32) | 0xFFFFFFFE}
    conf = {**DAC, "photo_fixed": fixed}
    assert simbev.photo_enabled(conf) and not simbev.photo_draws(conf)
    val = _dataset(conf, False)[0][8]
    want = np.stack([C.record(-40.0, 0.8, 1.0, 0.0, 8.0, (0xFFFFFFFE + i) & 0xFFFFFFFF, 7) for i in range(6)])
    assert torch.equal(val.view(torch.int32), torch.from_numpy(want).view(torch.int32))
    train_ds = _dataset(conf, True)
    np.random.seed(4)
    rec = train_ds[0][8]
    got = np.random.get_state()
    assert torch.equal(rec.view(torch.int32), torch.from_numpy(np.stack([C.record()] * 6)).view(torch.int32))
    np.random.seed(4)
    simbev.draw_augmentation(conf, True)
    assert _state_equal(got, np.random.get_state())  # training ignores it, and draws nothing for it
    with pytest.raises(ValueError):
        simbev.photo_enabled({**DAC, "photo_fixed": {"gamma": 2.0}})
    with pytest.raises(ValueError):
        simbev.photo_enabled({**DAC, "photo_fixed": {"noise": -1.0}})


@pytest.mark.parametrize("bad", [{"photo_brightness_lim": (5.0, -5.0)}, {"photo_contrast_lim": (-0.5, 1.0)},
                                 {"photo_noise_lim": (0.0, float("inf"))}, {"photo_hue_lim": (1.0,)},
                                 {"photo_saturation_lim": (0.5, 1.5), "photo_prob": 1.5}])
def test_a_bad_limit_raises_at_construction(bad):
    with pytest.raises(ValueError):
        simbev.photo_enabled({**DAC, **bad})
    with pytest.raises(ValueError):
        _dataset({**DAC, **bad}, True)
    with pytest.raises(ValueError):
        simbev.compile_data("", ROOT, {**DAC, **bad}, GC, bsz=2, nworkers=0, parser_name="segmentationdata",
                            device="cpu")


# ----------------------------------------------------------------------------- the record's layout
def test_ctypes_record_matches_the_header():
    P = _lib.ImgPhoto
    assert ctypes.sizeof(P) == 64 == 4 * simbev.PHOTO_WORDS
    assert (P.m.offset, P.t.offset, P.noise.offset, P.seed.offset, P.pad.offset) == (0, 36, 48, 52, 60)
    text = open(os.path.join(REPO, "include", "lss_simbev.h")).read()
    body = re.search(r"typedef struct lss_img_photo \{(.*?)\} lss_img_photo_t;", text, re.S).group(1)
    fields = re.findall(r"^\s*(float|uint32_t)\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    assert [(t, n, int(c or 1)) for t, n, c in fields] == [("float", "m", 9), ("float", "t", 3), ("float", "noise", 1),
                                                            ("uint32_t", "seed", 2), ("uint32_t", "pad", 1)]
    assert [n for n, _ in P._fields_] == [n for _, n, _ in fields]
    rec = simbev.photo_record(1.0, 1.1, 0.9, 3.0, 2.5, 0xDEADBEEF, 0x7FC00001)  # (a NaN's bits survive as a seed)
    p = P.from_buffer_copy(rec.tobytes())
    assert p.noise == 2.5 and list(p.seed) == [0xDEADBEEF, 0x7FC00001] and p.pad == 0
    assert _lib.ABI_VERSION >= 36  # the ABI that added the record; later ABIs keep it
    assert re.search(r"#define LSS_ABI_VERSION %d\b" % _lib.ABI_VERSION,
                     open(os.path.join(REPO, "include", "lss_hip.h")).read())


# ----------------------------------------------------------------------------- command lines
def test_trainer_cli_parses_the_photo_flags(monkeypatch):
    from lss_carla_amd import trainer
    seen, real_train = {}, trainer.train
    monkeypatch.setattr(trainer, "train", lambda **kw: seen.update(kw))
    trainer.main(["--dataroot", "/data", "--photo_brightness", "32", "--photo_contrast", "0.5,1.5",
                  "--photo_saturation", "0.6,1.4", "--photo_hue", "18", "--photo_noise", "0,8", "--photo_prob", "0.25",
                  "--photo_per_camera", "0"])
    assert (seen["photo_brightness"], seen["photo_contrast"], seen["photo_saturation"], seen["photo_hue"],
            seen["photo_noise"], seen["photo_prob"], seen["photo_per_camera"]) == \
        (32.0, (0.5, 1.5), (0.6, 1.4), 18.0, (0.0, 8.0), 0.25, False)
    trainer.main(["--dataroot", "/data"])
    assert (seen["photo_brightness"], seen["photo_contrast"], seen["photo_noise"], seen["photo_per_camera"]) == \
        (0.0, (1.0, 1.0), (0.0, 0.0), True)
    conf = trainer.photo_conf(32, (0.5, 1.5), (0.6, 1.4), 18, (0, 8), 0.25, False)
    assert conf["photo_brightness_lim"] == (-32.0, 32.0) and conf["photo_hue_lim"] == (-18.0, 18.0)
    assert conf["photo_per_camera"] == 0 and simbev.photo_draws(conf)
    assert not simbev.photo_draws(trainer.photo_conf())
    for bad in (dict(brightness=-1.0), dict(contrast=(1.5, 0.5)), dict(noise=(-1.0, 2.0)), dict(prob=2.0)):
        with pytest.raises(ValueError):
            trainer.photo_conf(**bad)
    with pytest.raises(ValueError):  # before anything is looked for or built (no GPU is asked for first)
        real_train("/nowhere", gpuid=-1, photo_contrast=(2.0, 1.0))


def test_predict_cli_parses_photo():
    from lss_carla_amd import predict as P
    a = P.parser().parse_args(["--modelf", "m", "--dataroot", "d", "--out", "o", "--photo",
                               "brightness=-40,contrast=0.8,noise=8"])
    assert P.parse_photo(a.photo) == {"brightness": -40.0, "contrast": 0.8, "noise": 8.0}
    assert P.parse_photo("seed=12, hue=3") == {"seed": 12, "hue": 3.0}
    assert P.parse_photo(None) is None and P.parse_photo("") is None
    assert P.parser().parse_args(["--modelf", "m", "--dataroot", "d", "--out", "o"]).photo is None
    for bad in ("gamma=2", "brightness", "brightness=abc", "noise=-3", "contrast=1,contrast=2"):
        with pytest.raises(ValueError):
            P.parse_photo(bad)
