"""staging.BatchStager(photo=True): the photometric records of a raw batch reach the image kernel on the staging
stream. stage + commit equals simbev.finish_batch with the same records bit for bit; neutral records equal a stager
without the option; a partial batch leaves the rest of the static tensors alone; nothing but ``imgs`` depends on the
option. Tiny synthetic raw batches (no dataset, no decode)."""
import numpy as np
import pytest
import torch

import photo_cases as C

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import simbev, synthetic as syn  # noqa: E402
from lss_carla_amd.staging import BatchStager  # noqa: E402

DEV = torch.device("cuda:0")
GC = {"xbound": [-8.0, 8.0, 0.5], "ybound": [-8.0, 8.0, 0.5], "zbound": [-10.0, 10.0, 20.0], "dbound": [4.0, 45.0, 1.0]}
B, N, SRC_HW, FD, X = 2, 3, (24, 40), (13, 21), 32
RIG = ("rots", "trans", "intrins", "post_rots", "post_trans")
NAMES = ("imgs",) + RIG + ("binimgs",)


def _raw(seed, records, bev_aug=False, b=B):
    """A collated raw batch as SegmentationData's samples collate: images, rig, aug, rotation, [records,]
    [index matrices,] BEV maps."""
    rng = np.random.default_rng(seed)
    imgs = torch.from_numpy(rng.integers(0, 256, (b, N) + SRC_HW + (3,), dtype=np.uint8))
    rig = syn.make_rig(b, N, FD, seed=seed)
    aug = torch.tensor([[32, 19, 5 + i, 3, 5 + i + FD[1], 3 + FD[0], i % 2] for i in range(b)], dtype=torch.int64)
    rot = torch.tensor([5.4, 0.0][:b], dtype=torch.float64)
    bev = torch.from_numpy((rng.random((b, 8, X, X)) < 0.1).astype(np.uint8))
    tail = ()
    if records is not None:
        tail += (torch.from_numpy(np.stack(records).reshape(b, N, 16)),)
    if bev_aug:
        mats = np.stack([simbev.label_index_matrix(simbev.bev_aug_matrix(10.0 * (i + 1), 1.05, bool(i), False), GC)
                         for i in range(b)])
        tail += (torch.from_numpy(mats),)
    return (imgs,) + tuple(rig[k] for k in RIG) + (aug, rot) + tail + (bev,)


def _records(b=B, neutral=False):
    if neutral:
        return [C.record() for _ in range(b * N)]
    return [C.record(10.0 * i - 20.0, 0.8 + 0.1 * i, 1.3 - 0.1 * i, 6.0 * i - 9.0, 1.5 * i, 100 + i, 7 * i)
            for i in range(b * N)]


def _stager(**kw):
    return BatchStager(FD, B, N, SRC_HW, GC, DEV, **kw)


def _static(st):
    return dict(zip(NAMES, st.inputs + (st.binimgs,)))


@pytest.mark.parametrize("bev_aug, mask", [(False, None), (True, "fov")])
def test_stage_commit_is_finish_batch_with_the_same_records(bev_aug, mask):
    kw = {"bev_aug": True} if bev_aug else {}
    st = _stager(photo=True, valid_mask=mask, **kw)
    plain = _stager(valid_mask=mask, **kw)
    for seed in (0, 1):
        raw = _raw(seed, _records(), bev_aug)
        fin = simbev.finish_batch(raw, FD, DEV, bev_aug=bev_aug, photo=True,
                                  valid_mask_conf=None if mask is None else (mask, GC, (0.0,)))
        st.stage(raw)
        assert st.commit() == B
        bare = raw[:8] + raw[9:]  # the same batch without its records
        plain.stage(bare)
        plain.commit()
        torch.cuda.synchronize()
        got, other = _static(st), _static(plain)
        for k, want in zip(NAMES, fin):
            assert got[k].shape == want.shape and torch.equal(got[k], want), k
        if mask is not None:
            assert torch.equal(st.valid, fin[-1]) and torch.equal(st.valid, plain.valid)
        for k in NAMES[1:]:  # rig and labels do not depend on the option
            assert torch.equal(got[k], other[k]), k
        assert not torch.equal(got["imgs"], other["imgs"])
        assert torch.equal(st.hinv.pinv, plain.hinv.pinv) and torch.equal(st.hinv.kinv, plain.hinv.kinv)
        # and the images are the restated chain's: per image, the records reached the right image
        want0 = simbev.augment_images(raw[0].reshape(B * N, *SRC_HW, 3).to(DEV),
                                      [{"resize_dims": (32, 19), "crop": tuple(raw[6][i // N, 2:6].tolist()),
                                        "flip": bool(raw[6][i // N, 6]), "rotate": float(raw[7][i // N])}
                                       for i in range(B * N)], FD, photo=raw[8].reshape(B * N, 16))
        assert torch.equal(got["imgs"].reshape(B * N, 3, *FD), want0)


def test_neutral_records_equal_a_stager_without_the_option():
    raw = _raw(2, _records(neutral=True))
    st, plain = _stager(photo=True), _stager()
    st.stage(raw)
    st.commit()
    plain.stage(raw[:8] + raw[9:])
    plain.commit()
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(_static(st)[k], _static(plain)[k]), k
    assert torch.equal(st.imgs, simbev.finish_batch(raw[:8] + raw[9:], FD, DEV)[0])


def test_partial_batch_leaves_the_rest():
    st = _stager(photo=True)
    st.stage(_raw(3, _records()))
    st.commit()
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in _static(st).items()}
    one = _raw(4, _records(b=1), b=1)
    want = dict(zip(NAMES, simbev.finish_batch(one, FD, DEV, photo=True)))
    st.stage(one)
    assert st.commit() == 1
    torch.cuda.synchronize()
    assert st.n_valid.item() == 1
    for k, got in _static(st).items():
        assert torch.equal(got[:1], want[k]), k
        assert torch.equal(got[1:], before[k][1:]), k


def test_a_batch_without_records_is_refused():
    st = _stager(photo=True)
    with pytest.raises(RuntimeError, match="photo records"):
        st.stage(_raw(5, None))
    with pytest.raises(RuntimeError, match="photo records"):
        st.stage(_raw(5, _records(), bev_aug=True))  # (the element there is the index matrices)
