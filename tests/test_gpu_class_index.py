"""lss_simbev_class_index (simbev.class_index) on the MI355X: the exclusive class map of K label groups, bit for bit
against numpy (exclusive_cases.class_index_ref / paint) and against the map derived from lss_simbev_class_masks'
and lss_simbev_class_masks_warp's planes. Shapes (2, 8, 5, 7) and (1, 8, 16, 24) -- odd sizes in one block, and two
blocks; K = 1, 3 and 7 with overlapping groups, so that the paint order decides cells."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import bev_aug_cases as BC  # noqa: E402
import exclusive_cases as E  # noqa: E402
from lss_carla_amd import _lib, simbev  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(2, 8, 5, 7), (1, 8, 16, 24)]
GROUPS = {1: [[1, 2, 3]], 3: [[0], [1, 2, 3], [6, 7, 0]],
          7: [[0], [1], [2, 1], [3], [4, 0], [5, 6], [7, 3]]}
EYE = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32)


def _index(theta, scale, gc):
    return simbev.label_index_matrix(simbev.bev_aug_matrix(theta, scale, False, False), gc)


@pytest.mark.parametrize("K", list(GROUPS))
@pytest.mark.parametrize("shape", SHAPES)
def test_unwarped_map_vs_numpy_and_vs_class_masks(shape, K):
    n, C, X, Y = shape
    groups = GROUPS[K]
    bev = BC.bev_maps(n, C, X, Y, seed=X + K)
    bev_d = torch.from_numpy(bev).to(DEV)
    got = simbev.class_index(bev_d, groups)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, X, Y)
    want = E.class_index_ref(bev, groups)
    assert np.array_equal(got.cpu().numpy(), want)
    assert K == 1 or (want == K).any() and ((want > 0) & (want < K)).any() and (want == 0).any()
    planes = simbev.class_masks(bev_d, groups).cpu().numpy()
    assert np.array_equal(got.cpu().numpy(), E.paint(planes))
    if K > 1:  # a later group wins: a cell in both the first and the last group is the last group's
        both = (planes[:, 0] != 0) & (planes[:, K - 1] != 0)
        assert both.any() and (got.cpu().numpy()[both] == K).all()
    assert np.array_equal(simbev.class_index_from_masks(planes), got.cpu().numpy())
    # out=: the caller's buffer, the identity warp: the same bytes
    buf = torch.full((n, X, Y), 77, device=DEV, dtype=torch.uint8)
    assert simbev.class_index(bev_d, groups, out=buf) is buf and torch.equal(buf, got)
    eye = np.stack([EYE] * n)
    assert torch.equal(simbev.class_index(bev_d, groups, index_mats=eye), got)
    assert torch.equal(simbev.class_index(bev_d, groups, index_mats=torch.from_numpy(eye).to(DEV)), got)


@pytest.mark.parametrize("K", list(GROUPS))
@pytest.mark.parametrize("shape", SHAPES)
def test_warped_map_vs_class_masks_warp(shape, K):
    n, C, X, Y = shape
    groups = GROUPS[K]
    bev = BC.bev_maps(n, C, X, Y, seed=3 * X + K)
    bev_d = torch.from_numpy(bev).to(DEV)
    gc = BC.grid_conf(X, Y)
    mats = np.stack([_index(33.0 + 10 * b, 0.9, gc) for b in range(n)])  # corners leave the grid
    got = simbev.class_index(bev_d, groups, index_mats=mats).cpu().numpy()
    planes = simbev.class_masks(bev_d, groups, index_mats=mats).cpu().numpy()
    assert np.array_equal(got, E.paint(planes))
    assert np.array_equal(got, E.paint(BC.warp_labels(bev, groups, mats)))
    # every source cell set: a 0 is then exactly a cell whose source is outside the grid
    full = torch.ones(n, C, X, Y, device=DEV, dtype=torch.uint8)
    outside = simbev.class_index(full, groups, index_mats=mats).cpu().numpy() == 0
    grid = simbev.valid_mask(None, None, gc, (8, 8), index_mats=mats, mode="grid",
                             out=torch.empty(n, X, Y, device=DEV, dtype=torch.uint8)).cpu().numpy()
    assert outside.any() and not outside.all() and np.array_equal(outside, grid == 0)
    assert outside[:, 0, 0].all() and (got[outside] == 0).all()


def test_rot90_is_rot90_of_the_unwarped_map():
    X = 16
    groups = GROUPS[3]
    bev_d = torch.from_numpy(BC.bev_maps(2, 8, X, X, seed=5)).to(DEV)
    plain = simbev.class_index(bev_d, groups)
    mats = np.stack([simbev.label_index_matrix(simbev.bev_aug_matrix(90.0, 1.0, False, False), BC.grid_conf(X, X))] * 2)
    got = simbev.class_index(bev_d, groups, index_mats=mats)
    assert torch.equal(got, torch.rot90(plain, 1, (1, 2)))


def test_entry_refuses_bad_arguments():
    lib = _lib.load()
    n, C, X, Y = 1, 8, 3, 5
    bev = torch.zeros(n, C, X, Y, device=DEV, dtype=torch.uint8)
    out = torch.zeros(n, X, Y, device=DEV, dtype=torch.uint8)
    mats = torch.from_numpy(np.stack([EYE] * 2)).to(DEV)
    st = _lib.stream_handle(DEV)

    def call(bits=(1, 14), bp=_lib.ptr(bev), op=_lib.ptr(out), nn=n, c=C, x=X, y=Y, k=None, mp=None, groups=True):
        host = (ctypes.c_uint32 * max(len(bits), 1))(*bits)
        return lib.lss_simbev_class_index(bp, nn, c, x, y, ctypes.cast(host, ctypes.c_void_p) if groups else None,
                                          len(bits) if k is None else k, mp, op, st)

    assert call() == 0 and call(mp=_lib.ptr(mats)) == 0 and call(bits=(1,) * 7) == 0
    for bad in (dict(bp=None), dict(op=None), dict(groups=False), dict(nn=0), dict(c=0), dict(c=33), dict(x=0),
                dict(y=0), dict(k=0), dict(bits=(1,) * 8), dict(bits=(1, 0)), dict(bits=(1, 1 << 8)),
                dict(x=(1 << 23) + 1), dict(y=(1 << 23) + 1),
                dict(mp=ctypes.c_void_p(mats.data_ptr() + 2))):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        simbev.class_index(bev, [[0]] * 8)
    with pytest.raises(RuntimeError):
        simbev.class_index(bev.cpu(), [[0]])
    with pytest.raises(RuntimeError):
        simbev.class_index(bev, [[0]], out=torch.zeros(n, X, Y, device=DEV))  # an fp32 out
    with pytest.raises(RuntimeError):
        simbev.class_index(bev, [[0]], index_mats=np.stack([EYE] * 2))  # one matrix per sample
