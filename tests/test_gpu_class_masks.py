"""lss_simbev_class_masks (simbev.class_masks): BEV labels by channel group,
out[b, k, i, j] = any(bev[b, c, X-1-i, j] > 0 for c in group k) -- the reference's merge + np.flipud per group --
against that numpy expression; [[1, 2, 3]] bit-equal to vehicle_masks; the entry's error codes; the (B, K, X, Y)
labels through finish_batch and BatchStager."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import _lib, simbev  # noqa: E402
from lss_carla_amd.staging import BatchStager  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.join(GOLDEN, "simbev_small")
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
GROUPS = {"vehicle": [[1, 2, 3]], "three": [[0], [1, 2, 3], [7]], "singletons": [[c] for c in range(8)]}


def _bev(n, C, X, Y, seed):
    rng = np.random.default_rng(seed)
    # sparse, and any value > 0 counts as set
    return (rng.random((n, C, X, Y)) < 0.2).astype(np.uint8) * rng.integers(1, 256, (n, C, X, Y)).astype(np.uint8)


def _numpy_masks(bev, groups):
    out = [np.flip(np.any(bev[:, g] > 0, axis=1), axis=1) for g in groups]  # flipud of each sample's (X, Y) map
    return np.stack(out, axis=1).astype(np.float32)


@pytest.mark.parametrize("groups", list(GROUPS))
@pytest.mark.parametrize("X,Y", [(1, 1), (3, 5), (200, 200)])
@pytest.mark.parametrize("C", [4, 8, 32])
def test_class_masks_match_numpy(C, X, Y, groups):
    gl = [[c for c in g if c < C] or [C - 1] for g in GROUPS[groups]]  # (a 4-channel npz has no channel 7)
    bev = _bev(2, C, X, Y, seed=C + X)
    got = simbev.class_masks(torch.from_numpy(bev).to(DEV), gl)
    assert got.shape == (2, len(gl), X, Y) and got.dtype == torch.float32 and got.is_contiguous()
    np.testing.assert_array_equal(got.cpu().numpy(), _numpy_masks(bev, gl))


def test_channel_31_of_a_32_class_map():
    bev = _bev(1, 32, 3, 5, seed=9)
    gl = [[31], [0, 31], [30]]
    got = simbev.class_masks(torch.from_numpy(bev).to(DEV), gl)
    np.testing.assert_array_equal(got.cpu().numpy(), _numpy_masks(bev, gl))


@pytest.mark.parametrize("X,Y", [(3, 5), (200, 200)])
def test_vehicle_group_is_vehicle_masks_bit_for_bit(X, Y):
    bev = torch.from_numpy(_bev(3, 8, X, Y, seed=X)).to(DEV)
    want = simbev.vehicle_masks(bev)
    assert torch.equal(simbev.class_masks(bev, [[1, 2, 3]]), want)
    assert torch.equal(simbev.class_masks(bev, None), want)  # the default: vehicle_masks itself
    out = torch.empty(3 * 2 * X * Y, device=DEV)
    got = simbev.class_masks(bev, [[1, 2, 3], [0]], out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out.view(3, 2, X, Y)[:, 0], want[:, 0])


def test_error_codes():
    lib = _lib.load()
    bev = torch.zeros(1, 8, 3, 5, device=DEV, dtype=torch.uint8)
    out = torch.full((1, 8, 3, 5), 7.0, device=DEV)
    st = _lib.stream_handle(DEV)

    def call(bits, C=8, K=None):
        host = (ctypes.c_uint32 * len(bits))(*bits)
        return lib.lss_simbev_class_masks(_lib.ptr(bev), 1, C, 3, 5, ctypes.cast(host, ctypes.c_void_p),
                                          len(bits) if K is None else K, _lib.ptr(out), st)

    assert call([0b1110, 0]) == -1          # an empty group
    assert call([0b1110, 1 << 8]) == -1     # channel 8 of an 8-channel map
    assert call([1] * 9) == -1              # more than 8 groups
    assert call([1], K=0) == -1
    assert call([1], C=33) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())         # refused before any launch
    assert call([0b1110, 1 << 7]) == 0
    with pytest.raises(ValueError):
        simbev.class_masks(bev, [[1], []])
    with pytest.raises(ValueError):
        simbev.class_masks(bev, [[32]])
    with pytest.raises(RuntimeError):
        simbev.class_masks(bev, [[8]])      # within 32 bits, outside this map: the entry's error code
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def raw_batches():
    tl, _ = simbev.compile_data("", ROOT, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV)
    np.random.seed(3)
    torch.manual_seed(3)
    return list(tl.loader)[:2]


def test_finish_batch_and_stager_labels(raw_batches):
    groups = [[0], [1, 2, 3], [4, 5]]
    for raw in raw_batches:
        want = simbev.finish_batch(raw, DAC["final_dim"], DEV, label_groups=groups)
        labels = want[6]
        assert labels.shape == (2, 3, 200, 200)
        np.testing.assert_array_equal(labels.cpu().numpy(), _numpy_masks(raw[-1].numpy(), groups))
        assert torch.equal(labels[:, 1:2], simbev.finish_batch(raw, DAC["final_dim"], DEV)[6])  # today's labels
        st = BatchStager(DAC["final_dim"], 2, 6, (DAC["H"], DAC["W"]), GC, DEV, label_groups=groups)
        assert st.binimgs.shape == (2, 3, 200, 200)
        st.stage(raw)
        assert st.commit() == 2
        torch.cuda.synchronize()
        assert torch.equal(st.binimgs, labels)
        for got, w in zip(st.inputs, want[:6]):
            assert torch.equal(got, w)
    assert labels[:, 1].sum().item() > 0


def test_compile_data_threads_label_groups(raw_batches):
    tl, vl = simbev.compile_data("", ROOT, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV,
                                 label_groups=[[1, 2, 3], [0]])
    batch = next(iter(vl))
    assert batch[6].shape == (2, 2, 200, 200) and tl.label_groups == [[1, 2, 3], [0]]
    with pytest.raises(ValueError):
        simbev.compile_data("", ROOT, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV,
                            label_groups=[[]])
