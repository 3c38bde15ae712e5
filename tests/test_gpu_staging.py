"""staging.BatchStager: a raw SimBEV batch into a captured step's static tensors. stage + commit leaves the
static tensors bit-identical to simbev.finish_batch on the same raw batch and the staged inverses
bit-identical to torch.inverse of the host rig; staging two batches ahead never synchronises the host; a
partial batch fills its samples only and sets n_valid."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import simbev  # noqa: E402
from lss_carla_amd.staging import BatchStager  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.join(GOLDEN, "simbev_small")
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
NAMES = ("imgs", "rots", "trans", "intrins", "post_rots", "post_trans", "binimgs")


class _SyncErrors:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")


@pytest.fixture(scope="module")
def raw_batches():
    """(train batches, val batches): the loaders' raw batches, drawn once from a fixed seed."""
    tl, vl = simbev.compile_data("", ROOT, DAC, GC, bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV)
    np.random.seed(3)
    torch.manual_seed(3)
    return list(tl.loader), list(vl.loader)


def _stager(B=2):
    return BatchStager(DAC["final_dim"], B, 6, (DAC["H"], DAC["W"]), GC, DEV)


def _static(st):
    return dict(zip(NAMES, st.inputs + (st.binimgs,)))


def test_stage_commit_is_finish_batch_bit_for_bit(raw_batches):
    train, val = raw_batches
    assert len(train) == 4 and len(val) == 1
    st = _stager()
    for raw in train + val:
        want = dict(zip(NAMES, simbev.finish_batch(raw, DAC["final_dim"], DEV)))
        st.stage(raw)
        assert st.commit() == 2
        torch.cuda.synchronize()
        for k, got in _static(st).items():
            assert got.shape == want[k].shape and got.dtype == want[k].dtype, k
            assert torch.equal(got, want[k]), k
        assert st.n_valid.item() == 2
        assert torch.equal(st.hinv.pinv.cpu(), torch.inverse(raw[4]).reshape(12, 9))
        assert torch.equal(st.hinv.kinv.cpu(), torch.inverse(raw[3]).reshape(12, 9))
    assert st.binimgs.sum().item() > 0 and not torch.equal(*[simbev.finish_batch(r, DAC["final_dim"], DEV)[0]
                                                             for r in train[:2]])


def test_staging_two_batches_ahead_never_synchronises(raw_batches):
    train, _ = raw_batches
    st = _stager()
    st.stage(train[2])  # (first use: the resize tables of these sizes are uploaded)
    st.commit()
    st2 = _stager()
    with _SyncErrors():
        st2.stage(train[0])
        st2.stage(train[1])
        assert st2.pending() == 2
        st2.commit()
        first = [t.clone() for t in st2.inputs + (st2.binimgs,)]
        st2.commit()
    torch.cuda.synchronize()
    for raw, got in ((train[0], first), (train[1], list(st2.inputs + (st2.binimgs,)))):
        for g, w in zip(got, simbev.finish_batch(raw, DAC["final_dim"], DEV)):
            assert torch.equal(g, w)
    with pytest.raises(RuntimeError):
        st2.commit()  # nothing staged
    st2.stage(train[0])
    st2.stage(train[1])
    with pytest.raises(RuntimeError):
        st2.stage(train[2])  # both slots hold uncommitted batches


def test_partial_batch_sets_n_valid_and_leaves_the_rest(raw_batches):
    train, _ = raw_batches
    st = _stager()
    st.stage(train[0])
    st.commit()
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in _static(st).items()}
    pinv, kinv = st.hinv.pinv.clone(), st.hinv.kinv.clone()
    one = tuple(t[:1] for t in train[1])
    want = dict(zip(NAMES, simbev.finish_batch(one, DAC["final_dim"], DEV)))
    st.stage(one)
    assert st.commit() == 1
    torch.cuda.synchronize()
    assert st.n_valid.item() == 1
    for k, got in _static(st).items():
        assert torch.equal(got[:1], want[k]), k
        assert torch.equal(got[1:], before[k][1:]), k
    assert torch.equal(st.hinv.pinv[:6].cpu(), torch.inverse(one[4]).reshape(6, 9))
    assert torch.equal(st.hinv.kinv[:6].cpu(), torch.inverse(one[3]).reshape(6, 9))
    assert torch.equal(st.hinv.pinv[6:], pinv[6:]) and torch.equal(st.hinv.kinv[6:], kinv[6:])
