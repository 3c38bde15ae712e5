"""The BEV-space augmentation on the MI355X: lss_simbev_class_masks_warp (simbev.class_masks, index_mats=) bit for
bit against the numpy restatement of tests/bev_aug_cases.py; the identity and the grid's pure symmetries against the
un-warped labels; the direction of the map and its axes from marked ego points; the geometry of the composed rig;
the eager and the staged loader paths; one seeded trainer run, twice."""
import json
import math
import os

import numpy as np
import pytest
import torch

import bev_aug_cases as C
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from oracle import lss_ref as ref  # noqa: E402
import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import simbev, synthetic as syn, trainer  # noqa: E402
from lss_carla_amd.staging import BatchStager  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.join(GOLDEN, "simbev_small")
KW = dict(H=56, W=120, resize_lim=(1.6, 1.8), final_dim=(64, 192), rot_lim=(-5.4, 5.4), rand_flip=True,
          bot_pct_lim=(0.0, 0.22), bsz=2, nworkers=0, use_wandb=False, miopen_find=False)
EYE = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32)


def _index(theta, scale, fx, fy, gc):
    return simbev.label_index_matrix(simbev.bev_aug_matrix(theta, scale, fx, fy), gc)


def _drawn(rng, gc):
    """One matrix as training draws it: theta in [-22.5, 22.5], s in [0.9, 1.1], two coins."""
    return _index(rng.uniform(-22.5, 22.5), rng.uniform(0.9, 1.1), bool(rng.integers(2)), bool(rng.integers(2)), gc)


def _matrices(kind, n, X, Y, seed):
    gc = C.grid_conf(X, Y)
    rng = np.random.default_rng(seed)
    mats = [_drawn(rng, gc) for _ in range(n)]
    if kind == "special":  # a half turn, and a scale that leaves most of the output outside the grid
        mats[0] = _index(180.0, rng.uniform(0.9, 1.1), False, False, gc)
        mats[1] = _index(rng.uniform(-22.5, 22.5), 0.5, bool(rng.integers(2)), False, gc)
    return np.stack(mats)


def _warp(bev, groups, mats, **kw):
    """class_masks under `mats` into a NaN-filled buffer: every element must come back written."""
    n, _, X, Y = bev.shape
    K = 1 if groups is None else len(groups)
    out = torch.full((n, K, X, Y), float("nan"), device=DEV)
    got = simbev.class_masks(torch.from_numpy(bev).to(DEV), groups, out=out, index_mats=mats, **kw)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy()


# ----------------------------------------------------------------------------- the kernel against the restatement
# 12 x 20 and 13 x 7: n * X * Y is no multiple of the block (256 threads) and a block straddles two samples
@pytest.mark.parametrize("kind", ["drawn", "special"])
@pytest.mark.parametrize("groups", [None, C.THREE], ids=["vehicle", "three"])
@pytest.mark.parametrize("n,X,Y", [(3, 12, 20), (2, 13, 7), (2, 200, 200)])
def test_kernel_matches_the_restatement_bit_for_bit(n, X, Y, groups, kind):
    bev = C.bev_maps(n, 8, X, Y, seed=n + X)
    mats = _matrices(kind, n, X, Y, seed=X + Y)
    assert len({m.tobytes() for m in mats}) == n  # a different matrix per sample
    want = C.warp_labels(bev, C.VEHICLE if groups is None else groups, mats)
    got = _warp(bev, groups, mats)
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got, want)
    assert 0.0 < want.mean() < 0.9
    if kind == "special":
        assert (want[1] == 0).mean() > 0.7  # scale 0.5: three quarters of the output is outside the grid
    # the matrices from the device give the same labels
    got_d = _warp(bev, groups, torch.from_numpy(mats).to(DEV))
    np.testing.assert_array_equal(got_d, want)


def test_nan_and_far_positions_write_zero():
    bev = C.bev_maps(2, 8, 13, 7, seed=4)
    mats = np.stack([EYE, EYE]).copy()
    mats[0, 0, 2] = np.nan
    mats[1, 1, 2] = 1e30
    got = _warp(bev, C.THREE, mats)
    np.testing.assert_array_equal(got, np.zeros_like(got))
    np.testing.assert_array_equal(got, C.warp_labels(bev, C.THREE, mats))


@pytest.mark.parametrize("X,Y", [(13, 7), (200, 200)])
def test_identity_is_todays_labels(X, Y):
    bev = C.bev_maps(3, 8, X, Y, seed=X)
    bev_d = torch.from_numpy(bev).to(DEV)
    eye = np.stack([EYE] * 3)
    assert torch.equal(simbev.class_masks(bev_d, C.THREE, index_mats=eye), simbev.class_masks(bev_d, C.THREE))
    assert torch.equal(simbev.class_masks(bev_d, None, index_mats=eye), simbev.vehicle_masks(bev_d))
    with pytest.raises(RuntimeError):
        simbev.class_masks(bev_d, C.THREE, index_mats=eye[:2])          # one matrix per sample
    with pytest.raises(RuntimeError):
        simbev.class_masks(bev_d, C.THREE, index_mats=eye.astype(np.float64))


@pytest.mark.parametrize("name", list(C.SYMMETRIES))
@pytest.mark.parametrize("X", [12, 200])
def test_symmetries_are_rot90_and_flip_of_the_unwarped_labels(X, name):
    """(tests/test_bev_aug_host.py shows the restatement exact on these; here the kernel itself.)"""
    (theta, fx, fy), _ = C.SYMMETRIES[name]
    bev = torch.from_numpy(C.bev_maps(2, 8, X, X, seed=X)).to(DEV)
    plain = simbev.class_masks(bev, C.THREE)
    mats = np.stack([_index(theta, 1.0, fx, fy, C.grid_conf(X, X))] * 2)
    got = simbev.class_masks(bev, C.THREE, index_mats=mats)
    want = {"rot90": lambda a: torch.rot90(a, 1, (2, 3)), "rot180": lambda a: torch.rot90(a, 2, (2, 3)),
            "rot270": lambda a: torch.rot90(a, 3, (2, 3)), "flip_x": lambda a: torch.flip(a, (2,)),
            "flip_y": lambda a: torch.flip(a, (3,)), "flip_xy": lambda a: torch.flip(a, (2, 3))}[name](plain)
    assert torch.equal(got, want)
    assert not torch.equal(got, plain)


# ----------------------------------------------------------------------------- direction and axes
def test_marked_points_land_at_A_p_and_not_at_A_inverse_p():
    """Ego points p at cell centres, a 3 x 3 block of source cells marked around each; under A (20 degrees, 0.95,
    flip_x) the label is 1 at the cell containing A p: an output centre within sqrt(1/2) cell of A p maps back to
    within 0.75 cell of p, inside the block. An inverted matrix would put it at A^-1 p, swapped axes elsewhere again:
    the label is 0 at the cell containing A^-1 p wherever that lies more than 3 cells from every marked image A q
    (a block reaches 1.5 * sqrt(2) * 0.95 = 2.02 cells from its A q, plus sqrt(1/2) to the cell's centre)."""
    X = Y = 200
    lo, d = -50.0, 0.5
    rng = np.random.default_rng(0)
    cells = []
    while len(cells) < 20:
        i, j = (int(v) for v in rng.integers(40, 160, 2))
        p = lo + (np.array([i, j]) + 0.5) * d
        if np.hypot(*p) <= 30.0:
            cells.append((i, j))
    bev = np.zeros((1, 8, X, Y), dtype=np.uint8)
    for i, j in cells:
        bev[0, 1, X - 1 - (i + 1):X - 1 - (i - 1) + 1, j - 1:j + 2] = 1  # rows X-1-i of the npz are x cell i
    A = simbev.bev_aug_matrix(20.0, 0.95, True, False)
    got = _warp(bev, None, simbev.label_index_matrix(A, C.GC)[None])[0, 0]
    A2 = A[:2, :2].astype(np.float64)
    P = np.array([lo + (np.array(c) + 0.5) * d for c in cells])
    fwd = (P @ A2.T - lo) / d              # A p in index units
    back = (P @ np.linalg.inv(A2).T - lo) / d
    checked = 0
    for k in range(len(cells)):
        fi, fj = (int(v) for v in np.floor(fwd[k]))
        assert got[fi, fj] == 1.0, (cells[k], fwd[k])
        if np.hypot(*(fwd - back[k]).T).min() > 3.0:
            bi, bj = (int(v) for v in np.floor(back[k]))
            assert got[bi, bj] == 0.0, (cells[k], back[k])
            checked += 1
    assert checked >= 10, checked
    assert 0 < got.sum() < 20 * 16  # about 9 / 0.95^2 cells per block


# ----------------------------------------------------------------------------- the geometry moves with it
def test_geometry_of_the_composed_rig():
    gc, dac = syn.grid_conf(), syn.data_aug_conf()
    rig = syn.make_rig(2, 6, dac["final_dim"], seed=3, aug=True)
    As = [simbev.bev_aug_matrix(20.0, 0.95, True, False), simbev.bev_aug_matrix(-17.0, 1.08, False, True)]
    rig2 = dict(rig)
    composed = [simbev.compose_rig(A, rig["rots"][b], rig["trans"][b]) for b, A in enumerate(As)]
    rig2["rots"] = torch.stack([c[0] for c in composed])
    rig2["trans"] = torch.stack([c[1] for c in composed])
    m = L.compile_model(gc, dac, 1).to(DEV)
    g0 = m.get_geometry(**{k: v.to(DEV) for k, v in rig.items()}).cpu().numpy()
    g1 = m.get_geometry(**{k: v.to(DEV) for k, v in rig2.items()}).cpu().numpy()
    for b, A in enumerate(As):
        want = g0[b].astype(np.float64) @ A.astype(np.float64).T
        err = np.abs(g1[b] - want).max()
        print(f"sample {b}: max |geom(composed) - A geom| = {err:.3e} m")
        # fp32 rounding at <= 64 m is about 4e-6 per operation over roughly ten operations on each side
        assert err < 1e-3
    frustum = ref.create_frustum(dac["final_dim"], gc["dbound"])
    np.testing.assert_array_equal(g1, ref.get_geometry(frustum, **rig2))  # bit-identical on the composed rig


# ----------------------------------------------------------------------------- loader paths
@pytest.fixture(scope="module")
def loaders():
    on = {**C.DAC, **C.BEV_ON}
    kw = dict(bsz=2, nworkers=0, parser_name="segmentationdata", device=DEV)
    tl, vl = simbev.compile_data("", ROOT, on, C.GC, **kw)
    tl_off, vl_off = simbev.compile_data("", ROOT, C.DAC, C.GC, **kw)
    assert tl.bev_aug and vl.bev_aug and not tl_off.bev_aug and not vl_off.bev_aug
    np.random.seed(3)
    torch.manual_seed(3)
    train = list(tl.loader)[:2]
    return {"train": train, "val": list(vl.loader), "val_off": list(vl_off.loader), "vl": vl, "vl_off": vl_off}


def _stager(**kw):
    return BatchStager(C.DAC["final_dim"], 2, 6, (C.DAC["H"], C.DAC["W"]), C.GC, DEV, **kw)


@pytest.mark.parametrize("groups", [None, C.THREE], ids=["vehicle", "three"])
def test_finish_batch_and_stager_agree(loaders, groups):
    fd = C.DAC["final_dim"]
    st = _stager(label_groups=groups, bev_aug=True)
    for raw in loaders["train"]:
        assert len(raw) == 10 and raw[8].shape == (2, 2, 3) and raw[8].dtype == torch.float32
        want = simbev.finish_batch(raw, fd, DEV, label_groups=groups, bev_aug=True)
        assert len(want) == 7
        st.stage(raw)
        assert st.commit() == 2
        torch.cuda.synchronize()
        for got, w in zip(st.inputs + (st.binimgs,), want):
            assert got.shape == w.shape and torch.equal(got, w)
        assert torch.equal(want[1].cpu(), raw[1]) and torch.equal(want[2].cpu(), raw[2])  # the rig arrives composed
        np.testing.assert_array_equal(want[6].cpu().numpy(), C.warp_labels(raw[9].numpy(), groups or C.VEHICLE,
                                                                          raw[8].numpy()))
        plain = simbev.class_masks(raw[9].to(DEV), groups)
        assert not torch.equal(want[6], plain) and want[6].sum().item() > 0
    with pytest.raises(RuntimeError):
        st.stage(loaders["val_off"][0])  # a raw batch without the matrices
    assert st.pending() == 0


def test_partial_batch_leaves_the_rest(loaders):
    fd = C.DAC["final_dim"]
    a, b = loaders["train"]
    st = _stager(bev_aug=True)
    st.stage(a)
    st.commit()
    torch.cuda.synchronize()
    before = [t.clone() for t in st.inputs + (st.binimgs,)]
    one = tuple(t[:1] for t in b)
    want = simbev.finish_batch(one, fd, DEV, bev_aug=True)
    st.stage(one)
    assert st.commit() == 1
    torch.cuda.synchronize()
    assert st.n_valid.item() == 1
    for got, w, old in zip(st.inputs + (st.binimgs,), want, before):
        assert torch.equal(got[:1], w) and torch.equal(got[1:], old[1:])
    assert not torch.equal(st.binimgs[:1], before[-1][:1])


def test_validation_is_never_augmented(loaders):
    """The validation loader's finished batches are the same with the option on and off, through both paths."""
    on, off = next(iter(loaders["vl"])), next(iter(loaders["vl_off"]))
    assert len(on) == len(off) == 7
    for x, y in zip(on, off):
        assert torch.equal(x, y)
    assert on[6].sum().item() > 0
    st = _stager(bev_aug=True)
    st.stage(loaders["val"][0])
    st.commit()
    torch.cuda.synchronize()
    for got, w in zip(st.inputs + (st.binimgs,), off):
        assert torch.equal(got, w)


# ----------------------------------------------------------------------------- trainer
def _events(logdir):
    return [json.loads(line) for line in open(os.path.join(str(logdir), "metrics.jsonl"))]


def test_trainer_runs_seeded_and_reproduces(tmp_path):
    """Four captured steps with the augmentation on: finite losses, no skipped step, the three values in the config
    event; the same seed again gives the same logged losses (MIOpen's deterministic solvers, as
    tests/test_gpu_trainer.py explains: without them no two runs at this shape agree, augmented or not)."""
    old = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    try:
        losses = []
        for tag in ("a", "b"):
            logdir = tmp_path / tag
            out = trainer.train(ROOT, nepochs=1, seed=0, graph=True, max_steps=4, loss_step=1, logdir=str(logdir),
                                bev_rot_lim=(-22.5, 22.5), bev_scale_lim=(0.9, 1.1), bev_flip=True, **KW)
            assert out["counter"] == 4 and out["skipped"] == 0 and math.isfinite(out["loss"])
            events = _events(logdir)
            cfg = events[0]
            assert cfg["event"] == "config" and cfg["bev_rot_lim"] == [-22.5, 22.5]
            assert cfg["bev_scale_lim"] == [0.9, 1.1] and cfg["bev_flip"] is True
            got = [e["loss"] for e in events if e["event"] == "train"]
            assert len(got) == 4 and all(math.isfinite(v) for v in got)
            print(f"run {tag}: losses {got}")
            losses.append(got)
        assert losses[0] == losses[1]
    finally:
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = old
