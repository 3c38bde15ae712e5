"""The plan kernels' camera-alive mask (lss_geometry_cells[_ordered]_masked, ABI 33), at plan level.

Shapes: B = 2, N = 3 and 6, a frustum of D = 5 over 3 x 7 pixels -- 105 points per camera, so the 256-point blocks
straddle cameras and samples -- on a 16 x 16 x 1 grid over +-50 m with synthetic.make_rig. Two mechanisms meet in
one equivalence: *masked* (all N cameras in the tensors, a (B, N) uint8 mask read on the device) and *compact*
(only the kept cameras in the tensors). Cell ids, CSR and the dead points' -1 are compared bit for bit against
oracle/lss_ref.py and against the compact plan; the lift + splat through a masked plan bit for bit against the
same call on a rig whose dead cameras are moved 1e6 m away (same shape, same kernels: any difference is the
mask's), and to the fp32 parity bar of tests/test_gpu_parity.py (1e-4) against the compact call."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import _lib, ops, simbev, synthetic as syn  # noqa: E402
from oracle import lss_ref as ref  # noqa: E402

DEV = torch.device("cuda:0")
ATOL = 1e-4  # tests/test_gpu_parity.py
B, D, FD = 2, 5, (48, 112)  # frustum (5, 3, 7, 3)
GC = syn.grid_conf(xy=(-50.0, 50.0, 6.25), z=(-10.0, 10.0, 20.0), dbound=(4.0, 44.0, 8.0))
GRID = ops.GridSpec.from_conf(GC)
FRUSTUM = ref.create_frustum(FD, GC["dbound"])
assert tuple(FRUSTUM.shape) == (5, 3, 7, 3)
DHW = 5 * 3 * 7
RIG_KEYS = ("rots", "trans", "intrins", "post_rots", "post_trans")
MODES = ["ordered", "unordered", "no_ws"]


def _patterns(N):
    ones = np.ones((B, N), dtype=np.uint8)
    one_dead = ones.copy()
    one_dead[:, 1] = 0
    per_sample = ones.copy()
    per_sample[0, 0] = 0
    per_sample[1, N - 1] = 0
    sample0 = ones.copy()
    sample0[0] = 0
    return {"all_alive": ones, "one_dead": one_dead, "per_sample": per_sample, "sample0_dead": sample0,
            "all_dead": np.zeros_like(ones)}


PATTERNS = ["all_alive", "one_dead", "per_sample", "sample0_dead", "all_dead"]


@pytest.fixture(autouse=True)
def _mode(request, monkeypatch):
    mode = request.node.callspec.params.get("mode") if hasattr(request.node, "callspec") else None
    if mode == "unordered":
        monkeypatch.setattr(ops, "USE_PLAN_ORDERED", False)
    elif mode == "no_ws":
        monkeypatch.setattr(ops, "USE_PLAN_WS", False)
    yield


def _rig(N, seed=0):
    return syn.make_rig(B, N, FD, seed=seed)


def _dev(rig):
    return {k: v.to(DEV) for k, v in rig.items()}


def _oracle_cells(rig):
    """(B, N, DHW) int32 cell ids (-1: out of grid) of a rig, oracle/lss_ref.py."""
    geom = ref.get_geometry(FRUSTUM, **rig)
    dx, bx, nx = ref.gen_dx_bx(GC["xbound"], GC["ybound"], GC["zbound"])
    ids, kept = ref.quantize(geom, dx, bx, nx)
    cell = np.where(kept, ref.output_cell(ids, nx), -1).astype(np.int32)
    return cell.reshape(rig["trans"].shape[0], rig["trans"].shape[1], -1)


def _compact(rig, alive):
    """The rig of the alive cameras alone, (B, k, ...), when every sample keeps the same k > 0; else None."""
    k = alive.sum(1)
    if k.min() != k.max() or k[0] == 0:
        return None
    idx = torch.from_numpy(np.stack([np.nonzero(a)[0] for a in alive]))  # (B, k)
    return {key: torch.stack([v[b, idx[b]] for b in range(B)]).contiguous() for key, v in rig.items()}


def _want_cells(rig, alive):
    """The masked plan's cell_of, from the oracle: the compact rig's voxel assignment scattered to the alive
    cameras' points (the full rig's where the pattern has no compact form), -1 on every dead point."""
    N = alive.shape[1]
    want = np.full((B, N, DHW), -1, dtype=np.int32)
    comp = _compact(rig, alive)
    if comp is not None:
        cc = _oracle_cells(comp)
        for b in range(B):
            want[b, np.nonzero(alive[b])[0]] = cc[b]
    else:
        full = _oracle_cells(rig)
        want[alive != 0] = full[alive != 0]
    return want.reshape(-1)


def _check_canonical_csr(plan, cell):
    """Ascending cell, then ascending point id; the sentinel key after the kept points; sorted_row = the pixel."""
    ncells = GRID.ncells(B)
    cs = plan.cell_start.cpu().numpy().astype(np.int64)
    total = int(cs[-1])
    kept = cell >= 0
    assert total == kept.sum()
    counts = np.bincount(cell[kept], minlength=ncells)
    np.testing.assert_array_equal(np.diff(cs), counts)
    sk_all = plan.sorted_key.cpu().numpy()
    sk = sk_all[:total]
    want_p = np.nonzero(kept)[0][np.argsort(cell[kept], kind="stable")]
    np.testing.assert_array_equal(sk & 0xFFFFFFFF, want_p)
    np.testing.assert_array_equal(sk >> 32, np.repeat(np.arange(counts.size), counts))
    assert (sk_all[total:] == -1).all()
    _, N, D_, H, W = plan.dims
    cam, rem = np.divmod(want_p, D_ * H * W)
    np.testing.assert_array_equal(plan.sorted_row.cpu().numpy()[:total], cam * H * W + rem % (H * W))


def _plan(rig, alive=None, **kw):
    t = None if alive is None else torch.from_numpy(np.ascontiguousarray(alive)).to(DEV)
    return ops.plan_from_cameras(FRUSTUM.to(DEV), **_dev(rig), grid=GRID, cam_alive=t, **kw)


def _far(rig, alive):
    """The rig with the dead cameras moved 1e6 m away: every one of their points is out of the grid."""
    out = {k: v.clone() for k, v in rig.items()}
    out["trans"][torch.from_numpy(alive == 0)] += 1.0e6
    return out


def test_the_rig_puts_a_quarter_of_the_alive_points_in_the_grid():
    for N in (3, 6):
        cell = _oracle_cells(_rig(N))
        for name, alive in _patterns(N).items():
            if alive.any():
                frac = (cell[alive != 0] >= 0).mean()
                assert frac >= 0.25, (N, name, frac)
        # the far-away rig's dead cameras land nowhere
        alive = _patterns(N)["per_sample"]
        assert (_oracle_cells(_far(_rig(N), alive))[alive == 0] == -1).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", [3, 6])
def test_all_alive_is_the_unmasked_plan_bit_for_bit(N, mode):
    rig = _rig(N)
    a = _plan(rig)
    b = _plan(rig, np.ones((B, N), dtype=np.uint8))
    total = int(a.cell_start[-1])
    assert total >= B * N * DHW // 4
    for name in ("cell_of", "cell_start", "sorted_key"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # (sorted_row is defined for the kept points only, include/lss_hip.h: the rest is never written)
    assert torch.equal(a.sorted_row[:total], b.sorted_row[:total])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N", [3, 6])
def test_masked_plan_against_the_oracle_and_the_compact_plan(N, pattern, mode):
    rig, alive = _rig(N), _patterns(N)[pattern]
    want = _want_cells(rig, alive)
    plan = _plan(rig, alive, want_geom=True)
    got = plan.cell_of.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    dead_pts = np.repeat(alive.reshape(-1) == 0, DHW)
    assert (got[dead_pts] == -1).all()
    _check_canonical_csr(plan, want)
    # out_geom is written for every point, dead cameras included
    np.testing.assert_array_equal(plan.geom.cpu().numpy(), ref.get_geometry(FRUSTUM, **rig))
    comp = _compact(rig, alive)
    if comp is None:
        return
    cplan = ops.plan_from_cameras(FRUSTUM.to(DEV), **_dev(comp), grid=GRID)
    assert torch.equal(plan.cell_start, cplan.cell_start)
    total = int(cplan.cell_start[-1])
    assert total == (want >= 0).sum() and (total > 0) == bool(alive.any())
    # compact point id (b, j, f) -> masked point id (b, cams[b][j], f)
    k = comp["trans"].shape[1]
    cams = np.stack([np.nonzero(a)[0] for a in alive])  # (B, k)
    ck = cplan.sorted_key.cpu().numpy()[:total]
    cp = ck & 0xFFFFFFFF
    cb, rem = np.divmod(cp, k * DHW)
    cj, f = np.divmod(rem, DHW)
    mapped = ((ck >> 32) << 32) | ((cb * N + cams[cb, cj]) * DHW + f)
    np.testing.assert_array_equal(plan.sorted_key.cpu().numpy()[:total], mapped)


@pytest.mark.parametrize("mode", ["ordered", "unordered"])
def test_masked_plans_leave_the_workspace_zero_filled(mode):
    N = 6
    rig, pats = _rig(N), _patterns(N)
    ops.PLAN_WS.clear()
    for name in ("one_dead", "sample0_dead", "per_sample"):
        plan = _plan(rig, pats[name])
        _check_canonical_csr(plan, _want_cells(rig, pats[name]))
    ws = ops.PLAN_WS.get(DEV, GRID.ncells(B), B * N * DHW, create=False)
    assert ws is not None and not ws.counts.any() and not ws.workspace.any()
    plan = _plan(rig)  # unmasked, on the same workspace
    _check_canonical_csr(plan, _oracle_cells(rig).reshape(-1))
    assert not ws.counts.any() and not ws.workspace.any()


def _bad_masks(N):
    ok = torch.ones(B, N, dtype=torch.uint8, device=DEV)
    return {"shape": torch.ones(B, N + 1, dtype=torch.uint8, device=DEV),
            "flat": torch.ones(B * N, dtype=torch.uint8, device=DEV),
            "dtype_bool": torch.ones(B, N, dtype=torch.bool, device=DEV),
            "dtype_int32": torch.ones(B, N, dtype=torch.int32, device=DEV),
            "host": torch.ones(B, N, dtype=torch.uint8),
            "strided": torch.ones(N, B, dtype=torch.uint8, device=DEV).t(),
            "not_a_tensor": np.ones((B, N), dtype=np.uint8)}, ok


@pytest.mark.parametrize("mode", MODES)
def test_bad_masks_raise_and_a_following_plan_is_correct(mode):
    N = 3
    rig = _rig(N)
    bad, ok = _bad_masks(N)
    for name, t in bad.items():
        with pytest.raises(RuntimeError, match="cam_alive") as e:
            ops.plan_from_cameras(FRUSTUM.to(DEV), **_dev(rig), grid=GRID, cam_alive=t)
        if torch.is_tensor(t):
            assert str(tuple(t.shape)) in str(e.value) and str(t.dtype) in str(e.value), (name, str(e.value))
    alive = _patterns(N)["one_dead"]
    _check_canonical_csr(_plan(rig, alive), _want_cells(rig, alive))
    ws = ops.PLAN_WS.get(DEV, GRID.ncells(B), B * N * DHW, create=False)
    if ws is not None:
        assert not ws.counts.any() and not ws.workspace.any()


# ----------------------------------------------------------------------------- lift + splat through a masked plan
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", [_lib.NCHW, _lib.NHWC])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_lift_splat_through_a_masked_plan(pattern, dtype, layout, mode):
    N = 6
    rig, alive = _rig(N), _patterns(N)[pattern]
    H, W = FRUSTUM.shape[1:3]
    dn = syn.make_depthnet_out(B, N, D, H, W, seed=4).to(DEV, dtype)

    def run(plan, x):
        x = x.clone().requires_grad_(True)
        bev = ops.lift_splat(x, plan, dtype, layout)
        torch.manual_seed(7)
        g = torch.randn(bev.shape, device=DEV).to(dtype)
        if layout == _lib.NHWC:
            g = g.contiguous(memory_format=torch.channels_last)
        bev.backward(g)
        return bev.detach(), x.grad.detach()

    bev_m, grad_m = run(_plan(rig, alive), dn)
    bev_f, grad_f = run(_plan(_far(rig, alive)), dn)
    assert bool(bev_m.any()) == bool(alive.any())
    assert torch.equal(bev_m, bev_f) and torch.equal(grad_m, grad_f)
    # the dead cameras' depthnet rows get exactly zero gradient
    dead = torch.from_numpy(alive.reshape(-1) == 0).to(DEV)
    assert not grad_m[dead].any() and bool(grad_m[~dead].any()) == bool(alive.any())
    comp = _compact(rig, alive)
    if comp is None or dtype != torch.float32:
        return
    # compact: only the alive cameras in the tensors, to the fp32 parity bar
    cplan = ops.plan_from_cameras(FRUSTUM.to(DEV), **_dev(comp), grid=GRID)
    bev_c, grad_c = run(cplan, dn[~dead])
    torch.testing.assert_close(bev_m, bev_c, rtol=0, atol=ATOL)
    torch.testing.assert_close(grad_m[~dead], grad_c, rtol=1e-4, atol=ATOL)


# ----------------------------------------------------------------------------- the full-size case
@pytest.mark.parametrize("mode", MODES)
def test_one_plan_at_c3_shape_with_one_dead_camera_per_sample(mode):
    cfg, gc, _ = syn.config_confs("c3")
    Bc, N, fd = cfg["B"], cfg["N"], cfg["final_dim"]
    assert (Bc, N) == (8, 6)
    rig = syn.make_rig(Bc, N, fd, seed=0)
    frustum = ref.create_frustum(fd, gc["dbound"]).to(DEV)
    assert tuple(frustum.shape[:3]) == (41, 8, 22)
    grid = ops.GridSpec.from_conf(gc)
    alive = np.ones((Bc, N), dtype=np.uint8)
    alive[np.arange(Bc), np.arange(Bc) % N] = 0
    far = {k: v.clone() for k, v in rig.items()}
    far["trans"][torch.from_numpy(alive == 0)] += 1.0e6
    dev = lambda r: {k: v.to(DEV) for k, v in r.items()}  # noqa: E731
    m = ops.plan_from_cameras(frustum, **dev(rig), grid=grid, cam_alive=torch.from_numpy(alive).to(DEV))
    f = ops.plan_from_cameras(frustum, **dev(far), grid=grid)
    u = ops.plan_from_cameras(frustum, **dev(rig), grid=grid)
    total = int(m.cell_start[-1])
    assert 0 < total < int(u.cell_start[-1])
    for name in ("cell_of", "cell_start"):
        assert torch.equal(getattr(m, name), getattr(f, name)), name
    assert torch.equal(m.sorted_key[:total], f.sorted_key[:total])
    assert torch.equal(m.sorted_row[:total], f.sorted_row[:total])
    dhw = 41 * 8 * 22
    assert (m.cell_of.view(Bc * N, dhw)[torch.from_numpy(alive.reshape(-1) == 0).to(DEV)] == -1).all()


# ----------------------------------------------------------------------------- the valid-cell mask
def test_valid_mask_counts_no_cell_for_a_dead_camera():
    """simbev.fov_cameras(alive=) through lss_simbev_valid_mask: a zero block sees nothing, so the mask with dead
    cameras is the mask of the alive cameras alone, and with every camera dead no cell is valid."""
    fd = (128, 352)
    gc = syn.grid_conf()
    rig = syn.make_rig(2, 6, fd, seed=3)
    per = torch.tensor([[1, 1, 1, 0, 1, 1], [0, 1, 1, 1, 1, 0]], dtype=torch.bool)
    out = torch.empty(2, 200, 200, device=DEV, dtype=torch.uint8)
    got = simbev.valid_mask(simbev.fov_cameras(**rig, alive=per), rig["post_trans"], gc, fd, out=out).clone()
    full = simbev.valid_mask(simbev.fov_cameras(**rig), rig["post_trans"], gc, fd, out=out).clone()
    assert full.float().mean() > 0.25 and (got <= full).all() and not torch.equal(got, full)
    for i in range(2):
        keep = [c for c in range(6) if per[i, c]]
        sub = {k: v[i:i + 1, keep].contiguous() for k, v in rig.items()}
        o1 = torch.empty(1, 200, 200, device=DEV, dtype=torch.uint8)
        want = simbev.valid_mask(simbev.fov_cameras(**sub), sub["post_trans"], gc, fd, out=o1)
        assert torch.equal(got[i], want[0]), i
    none = simbev.valid_mask(simbev.fov_cameras(**rig, alive=torch.zeros(6)), rig["post_trans"], gc, fd, out=out)
    assert not none.any()
