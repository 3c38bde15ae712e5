"""Every kernel-selection arm of lss_splat_bwd, lss_lift_prep, lss_splat_fwd and lss_dwconv_* on the GPU, against a
plain fp64 reference of the same operation from the rounded inputs.

The cases are tests/arm_cases.py's; tests/test_host.py proves (through the host-only queries lss_splat_bwd_arm,
lss_lift_prep_arm and lss_dwconv_arm, which the launchers themselves switch on) that they reach every arm. The
lift/splat cases call the C ABI directly with synthetic inputs. Every output buffer starts as NaN and is compared
whole, so an element a kernel does not write fails its case. The lift/splat tests also run on the debug library
(tests/test_gpu_debug.py), under its device-side index checks.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import arm_cases as A  # noqa: E402
from lss_carla_amd import _lib, ops  # noqa: E402
from lss_carla_amd import efficientnet as E  # noqa: E402
from test_gpu_convs import _reference  # noqa: E402  (the fp64 depthwise reference)

DEV = torch.device("cuda:0")
NAN = float("nan")
_DT = {A.F32: "f32", A.BF16: "bf16"}


def _nan(shape, dtype) -> torch.Tensor:
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _within(got: torch.Tensor, want: np.ndarray, bar: np.ndarray, what: str = "") -> None:
    g = got.float().cpu().numpy().astype(np.float64)
    assert g.shape == want.shape, (g.shape, want.shape)
    assert np.isfinite(g).all(), f"{what}: {np.count_nonzero(~np.isfinite(g))} elements not written or not finite"
    diff = np.abs(g - want)
    with np.errstate(divide="ignore"):  # (an exact result meets any bar, a zero bar included; anything else over it is inf)
        over = np.divide(diff, bar, out=np.zeros_like(diff), where=diff > 0)
    i = np.unravel_index(np.argmax(over), over.shape)
    assert over[i] <= 1.0, f"{what}: at {i} got {g[i]}, want {want[i]}, bar {bar[i]}"


def _bwd_id(c) -> str:
    return "%dx%dx%dx%d-D%d-Z%d" % (*c.shape, c.D, c.Z)


# ----------------------------------------------------------------------------- splat backward
def _splat_bwd(case, D, g_dt, d_dt, c_dt, layout):
    """(return code, d_depthnet_out, inputs) of one lss_splat_bwd call on NaN-filled output."""
    lib = _lib.load()
    B, N, H, W = case.shape
    X, Y = A.BWD_GRID
    depth, cell_of, ctx, g_rows = A.bwd_inputs(case._replace(D=D))
    ctx_r, g_r = A.rounded(ctx, c_dt), A.rounded(g_rows, g_dt)
    if layout == _lib.NHWC:  # the channels-last dbev itself: rows in (b, x, y, z) order
        g_dev = A.dbev_of_rows(g_r, B, case.Z).to(DEV).contiguous(memory_format=torch.channels_last)
    else:                    # the rows buffer of lss_bev_rows: cell order
        g_dev = g_r.to(DEV)
    depth_d, cell_d, ctx_d = torch.from_numpy(depth).to(DEV), torch.from_numpy(cell_of).to(DEV), ctx_r.to(DEV)
    out = _nan((B * N, D + A.C, H, W), d_dt)
    grid = ops.GridSpec((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (X, Y, case.Z)).c_struct()
    code = lib.lss_splat_bwd(_lib.ptr(g_dev), _lib.dtype_code(g_dt), layout, _lib.ptr(cell_d), _lib.ptr(depth_d),
                             _lib.ptr(ctx_d), _lib.dtype_code(c_dt), ops.make_dims(B, N, D, H, W), grid, _lib.ptr(out),
                             _lib.dtype_code(d_dt), _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    return code, out, (depth, cell_of, ctx_r.float().numpy(), g_r.float().numpy())


@pytest.mark.parametrize("g_dt,d_dt,c_dt,layout", A.BWD_COMBOS,
                         ids=["g_%s-d_%s-ctx_%s-%s" % (_DT[g], _DT[d], _DT[c], ("rows", "nhwc")[l])
                              for g, d, c, l in A.BWD_COMBOS])
@pytest.mark.parametrize("case", A.BWD_CASES, ids=_bwd_id)
def test_splat_bwd_arm(case, g_dt, d_dt, c_dt, layout):
    B, N, H, W = case.shape
    arm = _lib.load().lss_splat_bwd_arm(_lib.dtype_code(g_dt), ops.make_dims(B, N, case.D, H, W))
    assert arm == A.bwd_arm_of(case, g_dt)
    code, out, ins = _splat_bwd(case, case.D, g_dt, d_dt, c_dt, layout)
    _lib.check(code, "lss_splat_bwd")
    want = A.bwd_reference(*ins)
    _within(out, want, A.lss_bar(want, d_dt), A.BWD_ARM_NAMES[arm])


@pytest.mark.parametrize("g_dt,d_dt", [(A.F32, A.F32), (A.BF16, A.BF16)], ids=["f32", "bf16"])
def test_splat_bwd_refuses_more_than_256_bins(g_dt, d_dt):
    code, out, _ = _splat_bwd(A.BWD_CASES[0], 257, g_dt, d_dt, g_dt, _lib.NCHW)
    assert code == A.EUNSUPPORTED
    with pytest.raises(RuntimeError, match="code -2"):
        _lib.check(code, "lss_splat_bwd")
    assert torch.isnan(out).all()  # nothing was launched


# ----------------------------------------------------------------------------- lift prep
def _lift_prep(shape, D, in_dt, ctx_dt):
    lib = _lib.load()
    BN, H, W = shape
    x = A.rounded(A.prep_input(BN, D, H, W), in_dt)
    x_d = x.to(DEV)
    depth, ctx_t = _nan((BN, D, H, W), torch.float32), _nan((BN * H * W, A.C), ctx_dt)
    code = lib.lss_lift_prep(_lib.ptr(x_d), _lib.dtype_code(in_dt), ops.make_dims(1, BN, D, H, W), _lib.ptr(depth),
                             _lib.ptr(ctx_t), _lib.dtype_code(ctx_dt), _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    return code, x, depth, ctx_t


@pytest.mark.parametrize("in_dt,ctx_dt", A.PREP_COMBOS, ids=["in_%s-ctx_%s" % (_DT[i], _DT[c]) for i, c in A.PREP_COMBOS])
@pytest.mark.parametrize("D", sorted(A.PREP_D))
@pytest.mark.parametrize("shape", A.PREP_SHAPES, ids=["%dx%dx%d" % s for s in A.PREP_SHAPES])
def test_lift_prep_arm(shape, D, in_dt, ctx_dt):
    BN, H, W = shape
    assert _lib.load().lss_lift_prep_arm(ops.make_dims(1, BN, D, H, W)) == A.PREP_D[D]
    code, x, depth, ctx_t = _lift_prep(shape, D, in_dt, ctx_dt)
    _lib.check(code, "lss_lift_prep")
    want_depth, want_ctx = A.prep_reference(x.float().numpy(), D)
    _within(depth, want_depth, A.lss_bar(want_depth, A.F32), "depth")
    # the context rows are the input's values, transposed: bit-equal to x.to(ctx_dtype)
    assert torch.equal(ctx_t.cpu(), torch.from_numpy(np.ascontiguousarray(want_ctx)).to(ctx_dt))


@pytest.mark.parametrize("in_dt", [A.F32, A.BF16], ids=["f32", "bf16"])
def test_lift_prep_refuses_more_than_256_bins(in_dt):
    code, _, depth, ctx_t = _lift_prep((2, 3, 5), 257, in_dt, in_dt)
    assert code == A.EUNSUPPORTED
    with pytest.raises(RuntimeError, match="code -2"):
        _lib.check(code, "lss_lift_prep")
    assert torch.isnan(depth).all() and torch.isnan(ctx_t).all()


# ----------------------------------------------------------------------------- splat forward
@functools.lru_cache(maxsize=None)
def _fwd_plan(Z: int):
    geom, cells = A.fwd_geometry(Z)
    plan = ops.plan_from_geom(torch.from_numpy(geom).to(DEV), ops.GridSpec(*A.fwd_grid(Z)))
    assert np.array_equal(plan.cell_of.cpu().numpy(), cells)  # cell centres: no rounding in the quantiser
    return plan, cells


@pytest.mark.parametrize("layout,mode,out_dt,Z", A.FWD_CASES,
                         ids=["%s-%s-out_%s-Z%d" % (("nchw", "nhwc")[l], m, _DT[o], z) for l, m, o, z in A.FWD_CASES])
def test_splat_fwd_arm(layout, mode, out_dt, Z):
    lib = _lib.load()
    plan, cells = _fwd_plan(Z)
    B = A.FWD_DIMS[0]
    X, Y = A.FWD_XY
    depth, ctx, rows = A.fwd_inputs(Z)
    depth_d = ctx_d = rows_d = None
    ctx_code = _lib.F32
    if mode == "lifted":
        rows_d = torch.from_numpy(rows).to(DEV)
        want = A.fwd_reference(cells, Z, rows=rows)
    else:
        ctx_r = A.rounded(ctx, A.F32 if mode == "fused_f32" else A.BF16)
        depth_d, ctx_d, ctx_code = torch.from_numpy(depth).to(DEV), ctx_r.to(DEV), _lib.dtype_code(ctx_r.dtype)
        want = A.fwd_reference(cells, Z, depth, ctx_r.float().numpy())
    out = ops._new_bev(B, Z, X, Y, out_dt, layout, DEV).fill_(NAN)
    _lib.check(lib.lss_splat_fwd(_lib.ptr(depth_d), _lib.ptr(ctx_d), ctx_code, _lib.ptr(rows_d), _lib.ptr(plan.cell_start),
                                 _lib.ptr(plan.sorted_key), _lib.ptr(plan.sorted_row), plan.c_dims, plan.grid.c_struct(),
                                 _lib.ptr(out), _lib.dtype_code(out_dt), layout, _lib.stream_handle(DEV), None, None),
               "lss_splat_fwd")
    torch.cuda.synchronize()
    assert (want == 0).any()  # some cells are empty: written as zeros
    _within(out, want, A.lss_bar(want, out_dt, bev=True), mode)


# ----------------------------------------------------------------------------- depthwise
class _NanTorch:
    """torch, except that empty / empty_like hand out NaN-filled tensors: what _HipDepthwise allocates for its
    outputs and partials, so an element a kernel does not write shows."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*a, **k):
        return torch.empty(*a, **k).fill_(NAN)

    @staticmethod
    def empty_like(*a, **k):
        return torch.empty_like(*a, **k).fill_(NAN)


def _dw_id(c) -> str:
    return "K%dS%d-%dx%dx%dx%d-p%d%d%d%d" % (c.K, c.S, c.N, c.C, c.H, c.W, *c.pads)


def _run_depthwise(case, dtype, monkeypatch):
    monkeypatch.setattr(E, "torch", _NanTorch())
    x, w, dy = A.dw_inputs(case, dtype)
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    y = E._HipDepthwise.apply(xd, wd, case.S, case.pads)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    y_ref, dx_ref, dw_ref = _reference(x, w, case.S, case.pads, dy)
    assert y.shape == y_ref.shape and y.dtype == dtype and wd.grad.dtype == torch.float32
    tol, wtol = A.dw_tols(dtype)
    torch.testing.assert_close(y.detach().cpu().double(), y_ref, msg=lambda m: f"forward ({case.fwd}): {m}", **tol)
    torch.testing.assert_close(xd.grad.cpu().double(), dx_ref, msg=lambda m: f"dx ({case.bwd_data}): {m}", **tol)
    torch.testing.assert_close(wd.grad.cpu().double(), dw_ref, msg=lambda m: f"dw ({case.bwd_weight}): {m}", **wtol)


@pytest.mark.parametrize("dtype", [A.F32, A.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", A.DW_CASES, ids=_dw_id)
def test_depthwise_arm(case, dtype, monkeypatch):
    monkeypatch.setattr(E, "DW_FOLD", True)  # the weight gradient folded by each channel's last block
    _run_depthwise(case, dtype, monkeypatch)


@pytest.mark.parametrize("dtype", [A.F32, A.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", A.DW_FOLD_OFF, ids=_dw_id)
def test_depthwise_arm_partials_summed_by_the_caller(case, dtype, monkeypatch):
    monkeypatch.setattr(E, "DW_FOLD", False)  # lss_dwconv_bwd_weight, the groups summed by torch
    _run_depthwise(case, dtype, monkeypatch)
