"""Case tables of the kernel-selection arms (tests/test_gpu_dispatch_arms.py runs them on the GPU,
tests/test_host.py proves on the CPU that they cover every arm).

The C entry points choose among many kernel instantiations by shape and dtype; the library reports each
choice through a host-only query (lss_splat_bwd_arm, lss_lift_prep_arm, lss_dwconv_arm; the launchers
switch on the same functions). Every case here carries its arguments and the arm it is meant to hit.
No GPU is needed to import this module: inputs and references are numpy / CPU torch.
"""
from collections import namedtuple
from itertools import product

import numpy as np
import torch

C = 64  # camC, the context channels (include/lss_hip.h)
F32, BF16 = torch.float32, torch.bfloat16
EUNSUPPORTED = -2

# ----------------------------------------------------------------------------- tolerances (the project's own)
# Lift/splat, fp32 outputs: ATOL of tests/test_gpu_parity2.py (rtol = atol = 1e-4). bf16 outputs:
# test_finer_dbound_d82_fwd_bwd's bars, 2 * 2^-8 |want| + 1e-3 for gradients, 2^-8 |want| + 1e-4 for the BEV.
# Depthwise: test_depthwise_fwd_bwd_vs_fp64's (tests/test_gpu_convs.py).
# Room of a plain fp32 numpy / torch evaluation of each reference formula against its fp32 bar (largest
# |fp32 - fp64| / bar over the elements, test_host.py::test_arm_references_fp32_margins asserts <= 1/4):
#   splat backward, D = 256 on (1, 2, 2, 4):          0.0042 of the bar
#   lift prep, D = 256 on 195 pixels:                 0.0050
#   splat forward, Z = 2, crowded cell of 16 points:  0.0009 fused, 0.0037 lifted
#   depthwise, the banded 700 x 8 plane (K = 5):      y / dx 0.032, dw 0.013
#   depthwise, 3 x 2 planes of 128 x 176 (stride 2):  y / dx 0.010, dw 0.035
# (so every bar has 28x room or more over fp32 arithmetic: no input needed scaling)
F32_TOL = dict(rtol=1e-4, atol=1e-4)


def lss_bar(want: np.ndarray, out_dtype, bev: bool = False) -> np.ndarray:
    """The allowed |got - want| per element of a lift/splat output."""
    want = np.abs(want)
    if out_dtype == F32:
        return F32_TOL["atol"] + F32_TOL["rtol"] * want
    return 2.0 ** -8 * want + 1e-4 if bev else 2 * 2.0 ** -8 * want + 1e-3


def dw_tols(dtype):
    """(y and dx, dw) tolerances of test_depthwise_fwd_bwd_vs_fp64."""
    if dtype == F32:
        return dict(rtol=1e-5, atol=1e-5), dict(rtol=1e-4, atol=1e-3)
    return dict(rtol=1e-2, atol=2e-2), dict(rtol=1e-4, atol=5e-2)


def rounded(a: np.ndarray, dtype) -> torch.Tensor:
    """a as a CPU tensor of dtype (bf16: nearest even)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)


def softmax(x: np.ndarray, axis: int) -> np.ndarray:
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


# ----------------------------------------------------------------------------- splat backward
# lss_splat_bwd_arm's codes (include/lss_hip.h)
TILE4, TILE48, TILE64, REG1, REG2, REG4 = range(6)
BWD_ARM_NAMES = ("tile4", "tile48", "tile64", "reg1", "reg2", "reg4")
# bf16 rows take the 4-pixel tile wherever an 8-pixel tile with D <= 48 would do, fp32 rows never take it
BWD_ARMS = {F32: {TILE48, TILE64, REG1, REG2, REG4}, BF16: {TILE4, TILE64, REG1, REG2, REG4}}
BWD_GRID = (4, 5)  # X, Y cells
BWD_D = (1, 41, 48, 49, 64, 65, 128, 129, 256)

# shape (B, N, H, W), D, Z, the arm with fp32 rows, the arm with bf16 rows
BwdCase = namedtuple("BwdCase", "shape D Z arm_f32 arm_bf16")
_WHOLE8, _HW4, _HW12, _HW15, _HW6 = (1, 2, 2, 4), (1, 3, 2, 2), (1, 1, 3, 4), (1, 2, 3, 5), (1, 1, 2, 3)
BWD_CASES = [
    # H*W = 8, whole 8-pixel tiles: every tile arm, and the register chunks past D = 64
    BwdCase(_WHOLE8, 1, 1, TILE48, TILE4), BwdCase(_WHOLE8, 41, 2, TILE48, TILE4),
    BwdCase(_WHOLE8, 48, 1, TILE48, TILE4), BwdCase(_WHOLE8, 49, 2, TILE64, TILE64),
    BwdCase(_WHOLE8, 64, 1, TILE64, TILE64), BwdCase(_WHOLE8, 65, 1, REG2, REG2),
    BwdCase(_WHOLE8, 128, 2, REG2, REG2), BwdCase(_WHOLE8, 129, 1, REG4, REG4),
    BwdCase(_WHOLE8, 256, 2, REG4, REG4),
    # H*W = 15, 30 pixels: no tile; the register kernel's last block of four pixels is half empty
    BwdCase(_HW15, 48, 2, REG1, REG1), BwdCase(_HW15, 49, 1, REG1, REG1), BwdCase(_HW15, 64, 2, REG1, REG1),
    BwdCase(_HW15, 65, 2, REG2, REG2), BwdCase(_HW15, 128, 1, REG2, REG2), BwdCase(_HW15, 129, 2, REG4, REG4),
    # H*W = 4: the 4-pixel tile is allowed, the 8-pixel tile is not
    BwdCase(_HW4, 41, 1, REG1, TILE4), BwdCase(_HW4, 49, 2, REG1, REG1),
    # H*W = 12: a multiple of 4, not of 8
    BwdCase(_HW12, 48, 2, REG1, TILE4),
    # H*W = 6
    BwdCase(_HW6, 1, 1, REG1, REG1), BwdCase(_HW6, 256, 1, REG4, REG4),
]
# (shape, D below, D above, split): the neighbours across each bound of the rule, on a shape where a tile is
# eligible and on one where it is not; they land on different arms, except that 48 | 49 bounds the tiles only
BWD_BOUNDARIES = [(s, lo, lo + 1, s == _WHOLE8 or lo != 48) for s in (_WHOLE8, _HW15) for lo in (48, 64, 128)]
# g dtype, d dtype, ctx dtype, rows layout (0 = the rows buffer in cell order, 1 = the channels-last dbev)
BWD_COMBOS = list(product((F32, BF16), (F32, BF16), (F32, BF16), (0, 1)))


def bwd_arm_of(case: BwdCase, g_dtype) -> int:
    return case.arm_f32 if g_dtype == F32 else case.arm_bf16


def bwd_inputs(case: BwdCase):
    """depth (BN, D, H, W) fp32, cell_of (BN, D, H, W) int32, ctx (npix, C), gradient rows (ncells, C) in cell
    order; pixel 0 has every bin dropped, pixel 1 has every bin in one cell, about a quarter of the rest dropped."""
    B, N, H, W = case.shape
    D, Z = case.D, case.Z
    X, Y = BWD_GRID
    ncells = B * Z * X * Y
    rng = np.random.default_rng(1000 * D + 10 * H * W + Z)
    depth = softmax(rng.standard_normal((B * N, D, H, W)) * 2.0, axis=1).astype(np.float32)
    cell_of = rng.integers(0, ncells, size=(B * N, D, H, W)).astype(np.int32)
    cell_of[rng.random(cell_of.shape) < 0.25] = -1
    cell_of[0, :, 0, 0] = -1
    cell_of[0, :, 0, 1] = 7
    ctx = rng.standard_normal((B * N * H * W, C)).astype(np.float32)
    g_rows = rng.standard_normal((ncells, C)).astype(np.float32)
    return depth, cell_of, ctx, g_rows


def dbev_of_rows(g_rows: torch.Tensor, B: int, Z: int) -> torch.Tensor:
    """The (B, Z*C, X, Y) gradient whose cell ((b*Z + z)*X + x)*Y + y has the row g_rows[cell]."""
    X, Y = BWD_GRID
    return g_rows.reshape(B, Z, X, Y, C).permute(0, 1, 4, 2, 3).reshape(B, Z * C, X, Y)


def bwd_reference(depth, cell_of, ctx, g_rows, dtype=np.float64):
    """d_depthnet_out (BN, D + C, H, W) from the (rounded) inputs: with r the gradient row of point (q, d), zero
    where cell_of is -1: d_ctx[q, c] = sum_d depth[q, d] r[c]; dd[q, d] = sum_c r[c] ctx[q, c];
    d_logit = depth (dd - sum_d depth dd)."""
    BN, D, H, W = depth.shape
    dep = depth.transpose(0, 2, 3, 1).reshape(-1, D).astype(dtype)
    cel = cell_of.transpose(0, 2, 3, 1).reshape(-1, D)
    r = np.where(cel[..., None] >= 0, g_rows.astype(dtype)[np.maximum(cel, 0)], dtype(0))
    d_ctx = np.einsum("qd,qdc->qc", dep, r)
    dd = np.einsum("qdc,qc->qd", r, ctx.astype(dtype))
    d_logit = dep * (dd - (dep * dd).sum(axis=1, keepdims=True))
    out = np.concatenate([d_logit, d_ctx], axis=1)  # (npix, D + C)
    return out.reshape(BN, H, W, D + C).transpose(0, 3, 1, 2)


# ----------------------------------------------------------------------------- lift prep
PREP_ARMS = {16, 32, 64}  # depth bins per wave part (lss_lift_prep_arm)
PREP_D = {1: 16, 2: 16, 41: 16, 64: 16, 65: 32, 128: 32, 129: 64, 255: 64, 256: 64}
PREP_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 5, 13)]  # (B*N, H, W); the last: three 64-pixel blocks and 3 pixels
PREP_BOUNDARIES = [(64, 65), (128, 129)]
PREP_COMBOS = list(product((F32, BF16), (F32, BF16)))  # in dtype, ctx dtype


def prep_input(BN: int, D: int, H: int, W: int) -> np.ndarray:
    """(BN, D + C, H, W): logits scaled by 8, the last pixel's alternating +-80 (a softmax without the max
    subtraction overflows there)."""
    rng = np.random.default_rng(D * 100 + H * W)
    x = rng.standard_normal((BN, D + C, H, W)).astype(np.float32)
    x[:, :D] *= 8.0
    x[-1, :D, -1, -1] = np.where(np.arange(D) % 2 == 0, 80.0, -80.0)
    return x


def prep_reference(x: np.ndarray, D: int, dtype=np.float64):
    """depth (BN, D, H, W) = softmax over the D logits; the context as pixel-major rows (exact)."""
    return softmax(x[:, :D].astype(dtype), axis=1), x[:, D:].transpose(0, 2, 3, 1).reshape(-1, C)


# ----------------------------------------------------------------------------- splat forward
FWD_DIMS = (2, 2, 7, 3, 5)  # B, N, D, H, W
FWD_XY = (8, 8)
# mode: the fused lift with fp32 / bf16 context rows, or per-point rows; out dtype; layout (0 NCHW, 1 NHWC)
FWD_MODES = ("fused_f32", "fused_bf16", "lifted")
FWD_ARMS = set(product((0, 1), FWD_MODES, (F32, BF16)))  # the 12 instantiations of lss_splat_fwd
FWD_CASES = [(layout, mode, out, Z) for (layout, mode, out) in sorted(FWD_ARMS, key=str) for Z in (1, 2)]
FWD_CROWD = 16  # points put into one cell


def fwd_grid(Z: int):
    """(lo, dx, nx) of the 8 x 8 x Z unit-cell grid."""
    X, Y = FWD_XY
    return (-4.0, -4.0, 0.0), (1.0, 1.0, 1.0), (X, Y, Z)


def fwd_geometry(Z: int):
    """geom (B, N, D, H, W, 3) fp32 at cell centres and the cell of every point (-1 outside the grid: about one
    coordinate in ten lies two cells outside); the first FWD_CROWD points of sample 1 share one cell."""
    B, N, D, H, W = FWD_DIMS
    X, Y = FWD_XY
    lo, dx, nx = fwd_grid(Z)
    rng = np.random.default_rng(77 + Z)
    idx = np.stack([rng.integers(0, n, size=(B, N, D, H, W)) for n in nx], axis=-1)
    out = rng.random(idx.shape) < 0.1
    idx = np.where(out, np.where(rng.random(idx.shape) < 0.5, -2, np.array(nx) + 1), idx)
    flat = idx.reshape(B, -1, 3)
    flat[1, :FWD_CROWD] = (3, 5, Z - 1)
    idx = flat.reshape(B, N, D, H, W, 3)
    geom = (np.array(lo) + (idx + 0.5) * np.array(dx)).astype(np.float32)
    kept = ((idx >= 0) & (idx < np.array(nx))).all(axis=-1)
    b = np.arange(B).reshape(B, 1, 1, 1, 1)
    cell = ((b * Z + idx[..., 2]) * X + idx[..., 0]) * Y + idx[..., 1]
    return geom, np.where(kept, cell, -1).reshape(-1).astype(np.int32)


def fwd_inputs(Z: int):
    """depth (BN, D, H, W) fp32 softmax, ctx (npix, C), per-point rows (Nprime, C)."""
    B, N, D, H, W = FWD_DIMS
    rng = np.random.default_rng(5 + Z)
    depth = softmax(rng.standard_normal((B * N, D, H, W)), axis=1).astype(np.float32)
    ctx = rng.standard_normal((B * N * H * W, C)).astype(np.float32)
    rows = rng.standard_normal((B * N * D * H * W, C)).astype(np.float32)
    return depth, ctx, rows


def fwd_reference(cell_of, Z: int, depth=None, ctx=None, rows=None, dtype=np.float64):
    """The BEV (B, Z*C, X, Y): scatter-add of depth x context (lifted mode: of the rows) into the cells."""
    B, N, D, H, W = FWD_DIMS
    X, Y = FWD_XY
    if rows is None:
        # point p = ((bn*D + d)*H + h)*W + w reads pixel q = bn*H*W + h*W + w
        dep = depth.astype(dtype).reshape(B * N, D, H * W)
        rows = (dep[..., None] * ctx.astype(dtype).reshape(B * N, 1, H * W, C)).reshape(-1, C)
    bev = np.zeros((B * Z * X * Y, C), dtype=dtype)
    keep = cell_of >= 0
    np.add.at(bev, cell_of[keep], rows.astype(dtype)[keep])
    return bev.reshape(B, Z, X, Y, C).transpose(0, 1, 4, 2, 3).reshape(B, Z * C, X, Y)


# ----------------------------------------------------------------------------- depthwise
DW_FWD, DW_BWD_DATA, DW_BWD_WEIGHT = 0, 1, 2  # lss_dwconv_arm's passes
DW_FAMILIES = ("lds_seg", "lds_tile", "planes22", "planes11", "reg", "s2_par0", "s2_par1", "s2_par2", "s2_par3")


def dw_arm_name(family: int, seg: int, banded: int, pb: int) -> str:
    """lss_dw_arm_t as the table writes it: family, and for the LDS families /SEG/ and banded | pb1 | pbN."""
    name = DW_FAMILIES[family]
    if name.startswith("lds"):
        name += "/%d/%s" % (seg, "banded" if banded else "pb1" if pb == 1 else "pbN")
    return name


def dw_arms(pas: int, K: int, S: int) -> set:
    """Every arm include/lss_convs.h enumerates for a pass at (K, stride)."""
    if pas == DW_BWD_DATA and S == 2:
        return {"s2_par%d" % i for i in range(4)}
    fam = "lds_tile" if pas == DW_BWD_WEIGHT or (K, S) == (3, 1) else "lds_seg"
    arms = {"%s/%d/%s" % (fam, seg, m) for seg in (8, 4) for m in ("pbN", "pb1", "banded")} | {"reg"}
    if pas == DW_BWD_WEIGHT or S == 1:
        arms |= {"planes22", "planes11"}
    return arms


def dw_out(case):
    pl, pr, pt, pb = case.pads
    return (case.H + pt + pb - case.K) // case.S + 1, (case.W + pl + pr - case.K) // case.S + 1


def dw_groups(case) -> int:
    """The image groups _HipDepthwise gives the weight gradient."""
    Ho, Wo = dw_out(case)
    return max(1, min(case.N, (case.N * Ho * Wo) // 8192))


# K, stride, N, C, H, W (input), pads (left, right, top, bottom), the arm of each pass
DwCase = namedtuple("DwCase", "K S N C H W pads fwd bwd_data bwd_weight note")
DW_CASES = [
    DwCase(3, 1, 3, 24, 4, 8, (1, 1, 1, 1), 'lds_tile/8/pbN', 'lds_tile/8/pbN', 'lds_tile/8/pbN', 'PB > 1, SEG 8'),
    DwCase(3, 1, 3, 2, 4, 12, (1, 1, 1, 1), 'lds_tile/4/pbN', 'lds_tile/4/pbN', 'lds_tile/4/pbN', 'PB > 1, SEG 4'),
    DwCase(3, 1, 2, 2, 320, 8, (1, 1, 1, 1), 'lds_tile/8/pb1', 'lds_tile/8/pb1', 'lds_tile/8/pb1', 'whole plane, PB = 1, SEG 8'),
    DwCase(3, 1, 2, 2, 260, 12, (1, 1, 1, 1), 'lds_tile/4/pb1', 'lds_tile/4/pb1', 'lds_tile/4/pb1', 'whole plane, PB = 1, SEG 4'),
    DwCase(3, 1, 1, 1, 620, 8, (1, 1, 1, 1), 'lds_tile/8/banded', 'lds_tile/8/banded', 'lds_tile/8/banded', 'banded, SEG 8'),
    DwCase(3, 1, 1, 1, 480, 12, (1, 1, 1, 1), 'lds_tile/4/banded', 'lds_tile/4/banded', 'lds_tile/4/banded', 'banded, SEG 4'),
    DwCase(3, 1, 3, 2, 5, 22, (1, 1, 1, 1), 'planes22', 'planes22', 'planes22', 'planes 22'),
    DwCase(3, 1, 1, 3, 6, 11, (1, 1, 1, 1), 'planes11', 'planes11', 'planes11', 'planes 11'),
    DwCase(3, 1, 3, 2, 5, 7, (1, 1, 1, 1), 'reg', 'reg', 'reg', 'fallback, Wo 7'),
    DwCase(3, 1, 1, 2, 9, 10, (1, 1, 1, 1), 'reg', 'reg', 'reg', 'fallback, Wo 10'),
    DwCase(3, 1, 3, 2, 64, 88, (1, 1, 1, 1), 'lds_tile/8/pb1', 'lds_tile/8/pb1', 'lds_tile/8/pb1', 'two weight-gradient groups'),
    DwCase(3, 2, 3, 24, 8, 16, (0, 1, 0, 1), 'lds_seg/8/pbN', 's2_par0', 'lds_tile/8/pbN', 'PB > 1, SEG 8'),
    DwCase(3, 2, 3, 2, 8, 24, (0, 1, 0, 1), 'lds_seg/4/pbN', 's2_par0', 'lds_tile/4/pbN', 'PB > 1, SEG 4'),
    DwCase(3, 2, 2, 2, 280, 16, (0, 1, 0, 1), 'lds_seg/8/pb1', 's2_par0', 'lds_tile/8/pb1', 'whole plane, PB = 1, SEG 8'),
    DwCase(3, 2, 2, 2, 200, 24, (0, 1, 0, 1), 'lds_seg/4/pb1', 's2_par0', 'lds_tile/4/pb1', 'whole plane, PB = 1, SEG 4'),
    DwCase(3, 2, 1, 1, 560, 16, (0, 1, 0, 1), 'lds_seg/8/banded', 's2_par0', 'lds_tile/8/banded', 'banded, SEG 8'),
    DwCase(3, 2, 1, 1, 400, 24, (0, 1, 0, 1), 'lds_seg/4/banded', 's2_par0', 'lds_tile/4/banded', 'banded, SEG 4'),
    DwCase(3, 2, 3, 2, 10, 44, (0, 1, 0, 1), 'reg', 's2_par0', 'planes22', 'planes 22'),
    DwCase(3, 2, 1, 3, 12, 22, (0, 1, 0, 1), 'reg', 's2_par0', 'planes11', 'planes 11'),
    DwCase(3, 2, 3, 2, 10, 14, (0, 1, 0, 1), 'reg', 's2_par0', 'reg', 'fallback, Wo 7'),
    DwCase(3, 2, 1, 2, 18, 20, (0, 1, 0, 1), 'reg', 's2_par0', 'reg', 'fallback, Wo 10'),
    DwCase(3, 2, 3, 2, 128, 176, (0, 1, 0, 1), 'lds_seg/8/banded', 's2_par0', 'lds_tile/8/banded', 'two weight-gradient groups'),
    DwCase(3, 2, 3, 2, 5, 6, (0, 1, 0, 1), 'reg', 's2_par0', 'reg', 'stride-2 data parity (0, 0)'),
    DwCase(3, 2, 3, 2, 5, 6, (1, 1, 0, 1), 'reg', 's2_par1', 'reg', 'stride-2 data parity (0, 1)'),
    DwCase(3, 2, 3, 2, 5, 6, (0, 1, 1, 1), 'reg', 's2_par2', 'reg', 'stride-2 data parity (1, 0)'),
    DwCase(3, 2, 3, 2, 5, 6, (1, 1, 1, 1), 'reg', 's2_par3', 'reg', 'stride-2 data parity (1, 1)'),
    DwCase(3, 2, 3, 2, 6, 5, (0, 1, 0, 1), 'reg', 's2_par0', 'reg', 'stride-2 data parity (0, 0)'),
    DwCase(3, 2, 3, 2, 6, 5, (1, 1, 0, 1), 'reg', 's2_par1', 'reg', 'stride-2 data parity (0, 1)'),
    DwCase(3, 2, 3, 2, 6, 5, (0, 1, 1, 1), 'reg', 's2_par2', 'reg', 'stride-2 data parity (1, 0)'),
    DwCase(3, 2, 3, 2, 6, 5, (1, 1, 1, 1), 'reg', 's2_par3', 'reg', 'stride-2 data parity (1, 1)'),
    DwCase(3, 2, 3, 2, 4, 16, (2, 0, 1, 1), 'reg', 's2_par2', 'reg', 'Wo 8 but the right edge is not covered: no LDS'),
    DwCase(5, 1, 3, 24, 4, 8, (2, 2, 2, 2), 'lds_seg/8/pbN', 'lds_seg/8/pbN', 'lds_tile/8/pbN', 'PB > 1, SEG 8'),
    DwCase(5, 1, 3, 2, 4, 12, (2, 2, 2, 2), 'lds_seg/4/pbN', 'lds_seg/4/pbN', 'lds_tile/4/pbN', 'PB > 1, SEG 4'),
    DwCase(5, 1, 2, 2, 360, 8, (2, 2, 2, 2), 'lds_seg/8/pb1', 'lds_seg/8/pb1', 'lds_tile/8/pb1', 'whole plane, PB = 1, SEG 8'),
    DwCase(5, 1, 2, 2, 260, 12, (2, 2, 2, 2), 'lds_seg/4/pb1', 'lds_seg/4/pb1', 'lds_tile/4/pb1', 'whole plane, PB = 1, SEG 4'),
    DwCase(5, 1, 1, 1, 700, 8, (2, 2, 2, 2), 'lds_seg/8/banded', 'lds_seg/8/banded', 'lds_tile/8/banded', 'banded, SEG 8'),
    DwCase(5, 1, 1, 1, 540, 12, (2, 2, 2, 2), 'lds_seg/4/banded', 'lds_seg/4/banded', 'lds_tile/4/banded', 'banded, SEG 4'),
    DwCase(5, 1, 3, 2, 5, 22, (2, 2, 2, 2), 'planes22', 'planes22', 'planes22', 'planes 22'),
    DwCase(5, 1, 1, 3, 6, 11, (2, 2, 2, 2), 'planes11', 'planes11', 'planes11', 'planes 11'),
    DwCase(5, 1, 3, 2, 5, 7, (2, 2, 2, 2), 'reg', 'reg', 'reg', 'fallback, Wo 7'),
    DwCase(5, 1, 1, 2, 9, 10, (2, 2, 2, 2), 'reg', 'reg', 'reg', 'fallback, Wo 10'),
    DwCase(5, 1, 3, 2, 64, 88, (2, 2, 2, 2), 'lds_seg/8/pb1', 'lds_seg/8/pb1', 'lds_tile/8/pb1', 'two weight-gradient groups'),
    DwCase(5, 2, 3, 24, 8, 16, (1, 2, 1, 2), 'lds_seg/8/pbN', 's2_par3', 'lds_tile/8/pbN', 'PB > 1, SEG 8'),
    DwCase(5, 2, 3, 2, 8, 24, (1, 2, 1, 2), 'lds_seg/4/pbN', 's2_par3', 'lds_tile/4/pbN', 'PB > 1, SEG 4'),
    DwCase(5, 2, 2, 2, 280, 16, (1, 2, 1, 2), 'lds_seg/8/pb1', 's2_par3', 'lds_tile/8/pb1', 'whole plane, PB = 1, SEG 8'),
    DwCase(5, 2, 2, 2, 200, 24, (1, 2, 1, 2), 'lds_seg/4/pb1', 's2_par3', 'lds_tile/4/pb1', 'whole plane, PB = 1, SEG 4'),
    DwCase(5, 2, 1, 1, 480, 16, (1, 2, 1, 2), 'lds_seg/8/banded', 's2_par3', 'lds_tile/8/banded', 'banded, SEG 8'),
    DwCase(5, 2, 1, 1, 360, 24, (1, 2, 1, 2), 'lds_seg/4/banded', 's2_par3', 'lds_tile/4/banded', 'banded, SEG 4'),
    DwCase(5, 2, 3, 2, 10, 44, (1, 2, 1, 2), 'reg', 's2_par3', 'planes22', 'planes 22'),
    DwCase(5, 2, 1, 3, 12, 22, (1, 2, 1, 2), 'reg', 's2_par3', 'planes11', 'planes 11'),
    DwCase(5, 2, 3, 2, 10, 14, (1, 2, 1, 2), 'reg', 's2_par3', 'reg', 'fallback, Wo 7'),
    DwCase(5, 2, 1, 2, 18, 20, (1, 2, 1, 2), 'reg', 's2_par3', 'reg', 'fallback, Wo 10'),
    DwCase(5, 2, 3, 2, 128, 176, (1, 2, 1, 2), 'lds_seg/8/banded', 's2_par3', 'lds_tile/8/banded', 'two weight-gradient groups'),
    DwCase(5, 2, 3, 2, 5, 6, (1, 2, 1, 2), 'reg', 's2_par3', 'reg', 'stride-2 data parity (1, 1)'),
    DwCase(5, 2, 3, 2, 5, 6, (2, 2, 1, 2), 'reg', 's2_par2', 'reg', 'stride-2 data parity (1, 0)'),
    DwCase(5, 2, 3, 2, 5, 6, (1, 2, 2, 2), 'reg', 's2_par1', 'reg', 'stride-2 data parity (0, 1)'),
    DwCase(5, 2, 3, 2, 5, 6, (2, 2, 2, 2), 'reg', 's2_par0', 'reg', 'stride-2 data parity (0, 0)'),
    DwCase(5, 2, 3, 2, 6, 5, (1, 2, 1, 2), 'reg', 's2_par3', 'reg', 'stride-2 data parity (1, 1)'),
    DwCase(5, 2, 3, 2, 6, 5, (2, 2, 1, 2), 'reg', 's2_par2', 'reg', 'stride-2 data parity (1, 0)'),
    DwCase(5, 2, 3, 2, 6, 5, (1, 2, 2, 2), 'reg', 's2_par1', 'reg', 'stride-2 data parity (0, 1)'),
    DwCase(5, 2, 3, 2, 6, 5, (2, 2, 2, 2), 'reg', 's2_par0', 'reg', 'stride-2 data parity (0, 0)'),
    DwCase(5, 2, 3, 2, 4, 16, (4, 0, 2, 2), 'reg', 's2_par0', 'reg', 'Wo 8 but the right edge is not covered: no LDS'),
    DwCase(3, 1, 3, 2, 5, 10, (0, 0, 1, 1), 'lds_tile/8/pbN', 'reg', 'lds_tile/8/pbN', 'no padding: forward (Wo 8) on LDS, backward-data not'),
    DwCase(3, 1, 3, 2, 5, 8, (2, 2, 1, 1), 'reg', 'lds_tile/8/pbN', 'reg', 'wide padding: backward-data (8 wide) on LDS, forward not'),
]
DW_FOLD_OFF = [c for c in DW_CASES if c.note in ("two weight-gradient groups", "PB > 1, SEG 8", "planes 11")]


def dw_inputs(case, dtype):
    """x, w, dy as CPU tensors (x and dy rounded to dtype), drawn as test_depthwise_fwd_bwd_vs_fp64 draws them."""
    Ho, Wo = dw_out(case)
    g = torch.Generator().manual_seed(case.K * 100 + case.S * 10 + case.H + case.W)
    x = torch.randn(case.N, case.C, case.H, case.W, generator=g).to(dtype)
    w = torch.randn(case.C, 1, case.K, case.K, generator=g) * 0.2
    dy = torch.randn(case.N, case.C, Ho, Wo, generator=g).to(dtype)
    return x, w, dy
